#!/usr/bin/env python3
"""Times the DCS generator bank beside the tone generator call and the audio call over the same bytes, and prints one JSON line
(also written to profiles/dcsgen_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16, one transmit batch), data resident, warm, in place.  Four
cases of hrfd_dcsgen_process_device: every channel idle (nothing is read or written), a code without an end on every channel
at T = 1 (the single tap) and at T = 255 (api.dcs_lowpass_taps as shaping), and the last with the active bytes.  The clock is
set back to 0 in front of every call (a host store), so every call computes the same stretch of the stream; every case has
rows of its own, and the code's amplitude is 20, so that the rows stay far from saturation over the whole run.  Beside them,
under the same clock: the tone generator's call with one CTCSS sub-tone per channel, in place, and the audio call at T = 255,
whose dense stage (audio_fir_run) is the work the generator's shaping filter does.  Device time between two events around
--burst back-to-back calls; the variants take turns over --rounds rounds after --warmup, and the median and the range are
reported.  The bank is judged against the audio call of the same run, never against an earlier figure.

    python tools/dcsgen_time.py [--rounds 15] [--warmup 3] [--burst 20] [--out profiles/dcsgen_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hackrfdiags_amd import api  # noqa: E402

C, BLOCKS = 1024, 16


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcsgen_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/dcsgen_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    x = np.round(rng.normal(0.0, 1500.0, size=(C, BLOCKS, 512))).astype(np.int16)
    pcm = torch.from_numpy(x).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    active = torch.zeros((C, BLOCKS), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    variants, keep = {}, []

    def generator(name, taps, codes, d_active):
        gen = api.DcsGen(C, device=0)
        if taps is not None:
            gen.set_taps(taps)
        if codes:
            for c in range(C):
                gen.send(c, (0o023 + 9 * c) % 512, inverted=bool(c & 1), amplitude=20, start=0)
        rows = pcm.clone()
        keep.extend([gen, rows])

        def call():
            gen.set_time(0)
            gen.process_device(rows.data_ptr(), 1024 * BLOCKS, BLOCKS, rows.data_ptr(), 0, d_active, sp)
        variants[name] = call
        return gen

    generator("dcsgen_idle_ms", None, False, None)
    generator("dcsgen_T1_ms", None, True, None)
    g255 = generator("dcsgen_T255_ms", api.dcs_lowpass_taps(), True, None)
    generator("dcsgen_T255_active_ms", api.dcs_lowpass_taps(), True, active.data_ptr())

    tonegen = api.ToneGen(C, device=0)
    for c in range(C):
        tonegen.ctcss(c, api.CTCSS_HZ[c % len(api.CTCSS_HZ)], amplitude=20, start=0)
    tone_rows = pcm.clone()

    def tonegen_call():
        tonegen.set_time(0)
        tonegen.process_device(tone_rows.data_ptr(), 1024 * BLOCKS, BLOCKS, tone_rows.data_ptr(), 0, None, sp)
    variants["tonegen_ctcss_ms"] = tonegen_call

    audio = api.Audio(C, 1, device=0)
    audio.set_taps(api.audio_highpass_taps(255))
    out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    variants["audio_T255_ms"] = lambda: audio.process_device(pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), None, BLOCKS,
                                                             out.data_ptr(), 0, None, None, sp)

    times = {name: [] for name in variants}
    torch.cuda.synchronize()
    for r in range(a.warmup + a.rounds):
        for name, call in variants.items():                # the variants take turns
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                for _ in range(a.burst):
                    call()
                e1.record()
            stream.synchronize()
            if r >= a.warmup:
                times[name].append(e0.elapsed_time(e1) / a.burst)
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "rounds": a.rounds, "warmup": a.warmup,
            "burst": a.burst, "clock": "device time per call of a burst, the variants taking turns: median, least, most over the rounds"}
    for name, t in times.items():
        line[name] = {"p50": round(float(np.median(t)), 4), "min": round(min(t), 4), "max": round(max(t), 4)}
    for name in ("dcsgen_T1_ms", "dcsgen_T255_ms", "dcsgen_T255_active_ms"):
        line[name]["over_audio"] = round(line[name]["p50"] / line["audio_T255_ms"]["p50"], 3)
        line[name]["over_tonegen"] = round(line[name]["p50"] / line["tonegen_ctcss_ms"]["p50"], 3)
    line["active_blocks"] = int(active.sum().item())      # of 1024 x 16: the call keys every block
    line["clips_channel_0"] = g255.clips(0)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
