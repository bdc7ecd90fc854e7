#!/usr/bin/env python3
"""Times the DCS bank beside the audio call whose filter is the same dense work and the tone call that decodes the other kind of
sub-audible signalling, and prints one JSON line (also written to profiles/dcs_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16, what one wbfm_1024x16 receive call writes), data resident,
warm: every fourth channel carries a DCS code under noise, the rest noise alone.  hrfd_dcs_process_device with the default
low-pass of 255 taps and all three outputs at K = 1, 50 and 128 listed codes; hrfd_audio_process_device at T = 255 (the voice
high-pass, no bus) over the same PCM; hrfd_tone_process_device with the 50 CTCSS tones at a frame of 4096 and every output.
The variants take turns: a round times a burst of --burst back-to-back calls of each between two events on one stream (the
launch overhead and the host's wait drop out), and the rounds' median, least and most are reported per variant, so a drift
of the clocks falls on all alike.  The DCS call is judged against the audio and tone calls of the same run, never against an
earlier figure of its own.

    python tools/dcs_time.py [--rounds 15] [--warmup 3] [--burst 20] [--out profiles/dcs_time.json]
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

C, BLOCKS, TONE_L = 1024, 16, 4096


def distinct_codes(K):
    """K codes no two of which are aliases, D754 first"""
    out, seen = [], set()
    for code in [0o754] + list(range(512)):
        cw = api.dcs_canonical(api.dcs_word(code))
        if cw not in seen and len(out) < K:
            seen.add(cw)
            out.append(code)
    return out


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcs_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/dcs_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    n = BLOCKS * 512
    x = rng.normal(0.0, 1500.0, size=(C, n))
    x[::4] += api.dcs_levels(0o754, n, 2000).astype(np.float64)[None, :]
    pcm = torch.from_numpy(np.clip(np.round(x), -32768, 32767).astype(np.int16).reshape(C, BLOCKS, 512)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    best = torch.zeros((C, BLOCKS, 4), dtype=torch.uint8, device=dev)
    present = torch.zeros((C, BLOCKS, 4), dtype=torch.uint8, device=dev)
    variants, keep = {}, []

    for K in (1, 50, 128):
        bank = api.Dcs(C, device=0)
        bank.set_taps(api.dcs_lowpass_taps())
        bank.set_codes(distinct_codes(K), groups=[k % 4 for k in range(K)])
        hits = torch.zeros((C, BLOCKS, K), dtype=torch.int16, device=dev)
        keep += [bank, hits]
        variants[f"dcs_T255_K{K}_ms"] = (lambda b=bank, h=hits: b.process_device(
            pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, h.data_ptr(), best.data_ptr(), present.data_ptr(), sp))

    audio = api.Audio(C, 1, device=0)
    audio.set_taps(api.audio_highpass_taps(255))
    out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    variants["audio_T255_ms"] = lambda: audio.process_device(pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), None, BLOCKS,
                                                             out.data_ptr(), 0, None, None, sp)

    tones = api.Tones(C, TONE_L, device=0)
    tones.set_tones(freqs_hz=api.CTCSS_HZ)
    F = BLOCKS * 512 // TONE_L
    power = torch.zeros((C, F, len(api.CTCSS_HZ)), dtype=torch.int64, device=dev)
    energy = torch.zeros((C, F), dtype=torch.int64, device=dev)
    valid = torch.zeros((C, F), dtype=torch.int32, device=dev)
    t_best = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
    t_present = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
    variants["tone_50_L4096_ms"] = lambda: tones.process_device(pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, power.data_ptr(),
                                                                energy.data_ptr(), valid.data_ptr(), t_best.data_ptr(), t_present.data_ptr(), sp)

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
    for K in (1, 50, 128):
        line[f"dcs_K{K}_over_audio"] = round(line[f"dcs_T255_K{K}_ms"]["p50"] / line["audio_T255_ms"]["p50"], 3)
    line["dcs_K50_over_tone"] = round(line["dcs_T255_K50_ms"]["p50"] / line["tone_50_L4096_ms"]["p50"], 3)
    line["present_blocks_of_signal_channels"] = int(present[::4, 4:, 0].sum().item())      # of 256 x 12: the call decodes something
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
