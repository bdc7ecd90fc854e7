#!/usr/bin/env python3
"""Times the audio bank beside the receive call whose PCM it reads and the tone calls whose verdicts gate it, and prints one
JSON line (also written to profiles/audio_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16, what one wbfm_1024x16 receive call writes), data resident,
warm.  Every eighth channel carries a 100.0 Hz CTCSS tone over its noise (0.77 of the energy); a CTCSS tone call (K = 50,
L = 4096) and hrfd_audio_gate_device (want = that tone) give the gates, so an eighth of the channels is open.  Then, all
three outputs asked for (out, mix, clips):
  - T = 255 and T = 511 (the high-pass helper's taps)
  - one bus of 16 channels, and 64 buses of 16
each as host clock around hrfd_audio_process_device + stream synchronise, p50 / p99 over --calls calls after --warmup, and as
device time between two events around --burst back-to-back calls (the launch overhead and the host's wait drop out).  The
gate call, the two tone calls of tools/tone_time.py (ctcss, dtmf) and the receive call of the same batch
(hrfd_rx_process_device, 1024 WBFM channels x 16 blocks of 262144 bytes) are timed in the same run under the same clocks: the
audio call is judged against that receive call, never against an earlier figure of its own.

    python tools/audio_time.py [--calls 200] [--warmup 20] [--burst 20] [--no-rx] [--out profiles/audio_time.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hackrfdiags_amd import api  # noqa: E402

C, BLOCKS = 1024, 16
CTCSS_L, CTCSS_INDEX = 4096, 12                            # 100.0 Hz
TONE_SHAPES = {"ctcss": (CTCSS_L, api.CTCSS_HZ, [2] * len(api.CTCSS_HZ)),
               "dtmf": (256, api.DTMF_LOW_HZ + api.DTMF_HIGH_HZ, [0] * 4 + [1] * 4)}


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def timed(fn, sync, calls, warmup):
    t = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return {"p50": round(pct(t, 50), 4), "p99": round(pct(t, 99), 4)}


def both_clocks(torch, stream, call, a):
    """{"p50", "p99", "device"}: the host clock around call + synchronise, the device time per call of a burst"""
    torch.cuda.synchronize()
    r = timed(call, stream.synchronize, a.calls, a.warmup)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record()
        for _ in range(a.burst):
            call()
        e1.record()
    stream.synchronize()
    r["device"] = round(e0.elapsed_time(e1) / a.burst, 4)
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--no-rx", action="store_true", help="leave the receive call out (it needs 4 GiB of device memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/audio_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    x = rng.integers(-4000, 4001, size=(C, BLOCKS * 512)).astype(np.float64)
    x[::8] += 6000.0 * np.sin(2 * np.pi * api.CTCSS_HZ[CTCSS_INDEX] * np.arange(BLOCKS * 512) / api.TONE_FS)
    pcm = torch.from_numpy(np.round(x).astype(np.int16).reshape(C, BLOCKS, 512)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}

    # the tone calls, and the verdicts of the CTCSS one for the gate
    verdicts = {}
    for name, (L, freqs, groups) in TONE_SHAPES.items():
        F, K = 512 * BLOCKS // L, len(freqs)
        t = api.Tones(C, L, device=0)
        t.set_tones(freqs, groups)
        power = torch.zeros((C, F, K), dtype=torch.int64, device=dev)
        energy = torch.zeros((C, F), dtype=torch.int64, device=dev)
        valid = torch.zeros((C, F), dtype=torch.int32, device=dev)
        best = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
        present = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
        line[f"tone_{name}_ms"] = both_clocks(torch, stream, lambda: t.process_device(
            pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, power.data_ptr(), energy.data_ptr(), valid.data_ptr(),
            best.data_ptr(), present.data_ptr(), sp), a)
        verdicts[name] = (best, present)

    d_open = torch.zeros((C, BLOCKS), dtype=torch.uint8, device=dev)
    best, present = verdicts["ctcss"]
    out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    for T in (255, 511):
        for M in (1, 64):
            bank = api.Audio(C, M, device=0)
            bank.set_taps(api.audio_highpass_taps(T))
            bank.set_want(CTCSS_INDEX)
            for m in range(M):
                bank.set_bus(m, [(8 * (16 * m + j)) % C for j in range(16)], [api.AUDIO_UNITY_GAIN // 4] * 16)
            mix = torch.zeros((M, BLOCKS, 512), dtype=torch.int16, device=dev)
            clips = torch.zeros(M, dtype=torch.int32, device=dev)
            if T == 255 and M == 1:
                line["gate_ms"] = both_clocks(torch, stream, lambda: bank.gate_device(
                    best.data_ptr(), present.data_ptr(), CTCSS_L, 2, BLOCKS, d_open.data_ptr(), sp), a)
                line["open_blocks"] = int(d_open.sum().item())
            else:
                bank.gate_device(best.data_ptr(), present.data_ptr(), CTCSS_L, 2, BLOCKS, d_open.data_ptr(), sp)
            line[f"audio_T{T}_M{M}_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
                pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), d_open.data_ptr(), BLOCKS, out.data_ptr(), 0, mix.data_ptr(),
                clips.data_ptr(), sp), a)
            line[f"audio_T{T}_M{M}_clips"] = int(clips.sum().item())
            bank.close()

    if not a.no_rx:
        block = 262144
        rx = api.Rx(C, device=0)
        rx.set_mode(api.WBFM)
        iq = torch.randint(-40, 41, (C, BLOCKS * block), dtype=torch.int8, device=dev)      # 4 GiB: made where it is used
        out_pcm = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
        out_n = torch.zeros((C, BLOCKS), dtype=torch.int32, device=dev)
        mag = torch.zeros((C, BLOCKS), dtype=torch.int32, device=dev)
        allowed = torch.zeros((C, BLOCKS), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        line["rx_wbfm_1024x16_ms"] = timed(
            lambda: rx.process_device(iq.data_ptr(), BLOCKS * block, block, BLOCKS, out_pcm.data_ptr(), out_n.data_ptr(),
                                      mag.data_ptr(), allowed.data_ptr(), stream=sp), lambda: rx.sync(), max(a.calls // 10, 5), 3)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
