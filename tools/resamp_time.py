#!/usr/bin/env python3
"""Times the resampler bank beside the audio call whose rows it reads and the receive call of the same batch, and prints one
JSON line (also written to profiles/resamp_time.json).

Data resident, warm, the taps of api.resample_taps:
  - up_6_1: 1024 channels x 16 blocks of 512 samples at 8 kS/s (16 MiB of int16, what one wbfm_1024x16 receive call or one
    audio call writes) to 48 kS/s, K = 40 taps per branch (96 MiB out)
  - down_1_6: 1024 channels of 49152 samples at 48 kS/s (the same second of audio, 96 MiB) to 8 kS/s, K = 240 (16 MiB out)
each as host clock around hrfd_resamp_process_device + stream synchronise, p50 / p99 over --calls calls after --warmup, and as
device time between two events around --burst back-to-back calls (the launch overhead and the host's wait drop out).  The
audio call (hrfd_audio_process_device, T = 255, one bus of 16 channels, all open) and the receive call of the same batch
(hrfd_rx_process_device, 1024 WBFM channels x 16 blocks of 262144 bytes) are timed in the same run under the same clocks: the
resampler is judged against that receive call, never against an earlier figure of its own.

    python tools/resamp_time.py [--calls 200] [--warmup 20] [--burst 20] [--no-rx] [--out profiles/resamp_time.json]
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
N8 = BLOCKS * 512
SHAPES = {"up_6_1": (6, 1, 40, N8), "down_1_6": (1, 6, 240, 6 * N8)}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resamp_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/resamp_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS}, "calls": a.calls, "warmup": a.warmup, "burst": a.burst}

    for name, (L, M, K, n_in) in SHAPES.items():
        x = torch.from_numpy(rng.integers(-8000, 8001, size=(C, n_in)).astype(np.int16)).to(dev)
        n_out = n_in * L // M
        y = torch.zeros((C, n_out), dtype=torch.int16, device=dev)
        bank = api.Resampler(C, L, M, device=0)
        taps = api.resample_taps(L, M, K)
        bank.set_taps(taps)
        counts = []
        line[f"{name}_ms"] = both_clocks(torch, stream, lambda: counts.append(
            bank.process_device(x.data_ptr(), 2 * n_in, None, n_in, y.data_ptr(), 0, n_out, sp)), a)
        assert set(counts) == {n_out}
        line[f"{name}_shape"] = {"taps": int(taps.size), "n_in": n_in, "n_out": n_out, "in_bytes": 2 * C * n_in, "out_bytes": 2 * C * n_out}
        bank.close()
        del x, y

    pcm = torch.from_numpy(rng.integers(-8000, 8001, size=(C, BLOCKS, 512)).astype(np.int16)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    audio = api.Audio(C, 1, device=0)
    audio.set_taps(api.audio_highpass_taps(255))
    audio.set_bus(0, [8 * j for j in range(16)], [api.AUDIO_UNITY_GAIN // 4] * 16)
    out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    mix = torch.zeros((1, BLOCKS, 512), dtype=torch.int16, device=dev)
    clips = torch.zeros(1, dtype=torch.int32, device=dev)
    line["audio_T255_M1_ms"] = both_clocks(torch, stream, lambda: audio.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), None, BLOCKS, out.data_ptr(), 0, mix.data_ptr(), clips.data_ptr(), sp), a)
    audio.close()

    if not a.no_rx:
        block = 262144
        rx = api.Rx(C, device=0)
        rx.set_mode(api.WBFM)
        iq = torch.randint(-40, 41, (C, BLOCKS * block), dtype=torch.int8, device=dev)      # 4 GiB: made where it is used
        out_n = torch.zeros((C, BLOCKS), dtype=torch.int32, device=dev)
        mag = torch.zeros((C, BLOCKS), dtype=torch.int32, device=dev)
        allowed = torch.zeros((C, BLOCKS), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        line["rx_wbfm_1024x16_ms"] = timed(
            lambda: rx.process_device(iq.data_ptr(), BLOCKS * block, block, BLOCKS, out.data_ptr(), out_n.data_ptr(),
                                      mag.data_ptr(), allowed.data_ptr(), stream=sp), lambda: rx.sync(), max(a.calls // 10, 5), 3)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
