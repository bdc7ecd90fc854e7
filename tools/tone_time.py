#!/usr/bin/env python3
"""Times the tone bank beside the receive launch whose PCM it reads and prints one JSON line (also written to
profiles/tone_time.json).

1024 channels x 16 blocks of 512 PCM samples (8 MiB of int16, what one wbfm_1024x16 receive call writes), data resident,
warm, all five outputs asked for:
  - ctcss: K = 50 (the CTCSS tones in one group), L = 4096: 2 frames per channel
  - dtmf:  K = 8 (rows in group 0, columns in group 1), L = 256: 32 frames per channel
each as host clock around hrfd_tone_process_device + stream synchronise, p50 / p99 over --calls calls after --warmup, and as
device time between two events around --burst back-to-back calls (the launch overhead and the host's wait drop out).
--rx adds the receive call of the same batch (hrfd_rx_process_device, 1024 WBFM channels x 16 blocks of 262144 bytes) under the
same host clock, so that the two stand side by side from one run.

    python tools/tone_time.py [--calls 200] [--warmup 20] [--burst 20] [--rx] [--out profiles/tone_time.json]
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
SHAPES = {"ctcss": (4096, api.CTCSS_HZ, [2] * len(api.CTCSS_HZ)),
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--only", choices=sorted(SHAPES), help="one shape, for a counter run of its own")
    ap.add_argument("--rx", action="store_true", help="also time the receive call of the same batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tone_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/tone_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    pcm = torch.from_numpy(rng.integers(-8000, 8001, size=(C, BLOCKS, 512), dtype=np.int16)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}
    for name, (L, freqs, groups) in SHAPES.items():
        if a.only and name != a.only:
            continue
        F, K = 512 * BLOCKS // L, len(freqs)
        t = api.Tones(C, L, device=0)
        t.set_tones(freqs, groups)
        power = torch.zeros((C, F, K), dtype=torch.int64, device=dev)
        energy = torch.zeros((C, F), dtype=torch.int64, device=dev)
        valid = torch.zeros((C, F), dtype=torch.int32, device=dev)
        best = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
        present = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)

        def call():
            t.process_device(pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, power.data_ptr(), energy.data_ptr(),
                             valid.data_ptr(), best.data_ptr(), present.data_ptr(), sp)

        torch.cuda.synchronize()
        line[f"{name}_ms"] = timed(call, stream.synchronize, a.calls, a.warmup)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            for _ in range(a.burst):
                call()
            e1.record()
        stream.synchronize()
        line[f"{name}_device_ms"] = round(e0.elapsed_time(e1) / a.burst, 4)
        line[f"{name}_shape"] = {"frame_len": L, "tones": K, "frames_per_channel": F}
    if a.rx:
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
