#!/usr/bin/env python3
"""Times the DUC bank at the north-star shape and prints one JSON line.

16 captures x 64 channels = 1024 channels, R = 8 (16.384 MS/s captures), default filters, one 64 ms block per call
(131 072 channel samples, 262 144 bytes per channel in, 2 MiB per capture out):
  - hrfd_duc_process_device alone (host clock around launch + stream synchronise)
  - hrfd_duc_transmit in WBFM (the modulator bank, then the DUC over its output; synchronised after each call)
p50 / p99 over --calls calls after --warmup, and the work per call counted from the shapes.  Kernel time comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/duc_time.py [--calls 200] [--warmup 20]
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

W, C, R = 16, 64 * 16, 8
BLOCK = 262144
BUDGET_MS = 64.0


def counts(ta: int, tb: int) -> dict:
    """work per call from the shapes: MACs of the two FIRs and the mixer, and the kernel's lane instructions by its
    structure (packed dot2 per (tap pair, output, rail) of stage B over the tile and its look-back; stage A's dot2 per
    (tap pair, branch, position pair, rail); the mixer's ~15 instructions per wideband sample)"""
    m = BLOCK // 2                                         # channel samples per channel
    tile = 1024
    la = (ta - 1) // R
    b_out = m * (tile + la + 3) / tile                     # stage B outputs incl. stage A's look-back
    ja = (la + 1) // 2 + 1
    macs = C * (2 * m * tb + 2 * R * m * (ta / R) + 4 * R * m)
    dot2 = C * (2 * b_out * (tb // 2 + 1) + (m / 2) * R * ja * 4 + 2 * R * m)
    mixer_other = C * R * m * 13
    return {"macs": macs, "lane_instr_est": dot2 + mixer_other, "outputs": W * R * m}


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/duc_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    d = api.Duc(W, C, R, device=0)
    for c in range(C):
        d.tune(c, c % W, float(rng.uniform(-7.5e6, 7.5e6)))
    d.set_output_shift(14)                                 # 64 channels per capture
    chans = torch.from_numpy(rng.integers(-128, 128, size=(C, BLOCK), dtype=np.int8)).to(dev)
    caps = torch.zeros((W, R * BLOCK), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    t_duc = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        d.process_device(chans.data_ptr(), BLOCK, BLOCK, caps.data_ptr(), R * BLOCK, sp)
        stream.synchronize()
        if i >= a.warmup:
            t_duc.append((time.perf_counter() - t0) * 1e3)

    mod = api.Mod(api.MOD_WBFM, C, device=0)
    pcm = torch.from_numpy(rng.integers(-20000, 20000, size=(C, 512), dtype=np.int16)).to(dev)
    torch.cuda.synchronize()
    t_tx = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        d.transmit(mod, pcm.data_ptr(), 512, caps.data_ptr(), R * BLOCK, sp)
        stream.synchronize()
        if i >= a.warmup:
            t_tx.append((time.perf_counter() - t0) * 1e3)

    ta, tb = api.q15_table("DUC_A8").size, api.q15_table("DDC_B").size
    k = counts(ta, tb)
    p50 = pct(t_duc, 50)
    line = {
        "shape": {"captures": W, "channels": C, "interpolation": R, "block_bytes": BLOCK, "taps_a": int(ta),
                  "taps_b": int(tb)},
        "calls": a.calls, "warmup": a.warmup,
        "duc_process_device_ms": {"p50": round(p50, 4), "p99": round(pct(t_duc, 99), 4),
                                  "budget_share_p50": round(p50 / BUDGET_MS, 4)},
        "duc_transmit_wbfm_ms": {"p50": round(pct(t_tx, 50), 4), "p99": round(pct(t_tx, 99), 4),
                                 "budget_share_p99": round(pct(t_tx, 99) / BUDGET_MS, 4)},
        "clips_capture0": d.clips(0),
        "per_call": {"macs": k["macs"], "lane_instr_est": k["lane_instr_est"], "outputs": k["outputs"]},
        "implied_at_p50": {"gmac_per_s": round(k["macs"] / (p50 * 1e-3) / 1e9, 1),
                           "t_lane_instr_per_s": round(k["lane_instr_est"] / (p50 * 1e-3) / 1e12, 2)},
        "targets": {"duc_process_device_ms": 3.2},
    }
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
