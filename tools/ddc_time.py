#!/usr/bin/env python3
"""Times the DDC bank at the north-star shape and prints one JSON line.

16 captures x 64 channels = 1024 channels, R = 8 (16.384 MS/s captures), default filters, one 64 ms block per call:
  - hrfd_ddc_process_device alone (host clock around launch + stream synchronise)
  - hrfd_ddc_receive in WBFM (the DDC, then the rx bank over its output; blocking)
p50 / p99 over --calls calls after --warmup, and the work per call counted from the shapes.  Kernel time comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script.

    python tools/ddc_time.py [--calls 200] [--warmup 20]
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
    structure (packed dot2 per (tap pair, output, rail); the mixer's per-sample work; the halos of a 1024-output tile)"""
    m = BLOCK // 2                                         # outputs per channel
    tile = 1024
    halo_b = (tb - 1 + 1) & ~1
    a16 = m * (tile + halo_b) / tile                       # stage A outputs incl. stage B's look-back
    y = a16 * R + (m / tile) * ta                          # mixed input samples per channel
    macs = C * (2 * a16 * ta + 2 * m * tb + 4 * y)
    dot2 = C * (2 * a16 * (ta // 2 + 1) + 2 * m * (tb // 2 + 1) + 2 * y)
    mixer_other = C * y * 12                               # phase, index, table read, packing, shifts, stores
    return {"macs": macs, "lane_instr_est": dot2 + mixer_other, "outputs": C * m}


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/ddc_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    d = api.Ddc(W, C, R, device=0)
    for c in range(C):
        d.tune(c, c % W, float(rng.uniform(-7.5e6, 7.5e6)))
    cap = torch.from_numpy(rng.integers(-40, 41, size=(W, R * BLOCK), dtype=np.int8)).to(dev)
    out = torch.zeros((C, BLOCK), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream

    def ddc_call():
        d.process_device(cap.data_ptr(), R * BLOCK, BLOCK, out.data_ptr(), BLOCK, sp)
        stream.synchronize()

    t_ddc = []
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        ddc_call()
        if i >= a.warmup:
            t_ddc.append((time.perf_counter() - t0) * 1e3)

    rx = api.Rx(C, device=0)
    rx.set_mode(api.WBFM)
    pcm = torch.zeros((C, 1, 512), dtype=torch.int16, device=dev)
    npcm = torch.zeros((C, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t_rx, replayed = [], 0
    for i in range(a.warmup + a.calls):
        t0 = time.perf_counter()
        replayed += d.receive(rx, cap.data_ptr(), R * BLOCK, BLOCK, 1, pcm.data_ptr(), npcm.data_ptr())
        if i >= a.warmup:
            t_rx.append((time.perf_counter() - t0) * 1e3)

    ta, tb = api.q15_table("DDC_A8").size, api.q15_table("DDC_B").size
    k = counts(ta, tb)
    p50 = pct(t_ddc, 50)
    line = {
        "shape": {"captures": W, "channels": C, "decimation": R, "block_bytes": BLOCK, "taps_a": int(ta), "taps_b": int(tb)},
        "calls": a.calls, "warmup": a.warmup,
        "ddc_process_device_ms": {"p50": round(p50, 4), "p99": round(pct(t_ddc, 99), 4)},
        "ddc_receive_wbfm_ms": {"p50": round(pct(t_rx, 50), 4), "p99": round(pct(t_rx, 99), 4),
                                "budget_share_p99": round(pct(t_rx, 99) / BUDGET_MS, 4)},
        "receive_channels_replayed": int(replayed),
        "per_call": {"macs": k["macs"], "lane_instr_est": k["lane_instr_est"], "outputs": k["outputs"]},
        "implied_at_p50": {"gmac_per_s": round(k["macs"] / (p50 * 1e-3) / 1e9, 1),
                           "t_lane_instr_per_s": round(k["lane_instr_est"] / (p50 * 1e-3) / 1e12, 2),
                           "lane_instr_per_output": round(k["lane_instr_est"] / k["outputs"], 1)},
        "targets": {"ddc_process_device_ms": 1.5, "ddc_receive_budget_share_p99": 0.05},
    }
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
