#!/usr/bin/env python3
"""Times the spectrum bank beside the DDC it steers and prints one JSON line (also written to profiles/spec_time.json).

16 captures at R = 8 (16.384 MS/s), one 64 ms block per call (2 MiB per capture, 33.5 MB in all), data resident, warm:
  - hrfd_spec_process_device at L = 11 (512 frames per capture) and L = 13 (128 frames), no bands
  - the library's plain read kernel (hrfd_debug_membw, kind 0) over the same 33.5 MB
  - hrfd_ddc_process_device for 16 x 64 channels at R = 8
each as host clock around launch + stream synchronise, p50 / p99 over --calls calls after --warmup, all from this one run.

    python tools/spec_time.py [--calls 200] [--warmup 20] [--out profiles/spec_time.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hackrfdiags_amd import _lib, api  # noqa: E402

W, R, CH = 16, 8, 64 * 16
BLOCK = 262144


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spec_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/spec_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    cap = torch.from_numpy(rng.integers(-40, 41, size=(W, R * BLOCK), dtype=np.int8)).to(dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"captures": W, "decimation": R, "bytes_per_capture": R * BLOCK, "bytes": W * R * BLOCK},
            "calls": a.calls, "warmup": a.warmup}
    for L in (11, 13):
        s = api.Spectrum(W, R, L, device=0)
        power = torch.zeros((W, 1 << L), dtype=torch.int64, device=dev)
        nf = R * BLOCK // (2 << L)
        torch.cuda.synchronize()
        line[f"spec_process_device_ms_L{L}"] = timed(
            lambda: s.process_device(cap.data_ptr(), R * BLOCK, nf, power.data_ptr(), None, None, sp), stream.synchronize,
            a.calls, a.warmup)
        s.close()
    lib = _lib.load()
    nbytes = W * R * BLOCK

    def read():
        assert lib.hrfd_debug_membw(0, ctypes.c_void_p(cap.data_ptr()), nbytes, None, ctypes.c_void_p(sp)) == 0

    line["read_ms"] = timed(read, stream.synchronize, a.calls, a.warmup)
    d = api.Ddc(W, CH, R, device=0)
    for c in range(CH):
        d.tune(c, c % W, float(rng.uniform(-7.5e6, 7.5e6)))
    out = torch.zeros((CH, BLOCK), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    line["ddc_process_device_ms"] = timed(
        lambda: d.process_device(cap.data_ptr(), R * BLOCK, BLOCK, out.data_ptr(), BLOCK, sp), stream.synchronize,
        a.calls, a.warmup)
    for L in (11, 13):
        p = line[f"spec_process_device_ms_L{L}"]["p50"]
        line[f"spec_over_ddc_L{L}"] = round(p / line["ddc_process_device_ms"]["p50"], 4)
        line[f"spec_over_read_L{L}"] = round(p / line["read_ms"]["p50"], 3)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
