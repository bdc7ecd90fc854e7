#!/usr/bin/env python3
"""Times the conditioner bank beside the plain read kernel and the DDC it precedes and prints one JSON line (also written
to profiles/cal_time.json).

16 captures at R = 8 (16.384 MS/s), one 64 ms block per call (2 MiB per capture, 33.5 MB in all), data resident, warm:
  - hrfd_cal_process_device in its three modes: apply only (in place), measure only, both (in place), with the
    correction of tests/cal_model.py's recipe on every capture
  - the library's plain read kernel (hrfd_debug_membw, kind 0) over the same 33.5 MB
  - hrfd_ddc_process_device for 16 x 64 channels at R = 8
each as host clock around launch + stream synchronise, p50 / p99 over --calls calls after --warmup, all from this one run.
Apply reads and writes every byte, so its floor is twice the read kernel's time; measure only reads.

    python tools/cal_time.py [--calls 200] [--warmup 20] [--out profiles/cal_time.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cal_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/cal_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    n = R * BLOCK
    cap = torch.from_numpy(rng.integers(-40, 41, size=(W, n), dtype=np.int8)).to(dev)
    work = cap.clone()
    mom = torch.zeros((W, 8), dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"captures": W, "decimation": R, "bytes_per_capture": n, "bytes": W * n}, "calls": a.calls, "warmup": a.warmup}
    c = api.Conditioner(W, device=0)
    c.set_correction((588, -436), (16384, 0, -1145, 15495))
    torch.cuda.synchronize()
    modes = {"apply": lambda: c.process_device(work.data_ptr(), n, n, work.data_ptr(), n, None, sp),
             "measure": lambda: c.process_device(cap.data_ptr(), n, n, None, 0, mom.data_ptr(), sp),
             "both": lambda: c.process_device(work.data_ptr(), n, n, work.data_ptr(), n, mom.data_ptr(), sp)}
    for name, fn in modes.items():
        line[f"cal_{name}_ms"] = timed(fn, stream.synchronize, a.calls, a.warmup)
    lib = _lib.load()
    nbytes = W * n

    def read():
        assert lib.hrfd_debug_membw(0, ctypes.c_void_p(cap.data_ptr()), nbytes, None, ctypes.c_void_p(sp)) == 0

    line["read_ms"] = timed(read, stream.synchronize, a.calls, a.warmup)
    d = api.Ddc(W, CH, R, device=0)
    for ch in range(CH):
        d.tune(ch, ch % W, float(rng.uniform(-7.5e6, 7.5e6)))
    out = torch.zeros((CH, BLOCK), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    line["ddc_process_device_ms"] = timed(
        lambda: d.process_device(cap.data_ptr(), n, BLOCK, out.data_ptr(), BLOCK, sp), stream.synchronize, a.calls, a.warmup)
    for name in modes:
        p = line[f"cal_{name}_ms"]["p50"]
        line[f"cal_{name}_over_read"] = round(p / line["read_ms"]["p50"], 3)
        line[f"cal_{name}_over_ddc"] = round(p / line["ddc_process_device_ms"]["p50"], 4)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
