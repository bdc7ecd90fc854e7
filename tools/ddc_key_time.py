#!/usr/bin/env python3
"""Times the DDC bank's receive key at tools/ddc_time.py's shape and prints one JSON line.

16 captures x 64 channels = 1024 channels, R = 8, default filters, one 64 ms block per call (131 072 output samples, one key
byte per channel at the default key block 2^17).  Six variants, one call of each in turn within one run, so that whatever
else the machine does meets all of them alike:
  a  hrfd_ddc_process_device, unkeyed
  b  keyed, every channel on                 (the price of the key when every station is on the air)
  c  keyed, 8 of every capture's 64 channels on
  d  keyed, every channel off
  e  hrfd_ddc_receive in WBFM, unkeyed
  f  hrfd_ddc_receive in WBFM, keyed as in c
Host clock around the call and the stream's synchronise (receive blocks by itself); p50 / p99 over --calls calls after
--warmup, and key_skips per call.  Every variant has its own handle, so the meter is its own.  The work model: a unit that
is on costs what it costs unkeyed, one that is off stores 2 KiB of zeros: c does 1/8 and d none of a's arithmetic, and the
output rows are written in full either way (1024 rows of 256 KiB = 256 MiB per call; `zero_bytes_per_call` says how much
of it is zeros).

    python tools/ddc_key_time.py [--calls 200] [--warmup 20] [--out profiles/ddc_key_time.json]
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
TILES = BLOCK // 2 // 1024
MODEL_C = 1 / 8


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddc_key_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/ddc_key_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    offsets = [float(rng.uniform(-7.5e6, 7.5e6)) for _ in range(C)]         # tools/ddc_time.py's tuning and captures

    def bank():
        d = api.Ddc(W, C, R, device=0)
        for c in range(C):
            d.tune(c, c % W, offsets[c])
        return d

    cap = torch.from_numpy(rng.integers(-40, 41, size=(W, R * BLOCK), dtype=np.int8)).to(dev)
    out = torch.zeros((C, BLOCK), dtype=torch.int8, device=dev)
    pcm = torch.zeros((C, 1, 512), dtype=torch.int16, device=dev)
    npcm = torch.zeros((C, 1), dtype=torch.int32, device=dev)
    all_on = torch.ones((C, 1), dtype=torch.uint8, device=dev)
    all_off = torch.zeros((C, 1), dtype=torch.uint8, device=dev)
    # channel c listens to capture c % 16 as its (c // 16)-th: every eighth of them hears a station
    some = torch.from_numpy((np.arange(C) // W % 8 == 0).astype(np.uint8).reshape(C, 1)).to(dev)
    assert int(some.sum()) == C // 8
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    rxs = {}
    for v in "ef":
        rxs[v] = api.Rx(C, device=0)
        rxs[v].set_mode(api.WBFM)
    ddcs = {v: bank() for v in "abcdef"}
    keys = {"a": None, "b": all_on, "c": some, "d": all_off, "e": None, "f": some}
    torch.cuda.synchronize()

    def call(v):
        k = keys[v]
        kp = None if k is None else k.data_ptr()
        if v in "ef":
            ddcs[v].receive(rxs[v], cap.data_ptr(), R * BLOCK, BLOCK, 1, pcm.data_ptr(), npcm.data_ptr(), d_key=kp, key_stride=1)
        else:
            ddcs[v].process_device(cap.data_ptr(), R * BLOCK, BLOCK, out.data_ptr(), BLOCK, sp, d_key=kp, key_stride=1)
            stream.synchronize()

    t = {v: [] for v in "abcdef"}
    for i in range(a.warmup + a.calls):
        for v in "abcdef":
            t0 = time.perf_counter()
            call(v)
            if i >= a.warmup:
                t[v].append((time.perf_counter() - t0) * 1e3)

    n_calls = a.warmup + a.calls
    names = {"a": "unkeyed", "b": "keyed_all_on", "c": "keyed_8_of_64_on", "d": "keyed_all_off", "e": "receive_wbfm_unkeyed",
             "f": "receive_wbfm_keyed_8_of_64_on"}
    res = {}
    for v in "abcdef":
        skips = ddcs[v].key_skips()
        assert skips % n_calls == 0
        res[names[v]] = {"p50_ms": round(pct(t[v], 50), 4), "p99_ms": round(pct(t[v], 99), 4), "key_skips_per_call": skips // n_calls}
    pa = res["unkeyed"]["p50_ms"]
    line = {
        "shape": {"captures": W, "channels": C, "decimation": R, "block_bytes": BLOCK, "key_block_log2": 17},
        "calls": a.calls, "warmup": a.warmup, "variants": res,
        "units_per_call": C * TILES,
        "unkeyed_spread_ms": round(res["unkeyed"]["p99_ms"] - pa, 4),
        "keyed_all_on_minus_unkeyed_ms": round(res["keyed_all_on"]["p50_ms"] - pa, 4),
        "keyed_all_on_over_unkeyed": round(res["keyed_all_on"]["p50_ms"] / pa, 4),
        "keyed_8_of_64_over_unkeyed": round(res["keyed_8_of_64_on"]["p50_ms"] / pa, 4),
        "keyed_all_off_over_unkeyed": round(res["keyed_all_off"]["p50_ms"] / pa, 4),
        "work_model_8_of_64": MODEL_C,
        "zero_bytes_per_call": {"keyed_8_of_64_on": C * 7 // 8 * BLOCK, "keyed_all_off": C * BLOCK},
        "receive_saving_ms_p50": round(res["receive_wbfm_unkeyed"]["p50_ms"] - res["receive_wbfm_keyed_8_of_64_on"]["p50_ms"], 4),
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
