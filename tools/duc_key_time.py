#!/usr/bin/env python3
"""Times the DUC bank's transmit key at tools/duc_time.py's shape and prints one JSON line.

16 captures x 64 channels = 1024 channels, R = 8, default filters, one 64 ms block per call (131 072 channel samples, one key
byte per channel at the default key block 2^17).  Six variants, one call of each in turn within one run, so that whatever
else the machine does meets all of them alike:
  a  hrfd_duc_process_device, unkeyed
  b  keyed, every channel on                 (the price of the key when everything talks)
  c  keyed, 8 of every capture's 64 channels on
  d  keyed, every channel off
  e  hrfd_duc_transmit in WBFM, unkeyed
  f  hrfd_duc_transmit in WBFM, keyed as in c
Host clock around the call and the stream's synchronise; p50 / p99 over --calls calls after --warmup, and key_skips per
call.  Every variant has its own handle, so the meter is its own.  The work model of c: a channel that talks costs a unit
per tile, one that does not costs the call's first tile only: 1/8 + (7/8)/128 = 0.132 of a, plus what does not shrink (the
launch, the tables, the stores of 32 MiB of captures).

    python tools/duc_key_time.py [--calls 200] [--warmup 20] [--out profiles/duc_key_time.json]
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
MODEL_C = 1 / 8 + (7 / 8) / TILES


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duc_key_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/duc_key_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    offsets = [float(rng.uniform(-7.5e6, 7.5e6)) for _ in range(C)]

    def bank():
        d = api.Duc(W, C, R, device=0)
        for c in range(C):
            d.tune(c, c % W, offsets[c])
        d.set_output_shift(14)                             # 64 channels per capture
        return d

    chans = torch.from_numpy(rng.integers(-128, 128, size=(C, BLOCK), dtype=np.int8)).to(dev)
    pcm = torch.from_numpy(rng.integers(-20000, 20000, size=(C, 512), dtype=np.int16)).to(dev)
    caps = torch.zeros((W, R * BLOCK), dtype=torch.int8, device=dev)
    all_on = torch.ones((C, 1), dtype=torch.uint8, device=dev)
    all_off = torch.zeros((C, 1), dtype=torch.uint8, device=dev)
    # channel c sits on capture c % 16 as its (c // 16)-th: every eighth of them talks
    some = torch.from_numpy((np.arange(C) // W % 8 == 0).astype(np.uint8).reshape(C, 1)).to(dev)
    assert int(some.sum()) == C // 8
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    mods = {v: api.Mod(api.MOD_WBFM, C, device=0) for v in "ef"}
    ducs = {v: bank() for v in "abcdef"}
    keys = {"a": None, "b": all_on, "c": some, "d": all_off, "e": None, "f": some}
    torch.cuda.synchronize()

    def call(v):
        k = keys[v]
        kp = None if k is None else k.data_ptr()
        if v in "ef":
            ducs[v].transmit(mods[v], pcm.data_ptr(), 512, caps.data_ptr(), R * BLOCK, sp, d_key=kp, key_stride=1)
        else:
            ducs[v].process_device(chans.data_ptr(), BLOCK, BLOCK, caps.data_ptr(), R * BLOCK, sp, d_key=kp, key_stride=1)

    t = {v: [] for v in "abcdef"}
    for i in range(a.warmup + a.calls):
        for v in "abcdef":
            t0 = time.perf_counter()
            call(v)
            stream.synchronize()
            if i >= a.warmup:
                t[v].append((time.perf_counter() - t0) * 1e3)

    n_calls = a.warmup + a.calls
    names = {"a": "unkeyed", "b": "keyed_all_on", "c": "keyed_8_of_64_on", "d": "keyed_all_off", "e": "transmit_wbfm_unkeyed",
             "f": "transmit_wbfm_keyed_8_of_64_on"}
    res = {}
    for v in "abcdef":
        skips = ducs[v].key_skips()
        assert skips % n_calls == 0
        res[names[v]] = {"p50_ms": round(pct(t[v], 50), 4), "p99_ms": round(pct(t[v], 99), 4), "key_skips_per_call": skips // n_calls}
    pa = res["unkeyed"]["p50_ms"]
    line = {
        "shape": {"captures": W, "channels": C, "interpolation": R, "block_bytes": BLOCK, "key_block_log2": 17},
        "calls": a.calls, "warmup": a.warmup, "variants": res,
        "units_per_call": C * TILES,
        "keyed_all_on_over_unkeyed": round(res["keyed_all_on"]["p50_ms"] / pa, 4),
        "keyed_8_of_64_over_unkeyed": round(res["keyed_8_of_64_on"]["p50_ms"] / pa, 4),
        "keyed_all_off_over_unkeyed": round(res["keyed_all_off"]["p50_ms"] / pa, 4),
        "work_model_8_of_64": round(MODEL_C, 4),
        "transmit_saving_ms_p50": round(res["transmit_wbfm_unkeyed"]["p50_ms"] - res["transmit_wbfm_keyed_8_of_64_on"]["p50_ms"], 4),
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
