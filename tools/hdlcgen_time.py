#!/usr/bin/env python3
"""Times the HDLC framer bank beside the HDLC bank over the bits it produced and beside the two host framers, and prints one
JSON line (also written to profiles/hdlcgen_time.json).

1024 channels x one frame of 128 random bytes each, the default flag counts (12 in front, 3 behind), records resident,
warm: hrfd_hdlcgen_process_device with every count, rows of hrfd_hdlcgen_max_bits.  As host clock around the call + stream
synchronise, p50 / p99 over --calls calls after --warmup, and as device time between two events around --burst
back-to-back calls (the launch overhead and the host's wait drop out).  The bits of the timed call are checked against
api.hdlc_encode on a few channels first.  In the same run, under the same clocks: hrfd_hdlc_process_device (a fresh
handle's) over exactly those rows of bits and counts, which must give the payloads back; and on the host, over the same
batch, all 1024 channels on one thread, api.hdlc_encode (the per-bit loop in Python) and hrfd_hdlc_encode (the per-bit loop
in C).  A second device shape frames eight frames of 128 bytes a channel, where
the kernel's loop over a row's frames shows.  The framer is judged against the HDLC call of this run, never against an
earlier figure.

    python tools/hdlcgen_time.py [--calls 200] [--warmup 20] [--burst 20] [--out profiles/hdlcgen_time.json]
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

C, PAYLOAD = 1024, 128


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


def device_shape(torch, dev, stream, a, per):
    """the framer over `per` (per channel a list of payloads), then the HDLC bank over its bits: both timings"""
    n_ch = len(per)
    gen = api.HdlcGen(n_ch, device=0)
    rows, n_frames = gen.pack(per)
    max_bits = max(gen.max_bits(len(p), sum(map(len, p))) for p in per)
    d_rows = torch.from_numpy(rows).to(dev)
    d_nf = torch.from_numpy(n_frames.view(np.int32)).to(dev)
    d_bits = torch.zeros((n_ch, max_bits), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((6, n_ch), dtype=torch.int32, device=dev)
    sp = stream.cuda_stream
    framer = lambda: gen.process_device(d_rows.data_ptr(), rows.shape[1], rows.shape[1], d_nf.data_ptr(), d_bits.data_ptr(), max_bits,
                                        max_bits, d_cnt[0].data_ptr(), d_cnt[1].data_ptr(), d_cnt[2].data_ptr(), sp)
    framer()
    stream.synchronize()
    cnt, bits = d_cnt.cpu().numpy(), d_bits.cpu().numpy()
    for c in (0, n_ch // 2, n_ch - 1):
        want = api.hdlc_encode(per[c])
        if cnt[0][c] != want.size or not np.array_equal(bits[c, :want.size], want) or cnt[2][c] != 0:
            raise SystemExit(f"tools/hdlcgen_time.py: channel {c} of {n_ch} does not give api.hdlc_encode's bits")
    r = {"framer_ms": both_clocks(torch, stream, framer, a)}
    r["bits_per_call"] = int(cnt[0].sum())
    r["bits_row_bytes"] = max_bits

    bank = api.Hdlc(n_ch, 1, 512, device=0)
    ob = bank.max_out(max_bits)
    d_out = torch.zeros((n_ch, ob), dtype=torch.uint8, device=dev)
    deframer = lambda: bank.process_device(d_bits.data_ptr(), max_bits, d_cnt[0].data_ptr(), max_bits, d_out.data_ptr(), ob, ob,
                                           d_cnt[3].data_ptr(), d_cnt[4].data_ptr(), d_cnt[5].data_ptr(), sp)
    deframer()
    stream.synchronize()
    cnt, out = d_cnt.cpu().numpy(), d_out.cpu().numpy()
    for c in (0, n_ch // 2, n_ch - 1):
        if [p for _, p, _ in api.Hdlc.parse(out[c], cnt[3][c])] != per[c]:
            raise SystemExit(f"tools/hdlcgen_time.py: channel {c} of {n_ch}: the HDLC bank does not give the payloads back")
    r["hdlc_ms"] = both_clocks(torch, stream, deframer, a)
    r["framer_over_hdlc"] = round(r["framer_ms"]["device"] / r["hdlc_ms"]["device"], 4)
    gen.close()
    bank.close()
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdlcgen_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/hdlcgen_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    one = [[rng.integers(0, 256, size=PAYLOAD, dtype=np.uint8).tobytes()] for _ in range(C)]
    eight = [[rng.integers(0, 256, size=PAYLOAD, dtype=np.uint8).tobytes() for _ in range(8)] for _ in range(C)]
    line = {"shape": {"channels": C, "payload_bytes": PAYLOAD}, "calls": a.calls, "warmup": a.warmup, "burst": a.burst}
    line["device_1024x1"] = device_shape(torch, dev, stream, a, one)
    line["device_1024x8"] = device_shape(torch, dev, stream, a, eight)

    # the host's two framers over the first batch
    t0 = time.perf_counter()
    py = [api.hdlc_encode(p) for p in one]
    t_py = (time.perf_counter() - t0) * 1e3
    import ctypes
    lib = api._lib.load()
    rows = np.stack([api.hdlc_records(p) for p in one])
    room = api.hdlcgen_max_bits(1, PAYLOAD)
    out = np.zeros((C, room), dtype=np.uint8)
    n_bits = (ctypes.c_uint32 * C)()
    args = [(ctypes.c_void_p(rows[c].ctypes.data), ctypes.c_void_p(out[c].ctypes.data), ctypes.byref(n_bits, 4 * c)) for c in range(C)]
    t0 = time.perf_counter()
    for rec, bits, n in args:                              # the C loop itself: the rows are packed, the pointers made
        lib.hrfd_hdlc_encode(rec, rows.shape[1], 1, 12, 2, 3, bits, room, n, None, None)
    t_c = (time.perf_counter() - t0) * 1e3
    cc = [out[c, :n_bits[c]] for c in range(C)]
    if any(not np.array_equal(x, y) for x, y in zip(py, cc)):
        raise SystemExit("tools/hdlcgen_time.py: hrfd_hdlc_encode and api.hdlc_encode differ")
    line["host_ms"] = {"python_hdlc_encode": round(t_py, 2), "c_hrfd_hdlc_encode": round(t_c, 3)}
    dev_ms = line["device_1024x1"]["framer_ms"]
    line["python_over_device_call"] = round(t_py / dev_ms["p50"], 1)
    line["c_over_device_call"] = round(t_c / dev_ms["p50"], 1)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
