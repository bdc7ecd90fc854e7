#!/usr/bin/env python3
"""Times the AFSK generator bank beside the tone generator's call on the same bytes, the AFSK bank's decode call of the same
batch and the receive call, and prints one JSON line (also written to profiles/afskgen_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16), data resident, warm.  hrfd_afskgen_process_device in place
with every channel idle (no message: the rows are neither read nor written), with one Bell 202 message spanning the call on
every channel (8192 random bits, 54614 samples: the next is queued on every channel, outside the clock, whenever fewer than
two are pending, so the first call behind a queue also carries the upload of 1 MiB of levels: that shows in p99, not in p50),
and the same with the active bytes.  Each as host clock around the call + stream synchronise, p50 / p99 over --calls calls
after --warmup, and as device time between two events around --burst back-to-back calls (four messages are queued in front:
no upload inside the burst).  In the same run under the same clocks: the tone generator's call with one CTCSS tone per channel
in place on the same bytes, the AFSK bank's decode call (every output) of the batch the generator wrote, and the receive call
(hrfd_rx_process_device, 1024 WBFM channels x 16 blocks of 262144 bytes).  The generator is judged against those, never
against an earlier figure of its own.

    python tools/afskgen_time.py [--calls 200] [--warmup 20] [--burst 20] [--no-rx] [--out profiles/afskgen_time.json]
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


def pct(v, q):
    return float(np.percentile(np.asarray(v), q))


def timed(fn, sync, calls, warmup, before=None):
    t = []
    for i in range(warmup + calls):
        if before is not None:
            before()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return {"p50": round(pct(t, 50), 4), "p99": round(pct(t, 99), 4)}


def both_clocks(torch, stream, call, a, before=None, before_burst=None):
    """{"p50", "p99", "device"}: the host clock around call + synchronise, the device time per call of a burst"""
    torch.cuda.synchronize()
    r = timed(call, stream.synchronize, a.calls, a.warmup, before)
    if before_burst is not None:
        before_burst()
        call()                                                 # carries the upload
        stream.synchronize()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afskgen_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/afskgen_time.py needs a GPU")
    if a.burst * BLOCKS * 512 > 3 * 54614:
        raise SystemExit("--burst: four messages in front of the burst span at most 20 calls")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    pcm = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    active = torch.zeros((C, BLOCKS), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}

    gen = api.AfskGen(C, device=0)
    bits = rng.integers(0, 2, size=api.AFSKGEN_MAX_BITS, dtype=np.uint8)

    def call(d_active=None):
        # in place over rows that start as zeros: at amplitude 50 the sums of a whole run stay far from saturation
        gen.process_device(pcm.data_ptr(), 1024 * BLOCKS, BLOCKS, pcm.data_ptr(), 0, d_active, sp)

    def refill():
        while gen.pending(0)[0] < 2:
            gen.queue(api.ALL, bits, amplitude=50)

    def fill():
        gen.reset()
        for _ in range(api.AFSKGEN_MAX_MESSAGES):
            gen.queue(api.ALL, bits, amplitude=50)

    line["afskgen_idle_in_place_ms"] = both_clocks(torch, stream, call, a)
    line["afskgen_in_place_ms"] = both_clocks(torch, stream, call, a, refill, fill)
    line["afskgen_in_place_active_ms"] = both_clocks(torch, stream, lambda: call(active.data_ptr()), a, refill, fill)
    line["afskgen_active_blocks"] = int(active.sum().item())
    line["afskgen_clips"] = gen.clips(0)
    # one call at the amplitude a user sends, generate only, for the decoder below
    gen.reset()
    gen.queue(api.ALL, bits, amplitude=8000)
    batch = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    gen.process_device(None, 0, BLOCKS, batch.data_ptr(), 0, None, sp)
    stream.synchronize()
    gen.close()

    tg = api.ToneGen(C, device=0)
    tg.ctcss(api.ALL, 100.0, amplitude=50)
    line["tonegen_ctcss_in_place_ms"] = both_clocks(torch, stream, lambda: tg.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, BLOCKS, pcm.data_ptr(), 0, None, sp), a)
    tg.close()

    dec = api.Afsk(C, device=0)
    cap = dec.max_bits(BLOCKS)
    out_bits = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
    count = torch.zeros(C, dtype=torch.int32, device=dev)
    hard = torch.zeros((C, BLOCKS, 64), dtype=torch.uint8, device=dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    line["afsk_decode_ms"] = both_clocks(torch, stream, lambda: dec.process_device(
        batch.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, out_bits.data_ptr(), cap, count.data_ptr(), hard.data_ptr(), sp), a)
    line["afsk_bits_per_channel"] = {"mean": round(float(count.float().mean().item()), 1), "max_bits": cap}
    dec.close()
    line["afskgen_to_afsk_decode_device"] = round(line["afskgen_in_place_ms"]["device"] / line["afsk_decode_ms"]["device"], 3)
    line["afskgen_to_tonegen_device"] = round(line["afskgen_in_place_ms"]["device"] / line["tonegen_ctcss_in_place_ms"]["device"], 3)

    if not a.no_rx:
        block = 262144
        rx = api.Rx(C, device=0)
        rx.set_mode(api.WBFM)
        iq = torch.randint(-40, 41, (C, BLOCKS * block), dtype=torch.int8, device=dev)      # 4 GiB: made where it is used
        out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
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
