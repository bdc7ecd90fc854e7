#!/usr/bin/env python3
"""Times the AFSK bank beside the tone call on the same PCM and the receive call whose PCM both read, and prints one JSON
line (also written to profiles/afsk_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16, what one wbfm_1024x16 receive call writes), data resident,
warm, Bell 202 packet data with noise on every channel.  hrfd_afsk_process_device with every output (bits, n_bits, hard),
with bits alone, and with only hard: the call without bits skips the serial stage (the bit clock, one wave per channel), so
the difference is its share.  Then W = 32, the longest window (four times the dot products), and the same bytes the other
way round, 16 channels x 1024 blocks: k_afsk walks a row with one workgroup and its bits with one wave, so this is the shape
that does not fill the device.  Each as host clock around the call + stream synchronise, p50 / p99 over --calls calls after
--warmup, and as device time between two events around --burst back-to-back calls (the launch overhead and the host's wait
drop out).  The tone call (8 DTMF tones, L = 256, every output) and the receive call of the same batch
(hrfd_rx_process_device, 1024 WBFM channels x 16 blocks of 262144 bytes) are timed in the same run under the same clocks: the
AFSK call is judged against those, never against an earlier figure of its own.

    python tools/afsk_time.py [--calls 200] [--warmup 20] [--burst 20] [--no-rx] [--out profiles/afsk_time.json]
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


def packet_pcm(rng):
    """Bell 202 with random data on every channel, continuous phase, a level and a bit timing of its own, noise: [C, n]"""
    n = BLOCKS * 512
    spb = 8000.0 / 1200.0
    t = np.arange(n)[None, :] + rng.random((C, 1)) * spb
    bits = rng.integers(0, 2, size=(C, int(n / spb) + 2))
    f = np.where(np.take_along_axis(bits, (t / spb).astype(np.int64), axis=1) != 0, 1200.0, 2200.0)
    phase = 2.0 * np.pi * np.cumsum(f, axis=1) / 8000.0
    amp = 30000.0 * 10.0 ** (-rng.uniform(0.0, 30.0, size=(C, 1)) / 20.0)
    x = amp * np.cos(phase) + rng.normal(0.0, 200.0, size=(C, n))
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--no-rx", action="store_true", help="leave the receive call out (it needs 4 GiB of device memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "afsk_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/afsk_time.py needs a GPU")
    dev = torch.device("cuda:0")
    x = packet_pcm(np.random.default_rng(1))
    pcm = torch.from_numpy(x.reshape(C, BLOCKS, 512)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}

    bank = api.Afsk(C, device=0)
    cap = bank.max_bits(BLOCKS)
    bits = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
    count = torch.zeros(C, dtype=torch.int32, device=dev)
    hard = torch.zeros((C, BLOCKS, 64), dtype=torch.uint8, device=dev)
    line["afsk_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, bits.data_ptr(), cap, count.data_ptr(), hard.data_ptr(), sp), a)
    line["afsk_bits_per_channel"] = {"mean": round(float(count.float().mean().item()), 1), "max_bits": cap}
    line["afsk_bits_only_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, bits.data_ptr(), cap, count.data_ptr(), None, sp), a)
    line["afsk_hard_only_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, None, 0, None, hard.data_ptr(), sp), a)
    bank.set_modem(window=32)
    line["afsk_W32_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, bits.data_ptr(), cap, count.data_ptr(), hard.data_ptr(), sp), a)
    bank.close()
    # the same bytes as 16 rows of 1024 blocks: one workgroup per row, one wave for its bits
    few = api.Afsk(BLOCKS, device=0)
    cap_few = few.max_bits(C)
    bits_few = torch.zeros((BLOCKS, cap_few), dtype=torch.uint8, device=dev)
    line["afsk_16x1024_ms"] = both_clocks(torch, stream, lambda: few.process_device(
        pcm.data_ptr(), 1024 * C, None, C, bits_few.data_ptr(), cap_few, count.data_ptr(), hard.data_ptr(), sp), a)
    line["afsk_16x1024_hard_only_ms"] = both_clocks(torch, stream, lambda: few.process_device(
        pcm.data_ptr(), 1024 * C, None, C, None, 0, None, hard.data_ptr(), sp), a)
    few.close()

    L = 256
    tones = api.Tones(C, L, device=0)
    tones.set_tones(list(api.DTMF_LOW_HZ) + list(api.DTMF_HIGH_HZ), [0] * 4 + [1] * 4)
    F = BLOCKS * 512 // L
    power = torch.zeros((C, F, 8), dtype=torch.int64, device=dev)
    energy = torch.zeros((C, F), dtype=torch.int64, device=dev)
    valid = torch.zeros((C, F), dtype=torch.int32, device=dev)
    best = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
    present = torch.zeros((C, F, 4), dtype=torch.uint8, device=dev)
    line["tone_K8_L256_ms"] = both_clocks(torch, stream, lambda: tones.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, power.data_ptr(), energy.data_ptr(), valid.data_ptr(),
        best.data_ptr(), present.data_ptr(), sp), a)
    tones.close()

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
