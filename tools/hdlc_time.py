#!/usr/bin/env python3
"""Times the HDLC bank beside the AFSK call of the same batch, and prints one JSON line (also written to
profiles/hdlc_time.json).

1 258 496 bits of packet data (HDLC frames of 20..120 bytes with flags between them, and stretches of noise), a byte a bit,
data resident, warm, laid out the two ways the AFSK bank writes a 1.024 s batch: 1024 channels x 1229 bits (16 blocks of
Bell 202 a channel, rows hrfd_afsk_max_bits = 2253 bytes apart) and the same bytes as 16 channels x 78 656 bits (1024 blocks,
rows hrfd_afsk_max_bits of 1024 blocks apart).  hrfd_hdlc_process_device with every output, rows of hrfd_hdlc_max_out.  Each as host clock
around the call + stream synchronise, p50 / p99 over --calls calls after --warmup, and as device time between two events
around --burst back-to-back calls (the launch overhead and the host's wait drop out).  The frames the timed call returns
are checked against api.hdlc_frames on a few channels first.  The AFSK call of the same two shapes
(hrfd_afsk_process_device, bits alone, Bell 202 with random data and noise on every channel) is timed in the same run under
the same clocks: the HDLC call is judged against those, never against an earlier figure of its own.

    python tools/hdlc_time.py [--calls 200] [--warmup 20] [--burst 20] [--out profiles/hdlc_time.json]
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
BITS = 1229                                    # of 16 blocks of Bell 202: 8192 samples x 1200 / 8000


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


def packet_bits(rng, n):
    """n bits of frames and noise, one byte a bit with the carrier flag"""
    parts, have = [], 0
    while have < n:
        payloads = [rng.integers(0, 256, size=int(rng.integers(20, 121)), dtype=np.uint8).tobytes() for _ in range(8)]
        parts.append(api.hdlc_encode(payloads, n_lead_flags=2, n_between=int(rng.integers(1, 4)), n_tail_flags=1))
        parts.append(rng.integers(0, 2, size=int(rng.integers(0, 400)), dtype=np.uint8))
        have += len(parts[-1]) + len(parts[-2])
    return (np.concatenate(parts)[:n] | 2).astype(np.uint8)


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


def hdlc_shape(torch, dev, stream, a, bits, n_ch, n_bits, stride):
    """the bank over n_ch rows of n_bits bits `stride` bytes apart: the timing, and the frames of one call checked"""
    rows = np.zeros((n_ch, stride), dtype=np.uint8)
    rows[:, :n_bits] = bits.reshape(n_ch, n_bits)
    d_bits = torch.from_numpy(rows).to(dev)
    d_n = torch.full((n_ch,), n_bits, dtype=torch.int32, device=dev)
    bank = api.Hdlc(n_ch, device=0)
    ob = bank.max_out(n_bits)
    d_out = torch.zeros((n_ch, ob), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((3, n_ch), dtype=torch.int32, device=dev)
    sp = stream.cuda_stream
    call = lambda: bank.process_device(d_bits.data_ptr(), stride, d_n.data_ptr(), n_bits, d_out.data_ptr(), ob, ob, d_cnt[0].data_ptr(),
                                       d_cnt[1].data_ptr(), d_cnt[2].data_ptr(), sp)
    call()
    stream.synchronize()
    cnt, out = d_cnt.cpu().numpy(), d_out.cpu().numpy()
    for c in (0, n_ch // 2, n_ch - 1):
        got = [p for _, p, _ in api.Hdlc.parse(out[c], cnt[0][c])]
        want = [p for p in api.hdlc_frames(rows[c, :n_bits]) if len(p) <= 512]
        if got != want or cnt[2][c] != 0:
            raise SystemExit(f"tools/hdlc_time.py: channel {c} of {n_ch} gave {len(got)} frames, the host's walk {len(want)}")
    r = both_clocks(torch, stream, call, a)
    # (every call but the first starts inside the partial frame the one before left: the same work)
    r["frames_per_call"] = int(cnt[0].sum())
    r["bad_per_call"] = int(cnt[1].sum())
    r["out_row_bytes"] = ob
    bank.close()
    return r


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdlc_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/hdlc_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "bits_per_channel": BITS, "bits": C * BITS}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}

    # the AFSK calls whose output this bank reads, in both shapes
    pcm = torch.from_numpy(packet_pcm(rng).reshape(C, BLOCKS, 512)).to(dev)
    afsk = api.Afsk(C, device=0)
    cap = afsk.max_bits(BLOCKS)
    abits = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
    count = torch.zeros(C, dtype=torch.int32, device=dev)
    line["afsk_1024x16_ms"] = both_clocks(torch, stream, lambda: afsk.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, None, BLOCKS, abits.data_ptr(), cap, count.data_ptr(), None, sp), a)
    afsk.close()
    few = api.Afsk(BLOCKS, device=0)
    cap_few = few.max_bits(C)
    abits_few = torch.zeros((BLOCKS, cap_few), dtype=torch.uint8, device=dev)
    line["afsk_16x1024_ms"] = both_clocks(torch, stream, lambda: few.process_device(
        pcm.data_ptr(), 1024 * C, None, C, abits_few.data_ptr(), cap_few, count.data_ptr(), None, sp), a)
    few.close()

    bits = packet_bits(rng, C * BITS)
    line["hdlc_1024x16_ms"] = hdlc_shape(torch, dev, stream, a, bits, C, BITS, cap)
    line["hdlc_16x1024_ms"] = hdlc_shape(torch, dev, stream, a, bits, BLOCKS, C * BITS // BLOCKS, cap_few)
    for shape in ("1024x16", "16x1024"):
        line[f"hdlc_over_afsk_{shape}"] = round(line[f"hdlc_{shape}_ms"]["device"] / line[f"afsk_{shape}_ms"]["device"], 4)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
