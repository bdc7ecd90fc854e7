#!/usr/bin/env python3
"""Times the level bank beside the audio call that moves the same bytes and the receive call whose PCM both read, and prints
one JSON line (also written to profiles/level_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16, what one wbfm_1024x16 receive call writes), data resident,
warm, the channels' loudness spread over 40 dB.  hrfd_level_process_device with all three outputs (out, gain, peak), out of
place and in place, and as a meter (gain and peak alone); then the same handle shape the other way round, 16 channels x 1024
blocks (the same 16 MiB): k_level walks a row with one workgroup, so this is the shape that does not fill the device.  Each
as host clock around the call + stream synchronise, p50 / p99 over --calls calls after --warmup, and as device time between
two events around --burst back-to-back calls (the launch overhead and the host's wait drop out).  The audio call at T = 1
(the identity filter, one bus of 16 channels: it reads and writes the same 32 MiB) and the receive call of the same batch
(hrfd_rx_process_device, 1024 WBFM channels x 16 blocks of 262144 bytes) are timed in the same run under the same clocks:
the level call is judged against those, never against an earlier figure of its own.

    python tools/level_time.py [--calls 200] [--warmup 20] [--burst 20] [--no-rx] [--out profiles/level_time.json]
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


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--burst", type=int, default=20)
    ap.add_argument("--no-rx", action="store_true", help="leave the receive call out (it needs 4 GiB of device memory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "level_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/level_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    amp = 30000.0 * 10.0 ** (-rng.uniform(0.0, 40.0, size=(C, 1)) / 20.0)
    x = np.round(rng.uniform(-1.0, 1.0, size=(C, BLOCKS * 512)) * amp).astype(np.int16)
    pcm = torch.from_numpy(x.reshape(C, BLOCKS, 512)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}

    out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    gain = torch.zeros((C, 8 * BLOCKS), dtype=torch.int32, device=dev)
    peak = torch.zeros((C, 8 * BLOCKS), dtype=torch.int16, device=dev)
    bank = api.Leveler(C, device=0)
    line["level_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, out.data_ptr(), 0, gain.data_ptr(), peak.data_ptr(), sp), a)
    line["level_out_peak"] = int(out.abs().max().item())
    line["level_meter_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, None, 0, gain.data_ptr(), peak.data_ptr(), sp), a)
    work = pcm.clone()                                     # levelled again and again: the timing does not mind, the input must
    line["level_in_place_ms"] = both_clocks(torch, stream, lambda: bank.process_device(
        work.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, work.data_ptr(), 0, gain.data_ptr(), peak.data_ptr(), sp), a)
    bank.close()
    # the same bytes as 16 rows of 1024 blocks: one workgroup per row
    few = api.Leveler(BLOCKS, device=0)
    line["level_16x1024_ms"] = both_clocks(torch, stream, lambda: few.process_device(
        pcm.data_ptr(), 1024 * C, None, C, out.data_ptr(), 0, gain.data_ptr(), peak.data_ptr(), sp), a)
    few.close()

    audio = api.Audio(C, 1, device=0)                      # T = 1: the identity filter
    audio.set_bus(0, [64 * j for j in range(16)], [api.AUDIO_UNITY_GAIN // 4] * 16)
    mix = torch.zeros((1, BLOCKS, 512), dtype=torch.int16, device=dev)
    clips = torch.zeros(1, dtype=torch.int32, device=dev)
    line["audio_T1_M1_ms"] = both_clocks(torch, stream, lambda: audio.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), None, BLOCKS, out.data_ptr(), 0, mix.data_ptr(), clips.data_ptr(), sp), a)
    audio.close()

    if not a.no_rx:
        block = 262144
        rx = api.Rx(C, device=0)
        rx.set_mode(api.WBFM)
        iq = torch.randint(-40, 41, (C, BLOCKS * block), dtype=torch.int8, device=dev)      # 4 GiB: made where it is used
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
