#!/usr/bin/env python3
"""Times the tone generator bank beside the level call and the audio call that move the same bytes, and prints one JSON line
(also written to profiles/tonegen_time.json).

1024 channels x 16 blocks of 512 PCM samples (16 MiB of int16, one transmit batch), data resident, warm.  Four cases of
hrfd_tonegen_process_device: every channel idle in place (nothing is read or written), every channel idle out of place (a
copy), a CTCSS sub-tone without an end on every channel, and the sub-tone plus eight DTMF digits (96 ms on, 32 ms off: the
whole call) on every channel, the last two out of place: they read and write the 32 MiB the level and audio calls do, and
the input stays what it was from call to call.  The clock is set back to 0 in front of
every call (a host store), so every call computes the same stretch of the stream.  Each case as host clock around the call +
stream synchronise, p50 / p99 over --calls calls after --warmup, and as device time between two events around --burst
back-to-back calls (the launch overhead and the host's wait drop out).  The level call (out, gain and peak) and the audio
call at T = 1 (the identity filter, one bus of 16 channels) over the same batch are timed in the same run under the same
clocks: the bank is judged against those, never against an earlier figure of its own.

    python tools/tonegen_time.py [--calls 200] [--warmup 20] [--burst 20] [--out profiles/tonegen_time.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tonegen_time.json"))
    a = ap.parse_args()
    import torch
    if api.device_count() < 1:
        raise SystemExit("tools/tonegen_time.py needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    x = np.round(rng.uniform(-1.0, 1.0, size=(C, BLOCKS * 512)) * 8000.0).astype(np.int16)
    pcm = torch.from_numpy(x.reshape(C, BLOCKS, 512)).to(dev)
    n_pcm = torch.full((C, BLOCKS), 512, dtype=torch.int32, device=dev)
    out = torch.zeros((C, BLOCKS, 512), dtype=torch.int16, device=dev)
    work = pcm.clone()
    active = torch.zeros((C, BLOCKS), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    line = {"shape": {"channels": C, "blocks": BLOCKS, "pcm_bytes": C * BLOCKS * 1024}, "calls": a.calls, "warmup": a.warmup,
            "burst": a.burst}

    gen = api.ToneGen(C, device=0)

    def call(src, dst):
        gen.set_time(0)
        gen.process_device(src.data_ptr(), 1024 * BLOCKS, BLOCKS, dst.data_ptr(), 0, active.data_ptr(), sp)

    line["tonegen_idle_in_place_ms"] = both_clocks(torch, stream, lambda: call(work, work), a)
    line["tonegen_idle_out_of_place_ms"] = both_clocks(torch, stream, lambda: call(pcm, out), a)
    gen.set_time(0)
    for c in range(C):
        gen.ctcss(c, api.CTCSS_HZ[c % len(api.CTCSS_HZ)], start=0)
    line["tonegen_ctcss_ms"] = both_clocks(torch, stream, lambda: call(pcm, out), a)
    line["tonegen_ctcss_active_blocks"] = int((active == 2).sum().item())
    gen.set_time(0)
    gen.dial(api.ALL, "12345678", start=0)
    line["tonegen_ctcss_dtmf_ms"] = both_clocks(torch, stream, lambda: call(pcm, out), a)
    line["tonegen_ctcss_dtmf_active_blocks"] = int((active == 3).sum().item())
    line["tonegen_clips_channel_0"] = gen.clips(0)
    gen.close()

    gain = torch.zeros((C, 8 * BLOCKS), dtype=torch.int32, device=dev)
    peak = torch.zeros((C, 8 * BLOCKS), dtype=torch.int16, device=dev)
    level = api.Leveler(C, device=0)
    line["level_ms"] = both_clocks(torch, stream, lambda: level.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), BLOCKS, out.data_ptr(), 0, gain.data_ptr(), peak.data_ptr(), sp), a)
    level.close()

    audio = api.Audio(C, 1, device=0)                      # T = 1: the identity filter
    audio.set_bus(0, [64 * j for j in range(16)], [api.AUDIO_UNITY_GAIN // 4] * 16)
    mix = torch.zeros((1, BLOCKS, 512), dtype=torch.int16, device=dev)
    clips = torch.zeros(1, dtype=torch.int32, device=dev)
    line["audio_T1_M1_ms"] = both_clocks(torch, stream, lambda: audio.process_device(
        pcm.data_ptr(), 1024 * BLOCKS, n_pcm.data_ptr(), None, BLOCKS, out.data_ptr(), 0, mix.data_ptr(), clips.data_ptr(), sp), a)
    audio.close()

    for name in ("tonegen_idle_in_place_ms", "tonegen_idle_out_of_place_ms", "tonegen_ctcss_ms", "tonegen_ctcss_dtmf_ms"):
        line[name]["device_over_level"] = round(line[name]["device"] / line["level_ms"]["device"], 3)
        line[name]["device_over_audio"] = round(line[name]["device"] / line["audio_T1_M1_ms"]["device"], 3)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
