"""The tone generator bank on the device (hrfd_tonegen_*) against the numpy model (tests/tonegen_model.py), bit for bit: channel
and block counts on both sides of the kernel's tile, segments that start and end on every edge, 32 hits in one tile, both
tracks at once, a stream cut into calls with a queue and a cut between, the clock across and beyond 2^32, saturation with its
count, generate-only, out of place and in place at every even residue with padded strides and guard bytes around every buffer,
setters behind running calls, and what the bank exists for: its audio decoded by Tones on the device, and the closed loop
ToneGen -> Mod -> Duc.transmit -> Ddc.receive -> Tones.  No comparison has a tolerance."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import tone_model as tm
from tests import tonegen_model as gm
from tests.test_gpu_tone import Guarded
from tests.test_tonegen_model import ctcss_decoder, dtmf_check, dtmf_decoder, dtmf_queue

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
FOREVER = gm.FOREVER


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C):
    return api.ToneGen(C, device=0), gm.ToneGenModel(C)


def seg(length, step_a=0, amp_a=0, step_b=0, amp_b=0, gap=0):
    return (gap, length, step_a, step_b, amp_a, amp_b)


def steps(n, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 1 << 32, size=n, dtype=np.uint64)]


_reference = {}


def reference(C, n, seed=7):
    """random int16 over the full range, one array per shape, computed once and left unchanged"""
    key = (C, n, seed)
    if key not in _reference:
        x = np.random.default_rng(seed).integers(-32768, 32768, size=(C, n), dtype=np.int16)
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def scatter(hs, C, n, seed, base=0):
    """the same random queues on every handle of hs: every third channel idle, the others with a run of segments around the
    call's n samples on track 0 and, on every other one, a tone without an end or a long one on track 1"""
    rng = np.random.default_rng(seed)
    st = steps(16, seed + 1)
    for c in range(C):
        if c % 3 == 2:
            continue
        k = int(rng.integers(1, 9))
        run = [seg(int(rng.choice([1, 63, 64, 65, 300, 1000, 2500])), st[int(rng.integers(16))], int(rng.integers(0, 32768)),
                   st[int(rng.integers(16))], int(rng.integers(0, 32768)), gap=int(rng.choice([0, 0, 1, 200, 700]))) for _ in range(k)]
        start = base + int(rng.integers(0, max(n // 2, 2)))
        for h in hs:
            h.queue(c, 0, run, start)
        if c % 2 == 0:
            s = seg(FOREVER if c % 4 == 0 else n, st[c % 16], 20000, st[(c + 5) % 16], 12000)
            for h in hs:
                h.queue(c, 1, [s], base + int(c * 37 % max(n, 1)))


def same_state(d, m, what):
    assert d.time() == m.time(), what
    for c in range(m.C):
        assert d.clips(c) == m.clips(c), f"{what}: clips of channel {c}: {d.clips(c)} against {m.clips(c)}"
        for t in range(2):
            assert d.pending(c, t) == m.pending(c, t), f"{what}: pending({c}, {t})"


def run_device(torch_dev, d, m, pcm, n_blocks, what, mode="out", residue=0, pad=0, out_pad=0, want_active=True, stream=None):
    """process_device in one of three modes: "gen" (no input), "out" (input rows at `residue` modulo 16, 1024 n_blocks + pad
    bytes apart; out rows at 14 - residue, 1024 n_blocks + out_pad apart) or "in_place"; active at an odd address; every
    buffer between guards.  The model takes the same call; out, active, the guards, the input and the clips must be its"""
    torch, dev = torch_dev
    C, n = m.C, 512 * n_blocks
    stride = 2 * n + pad
    out_stride = stride if mode == "in_place" else 2 * n + out_pad
    src = None
    if mode != "gen":
        pcm = np.asarray(pcm).reshape(C, n)
        src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
        for c in range(C):
            src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
        src.put(0, pcm[0])
    want, want_act = m.process(None if mode == "gen" else pcm, n_blocks, want_active=True)
    out = src if mode == "in_place" else Guarded(torch_dev, out_stride * (C - 1) + 2 * n, 14 - residue, 16, 22)
    act = Guarded(torch_dev, C * n_blocks, 1, 2, 23)
    torch.cuda.synchronize()
    d.process_device(None if src is None else src.ptr, stride, n_blocks, out.ptr, out_stride, act.ptr if want_active else None, stream)
    torch.cuda.synchronize()
    rows = out.host[out.off:out.off + out.n].copy()           # the rows of out as they must lie between what was there before
    for c in range(C):
        rows[c * out_stride:c * out_stride + 2 * n] = want[c].reshape(-1).view(np.uint8)
    if mode == "out":
        src.check(None, what + ": the input")
    out.check(rows, f"{what}: out")
    act.check(want_act if want_active else None, f"{what}: active")
    same_state(d, m, what)
    return want, want_act


# 1. sizes: the tile is 4 blocks, and a row's workgroups stride over its tiles: 1 block (a quarter tile), 3, 4 and 5 (both sides
#    of one tile), 9 (a third tile begun); one channel, two, five, and 65
@pytest.mark.parametrize("C", [1, 2, 5, 65])
@pytest.mark.parametrize("n_blocks", [1, 3, 4, 5, 9])
def test_channel_and_block_counts(C, n_blocks):
    d, m = both(C)
    scatter((d, m), C, 512 * n_blocks, 100 * C + n_blocks)
    pcm = reference(C, 512 * n_blocks)
    got, act = d.process(pcm, want_active=True)
    want, want_act = m.process(pcm, want_active=True)
    assert got.dtype == want.dtype and got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:4].tolist()
    assert (act == want_act).all()
    got = d.process(None, n_blocks)                            # the second call: generate only, what is still queued
    assert (got == m.process(None, n_blocks)).all()
    same_state(d, m, f"C={C}, {n_blocks} blocks")


# 2. segment edges, on one call of 5 blocks: one channel per (start, length), a second track whose segment's last sample is
#    the same edge; 32 segments of 64 samples back to back in the first tile; both tracks on top of each other
EDGES = (0, 1, 511, 512, 2047, 2048, 2559)
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, FOREVER)


def test_segment_edges(torch_dev):
    n_blocks = 5
    pairs = [(s, n) for s in EDGES for n in LENGTHS]
    C = len(pairs) + 2
    d, m = both(C)
    st = steps(8, 31)
    for h in (d, m):
        for c, (s, n) in enumerate(pairs):
            h.queue(c, 0, [seg(n, st[c % 8], 30000, st[(c + 3) % 8], 30000)], s)
            first = max(0, s + 1 - (n if n != FOREVER else 100))
            h.queue(c, 1, [seg(s + 1 - first, st[(c + 1) % 8], 25000, st[(c + 6) % 8], 9000)], first)     # its last sample: s
        h.queue(C - 2, 0, [seg(64, st[i % 8], 1000 * i + 767, st[(i + 1) % 8], 32767 - 1000 * i) for i in range(32)], 0)
        h.queue(C - 1, 0, [seg(1700, st[0], 32767, st[1], 32767)], 300)
        h.queue(C - 1, 1, [seg(2200, st[2], 32767, st[3], 32767)], 100)
    assert d.pending(C - 2, 0) == (32, 2048)
    want, act = run_device(torch_dev, d, m, reference(C, 512 * n_blocks), n_blocks, "edges")
    assert act[C - 2].tolist() == [1, 1, 1, 1, 0] and act[C - 1].tolist() == [3, 3, 3, 3, 2]
    assert act[pairs.index((2559, 1))].tolist() == [0, 0, 0, 0, 3] and act[pairs.index((2048, 2))].tolist() == [0, 0, 0, 2, 3]
    # the same queues from a new pair, generate only: a segment of one sample at the peak of its ramp is v / 64
    d, m = both(1)
    for h in (d, m):
        h.queue(0, 0, [seg(1, 1 << 30, 32767), seg(2, 1 << 30, 32767, gap=9)], 5)
    want, act = run_device(torch_dev, d, m, None, 1, "the shortest segments", mode="gen")
    assert want[0, 0, 5] == 0 and want[0, 0, 16] == (32766 + 32) >> 6 and np.count_nonzero(want) == 1      # k = 0 is the zero crossing


# 3. a stream cut into calls
def test_call_cutting(torch_dev):
    C, cuts = 3, (1, 3, 5)
    n = 512 * sum(cuts)
    pcm = reference(C, n, 8).reshape(C, -1, 512)
    st = steps(6, 41)
    long = seg(4000, st[0], 20000, st[1], 15000)              # in progress across both cuts
    late = [seg(700, st[2], 9000, st[3], 32767, gap=30), seg(100, st[4], 32767, 0, 0)]       # queued between the calls
    parts, mp = both(C)
    for h in (parts, mp):
        h.queue(ALL, 0, [long], 100)
        h.queue(1, 1, [seg(FOREVER, st[5], 8000)], 7)
    got, at = [], 0
    for i, k in enumerate(cuts):
        out = parts.process(pcm[:, at:at + k])
        assert (out == mp.process(pcm[:, at:at + k])).all(), f"call {i}"
        got.append(out)
        at += k
        if i == 0:
            for h in (parts, mp):
                h.queue(0, 1, late)                            # appended at 512 + 30
                h.cut(1, 1)                                    # the endless tone ends at 512 + 64
                h.cut(2, 0)                                    # the long one as well, on channel 2
            assert parts.pending(1, 1) == mp.pending(1, 1) == (1, 576) and parts.pending(2, 0) == (1, 576)
    same_state(parts, mp, "cut into calls")
    # one call of 9 blocks over the queues the cut stream ended up with, through a second handle and its model
    whole, mw = both(C)
    for h in (whole, mw):
        h.queue(0, 0, [long], 100)
        h.queue(1, 0, [long], 100)
        h.queue(2, 0, [seg(576 - 100, st[0], 20000, st[1], 15000)], 100)
        h.queue(1, 1, [seg(576 - 7, st[5], 8000)], 7)
        h.queue(0, 1, late, 512)
    want, _ = run_device(torch_dev, whole, mw, pcm, sum(cuts), "one call")
    assert (np.concatenate(got, axis=1) == want).all()
    assert [whole.clips(c) for c in range(C)] == [parts.clips(c) for c in range(C)]


# 4. the clock: a segment across 2^32, and k at and above 2^32 under a tone queued at 0
def test_time_across_and_above_2_32(torch_dev):
    d, m = both(2)
    st = steps(4, 51)
    for h in (d, m):
        h.queue(1, 1, [seg(FOREVER, st[0], 30000, st[1], 2000)], 0)
        h.set_time((1 << 32) - 1024)
        h.queue(0, 0, [seg(1500, st[2], 25000, st[3], 7000)], (1 << 32) - 700)
    run_device(torch_dev, d, m, reference(2, 1024), 2, "up to 2^32")
    run_device(torch_dev, d, m, reference(2, 1024), 2, "from 2^32", mode="in_place")
    for h in (d, m):
        h.set_time((1 << 32) + 5)
    want, act = run_device(torch_dev, d, m, None, 5, "k above 2^32", mode="gen")
    # (the clock went back by 1019 samples: the segment of channel 0 has 795 samples left, and sounds them again)
    assert d.time() == (1 << 32) + 5 + 2560 and act.tolist() == [[1, 1, 0, 0, 0], [2] * 5]
    assert want[0].reshape(-1)[:795].any() and (want[0].reshape(-1)[795:] == 0).all()
    # moved back in front of the segment: it leaves the queue with the first call that starts behind its end, and no call
    # has; the output is a function of the stream time and the queue
    for h in (d, m):
        h.set_time((1 << 32) - 1024)
    again, _ = run_device(torch_dev, d, m, None, 2, "the clock moved back", mode="gen")
    assert (again[0].reshape(-1)[:324] == 0).all() and again[0].any() and np.abs(again[1]).max() > 20000
    third, _ = run_device(torch_dev, d, m, None, 4, "behind its end", mode="gen")
    assert d.pending(0, 0) == (0, (1 << 32) + 2048)


# 5. saturation: full-scale input under two tracks at full amplitude
def test_saturation_and_clips(torch_dev):
    d, m = both(3)
    st = steps(4, 61)
    for h in (d, m):
        h.queue(ALL, 0, [seg(1800, st[0], 32767, st[1], 32767)], 10)
        h.queue(ALL, 1, [seg(1500, st[2], 32767, st[3], 32767)], 400)
    x = np.zeros((3, 2048), dtype=np.int16)
    x[0], x[1] = 32767, -32768
    want, act = run_device(torch_dev, d, m, x, 4, "saturation", residue=6, pad=4)
    clips = [d.clips(c) for c in range(3)]
    assert clips == [m.clips(c) for c in range(3)] and min(clips) > 100
    assert want.max() == 32767 and want.min() == -32768 and act.tolist() == [[3, 3, 3, 3]] * 3
    for h in (d, m):
        h.reset()
    assert [d.clips(c) for c in range(3)] == [0, 0, 0] and d.time() == 0 and d.pending(0, 0) == (0, 0)
    run_device(torch_dev, d, m, x, 4, "behind reset", mode="in_place")
    assert [d.clips(c) for c in range(3)] == [0, 0, 0]


# 6. the three modes at every even residue, padded strides on both sides, with and without active; every third channel idle
@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_modes_addresses_and_strides(torch_dev, residue):
    C, n_blocks = 5, 5
    d, m = both(C)
    scatter((d, m), C, 3 * 512 * n_blocks, 70 + residue)
    pcm = reference(C, 512 * n_blocks, 9)
    for i, (pad, out_pad) in enumerate(((2, 6), (6, 16), (16, 2))):
        what = f"residue {residue} pads {pad} {out_pad}"
        mode = ("out", "in_place", "gen")[(residue // 2 + i) % 3]
        run_device(torch_dev, d, m, pcm, n_blocks, f"{what} {mode}", mode, residue, pad, out_pad, want_active=i != 1)
    # the two other modes over the same stretch of the stream
    for h in (d, m):
        h.set_time(0)
    run_device(torch_dev, d, m, pcm, n_blocks, f"residue {residue} in place", "in_place", residue, 0)
    run_device(torch_dev, d, m, pcm, n_blocks, f"residue {residue} out of place", "out", residue, 0, 0, want_active=False)


# 7. the queues of a call are those set before it, whatever still runs
def test_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    C, n_blocks = 64, 16
    d, m = both(C)
    scatter((d, m), C, 512 * n_blocks * 3, 81)
    pcm = reference(C, 512 * n_blocks, 10)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 7
    d_out = torch.zeros((calls, C, n_blocks, 512), dtype=torch.int16, device=dev)
    d_act = torch.zeros((calls, C, n_blocks), dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    st = steps(8, 82)
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        # four calls on one stream, then one on a second stream directly behind them, then the first stream again
        s = streams[1 if i == 4 else 0]
        d.process_device(d_pcm.data_ptr() if i % 3 != 2 else None, 1024 * n_blocks, n_blocks, d_out[i].data_ptr(), 0, d_act[i].data_ptr(),
                         s.cuda_stream)
        want.append(m.process(pcm if i % 3 != 2 else None, n_blocks, want_active=True))
        # behind the call that now runs
        for h in (d, m):
            if i in (0, 3):
                h.cut(ALL, i // 3)
            if i == 4:
                h.cut(ALL, 0)                                  # (nothing can follow the endless segment of call 1)
            if i in (1, 4):
                h.queue(ALL, 0, [seg(5000, st[i], 30000, st[i + 1], 30000, gap=100), seg(FOREVER, st[i + 2], 500)])
            if i == 2:
                h.cut(5, 0)
                h.queue(5, 0, [seg(77, st[0], 32767)], h.time() + 64)
            if i == 5:
                h.reset()
                h.queue(ALL, 1, [seg(3000, st[7], 32767, st[6], 32767)], 50)
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        out, act = d_out[i].cpu().numpy(), d_act[i].cpu().numpy()
        assert (out == want[i][0]).all(), f"call {i}: out differs at {np.argwhere(out != want[i][0])[:4].tolist()}"
        assert (act == want[i][1]).all(), f"call {i}: active"
    same_state(d, m, "behind seven calls")


# what needs a handle to be refused; a refused queue changes nothing
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    d, m = both(4)
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=dev)
    p = buf.data_ptr()
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_queue.*channel 4"):
        d.queue(4, 0, [seg(1)])
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_cut.*channel 4"):
        d.cut(4, 0)
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_pending.*channel 4"):
        d.pending(4, 0)
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_get_clips.*channel 4"):
        d.clips(4)
    for h in (d, m):
        h.queue(ALL, 0, [seg(100, 1 << 29, 5000), seg(50, 1 << 28, 5000, gap=10)], 1000)
        h.queue(0, 1, [seg(FOREVER, 1 << 27, 700)])
        h.queue(3, 1, [seg(1)] * 32, 600)
    for text, args in (("overlap on the track", (ALL, 0, [seg(5)], 1099)), ("overlap on the track", (2, 0, [seg(20)], 1095)),
                       ("behind the FOREVER segment at 0", (0, 1, [seg(5)], 4000)), ("appended behind a FOREVER", (0, 1, [seg(5)])),
                       ("33 segments", (3, 1, [seg(1)])), ("behind the FOREVER segment at 0", (ALL, 1, [seg(1)], 700)),
                       ("lies behind a FOREVER segment", (1, 1, [seg(FOREVER), seg(1)])), ("amp above 32767", (1, 1, [seg(1, 0, 32768)])),
                       ("length 0", (1, 1, [seg(0)])), ("2\\^63", (1, 1, [seg(0xFFFFFFFE)], (1 << 63) - 5))):
        with pytest.raises(api.HrfdError, match="hrfd_tonegen_queue.*" + text):
            d.queue(*args)
        with pytest.raises(ValueError):
            m.queue(*args)
    assert (d.process(None, 1) == m.process(None, 1)).all()
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_queue.*start 511 lies before the stream time 512"):
        d.queue(1, 1, [seg(5)], 511)
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_process_device.*overlaps"):      # behind the first input row, inside the fourth
        d.process_device(p, 1024, 1, p + 3 * 1024 + 1022, 1024)
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_process_device.*overlaps"):
        d.process_device(p, 1024, 1, p, 1026)
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_process_device.*NULL argument"):
        d.process_device(p, 1024, 1, None, 1024)
    for h in (d, m):
        h.set_time((1 << 63) - 512)
    with pytest.raises(api.HrfdError, match="hrfd_tonegen_process.*below 2\\^63"):
        d.process(None, 2)
    for h in (d, m):
        h.set_time(512)
    same_state(d, m, "behind the refusals")                    # every refused call left the queues and the clock alone
    x = reference(4, 1024)
    got, act = d.process(x, want_active=True)                  # the handle still works
    want, want_act = m.process(x, want_active=True)
    assert (got == want).all() and (act == want_act).all() and act[3].tolist() == [3, 1] and act[1].tolist() == [1, 1]


# 8. what the bank is for: its audio decoded by Tones, both on the device, no host copy between
def test_dtmf_and_ctcss_decode_on_the_device(torch_dev):
    torch, dev = torch_dev
    # every DTMF key at amplitude 1000, 96 ms on and 32 ms off
    gen, mg = both(1)
    for h in (gen, mg):
        dtmf_queue(h, 0, 1000)
    d_pcm = torch.zeros((1, 32, 512), dtype=torch.int16, device=dev)
    dec = api.Tones(1, 256, device=0)
    dec.set_tones(list(api.DTMF_LOW_HZ + api.DTMF_HIGH_HZ), [0] * 4 + [1] * 4)
    d_best = torch.zeros((1, 64, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((1, 64, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(None, 0, 32, d_pcm.data_ptr())
    torch.cuda.synchronize()
    dec.process_device(d_pcm.data_ptr(), 1024 * 32, None, 32, None, None, None, d_best.data_ptr(), d_present.data_ptr())
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy()
    assert (pcm == mg.process(None, 32)).all()
    md = tm.ToneModel(1, 256)
    dtmf_decoder(md)
    want = md.process(pcm)
    best, present = d_best.cpu().numpy(), d_present.cpu().numpy()
    assert (best == want[3]).all() and (present == want[4]).all()
    dtmf_check(best[0], present[0], "amp 1000 on the device")
    # every CTCSS tone at amplitude 300 on a channel of its own, decoded among all 50
    K = len(api.CTCSS_HZ)
    gen, mg = both(K)
    for h in (gen, mg):
        for c, f in enumerate(api.CTCSS_HZ):
            h.ctcss(c, f, amplitude=300)
    d_pcm = torch.zeros((K, 24, 512), dtype=torch.int16, device=dev)
    dec = api.Tones(K, 4096, device=0)
    dec.set_tones(list(api.CTCSS_HZ), [2] * K)
    d_best = torch.zeros((K, 3, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((K, 3, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(None, 0, 24, d_pcm.data_ptr())
    torch.cuda.synchronize()
    dec.process_device(d_pcm.data_ptr(), 1024 * 24, None, 24, None, None, None, d_best.data_ptr(), d_present.data_ptr())
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy()
    assert (pcm == mg.process(None, 24)).all()
    want = ctcss_decoder().process(pcm)
    best, present = d_best.cpu().numpy(), d_present.cpu().numpy()
    assert (best == want[3]).all() and (present == want[4]).all()
    assert (best[:, :, 2] == np.arange(K)[:, None]).all() and (present[:, :, 2] == 1).all()


# 9. the closed loop on the device
def test_closed_loop_generate_transmit_receive_decode(torch_dev, oracle):
    """tests/test_tonegen_model.py's closed loop on the device: two WBFM stations whose audio ToneGen writes on the device, a
    DTMF digit per 64 ms block and a 1000 Hz tone under the first, through Mod, Duc.transmit, Ddc.receive and
    Tones.process_device, no host copy between.  (a) the generated audio and the received PCM equal what the models and the
    oracle give, (b) the tone bank's outputs equal its model's on that PCM, (c) every frame that lies wholly inside a digit
    decodes the row, the column and the pilot's presence."""
    from tests import ddc_model as dm
    torch, dev = torch_dev
    audio, amps, duc_clips, ref_pcm, gen_clips = gm.loop_reference(oracle)
    R, B, FULL = dm.SEL_R, dm.SEL_BLOCKS, 262144
    gen = api.ToneGen(2, device=0)
    gm.loop_queue(gen)
    mod = api.Mod(api.MOD_WBFM, 2, device=0)
    duc = api.Duc(1, 2, R, device=0)
    ddc = api.Ddc(1, 2, R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.WBFM)
    for c, f in enumerate(dm.SEL_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(amps[c], c)
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(dm.SEL_GAIN_SHIFT[c], c)
    tones = api.Tones(2, tm.LOOP_L, device=0)
    tone_steps, groups, thresholds = tm.loop_settings(tones)
    tones.set_tones(steps=tone_steps, groups=groups)
    for g, r in thresholds:
        tones.set_threshold(g, ratio_q8=r, min_energy=256 * tm.LOOP_L)
    F = 512 * B // tm.LOOP_L
    d_audio = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_power = torch.zeros((2, F, len(tone_steps)), dtype=torch.int64, device=dev)
    d_energy = torch.zeros((2, F), dtype=torch.int64, device=dev)
    d_valid = torch.zeros((2, F), dtype=torch.int32, device=dev)
    d_best = torch.zeros((2, F, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((2, F, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(None, 0, B, d_audio.data_ptr())
    torch.cuda.synchronize()
    duc.transmit(mod, d_audio.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    tones.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_power.data_ptr(), d_energy.data_ptr(),
                         d_valid.data_ptr(), d_best.data_ptr(), d_present.data_ptr())
    torch.cuda.synchronize()
    assert (d_audio.cpu().numpy().reshape(2, -1) == audio).all() and gen.clips(0) == gen.clips(1) == 0 and duc.clips(0) == duc_clips
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    n_pcm = d_n.cpu().numpy().view(np.uint32)
    assert (n_pcm == 512).all()
    assert pcm.shape == ref_pcm.shape and (pcm == ref_pcm).all(), np.argwhere(pcm != ref_pcm)[:4].tolist()
    got = (d_power.cpu().numpy().view(np.uint64), d_energy.cpu().numpy().view(np.uint64), d_valid.cpu().numpy().view(np.uint32),
           d_best.cpu().numpy(), d_present.cpu().numpy())
    for name, g, w in zip(("power", "energy", "valid", "best", "present"), got, tm.loop_model().process(pcm, n_pcm)):
        assert g.shape == w.shape and (g == w).all(), f"the tone bank on the PCM receive wrote: {name}"
    tm.loop_check(got[3], got[4])
