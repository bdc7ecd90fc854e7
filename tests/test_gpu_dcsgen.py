"""The DCS generator bank on the device (hrfd_dcsgen_*) against the numpy model (tests/dcsgen_model.py), bit for bit: channel and
block counts on both sides of the kernel's tile under every filter length that takes another path, segments that start and
end on every edge, eight hits in one tile, abutting segments, a filter tail across a call boundary, the grid's wrap inside a
lane and at a tile's first sample, the top of the clock, saturation with its count, generate-only, out of place and in place at
every even residue with padded strides and guard bytes around every buffer, edits between calls, and what the bank exists
for: its audio decoded by Dcs on the device, and the closed loop DcsGen -> TxKey -> Mod -> Duc.transmit -> Ddc.receive -> Dcs.
No comparison has a tolerance."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import dcs_model as dm
from tests import dcsgen_model as gm
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
FOREVER = gm.FOREVER
W1, W2, W3 = api.dcs_word(0o754), api.dcs_word(0o023, True), 0x2AAAAA


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


_taps = {}


def taps_for(T):
    """one filter per length, computed once: the single tap, two taps of both signs, the DCS low-pass, and 512 random taps
    at the largest sum the bank takes"""
    if T not in _taps:
        if T == 1:
            h = np.array([16384])
        elif T == 2:
            h = np.array([-20000, 30000])
        elif T == 255:
            h = api.dcs_lowpass_taps()
        else:
            h = np.random.default_rng(T).integers(-32768, 32768, size=T).astype(np.int64)
            h = np.trunc(h * min(1.0, 65535.0 / np.abs(h).sum())).astype(np.int64)
        _taps[T] = h
    return _taps[T]


def both(C, T=1, N=0):
    d, m = api.DcsGen(C, device=0), gm.DcsGenModel(C)
    for h in (d, m):
        if T != 1:
            h.set_taps(taps_for(T))
        if N:
            h.set_time(N)
    return d, m


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
    call's n samples, the last of them without an end on every fourth channel"""
    rng = np.random.default_rng(seed)
    for c in range(C):
        if c % 3 == 2:
            continue
        k = int(rng.integers(1, 6))
        run = [(int(rng.choice([0, 0, 1, 200, 700])), int(rng.choice([1, 63, 300, 1000, 2500])), int(rng.choice([0, 1, 100, 1440])),
                int(rng.integers(0, 1 << 23)), int(rng.integers(0, 32768))) for _ in range(k)]
        if c % 4 == 0:
            run.append((5, FOREVER, 1440, W1, 30000))
        start = base + int(rng.integers(0, max(n // 2, 2)))
        for h in hs:
            h.queue(c, run, start)


def same_state(d, m, what):
    assert d.time() == m.N, what
    for c in range(m.C):
        assert d.clips(c) == int(m.clips[c]), f"{what}: clips of channel {c}: {d.clips(c)} against {int(m.clips[c])}"
        assert d.pending(c) == m.pending(c), f"{what}: pending({c})"


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
#    of one tile), 9 (a third tile begun); one channel, three, and 65 (gy = 32 and 1 tile, and tiles striding); T = 1 (odd, the
#    shortest), 2 (even: the other parity of the window), 255 and 512 (the longest, lead = 0)
@pytest.mark.parametrize("C", [1, 3, 65])
@pytest.mark.parametrize("n_blocks", [1, 3, 4, 5, 9])
def test_channel_and_block_counts(C, n_blocks):
    pcm = reference(C, 512 * n_blocks)
    for T in (1, 2, 255, 512):
        d, m = both(C, T)
        scatter((d, m), C, 512 * n_blocks, 100 * C + n_blocks + T)
        got, act = d.process(pcm, want_active=True)
        want, want_act = m.process(pcm, want_active=True)
        assert got.dtype == want.dtype and got.shape == want.shape and (got == want).all(), (T, np.argwhere(got != want)[:4].tolist())
        assert (act == want_act).all(), T
        got = d.process(None, n_blocks)                        # the second call: generate only, what is still queued
        assert (got == m.process(None, n_blocks)).all(), T
        same_state(d, m, f"C={C}, {n_blocks} blocks, T={T}")


# 2. segment edges, on one call of 5 blocks: S and E each at a block boundary and at a tile boundary - 1, 0, + 1
EDGES = (0, 1, 511, 512, 513, 2047, 2048, 2049, 2559)
SHAPES = ((1, 0), (1, 7), (3, 0), (600, 40), (FOREVER, 1440))


@pytest.mark.parametrize("T", [1, 255, 512])
def test_segment_edges(torch_dev, T):
    n_blocks = 5
    starts = [(s, L, Q) for s in EDGES for L, Q in SHAPES]
    ends = [(e, L, Q) for e in EDGES[1:] for L, Q in ((min(e, 700), 0), (1, min(e - 1, 30)))]     # E = e
    C = len(starts) + len(ends) + 3
    d, m = both(C, T)
    for h in (d, m):
        for c, (s, L, Q) in enumerate(starts):
            h.queue(c, [(0, L, Q, W1 if c % 2 else W2, 30000 - c)], s)
        for c, (e, L, Q) in enumerate(ends, len(starts)):
            h.queue(c, [(0, L, Q, W3, 20000 + c)], e - L - Q)
        # eight live segments inside one tile, abutting, with different words and amplitudes
        h.queue(C - 3, [(0, 100 + 13 * i, 20 * (i % 3), (W1 * (i + 1)) & 0x7FFFFF, 4000 * i + 767) for i in range(8)], 3)
        # two codes that abut without a tail, and one that abuts a tail
        h.queue(C - 2, [(0, 1000, 0, W1, 32767), (0, 1000, 300, W2, 1), (0, 200, 0, W3, 32767)], 511)
    assert d.pending(C - 3) == m.pending(C - 3) and d.pending(C - 3)[0] == 8
    want, act = run_device(torch_dev, d, m, reference(C, 512 * n_blocks), n_blocks, f"edges, T={T}")
    reach = T - 1
    assert act[starts.index((2559, 1, 0))].tolist() == [0, 0, 0, 0, 1]
    assert act[starts.index((2047, 1, 0))].tolist() == [0, 0, 0, 1, 1 if reach else 0]
    assert act[C - 1].tolist() == [0] * 5                       # nothing queued
    # the same from a new pair, generate only: the shortest segments
    d, m = both(1)
    for h in (d, m):
        h.queue(0, [(0, 1, 0, 0x7FFFFF, 123), (9, 1, 1, 0, 321)], 5)
    want, act = run_device(torch_dev, d, m, None, 1, "the shortest segments", mode="gen")
    assert want[0, 0, 5] == 123 and want[0, 0, 15] == -321 and abs(int(want[0, 0, 16])) == 321 and np.count_nonzero(want) == 3


# 3. a segment that ends in one call, its filter tail in the next: E + T - 1 on both sides of the boundary at 1024
def test_filter_tail_across_a_call_boundary(torch_dev):
    T = 255
    ends = (1024 - 254 - 1, 1024 - 254, 1024 - 254 + 1, 1000, 1023, 1024, 1025)
    C = len(ends)
    d, m = both(C, T)
    for h in (d, m):
        for c, e in enumerate(ends):
            h.queue(c, [(0, 300, 50, W1, 25000)], e - 350)
    pcm = reference(C, 4 * 512, 9).reshape(C, 4, 512)
    _, a0 = run_device(torch_dev, d, m, pcm[:, :2], 2, "the call the segments end in")
    want, a1 = run_device(torch_dev, d, m, pcm[:, 2:], 2, "the call behind it", mode="in_place")
    assert a1[:, 0].tolist() == [0, 0, 1, 1, 1, 1, 1] and not a1[:, 1].any() and a0[:, 1].all()
    assert (want[0] == pcm[0, 2:]).all() and (want[3] != pcm[3, 2:]).any()      # E + T - 1 = 1023: nothing is left; E = 1000: 230 samples are
    third = d.process(None, 1)
    assert not third.any() and (third == m.process(None, 1)).all() and d.pending(0) == m.pending(0) == (0, m.N)


# 4. the clock: the grid's wrap (a stream time that is a multiple of 28750) inside a lane's 8 samples, at a tile's first sample,
#    at a call's first sample, and inside the 512 samples in front of a tile; and the top of the clock
@pytest.mark.parametrize("T", [1, 255])
@pytest.mark.parametrize("wrap_at", [1027, 2048, 0, 2048 - 100, 8 * 251 + 7])
def test_the_grid_wraps_anywhere(torch_dev, T, wrap_at):
    N = 28750 * 1000003 - wrap_at
    d, m = both(2, T, N)
    for h in (d, m):
        h.queue(0, [(0, FOREVER, 0, W1, 20000)], N)
        h.queue(1, [(0, 1, 5000, W2, 20000)], N + 1)           # the turn-off grid across the wrap as well
    run_device(torch_dev, d, m, reference(2, 9 * 512), 9, f"wrap at {wrap_at}, T={T}")


def test_the_top_of_the_clock(torch_dev):
    N = (1 << 63) - 3 * 512
    for T in (1, 512):
        d, m = both(2, T, N - 512)
        for h in (d, m):
            h.queue(0, [(0, FOREVER, 1440, W1, 32767)], N - 400)
            h.queue(1, [(0, 100, 50, W2, 32767), (0, 1, 1383, W3, 100)], N + 1)      # the last E: 2^63 - 1
        assert d.pending(1) == m.pending(1) == (2, (1 << 63) - 1)
        run_device(torch_dev, d, m, None, 1, "in front of the top", mode="gen")
        want, _ = run_device(torch_dev, d, m, reference(2, 3 * 512), 3, f"the top of the clock, T={T}")
        if T == 1:
            w = [(32767 if (W1 >> ((21 * ((N + i) % 28750) // 1250) % 23)) & 1 else -32767) for i in range(1536)]
            assert (np.clip(reference(2, 3 * 512)[0].astype(np.int64) + w, -32768, 32767) == want[0].ravel()).all()
        with pytest.raises(api.HrfdError, match="below 2\\^63"):
            d.process(None, 1)
    # a cut less than a tail in front of the top: the tail's end stays below 2^63
    d, m = both(1, 2, (1 << 63) - 1024)
    for h in (d, m):
        h.queue(0, [(0, FOREVER, 1440, W1, 1000)])
    run_device(torch_dev, d, m, None, 1, "in front of the cut", mode="gen")
    for h in (d, m):
        h.cut(0, True)
    assert d.pending(0) == m.pending(0) == (1, (1 << 63) - 1)
    run_device(torch_dev, d, m, None, 1, "the tail up to the top", mode="gen")


# 5. the buffers: every even residue of the rows' addresses, padded strides, the three modes, guards around everything; an idle
#    row stays as it is in place
@pytest.mark.parametrize("mode", ["out", "in_place", "gen"])
def test_buffers_at_every_even_residue(torch_dev, mode):
    C, n_blocks = 4, 5
    for residue in range(0, 16, 2):
        d, m = both(C, 255 if residue % 4 else 2)
        scatter((d, m), C, 512 * n_blocks, 60 + residue)
        pad, out_pad = (2 + residue, 30 - residue) if residue % 4 else (0, 6)
        want, act = run_device(torch_dev, d, m, reference(C, 512 * n_blocks, residue), n_blocks, f"{mode} at residue {residue}", mode=mode,
                               residue=residue, pad=pad, out_pad=out_pad, want_active=residue != 6)
        assert not act[2].any() and act[0].any()
        if mode != "gen":
            assert (want[2].ravel() == reference(C, 512 * n_blocks, residue)[2]).all()
        else:
            assert not want[2].any()


# 6. saturation and its count
def test_clips_are_counted(torch_dev):
    C, n_blocks = 3, 5
    x = np.zeros((C, n_blocks * 512), dtype=np.int16)
    x[0, :], x[1, :], x[2, ::2] = 32767, -32767, 32767
    for T in (1, 255):
        d, m = both(C, T)
        for h in (d, m):
            h.queue(ALL, [(0, 1800, 300, W1, 1)], 100)
            h.queue(2, [(7, FOREVER, 0, W2, 32767)])
        run_device(torch_dev, d, m, x, n_blocks, f"clips, T={T}")
        assert d.clips(0) > 0 and d.clips(1) == 0 and d.clips(2) > 0 and d.clips(0) == int(m.clips[0])
        if T == 1:
            high = int((api.dcs_levels(0o754, 1800, 1, 100) == 1).sum()) + int((gm.sq_sign(np.arange(1900, 2200)) == 1).sum())
            assert d.clips(0) == high                           # 32767 + 1 wherever the code or its tail is high
        run_device(torch_dev, d, m, x, n_blocks, "clips add up", mode="in_place")
        d.reset()
        m.reset()
        assert d.clips(2) == 0
        run_device(torch_dev, d, m, x[:, :512], 1, "behind a reset", mode="out")
        assert d.clips(0) == d.clips(2) == 0 and d.time() == 512


# 7. active alone is the segments' reach: [S, E + T - 1)
def test_active_follows_the_filters_reach():
    for T in (1, 2, 512):
        d, m = both(3, T)
        for h in (d, m):
            h.queue(0, [(0, 10, 2, W1, 0)], 1012)               # E = 1024; amp 0 is active all the same
            h.queue(1, [(0, 1, 0, W1, 5)], 2047)
            h.queue(2, [(0, 1, 0, W1, 5)], 3072 + 511)
        out, act = d.process(None, 9, want_active=True)
        want, want_act = m.process(None, 9, want_active=True)
        assert (out == want).all() and (act == want_act).all()
        assert act[0].tolist() == [0, 1, int(T > 1), 0, 0, 0, 0, 0, 0]
        assert act[1].tolist() == [0, 0, 0, 1, int(T > 1), 0, 0, 0, 0]
        assert act[2].tolist() == [0, 0, 0, 0, 0, 0, 1, int(T > 1), 0]


# 8. queue(ALL), and its refusal as a whole; the refusals that need a handle
def test_broadcast_and_refusals_that_need_a_handle(torch_dev):
    C = 5
    d, m = both(C, 2)
    for h in (d, m):
        h.queue(3, [(0, FOREVER, 10, W2, 900)], 4000)
        h.queue(ALL, [(10, 500, 100, W1, 7000), (0, 300, 0, W3, 100)], 20)
    for h, err in ((d, api.HrfdError), (m, gm.Refused)):
        with pytest.raises(err):
            h.queue(ALL, [(0, 10, 0, W1, 1)])                   # appended: behind channel 3's FOREVER segment, so nowhere
        with pytest.raises(err):
            h.queue(ALL, [(0, 10, 0, W1, 1)], 3995)             # overlaps on channel 3 only
    same_state(d, m, "refused whole")
    for call, word in ((lambda: d.queue(5, [(0, 1, 0, 0, 0)]), "channel 5"), (lambda: d.cut(5), "channel 5"), (lambda: d.pending(5), "channel 5"),
                       (lambda: d.clips(5), "channel 5"), (lambda: d.set_taps([32767, 32767, 2]), "sum \\|h\\|"),
                       (lambda: d.queue(0, [(0, 1, 0, 1 << 23, 0)]), "the word 0x800000"), (lambda: d.set_time(1 << 63), "below 2\\^63")):
        with pytest.raises(api.HrfdError, match=word):
            call()
    with pytest.raises(ValueError, match="int16"):
        d.set_taps([16384, 40000])                              # refused before a conversion could wrap it
    run_device(torch_dev, d, m, reference(C, 9 * 512), 9, "broadcast")
    for h in (d, m):
        h.set_time(0)
    with pytest.raises(api.HrfdError, match="lies before the stream time"):
        d.set_time(100)
        d.queue(0, [(0, 1, 0, 0, 0)], 99)
    # out against the rows of every channel, which only the handle's count can decide
    torch, dev = torch_dev
    buf = torch.zeros(C * 512 + 4096, dtype=torch.int16, device=dev)
    with pytest.raises(api.HrfdError, match="overlaps the input"):
        d.process_device(buf.data_ptr(), 1024, 1, buf.data_ptr() + 1024 * (C - 1) + 2, 1024)


# 9. six calls of one block against one call of six
def test_six_calls_of_one_block_are_one_call_of_six(torch_dev):
    C = 3
    pcm = reference(C, 6 * 512, 3).reshape(C, 6, 512)
    outs = {}
    for T in (1, 255):
        whole, mw = both(C, T, 28750 - 1500)
        parts, mp = both(C, T, 28750 - 1500)
        for h in (whole, mw, parts, mp):
            h.queue(ALL, [(40, 700, 200, W1, 9000), (300, FOREVER, 0, W2, 4000)])
            h.queue(1, [(0, 39, 1, W3, 32767)], 28750 - 1500)
        want, act = run_device(torch_dev, whole, mw, pcm, 6, f"one call, T={T}")
        got = [run_device(torch_dev, parts, mp, pcm[:, b:b + 1], 1, f"call {b}, T={T}") for b in range(6)]
        assert (np.concatenate([g[0] for g in got], axis=1) == want).all() and (np.concatenate([g[1] for g in got], axis=1) == act).all()
        assert [whole.clips(c) for c in range(C)] == [parts.clips(c) for c in range(C)]


# 10. edits between calls: cut with and without the tail, set_taps, set_time and reset, each on the device and on the model
def test_edits_between_calls(torch_dev):
    C = 4
    pcm = reference(C, 16 * 512, 5).reshape(C, 16, 512)
    d, m = both(C, 255)
    stream = torch_dev[0].cuda.Stream(device=torch_dev[1])
    for h in (d, m):
        h.queue(ALL, [(0, FOREVER, 1440, W1, 5000)], 100)
        h.queue(3, [(0, 1, 0, 0, 0)], 0)
    run_device(torch_dev, d, m, pcm[:, 0:3], 3, "before the edits")
    for h in (d, m):
        h.cut(0, True)                                          # the code ends at 1536, its tail at 2976
        h.cut(1, False)                                         # ends at 1536
        h.set_taps(taps_for(512))                               # from the next call on; the queue and the clock stay
    assert d.pending(0) == m.pending(0) == (1, 1536 + 1440) and d.pending(1) == (1, 1536) and d.pending(2) == (1, gm.NO_END)
    run_device(torch_dev, d, m, pcm[:, 3:5], 2, "behind the cuts", mode="in_place", stream=stream.cuda_stream)
    for h in (d, m):
        h.cut(0, False)                                         # in its tail: it ends now
        h.cut(1, True)                                          # ended at 1536 and out of reach by now: it leaves
        h.queue(1, [(0, 600, 0, W1, 5000)])                     # goes on in phase at N
        h.set_taps(taps_for(2))
    assert d.pending(0) == m.pending(0) == (1, 2560) and d.pending(1) == m.pending(1) == (1, 2560 + 600)
    want, _ = run_device(torch_dev, d, m, pcm[:, 5:8], 3, "a code queued again")
    assert d.pending(0) == (0, d.time())
    for h in (d, m):
        h.set_time(28750 * 5 - 700)                             # the clock only: channel 2's code goes on, on the grid there
        h.cut(3, True)
    run_device(torch_dev, d, m, pcm[:, 8:11], 3, "behind set_time", stream=stream.cuda_stream)
    for h in (d, m):
        h.reset()                                               # queues, clock and clips; the taps stay
    assert d.time() == 0 and d.pending(2) == (0, 0)
    want, act = run_device(torch_dev, d, m, pcm[:, 11:12], 1, "behind reset")
    assert (want == pcm[:, 11:12]).all() and not act.any()
    for h in (d, m):
        h.queue(2, [(0, 400, 30, W2, 32767)], 512)
    want, _ = run_device(torch_dev, d, m, pcm[:, 12:16], 4, "the taps outlive a reset", mode="in_place")
    assert (want[2] != pcm[2, 12:16]).any()


# 11. DcsGen.process_device -> Dcs.process_device -> Audio.gate_device on one stream, no host copy in between
def test_the_generator_opens_the_dcs_squelch_on_the_device(torch_dev):
    from tests.audio_model import AudioModel
    torch, dev = torch_dev
    C, B = 4, 12
    codes = [(0o754, False), (0o023, True), (0o445, False)]
    n = B * 512
    tone = np.round(5000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / 8000.0)).astype(np.int16)
    pcm = np.stack([tone] * C)
    g, gmod = both(C, 255)
    for h in (g, gmod):
        for c, (code, inv) in enumerate(codes):
            h.send(c, code, inv) if h is g else h.queue(c, [api.dcsgen_segment(FOREVER, code, inv)])
    dcs, dmod = api.Dcs(C, device=0), dm.DcsModel(C)
    a, am = api.Audio(C, 1, device=0), AudioModel(C, 1)
    for b in (dcs, dmod):
        b.set_taps(api.dcs_lowpass_taps())
        b.set_codes([c for c, _ in codes], [i for _, i in codes])
    for b in (a, am):
        for c in range(C):
            b.set_want(min(c, 2), c)                            # channel 3 waits for a code nobody sends it
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    d_active = torch.zeros((C, B), dtype=torch.uint8, device=dev)
    d_best = torch.zeros((C, B, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((C, B, 4), dtype=torch.uint8, device=dev)
    d_open = torch.zeros((C, B), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    g.process_device(d_pcm.data_ptr(), 1024 * B, B, d_pcm.data_ptr(), 0, d_active.data_ptr(), s.cuda_stream)      # in place
    dcs.process_device(d_pcm.data_ptr(), 1024 * B, None, B, None, d_best.data_ptr(), d_present.data_ptr(), s.cuda_stream)
    a.gate_device(d_best.data_ptr(), d_present.data_ptr(), 512, 0, B, d_open.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    y, act = gmod.process(pcm, B, want_active=True)
    hits, best, present = dmod.process(y)
    opened = am.gate(best, present, 512, 0)
    assert (d_pcm.cpu().numpy().reshape(C, B, 512) == y).all() and (d_active.cpu().numpy() == act).all()
    assert (d_best.cpu().numpy() == best).all() and (d_present.cpu().numpy() == present).all() and (d_open.cpu().numpy() == opened).all()
    assert opened[:3, 4:].all() and not opened[3].any() and act[:3].all() and not act[3].any()


# 12. the closed loop
def test_closed_loop_generate_key_transmit_receive_decode(torch_dev, oracle):
    """tests/test_gpu_dcs.py's closed loop with the generator in front: two WBFM stations, D754N and D023I under a 1 kHz tone.
    DcsGen adds the codes to the tone on the device, TxKey turns its active bytes into the key, Mod and the keyed
    Duc.transmit send, Ddc.receive and Dcs decode.  (a) the PCM sent is the host-made audio of that loop, sample for sample
    (dcs_model.loop_audio: dcs_levels under the tone), so the CPU oracle's chain has been run on this very input (b) the
    outputs equal the models' on the PCM received (c) the presence pattern is the one that chain gave: from block 4 on every
    block has its station's code present as the best of its group (dcs_model.loop_check)."""
    from tests import ddc_model as ddm
    from tests import tone_model as tm
    torch, dev = torch_dev
    B = dm.LOOP_BLOCKS
    n = B * 512
    tone = np.round(dm.LOOP_TONE_AMP * np.sin(2 * np.pi * dm.LOOP_TONE_HZ * np.arange(n) / 8000.0)).astype(np.int16)
    gen, gmod = both(2)
    for c, (code, inv) in enumerate(dm.LOOP_CODES):
        gen.send(c, code, inv, amplitude=dm.LOOP_DCS_AMP)
        gmod.queue(c, [api.dcsgen_segment(FOREVER, code, inv, dm.LOOP_DCS_AMP)])
    d_pcm_in = torch.from_numpy(np.stack([tone, tone])).to(dev)
    d_active = torch.zeros((2, B), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(d_pcm_in.data_ptr(), 1024 * B, B, d_pcm_in.data_ptr(), 0, d_active.data_ptr())
    torch.cuda.synchronize()
    audio = dm.loop_audio()
    sent = d_pcm_in.cpu().numpy()
    assert (sent == np.stack(audio)).all() and (sent.reshape(2, B, 512) == gmod.process(np.stack([tone, tone]), B)).all()
    key = api.TxKey(2, hold=1)(d_active)
    assert key.cpu().numpy().all()
    streams, amps = tm.loop_streams(oracle, audio)
    R, FULL = ddm.SEL_R, 262144
    assert B == ddm.SEL_BLOCKS
    mod = api.Mod(api.MOD_WBFM, 2, device=0)
    duc = api.Duc(1, 2, R, device=0)
    ddc = api.Ddc(1, 2, R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.WBFM)
    for c, f in enumerate(ddm.SEL_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(amps[c], c)
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(ddm.SEL_GAIN_SHIFT[c], c)
    model = dm.loop_model()
    dcs = api.Dcs(2, device=0)
    dcs.set_taps(model.taps)
    dcs.set_codes([c for c, _ in dm.LOOP_CODES], [i for _, i in dm.LOOP_CODES])
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_hits = torch.zeros((2, B, 2), dtype=torch.int16, device=dev)
    d_best = torch.zeros((2, B, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((2, B, 4), dtype=torch.uint8, device=dev)
    assert duc.n_keys(B * FULL) == B
    torch.cuda.synchronize()
    duc.transmit(mod, d_pcm_in.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL, d_key=key.data_ptr(), key_stride=B)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    dcs.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_hits.data_ptr(), d_best.data_ptr(), d_present.data_ptr())
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    n_pcm = d_n.cpu().numpy().view(np.uint32)
    assert (n_pcm == 512).all()
    got = (d_hits.cpu().numpy().view(np.uint16), d_best.cpu().numpy(), d_present.cpu().numpy())
    want = model.process(pcm, n_pcm)
    for name, a, b in zip(("hits", "best", "present"), got, want):
        assert (a == b).all(), name
    print("hits of each station's own code per block:", got[0][0, :, 0].tolist(), got[0][1, :, 1].tolist())
    dm.loop_check(*got)
