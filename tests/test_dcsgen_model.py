"""tests/dcsgen_model.py against the host's restatement of the default-tap law (api.dcs_levels), against the library's own slow
loop and queue rules (hrfd_dcsgen_debug_slow, hrfd_dcsgen_debug_edit: include/hrfd.h in plain C++), the same bytes for every
cut of a stream into calls, the cut rules case by case, when a segment leaves the queue, and detection: what the DCS bank's
model makes of the generator's output under a voice tone.  No GPU, and no tolerance anywhere: everything is integer."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import dcs_model as dm
from tests import dcsgen_model as gm

EINVAL = -1
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def q6(segs):
    return np.ascontiguousarray(np.array(segs, dtype=np.uint64).reshape(-1, 6))


def slow(lib, taps, segs, N, pcm_row, n_blocks, want_active=True):
    """one channel and one call through hrfd_dcsgen_debug_slow -> (out [n_blocks, 512], active, clips)"""
    h = np.ascontiguousarray(taps, dtype=np.int16)
    q = q6(segs)
    x = None if pcm_row is None else np.ascontiguousarray(pcm_row, dtype=np.int16).ravel()
    out = np.zeros((n_blocks, 512), dtype=np.int16)
    active = np.zeros(n_blocks, dtype=np.uint8) if want_active else None
    clips = C.c_uint64(0)
    rc = lib.hrfd_dcsgen_debug_slow(p(h), h.size, p(q) if len(segs) else None, len(segs), N, p(x), n_blocks, p(out), p(active),
                                    C.byref(clips))
    assert rc == 0, lib.hrfd_last_error().decode()
    return out, active, int(clips.value)


def edit(lib, segs, N, op, new=(), arg=0):
    """one edit through hrfd_dcsgen_debug_edit -> the queue behind it as rows of six, or None where it is refused"""
    q = np.zeros((8, 6), dtype=np.uint64)
    if len(segs):
        q[:len(segs)] = q6(segs)
    n = C.c_uint32(len(segs))
    a = np.ascontiguousarray(new, dtype=np.uint32).reshape(-1, 5) if len(new) else None
    rc = lib.hrfd_dcsgen_debug_edit(p(q), C.byref(n), N, op, p(a), 0 if a is None else a.shape[0], arg)
    if rc != 0:
        assert rc == EINVAL
        return None
    return [[int(v) for v in row] for row in q[:n.value]]


def taps_for(T, rng):
    if T == 1:
        return np.array([16384])
    if T == 2:
        return np.array([-20000, 30000])
    if T == 255:
        return api.dcs_lowpass_taps()
    h = rng.integers(-32768, 32768, size=T).astype(np.int64)
    return np.trunc(h * min(1.0, 65535.0 / np.abs(h).sum())).astype(np.int64)


# a. the default tap is the host's restatement
@pytest.mark.parametrize("t0", [0, 28749, 28750, 1 << 58])
def test_default_tap_is_dcs_levels(t0):
    for code, inv in ((0o023, False), (0o754, True)):
        m = gm.DcsGenModel(1)
        m.set_time(t0)
        m.queue(0, [api.dcsgen_segment(gm.FOREVER, code, inv, 1234)])
        got = m.process(None, 60)[0].ravel()                # 30720 samples: more than one period of the grid
        assert (got == api.dcs_levels(code, got.size, 1234, t0, inv)).all()
    # and off the block grid: a segment that starts anywhere reads the same absolute grid
    for s in (28749, 28750, (1 << 58) + 17):
        m = gm.DcsGenModel(1)
        m.set_time(s - s % 512)
        m.queue(0, [api.dcsgen_segment(2000, 0o023, False, 77, tail=0)], start=s)
        got = m.process(None, 6)[0].ravel()
        k = s % 512
        assert (got[k:k + 2000] == api.dcs_levels(0o023, 2000, 77, s)).all() and not got[:k].any() and not got[k + 2000:].any()


def test_reduced_grid_at_the_top_of_the_clock(lib):
    """N = 2^63 - 3 * 512, where 21 n no longer fits int64: the grid over u = n mod 28750 in Python integers"""
    N = (1 << 63) - 3 * 512
    w = api.dcs_word(0o754)
    m = gm.DcsGenModel(1)
    m.set_time(N)
    m.queue(0, [api.dcsgen_segment(gm.FOREVER, 0o754, amplitude=900)])
    got = m.process(None, 3)[0].ravel()
    want = [900 if (w >> ((21 * ((N + i) % 28750) // 1250) % 23)) & 1 else -900 for i in range(3 * 512)]
    assert got.tolist() == want
    assert (slow(lib, [16384], [[N, gm.NO_END, gm.NO_END, w, 900, 0]], N, None, 3)[0].ravel() == got).all()
    with pytest.raises(gm.Refused):
        m.process(None, 1)                                  # the next sample would be 2^63


def test_turn_off_code_is_a_square_wave_of_one_bit_time():
    m = gm.DcsGenModel(1)
    m.queue(0, [api.dcsgen_segment(1, 0o023, amplitude=5, tail=28750 * 2)], start=0)
    y = m.process(None, 113)[0].ravel()[1:1 + 57500].astype(np.int64)
    assert set(np.unique(y)) == {-5, 5}
    edges = np.flatnonzero(np.diff(y)) + 2                  # stream times where the level changes
    assert edges.size == 2 * 2 * 483                        # 483 periods in 28750 samples, two edges each, the wrap among them
    assert y[0] == 5 and all((42 * (int(e) % 28750)) // 1250 != (42 * (int(e) % 28750 - 1)) // 1250 for e in edges)


# b. the model against the library's slow loop, the queue after every edit
def same_queue(lib, model_q, c_q):
    assert c_q is not None and model_q.segs == c_q, (model_q.segs, c_q)


@pytest.mark.parametrize("T", [1, 2, 255, 512])
def test_model_equals_the_slow_loop(lib, T):
    rng = np.random.default_rng(50 + T)
    m = gm.DcsGenModel(1)
    m.set_taps(taps_for(T, rng))
    cq = []                                                 # the C side's queue, carried through hrfd_dcsgen_debug_edit
    m.set_time(28750 * 7 - 1024)                            # u wraps inside the second block

    def both_queue(segs, start):
        nonlocal cq
        got = edit(lib, cq, m.N, 0, segs, start)
        try:
            m.queue(0, segs, start)
        except gm.Refused:
            assert got is None
            return
        cq = got
        same_queue(lib, m.q[0], cq)

    def both_cut(with_tail):
        nonlocal cq
        m.cut(0, with_tail)
        cq = edit(lib, cq, m.N, 1, arg=int(with_tail))
        same_queue(lib, m.q[0], cq)

    def both_process(n_blocks, with_input):
        nonlocal cq
        x = rng.integers(-32768, 32768, size=(1, n_blocks, 512)).astype(np.int16) if with_input else None
        if with_input:
            x[0, 0, :40] = 32767
            x[0, -1, -40:] = -32768
        cq = edit(lib, cq, m.N, 2)
        before = int(m.clips[0])
        out_c, act_c, clips_c = slow(lib, m.taps, cq, m.N, x, n_blocks)
        out_m, act_m = m.process(x, n_blocks, want_active=True)
        same_queue(lib, m.q[0], cq)
        assert (out_m[0] == out_c).all() and (act_m[0] == act_c).all() and int(m.clips[0]) - before == clips_c

    w1, w2 = api.dcs_word(0o754), api.dcs_word(0o023, True)
    both_queue([(100, 700, 300, w1, 32767), (0, 1, 0, w2, 32767), (5, 900, 0, 0x2AAAAA, 12000)], gm.APPEND)
    both_process(3, True)
    both_queue([(0, gm.FOREVER, 1440, w2, 2000)], m.N + 600)
    both_queue([(0, 5, 5, w1, 1)], gm.APPEND)              # behind FOREVER: refused on both sides
    both_queue([(0, 5, 5, w1, 1)], m.N - 1)                # before N
    both_process(2, False)
    both_cut(True)                                          # FOREVER in its code part: the tail follows
    both_process(2, True)
    both_cut(False)                                         # in the tail: it ends now
    both_process(2, True)                                   # the filter's own tail, then silence
    both_queue([(0, 3000, 0, w1, 9000)] * 8, gm.APPEND)
    both_queue([(0, 1, 0, w1, 1)], gm.APPEND)              # a ninth
    both_process(4, False)
    both_cut(True)
    both_process(1, True)


# c. however the stream is cut into calls: every call and every edit goes through the model and through the library's own
#    loop and queue rules (hrfd_dcsgen_debug_slow, hrfd_dcsgen_debug_edit), and both must give the same bytes
class Both:
    """one channel on the model and on the C side, whose queue is carried through hrfd_dcsgen_debug_edit"""

    def __init__(self, lib, N=0):
        self.lib, self.m, self.cq, self.c_clips = lib, gm.DcsGenModel(1), [], 0
        self.m.set_time(N)

    def set_taps(self, taps):
        self.m.set_taps(taps)

    def queue(self, segs, start=gm.APPEND):
        self.m.queue(0, segs, start)
        self.cq = edit(self.lib, self.cq, self.m.N, 0, segs, start)
        same_queue(self.lib, self.m.q[0], self.cq)

    def cut(self, with_tail):
        self.m.cut(0, with_tail)
        self.cq = edit(self.lib, self.cq, self.m.N, 1, arg=int(with_tail))
        same_queue(self.lib, self.m.q[0], self.cq)

    def process(self, x, n_blocks):
        self.cq = edit(self.lib, self.cq, self.m.N, 2)
        out_c, act_c, clips_c = slow(self.lib, self.m.taps, self.cq, self.m.N, x, n_blocks)
        self.c_clips += clips_c
        out_m, act_m = self.m.process(None if x is None else x[None], n_blocks, want_active=True)
        same_queue(self.lib, self.m.q[0], self.cq)
        assert (out_m[0] == out_c).all() and (act_m[0] == act_c).all() and int(self.m.clips[0]) == self.c_clips
        return out_c, act_c


N0 = 28750 - 2 * 512                                        # u wraps inside the third block
WA, WB = api.dcs_word(0o754), api.dcs_word(0o023, True)


def twelve_blocks():
    x = np.random.default_rng(7).integers(-32768, 32768, size=(12, 512)).astype(np.int16)
    x[2, :200], x[7, 100:300] = 32767, -32768
    return x


def run_cuts(lib, cuts, edits, taps=None, up_front=()):
    """12 blocks in calls of `cuts` blocks; edits: {block: function of the pair}, run where a call begins at that block;
    up_front: what is queued before the first call -> (out, active, clips)"""
    assert sum(cuts) == 12
    x = twelve_blocks()
    p = Both(lib, N0)
    if taps is not None:
        p.set_taps(taps)
    for segs, start in up_front:
        p.queue(segs, start)
    outs, acts, b = [], [], 0
    for nb in cuts:
        if b in edits:
            edits[b](p)
        o, a = p.process(x[b:b + nb], nb)
        outs.append(o)
        acts.append(a)
        b += nb
    assert not set(edits) - set(np.cumsum([0] + list(cuts)).tolist()), "an edit fell inside a call"
    return np.concatenate(outs), np.concatenate(acts), p.c_clips


CUTS = ([12], [1] * 12, [5, 1, 6], [3, 3, 3, 3])
T6 = N0 + 6 * 512                                           # the one boundary 5 + 1 + 6 and 3 + 3 + 3 + 3 share behind the start
FOREVER_CODE = ([(10, gm.FOREVER, 700, WA, 30000)], N0)
LATE = [(0, 900, 200, WB, 25000)]


def test_twelve_blocks_however_they_are_cut(lib):
    """no edits: a run of segments queued before the first call, which ends in front of the last two blocks"""
    up_front = (([(10, 1500, 300, WA, 30000), (40, 1, 0, WB, 32767), (0, 1200, 1440, WB, 9000)], N0),)
    for taps in (None, api.dcs_lowpass_taps(), taps_for(512, np.random.default_rng(3))):
        ref = run_cuts(lib, [12], {}, taps, up_front)
        assert ref[2] > 0 and ref[1].any() and not ref[1].all()
        for cuts in CUTS[1:]:
            got = run_cuts(lib, cuts, {}, taps, up_front)
            assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and got[2] == ref[2], cuts


def test_a_cut_and_a_queue_between_calls_for_every_cut(lib):
    """a cut and a queue behind block 6, the boundary every cutting but the single call has; the single call gets the queue
    those edits leave, queued up front: the code part ending at T6 with its tail, and the late segment at its start"""
    def at6(p):
        p.cut(True)
        p.queue(LATE, T6 + 1000)
    for taps in (None, api.dcs_lowpass_taps()):
        ref = run_cuts(lib, [12], {}, taps, (([(10, 6 * 512 - 10, 700, WA, 30000)], N0), (LATE, T6 + 1000)))
        for cuts in CUTS[1:]:
            got = run_cuts(lib, cuts, {6: at6}, taps, (FOREVER_CODE,))
            assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and got[2] == ref[2], cuts
    # the late segment lies on the absolute grid, in phase with any other code
    flat = run_cuts(lib, [5, 1, 6], {6: at6}, None, (FOREVER_CODE,))[0].ravel().astype(np.int64) - twelve_blocks().ravel()
    s = 6 * 512 + 1000
    keep = np.abs(twelve_blocks().ravel()[s:s + 900].astype(np.int64)) < 7000          # where nothing saturates
    assert (flat[s:s + 900][keep] == api.dcs_levels(0o023, 900, 25000, T6 + 1000, True)[keep]).all()


def test_a_queue_a_cut_and_set_taps_between_calls_for_every_cut(lib):
    """set_taps applies from the next call on, so a single call of 12 cannot show it: the cuttings that have a call boundary
    behind block 6 against 6 + 6, with a queue, a cut and a set_taps there"""
    def at6(p):
        p.cut(True)                                         # the code ends, its tail follows
        p.queue(LATE, T6 + 1000)
        p.cut(False)                                        # the tail ends now; the late segment has not begun and is dropped
        p.queue(LATE, T6 + 1200)
        p.set_taps(api.dcs_lowpass_taps(63))                # the queue and the clock stay
    ref = run_cuts(lib, [6, 6], {6: at6}, api.dcs_lowpass_taps(), (FOREVER_CODE,))
    for cuts in CUTS[1:]:
        got = run_cuts(lib, cuts, {6: at6}, api.dcs_lowpass_taps(), (FOREVER_CODE,))
        assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and got[2] == ref[2], cuts
    # and edits behind blocks 3, 6 and 9 for every cutting that has those boundaries
    edits = {3: lambda p: p.cut(True), 6: lambda p: p.queue([(100, 800, 200, WA, 6000)]),
             9: lambda p: p.set_taps(api.dcs_lowpass_taps(63))}
    ref = run_cuts(lib, [3, 3, 3, 3], edits, None, (FOREVER_CODE,))
    for cuts in ([1] * 12, [3, 2, 1, 3, 3], [3, 3, 1, 2, 2, 1]):
        got = run_cuts(lib, cuts, edits, None, (FOREVER_CODE,))
        assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all() and got[2] == ref[2], cuts


# d. the cut, case by case
def test_cut_rules_case_by_case(lib):
    w = 0x123456
    N = 10000
    cases = {
        "code part, with tail": ([[9000, 12000, 12500, w, 5, 500]], True, [[9000, N, N + 500, w, 5, 500]]),
        "code part, without": ([[9000, 12000, 12500, w, 5, 500]], False, [[9000, N, N, w, 5, 500]]),
        "forever, with tail": ([[9000, gm.NO_END, gm.NO_END, w, 5, 1440]], True, [[9000, N, N + 1440, w, 5, 1440]]),
        "forever, without": ([[9000, gm.NO_END, gm.NO_END, w, 5, 1440]], False, [[9000, N, N, w, 5, 1440]]),
        "begins now": ([[N, 12000, 12500, w, 5, 500]], True, []),
        "in its tail, with": ([[9000, 9900, 10400, w, 5, 500]], True, [[9000, 9900, 10400, w, 5, 500]]),
        "in its tail, without": ([[9000, 9900, 10400, w, 5, 500]], False, [[9000, 9900, N, w, 5, 500]]),
        "tail ends now": ([[9000, 9900, N, w, 5, 100]], False, [[9000, 9900, N, w, 5, 100]]),
        "not yet begun": ([[N + 1, 12000, 12500, w, 5, 500]], True, []),
        "ended, within reach": ([[9000, 9400, 9500, w, 5, 100]], False, [[9000, 9400, 9500, w, 5, 100]]),
        "ended, out of reach": ([[9000, 9400, N - 511, w, 5, 100]], True, []),
        "one of each": ([[9000, 9400, 9600, w, 5, 200], [9600, 10500, 10600, w, 6, 100], [10600, 10700, 10800, w, 7, 100]], True,
                        [[9000, 9400, 9600, w, 5, 200], [9600, N, N + 100, w, 6, 100]]),
    }
    for name, (before, with_tail, after) in cases.items():
        q = gm.Queue()
        q.segs = [list(s) for s in before]
        q.cut(N, with_tail)
        assert q.segs == after, name
        assert edit(lib, before, N, 1, arg=int(with_tail)) == after, name
        # no edit changes r before N (what had ended, and no sample can reach any more, is forgotten)
        live = [s for s in before if not gm.ended(s, N)]
        assert (gm.raw_levels(live, N - 2000, 2000) == gm.raw_levels(after, N - 2000, 2000)).all(), name
    # at the top of the clock the tail's end stays below 2^63
    top = (1 << 63) - 512
    q = gm.Queue()
    q.segs = [[top - 100, gm.NO_END, gm.NO_END, w, 5, 1440]]
    q.cut(top, True)
    assert q.segs == [[top - 100, top, (1 << 63) - 1, w, 5, 1440]] == edit(lib, [[top - 100, gm.NO_END, gm.NO_END, w, 5, 1440]], top, 1, arg=1)


# e. a segment leaves at E + 511
def test_a_segment_leaves_at_e_plus_511_and_not_before(lib):
    m = gm.DcsGenModel(1)
    m.set_taps(np.full(512, 100))
    m.queue(0, [(0, 1000, 25, 0x7FFFFF, 1000)] + [(0, 1, 0, 0, 0)] * 7, start=0)      # E = 1025 for the first; 8 live
    E = 1025
    assert E + 511 == 3 * 512
    m.process(None, 2)                                      # N = 1024 < E
    assert m.pending(0) == (8, 1032)
    m.set_time(E + 510)
    assert m.pending(0) == (8, 1032)
    with pytest.raises(gm.Refused):
        m.queue(0, [(0, 1, 0, 0, 0)], start=5000)           # a ninth: the first has not ended
    m.set_time(E + 511)
    assert m.pending(0) == (7, 1032)                        # the seven of length 1 end one to seven samples later
    m.queue(0, [(0, 1, 0, 0, 0)], start=5000)
    assert m.pending(0) == (8, 5001) and m.q[0].segs[0][0] == 1025
    # the filter's last sample lies at E + 510, and active says so
    m = gm.DcsGenModel(1)
    m.set_taps(np.full(512, 100))
    m.queue(0, [(0, 1000, 25, 0x7FFFFF, 1000)], start=0)
    m.set_time(E + 511 - 512)
    y, a = m.process(None, 1, want_active=True)             # the block up to E + 510
    assert a[0, 0] == 1 and abs(int(y[0, 0, -1])) == 6      # one tap of 100 on one sample of 1000: (100000 + 8192) >> 14
    assert m.N == E + 511 and m.pending(0) == (0, m.N)
    y, a = m.process(None, 1, want_active=True)
    assert a[0, 0] == 0 and not y.any() and m.q[0].segs == []
    # and on the C side
    seg = [[0, 1000, E, 0x7FFFFF, 1000, 25]]
    assert edit(lib, seg, E + 510, 2) == seg and edit(lib, seg, E + 511, 2) == []


# f. detection: the generator under a voice tone through the DCS bank's model behind its low-pass
def detect(shaping, start, length=gm.FOREVER, n_blocks=16):
    g = gm.DcsGenModel(1)
    if shaping is not None:
        g.set_taps(shaping)
    g.queue(0, [api.dcsgen_segment(length, 0o754, amplitude=2000)], start=start)
    n = n_blocks * 512
    tone = np.round(5000.0 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / 8000.0)).astype(np.int16).reshape(1, n_blocks, 512)
    y = g.process(tone)
    d = dm.DcsModel(1)
    d.set_taps(api.dcs_lowpass_taps())
    d.set_codes([0o754, 0o023], [False, True])
    hits, best, present = d.process(y)
    return y, hits[0], best[0], present[0], g


@pytest.mark.parametrize("shaped", [False, True])
@pytest.mark.parametrize("start", [0, 777])
def test_the_dcs_bank_finds_the_code(shaped, start):
    y, hits, best, present, g = detect(api.dcs_lowpass_taps() if shaped else None, start)
    first = start // 512 + 4                                # a word's 1310 samples and the low-pass's 254 behind the start
    print("hits", hits[:, 0].tolist(), "peak", int(np.abs(y.astype(np.int64) - 0).max()))
    assert present[first:, 0].all() and (best[first:, 0] == 0).all()
    assert not hits[:, 1].any()
    assert not g.clips.any()
    if shaped:
        # the shaped code alone: the filter's overshoot, exact as everything here is (DESIGN 3.20 quotes it)
        g2 = gm.DcsGenModel(1)
        g2.set_taps(api.dcs_lowpass_taps())
        g2.queue(0, [api.dcsgen_segment(gm.FOREVER, 0o754, amplitude=2000)], start=start)
        peak = int(np.abs(g2.process(None, 16).astype(np.int64)).max())
        print("peak |g|", peak)
        assert peak == 2375


def test_the_turn_off_code_closes_the_squelch():
    cut_at = 9 * 512 + 200                                  # the code part ends inside block 9, 1440 samples of tail follow
    y, hits, best, present, g = detect(api.dcs_lowpass_taps(), 0, length=cut_at, n_blocks=16)
    print("hits", hits[:, 0].tolist())
    b = cut_at // 512                                       # the block of the cut
    assert present[4:b + 1, 0].all()                        # from the fourth block behind the start up to the block of the cut
    assert not present[b + 2:, 0].any()                     # 0 from the second block behind it on
    assert not hits[b + 2:, 0].any()
    assert hits[b:b + 2, 0].tolist() == [476, 83]           # what the model gives, as DESIGN 3.20 records it
    # the tail is a 134.4 Hz square wave: over the blocks it fills (10 and 11) the power there is far above that of any code
    # block, whose energy is spread over the word's spectrum: 185 times the largest of them (4.2e11 against 2.3e9; a float sum of integers, so the
    # ratio is held to a percent and not to the bit)
    t = np.arange(512)
    ref = np.exp(-2j * np.pi * 134.4 * t / 8000.0)
    code_only = gm.DcsGenModel(1)
    code_only.queue(0, [api.dcsgen_segment(cut_at, 0o754, amplitude=2000)], start=0)
    z = code_only.process(None, 16)[0].astype(np.float64)
    power = np.abs((z * ref).sum(axis=1)) ** 2
    print("power at 134.4 Hz", power.tolist())
    assert 183 < power[10:12].min() / power[:9].max() < 187
