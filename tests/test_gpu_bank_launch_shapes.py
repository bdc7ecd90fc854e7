"""The banks in the launch shapes and strides their own suites do not reach, tolerance 0 everywhere.

A. k_tonegen with several tiles per workgroup (gy < tiles): the clip count a lane carries across its tiles, the in-place
   `continue` on a tile without hits in front of a tile with hits, `active` for a workgroup's later tiles.
B. tonegen_stage with more than one upload through the pinned buffer, and an upload that starts at dirty_lo != 0.
C. k_cal past the widening inside cal_groups' loop (kCalWiden steps), under debug_set_workgroups.
D. every device entry that takes a byte stride, with two rows more than 4 GiB apart.
E. the PCM banks past 1024 channels.

A, B, C and E compare with the numpy models through the guarded run_device of the banks' own suites; D makes the same call on
twin handles with far and with dense rows and asserts equal outputs and untouched sentinels (dense against the model is the
business of the banks' own suites).  The dispatch arithmetic that decides whether a shape reaches its path is restated in
tests/test_bank_launch_shapes_model.py, checked there without a device, and asserted here next to every call."""
import gc
import time

import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import cal_model as cm
from tests import test_bank_launch_shapes_model as ls
from tests import test_gpu_audio as ta
from tests import test_gpu_cal as tc
from tests import test_gpu_level as tl
from tests import test_gpu_resamp as tr
from tests import test_gpu_tone as tt
from tests import test_gpu_tonegen as tg
from tests import tone_model as tm

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
MASK32 = 0xFFFFFFFF
FOREVER = tg.FOREVER
TILE = ls.TONEGEN_TILE


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and (got == want).all(), \
        f"{what}: differs at {np.argwhere(got != want)[:4].tolist()}"


# ================================================================ A. the tone generator: several tiles per workgroup
RECIPES = ("span", "forever", "second", "first", "clip")


def queue_recipe(hs, c, which, b, st):
    """one of the explicit queues of section A on channel c of every handle of hs; the workgroup (c, 0) takes the tile at 0
    and, next, the tile at b"""
    if which == "span":            # starts in the last 7 samples of tile 0, ends in the first samples of the tile at b
        q = [(0, [tg.seg(b + 3 - (TILE - 5), st[0], 30000, st[1], 20000)], TILE - 5)]
    elif which == "forever":
        q = [(1, [tg.seg(FOREVER, st[2], 20000, st[3], 9000)], 37)]
    elif which == "second":        # wholly inside the workgroup's second tile
        q = [(0, [tg.seg(300, st[4], 25000, st[5], 25000)], b + 10)]
    elif which == "first":         # wholly inside its first
        q = [(0, [tg.seg(1000, st[6], 25000, st[7], 25000)], 700)]
    else:                          # full amplitude in both tiles, over the same lanes: 12..52 of the tile
        q = [(0, [tg.seg(1500, st[0], 32767, st[5], 32767)], 100), (0, [tg.seg(400, st[3], 32767, st[6], 32767)], b + 20)]
    for track, segs, start in q:
        for h in hs:
            h.queue(c, track, segs, start)


def recipe_passes(C):
    """[(whether scatter's random queues go on, {recipe: channel})]: with enough channels one handle holds everything, the
    recipes on channels scatter leaves idle (c % 3 == 2), spread over the bank; with 1 or 3 channels one handle holds scatter
    and one more each recipe, alone on the last channel"""
    if C >= 18:
        idle = [c for c in range(C) if c % 3 == 2]
        k = len(idle)
        return [(True, dict(zip(RECIPES, (idle[0], idle[k // 4], idle[k // 2], idle[3 * k // 4], idle[-1]))))]
    return [(True, {})] + [(False, {r: C - 1}) for r in RECIPES]


_tonegen_input = {}


def tonegen_input(C, n, clip_channel):
    """the bank's random input with full scale on the clipping channel; one array per shape, left unchanged"""
    key = (C, n, clip_channel)
    if key not in _tonegen_input:
        x = tg.reference(C, n, 12)
        if clip_channel is not None:
            x = x.copy()
            x[clip_channel] = 32767
            x.setflags(write=False)
        _tonegen_input[key] = x
    return _tonegen_input[key]


@pytest.mark.parametrize("mode", ["gen", "out", "in_place"])
@pytest.mark.parametrize("C,n_blocks,gy", ls.TONEGEN_SHAPES)
def test_tonegen_several_tiles_per_workgroup(torch_dev, C, n_blocks, gy, mode):
    """Every shape has more tiles than the grid has workgroups per row, so workgroup (c, 0) walks the tiles 0, gy, ..: the
    dispatch is restated and asserted.  scatter's random queues plus the explicit ones of queue_recipe; the mode once with
    `active`, once (the clock moved back to 0) without, then a second call over what is still queued.  Out, active, the
    guards, clips, time and pending are the model's (run_device, same_state)."""
    tiles, want = -(-n_blocks // 4), -(-2048 // C)
    assert min(tiles, 64, want) == gy and tiles > gy, "the library's dispatch moved: this shape no longer has a second tile"
    assert (tiles, want, gy) == ls.tonegen_dispatch(C, n_blocks) and ls.tonegen_tiles_of(C, n_blocks, 0)[:2] == [0, gy]
    n, b = 512 * n_blocks, gy * TILE
    st = tg.steps(8, 1000 + C)
    for i, (scattered, where) in enumerate(recipe_passes(C)):
        d, m = tg.both(C)
        if scattered:
            tg.scatter((d, m), C, n, 7 * C + n_blocks)
        for r, c in where.items():
            queue_recipe((d, m), c, r, b, st)
        clip_c = where.get("clip")
        pcm = tonegen_input(C, n, clip_c)
        what = f"C={C} x {n_blocks} blocks, {mode}, pass {i}"
        out, act = tg.run_device(torch_dev, d, m, pcm, n_blocks, what + ", with active", mode, 2, 6, 2, want_active=True)
        if "second" in where:
            assert set(np.flatnonzero(act[where["second"]]) // 4) == {gy}, "the segment lies in the second tile alone"
        if "first" in where:
            assert set(np.flatnonzero(act[where["first"]]) // 4) == {0}
        if "span" in where:
            assert act[where["span"], 3] == 1 and act[where["span"], 4 * gy] == 1
        once = m.clips(clip_c) if clip_c is not None else 0
        if clip_c is not None:
            flat = np.abs(out[clip_c].reshape(-1).astype(np.int64))
            assert flat[:TILE].max() >= 32767 and flat[b:b + 512].max() >= 32767, "the model saturates in both tiles"
        for h in (d, m):
            h.set_time(0)
        tg.run_device(torch_dev, d, m, pcm, n_blocks, what + ", without active", mode, 10, 0, 16, want_active=False)
        if clip_c is not None:
            assert d.clips(clip_c) == m.clips(clip_c) == 2 * once and once > 0, "the channel under full amplitude clips in both tiles"
        _, act = tg.run_device(torch_dev, d, m, pcm, n_blocks, what + ", the second call", mode, 6, 2, 6, want_active=True)
        if "forever" in where:
            assert (act[where["forever"]] & 2).all()


# ================================================================ B. the tone generator: staging in several uploads
def test_tonegen_staging_in_several_uploads(torch_dev):
    """2049 channels, every channel's queue a function of c.  Four calls without a host synchronisation, alternating between
    two streams, each into its own output: (1) the create-time dirty range goes up as 1024 + 1024 + 1 channels; (2) queues on
    1023, 1024 and 1025 only: one upload that starts at dirty_lo = 1023; (3) queues on 0 and 2048: the whole bank again, in
    three uploads through the one pinned buffer while the call before may still run; (4) cut(ALL).  No segment ends inside
    the four calls, so no call widens the dirty range by dropping one."""
    torch, dev = torch_dev
    C, n_blocks = 2049, 5
    n = 512 * n_blocks
    assert ls.tonegen_uploads(0, C) == [(0, 1024), (1024, 1024), (2048, 1)] and ls.tonegen_uploads(1023, 1026) == [(1023, 3)]
    d, m = tg.both(C)

    def step(c, k):
        return (c * 2654435761 + k * 40503 + 12345) & MASK32

    for c in range(C):
        s = [tg.seg(30000 + c, step(c, 0), 1000 + (c * 13) % 30000, step(c, 1), (c * 29) % 20000)]
        for h in (d, m):
            h.queue(c, 0, s, c % 500)
    pcm = tg.reference(C, n, 13)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 4
    d_out = torch.zeros((calls, C, n_blocks, 512), dtype=torch.int16, device=dev)
    d_act = torch.zeros((calls, C, n_blocks), dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        d.process_device(d_pcm.data_ptr(), 1024 * n_blocks, n_blocks, d_out[i].data_ptr(), 0, d_act[i].data_ptr(),
                         streams[i % 2].cuda_stream)
        want.append(m.process(pcm, n_blocks, want_active=True))
        for h in (d, m):
            if i == 0:
                for c in (1023, 1024, 1025):
                    h.queue(c, 1, [tg.seg(40000, step(c, 2), 15000 + c)], h.time() + 100 + c % 7)
            elif i == 1:
                for c in (0, 2048):
                    h.queue(c, 1, [tg.seg(40000, step(c, 3), 9000 + c)], h.time() + 50 + c % 5)
            elif i == 2:
                h.cut(ALL)
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        equal(d_out[i].cpu().numpy(), want[i][0], f"call {i}: out")
        equal(d_act[i].cpu().numpy(), want[i][1], f"call {i}: active")
    assert want[1][1][1024].tolist() == [3] * n_blocks and want[1][1][1026].tolist() == [1] * n_blocks
    assert want[2][1][2048].tolist() == [3] * n_blocks and (want[3][1][:, 1:] & 1).max() == 0      # cut: track 0 is silent behind 64 samples
    tg.same_state(d, m, "behind the four calls")


# ================================================================ C. the conditioner: past the widening
MEASURE, BOTH = tc.MEASURE, tc.BOTH
CAL_CHUNK = 8 << 20
CAL_PATTERNS = ((-128, -128), (-128, 127))         # the second: S_IQ and S_I negative, S_Q positive
_cal_chunked = {}


def cal_closed_form(n_bytes, I, Q):
    N = n_bytes // 2
    return [N, I * N, Q * N, I * I * N, Q * Q * N, I * Q * N, 0, 0]


def cal_chunked(n_bytes, I, Q):
    """cal_model's moments over the row in chunks of at most 8 MiB, summed with api.cal_sum (the whole row as int64 would
    take a gigabyte); the row is constant, so chunks of one length are one array"""
    key = (n_bytes, I, Q)
    if key not in _cal_chunked:
        chunk = np.empty(CAL_CHUNK, dtype=np.int8)
        chunk[0::2], chunk[1::2] = I, Q
        of_length = {}
        moms = []
        for o in range(0, n_bytes, CAL_CHUNK):
            k = min(CAL_CHUNK, n_bytes - o)
            if k not in of_length:
                of_length[k] = cm.moments(chunk[:k])
            moms.append(of_length[k])
        _cal_chunked[key] = [int(v) for v in api.cal_sum(moms)]
    return _cal_chunked[key]


def cal_past_widening(torch_dev, wgs):
    from tests.hooks import HOOKS_ON
    if not HOOKS_ON:
        pytest.skip("debug_set_workgroups needs HRFD_DEBUG_HOOKS=1 (this run is the shipped state)")
    torch, dev = torch_dev
    n, res = ls.CAL_PAST_WIDENING_BYTES, ls.CAL_PAST_WIDENING_RESIDUE
    d = api.Conditioner(1, device=0)                       # the identity record
    d.debug_set_workgroups(wgs)
    buf = torch.empty(tc.GUARD + 16 + n + tc.GUARD, dtype=torch.int8, device=dev)
    off = tc.GUARD + (res - (buf.data_ptr() + tc.GUARD)) % 16
    guards = np.random.default_rng(wgs).integers(-128, 128, size=buf.numel() - n, dtype=np.int8)
    buf[:off].copy_(torch.from_numpy(guards[:off]))
    buf[off + n:].copy_(torch.from_numpy(guards[off:]))
    row = buf[off:off + n]
    assert row.data_ptr() % 16 == res
    pairs = row.view(-1, 2)
    d_mom = torch.empty((1, 8), dtype=torch.int64, device=dev)
    for I, Q in CAL_PATTERNS:
        pairs[:, 0], pairs[:, 1] = I, Q
        want = cal_closed_form(n, I, Q)
        assert want == cal_chunked(n, I, Q)
        for mode in (MEASURE, BOTH):
            d_mom.fill_(-7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d.process_device(row.data_ptr(), n, n, row.data_ptr() if mode == BOTH else None, n, d_mom.data_ptr())
            torch.cuda.synchronize()
            print(f"k_cal over {n} bytes in {wgs} workgroups, mode {mode}: {1e3 * (time.perf_counter() - t0):.1f} ms")
            got = [int(v) for v in d_mom.cpu().numpy()[0]]
            assert got == want, (f"({I}, {Q}) in {wgs} workgroups, mode {mode}", got, want)
            # the output under the identity is the input; MEASURE alone writes nothing
            assert bool((pairs[:, 0] == I).all()) and bool((pairs[:, 1] == Q).all()), f"({I}, {Q}) mode {mode}: the row changed"
            assert (buf[:off].cpu().numpy() == guards[:off]).all() and (buf[off + n:].cpu().numpy() == guards[off:]).all()


def test_cal_one_workgroup_past_the_widening(torch_dev):
    """W = 1 under debug_set_workgroups(1): 132 MiB + 10 at residue 6 (a head of 5 samples in front of 132 MiB of whole
    groups, which end with the row) is, by cal_launch's arithmetic, one workgroup of 33792 x 256 groups and 8448 steps per
    lane: four widenings inside the loop and a remainder of 256 steps.  Without the widening the signed partials would wrap
    behind 4096 steps and the unsigned ones behind 8192; a widening that never reset `steps` would wrap behind 2048 + 4096.
    Both patterns in MEASURE and in APPLY + MEASURE in place under the identity; the moments against the closed form in
    Python integers and against cal_model in chunks of 8 MiB.  Measured on an MI355X: the one workgroup takes 6.1 ms over
    the 132 MiB in MEASURE and 22 ms in APPLY + MEASURE, the whole test 0.4 s (most of it the model's chunks), so nothing
    of the issue's list was cut."""
    n, res = ls.CAL_PAST_WIDENING_BYTES, ls.CAL_PAST_WIDENING_RESIDUE
    assert n == 132 * (1 << 20) + 10 and ls.cal_row(n, res) == (10, 132 * (1 << 20) // 16, 0)
    assert ls.cal_dispatch(n, 1, 1) == (33792 * 256, 1) and ls.cal_steps(n, res, 1, 1) == [8448]
    assert 8448 // ls.CAL_WIDEN == 4 and 8448 > 8192 and 8448 > ls.CAL_WIDEN + 4096
    cal_past_widening(torch_dev, 1)


def test_cal_three_workgroups_past_the_widening(torch_dev):
    """the same bytes under debug_set_workgroups(3): three workgroups of 11264 x 256 groups, 2816 steps per lane each (one
    widening inside the loop and 768 steps behind it), their totals added into the zeroed row by 64-bit atomics"""
    n, res = ls.CAL_PAST_WIDENING_BYTES, ls.CAL_PAST_WIDENING_RESIDUE
    assert ls.cal_dispatch(n, 1, 3) == (11264 * 256, 3) and ls.cal_steps(n, res, 1, 3) == [2816] * 3
    assert 2816 // ls.CAL_WIDEN == 1
    cal_past_widening(torch_dev, 3)


# ================================================================ D. rows more than 4 GiB apart
FAR = 1 << 32
SENTINEL = 4096
FRONT = 64


class TwoRows:
    """Two rows of row_bytes in one allocation that is never filled: FRONT random bytes in front of each row and SENTINEL
    behind it are written, and the rows themselves.  Far: the rows lie 2^32 + row_bytes + 64 bytes apart (rounded up to 16),
    so the sentinel behind row 0 is where a stride truncated to 32 bits would put row 1.  Dense: the rows touch."""

    def __init__(self, torch_dev, row_bytes, seed, data, far):
        torch, dev = torch_dev
        self.torch, self.n, self.far = torch, row_bytes, far
        self.stride = (FAR + row_bytes + 64 + 15) // 16 * 16 if far else row_bytes
        rng = np.random.default_rng(seed)                   # the same bytes far and dense
        self.front = rng.integers(0, 256, size=(2, FRONT), dtype=np.uint8)
        self.behind = rng.integers(0, 256, size=(2, SENTINEL), dtype=np.uint8)
        rows = rng.integers(0, 256, size=(2, row_bytes), dtype=np.uint8)
        if data is not None:
            rows = np.ascontiguousarray(data).view(np.uint8).reshape(2, row_bytes).copy()
        self.rows = rows
        try:
            self.buf = torch.empty(FRONT + 16 + self.stride + row_bytes + SENTINEL, dtype=torch.uint8, device=dev)
        except torch.cuda.OutOfMemoryError:
            pytest.skip(f"no room for {self.stride + row_bytes} bytes on the device")
        self.off = FRONT + (-(self.buf.data_ptr() + FRONT)) % 16
        self.ptr = self.buf.data_ptr() + self.off
        for o, piece in self._pieces():
            self.buf[o:o + piece.size].copy_(torch.from_numpy(piece))

    def _pieces(self):
        """[(offset in buf, bytes)] of what is written, as it was written"""
        if self.far:
            return [(self.off + w * self.stride - FRONT, np.concatenate([self.front[w], self.rows[w], self.behind[w]])) for w in range(2)]
        return [(self.off - FRONT, np.concatenate([self.front[0], self.rows[0], self.rows[1], self.behind[1]]))]

    def check(self, what, unchanged=False):
        """the two rows as they are now; everything around them must be as written, and the rows too if `unchanged`"""
        got = []
        for o, piece in self._pieces():
            now = self.buf[o:o + piece.size].cpu().numpy()
            for r in range((piece.size - FRONT - SENTINEL) // self.n):
                a = FRONT + r * self.n
                got.append(now[a:a + self.n].copy())
                now[a:a + self.n] = piece[a:a + self.n]
            assert (now == piece).all(), f"{what}: bytes around a row changed at {np.flatnonzero(now != piece)[:5].tolist()} (far: {self.far})"
        got = np.stack(got)
        if unchanged:
            assert (got == self.rows).all(), f"{what}: the rows changed"
        return got


def far_rows(torch_dev, row_bytes, seed, data=None, far=True):
    return TwoRows(torch_dev, row_bytes, seed, data, far)


def zeros(torch_dev, shape, dtype):
    torch, dev = torch_dev
    return torch.zeros(shape, dtype=getattr(torch, dtype), device=dev)


def release(torch_dev):
    gc.collect()
    torch_dev[0].cuda.empty_cache()


@pytest.fixture
def big(torch_dev):
    """at most two of the 4 GiB allocations live at once: whatever a test held goes back to the device behind it"""
    yield
    release(torch_dev)


def far_equals_dense(torch_dev, call, what):
    """call(far) makes a handle and the call, checks its sentinels and returns {name: array}"""
    far = call(True)
    release(torch_dev)
    dense = call(False)
    release(torch_dev)
    assert far.keys() == dense.keys()
    for k in far:
        equal(far[k], dense[k], f"{what}: {k} with far rows against dense rows")
    return far


def host(*tensors):
    return [t.cpu().numpy() for t in tensors]


FAR_TONE_STEPS = [tm.tone_step(f) for f in (67.0, 697.0, 1000.0, 1633.0, 3999.0)]


def test_far_rows_tones(torch_dev, big):
    pcm = tt.reference(2, 512, 31)

    def call(far):
        torch = torch_dev[0]
        d = api.Tones(2, 128, device=0)
        d.set_tones(steps=FAR_TONE_STEPS, groups=[0, 1, 2, 3, 0])
        d.set_threshold(ALL, ratio_q8=1 << 10, min_energy=0)
        src = far_rows(torch_dev, 1024, 41, pcm, far)
        outs = [zeros(torch_dev, (2, 4, 5), "int64"), zeros(torch_dev, (2, 4), "int64"), zeros(torch_dev, (2, 4), "int32"),
                zeros(torch_dev, (2, 4, 4), "uint8"), zeros(torch_dev, (2, 4, 4), "uint8")]
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, None, 1, *[t.data_ptr() for t in outs])
        torch.cuda.synchronize()
        src.check("the input", unchanged=True)
        return dict(zip(tt.OUTPUTS, host(*outs)))

    got = far_equals_dense(torch_dev, call, "Tones")
    assert (got["power"][0] != got["power"][1]).any() and got["power"][1].any()


def test_far_rows_audio(torch_dev, big):
    pcm = ta.reference(2, 512, 32)

    def call(far):
        torch = torch_dev[0]
        d = api.Audio(2, 1, device=0)
        d.set_taps(ta.random_taps(64, 5))
        d.set_bus(0, [0, 1], [4096, -3000])
        src, out = far_rows(torch_dev, 1024, 42, pcm, far), far_rows(torch_dev, 1024, 43, None, far)
        mix, clips = zeros(torch_dev, (2, 1, 512), "int16"), zeros(torch_dev, (2, 1), "int32")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, None, None, 1, out.ptr, out.stride, mix[0].data_ptr(), clips[0].data_ptr())
        d.process_device(src.ptr, src.stride, None, None, 1, None, 0, mix[1].data_ptr(), clips[1].data_ptr())      # mix only
        torch.cuda.synchronize()
        src.check("the input", unchanged=True)
        return dict(zip(("out", "mix", "clips"), [out.check("out")] + host(mix, clips)))

    got = far_equals_dense(torch_dev, call, "Audio")
    assert (got["out"][0] != got["out"][1]).any() and got["out"][1].any() and got["mix"][1].any()


def test_far_rows_resampler(torch_dev, big):
    pcm = tr.reference(2, 512, 33)

    def call(far):
        torch = torch_dev[0]
        d = api.Resampler(2, 3, 2, device=0)
        d.set_taps(tr.random_taps(3 * 34, 3, 9))
        cap = d.out_count(512)
        assert cap == 768
        src, out = far_rows(torch_dev, 1024, 44, pcm, far), far_rows(torch_dev, 2 * cap, 45, None, far)
        torch.cuda.synchronize()
        n_out = d.process_device(src.ptr, src.stride, None, 512, out.ptr, out.stride, cap)
        torch.cuda.synchronize()
        assert n_out == cap
        src.check("the input", unchanged=True)
        return {"out": out.check("out")}

    got = far_equals_dense(torch_dev, call, "Resampler")
    assert (got["out"][0] != got["out"][1]).any() and got["out"][1].any()


def leveler():
    d = api.Leveler(2, device=0)
    d.set(20000, 40, 0)
    d.set(9000, 100, 1)
    return d


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_far_rows_leveler(torch_dev, big, in_place):
    pcm = tl.reference(2, 512, 34)

    def call(far):
        torch = torch_dev[0]
        d = leveler()
        src = far_rows(torch_dev, 1024, 46, pcm, far)
        out = src if in_place else far_rows(torch_dev, 1024, 47, None, far)
        gain, peak = zeros(torch_dev, (2, 8), "int32"), zeros(torch_dev, (2, 8), "int16")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, None, 1, out.ptr, out.stride, gain.data_ptr(), peak.data_ptr())
        torch.cuda.synchronize()
        if not in_place:
            src.check("the input", unchanged=True)
        return dict(zip(("out", "gain", "peak"), [out.check("out")] + host(gain, peak)))

    got = far_equals_dense(torch_dev, call, "Leveler")
    assert (got["out"][0] != got["out"][1]).any() and got["out"][1].any() and (got["out"] != pcm.view(np.uint8)).any()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_far_rows_tonegen(torch_dev, big, in_place):
    """one tile (4 blocks) per row; channel 1 has queues of its own on both tracks"""
    pcm = tg.reference(2, 2048, 35)
    st = tg.steps(5, 36)

    def call(far):
        torch = torch_dev[0]
        d = api.ToneGen(2, device=0)
        d.queue(0, 0, [tg.seg(1500, st[0], 20000, st[1], 9000)], 100)
        d.queue(1, 1, [tg.seg(FOREVER, st[2], 32767)], 300)
        d.queue(1, 0, [tg.seg(700, st[3], 32767, st[4], 32767)], 1200)
        src = far_rows(torch_dev, 4096, 48, pcm, far)
        out = src if in_place else far_rows(torch_dev, 4096, 49, None, far)
        act = zeros(torch_dev, (2, 4), "uint8")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, 4, out.ptr, out.stride, act.data_ptr())
        torch.cuda.synchronize()
        if not in_place:
            src.check("the input", unchanged=True)
        return {"out": out.check("out"), "active": host(act)[0], "clips": np.array([d.clips(0), d.clips(1)])}

    got = far_equals_dense(torch_dev, call, "ToneGen")
    assert got["active"].tolist() == [[1, 1, 1, 1], [2, 2, 3, 3]] and got["clips"][1] > 0
    assert (got["out"][1] != pcm[1].view(np.uint8)).any()


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place_with_moments", "in_place"])
def test_far_rows_conditioner(torch_dev, big, in_place):
    n = 4098
    cap = tc.reference(2, n, seed=6)

    def call(far):
        torch = torch_dev[0]
        d, _ = tc.both(2, first_record=2)
        src = far_rows(torch_dev, n, 50, cap, far)
        out = src if in_place else far_rows(torch_dev, n, 51, None, far)
        mom = zeros(torch_dev, (2, 8), "int64")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, n, out.ptr, out.stride, None if in_place else mom.data_ptr())
        torch.cuda.synchronize()
        if not in_place:
            src.check("the input", unchanged=True)
        return {"out": out.check("out"), "moments": host(mom)[0]}

    got = far_equals_dense(torch_dev, call, "Conditioner")
    assert (got["out"][1] != cap[1].view(np.uint8)).any()
    if not in_place:
        equal(got["moments"][1, :6], cm.moments(cap[1])[:6], "the moments of the far row")


def test_far_rows_spectrum(torch_dev, big):
    cap = tc.reference(2, 512, seed=7)

    def call(far):
        torch = torch_dev[0]
        d = api.Spectrum(2, 2, 8, device=0)
        src = far_rows(torch_dev, 512, 52, cap, far)
        power = zeros(torch_dev, (2, 256), "int64")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, 1, power.data_ptr())
        torch.cuda.synchronize()
        src.check("the captures", unchanged=True)
        return {"power": host(power)[0]}

    got = far_equals_dense(torch_dev, call, "Spectrum")
    assert (got["power"][0] != got["power"][1]).any() and got["power"][1].any()


def test_far_rows_ddc(torch_dev, big):
    """channel 0 tuned to capture 0, channel 1 to capture 1: both the far capture and the far output row are used"""
    R, ob = 2, 512
    cap = tc.reference(2, R * ob, seed=8)

    def call(far):
        torch = torch_dev[0]
        d = api.Ddc(2, 2, R, device=0)
        d.set_step(0, 0, 0x12345678)
        d.set_step(1, 1, 0xC0000000)
        d.set_gain_shift(3)
        src, out = far_rows(torch_dev, R * ob, 53, cap, far), far_rows(torch_dev, ob, 54, None, far)
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, ob, out.ptr, out.stride)
        torch.cuda.synchronize()
        src.check("the captures", unchanged=True)
        return {"out": out.check("out")}

    got = far_equals_dense(torch_dev, call, "Ddc")
    assert (got["out"][0] != got["out"][1]).any() and got["out"][1].any()


def test_far_rows_duc(torch_dev, big):
    """channel 0 into capture 0, channel 1 into capture 1"""
    R, ib = 2, 512
    x = tc.reference(2, ib, seed=9)

    def call(far):
        torch = torch_dev[0]
        d = api.Duc(2, 2, R, device=0)
        d.set_step(0, 0, 0x12345678)
        d.set_step(1, 1, 0xC0000000)
        src, out = far_rows(torch_dev, ib, 55, x, far), far_rows(torch_dev, R * ib, 56, None, far)
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, ib, out.ptr, out.stride)
        torch.cuda.synchronize()
        src.check("the channels", unchanged=True)
        return {"out": out.check("captures")}

    got = far_equals_dense(torch_dev, call, "Duc")
    assert (got["out"][0] != got["out"][1]).any() and got["out"][1].any()


# ================================================================ E. the PCM banks past 1024 channels
MANY = 1300
SCATTERED = (0, 1024, 1299)


@pytest.mark.parametrize("L,n_blocks", [(128, 1), (128, 2), (1024, 2)])
def test_many_channels_tones(torch_dev, L, n_blocks):
    """1300 channels.  L = 128 gives 16 frames per workgroup and 325 or 650 whole workgroups (1300 F is a multiple of 16 for
    every F that is a multiple of 4); at L = 1024 over two blocks a channel is one frame, and the 82nd workgroup holds 4"""
    F, FT = 512 * n_blocks // L, min(16, 16384 // L)
    assert (MANY * F) % FT == (0 if L == 128 else 4) and -(-MANY * F // FT) > 64
    d, m = tt.both(MANY, L, FAR_TONE_STEPS + [tm.tone_step(2400.0)], [0, 1, 2, 3, 0, 1])
    pcm = tt.reference(MANY, 512 * n_blocks, 21)
    n_pcm = np.random.default_rng(L + n_blocks).choice(np.array([512, 512, 600, 100, 0], dtype=np.uint32), size=(MANY, n_blocks))
    tt.run_device(torch_dev, d, m, pcm, None, f"L={L} x {n_blocks} blocks", residue=2, pad=6)
    want = tt.run_device(torch_dev, d, m, pcm, n_pcm, f"L={L} x {n_blocks} blocks with n_pcm")
    assert (want["valid"][list(SCATTERED), :] <= L).all() and want["power"][MANY - 1].any()


@pytest.mark.parametrize("T", [63, 64])
def test_many_channels_audio(torch_dev, T):
    """1300 channels x 2 blocks: buses that list channels on both sides of 1024, a `want` per channel behind gate, reset of
    channels 0, 1024 and 1299 between two calls"""
    C, n_blocks, L = MANY, 2, 256
    buses = [([0, 1023, 1024, 1299], [4096, -3000, 2500, 32767]), ([1299, 1024, 0], [4096, 4096, -4096])]
    d, m = ta.both(C, 2, ta.random_taps(T, 60 + T), buses)
    for c in range(C):
        w = (0, 1, 2, 3, 4, api.AUDIO_ANY_TONE, api.AUDIO_NO_TONE)[c % 7]
        for h in (d, m):
            h.set_want(w, c)
    rng = np.random.default_rng(T)
    opens = []
    for call in range(2):
        best = rng.integers(0, 5, size=(C, 512 * n_blocks // L, 4), dtype=np.uint8)
        present = rng.integers(0, 2, size=best.shape, dtype=np.uint8)
        want = m.gate(best, present, L, 1)
        equal(d.gate(best, present, L, 1), want, f"gate, call {call}")
        assert 0 < int(want.sum()) < want.size and (want[6::7] == 1).all()
        opens.append(want)
    n_pcm = rng.choice(np.array([512, 512, 600, 100, 0], dtype=np.uint32), size=(C, n_blocks))
    first = ta.run_device(torch_dev, d, m, ta.reference(C, 512 * n_blocks, 22), n_pcm, opens[0], f"T={T}", residue=2, pad=6, out_pad=2)
    assert first["mix"][0].any() and first["mix"][1].any()
    for c in SCATTERED:
        for h in (d, m):
            h.reset(c)
    ta.run_device(torch_dev, d, m, ta.reference(C, 512 * n_blocks, 23), None, opens[1], f"T={T}, behind the resets", residue=4, pad=2,
                  out_pad=6)


def test_many_channels_resampler(torch_dev):
    """1300 channels at 3 / 2, one block a call, reset of channels 0, 1024 and 1299 between two calls"""
    C = MANY
    d, m = tr.both(C, 3, 2, tr.random_taps(3 * 33 - 1, 3, 71))
    pcm = tr.reference(C, 1024, 24)
    first = tr.run_device(torch_dev, d, m, pcm[:, :512], None, "3/2", residue=2, out_residue=6, pad=6, out_pad=2)
    assert first.shape == (C, 768)
    for c in SCATTERED:
        for h in (d, m):
            h.reset(c)
    n_pcm = np.random.default_rng(24).choice(np.array([512, 600, 100, 0], dtype=np.uint32), size=(C, 1))
    tr.run_device(torch_dev, d, m, pcm[:, 512:], n_pcm, "3/2, behind the resets", spare=3)


def test_many_channels_leveler(torch_dev):
    """1300 channels x 2 blocks, another target and floor on every channel, reset of scattered channels between two calls,
    the second in place"""
    C = MANY
    d, m = tl.both(C, tl.random_weights(7, 3))
    for c in range(C):
        for h in (d, m):
            h.set(1000 + (c * 23) % 31000, 16 + (c * 7) % 3000, c)
    n_pcm = np.random.default_rng(25).choice(np.array([512, 512, 600, 100, 0], dtype=np.uint32), size=(C, 2))
    first = tl.run_device(torch_dev, d, m, tl.bursts(C, 1024, 5), n_pcm, "every channel its own target", residue=2, pad=6, out_pad=2)
    assert len({int(v) for v in first["gain"][:, -1]}) > 100
    for c in (0, 5, 1023, 1024, 1025, 1299):
        for h in (d, m):
            h.reset(c)
    tl.run_device(torch_dev, d, m, tl.bursts(C, 1024, 6), None, "behind the resets, in place", residue=4, pad=2, in_place=True)
