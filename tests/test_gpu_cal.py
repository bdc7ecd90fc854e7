"""The conditioner bank on the device (hrfd_cal_*) against the numpy model (tests/cal_model.py), tolerance 0: every length
at which k_cal takes another path, every residue of input and output, odd strides with guard bytes, in place, the three
modes, records at their limits, sums past 32 bits, setter changes behind running calls, and the closed loop the bank exists
for: inject an impairment -> measure -> hrfd_cal_solve -> apply in place -> Spectrum -> find_stations."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import cal_model as cm
from tests import spec_model as sm

pytestmark = pytest.mark.gpu

APPLY, MEASURE, BOTH = 1, 2, 3
RECORDS = [((588, -436), (16384, 0, -1145, 15495)), ((0, 0), cm.IDENTITY), ((-32512, 32512), (32767, 1, -1, -32767)),
           ((32512, -32512), (-32768, 0, 16384, -16384)), ((100, -100), (16384, 16384, -20000, 12768))]
GUARD = 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(W, first_record=0):
    d, m = api.Conditioner(W, device=0), cm.CalModel(W)
    for w in range(W):
        dc, mat = RECORDS[(first_record + w) % len(RECORDS)]
        d.set_correction(dc, mat, w)
        m.set_correction(dc, mat, w)
    return d, m


_reference = {}


def reference(W, n, seed=3):
    """the captures of one shape, computed once and left unchanged"""
    key = (W, n, seed)
    if key not in _reference:
        cap = sm.lcg_captures(W, max(n, 4096), seed)[:, :n].copy()
        cap.setflags(write=False)
        _reference[key] = cap
    return _reference[key]


class Rows:
    """W rows of n bytes in a device buffer of random bytes, the first row at an address of the given residue modulo 16,
    the rows `stride` apart, GUARD bytes and more before the first and behind the last"""

    def __init__(self, torch_dev, W, n, residue, stride, seed):
        torch, dev = torch_dev
        self.torch, self.W, self.n, self.stride = torch, W, n, stride
        size = GUARD + 16 + stride * (W - 1) + n + GUARD
        self.host = np.random.default_rng(seed).integers(-128, 128, size=size, dtype=np.int8)
        self.dev = torch.from_numpy(self.host).to(dev)
        self.off = GUARD + (residue - (self.dev.data_ptr() + GUARD)) % 16
        self.ptr = self.dev.data_ptr() + self.off
        assert self.ptr % 16 == residue

    def put(self, cap):
        for w in range(self.W):
            o = self.off + w * self.stride
            self.host[o:o + self.n] = cap[w]
        self.dev.copy_(self.torch.from_numpy(self.host))

    def expect(self, rows):
        """the buffer as it must look when only the rows have changed"""
        want = self.host.copy()
        if rows is not None:
            for w in range(self.W):
                o = self.off + w * self.stride
                want[o:o + self.n] = rows[w]
        return want

    def check(self, rows, what):
        got = self.dev.cpu().numpy()
        want = self.expect(rows)
        assert (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:5].ravel()} (rows start at {self.off})"


def run_case(torch_dev, d, m, cap, mode, in_res, out_res, in_pad, out_pad, what, in_place=False):
    torch, dev = torch_dev
    W, n = cap.shape
    src = Rows(torch_dev, W, n, in_res, n + in_pad, 11)
    src.put(cap)
    dst = src if in_place else Rows(torch_dev, W, n, out_res, n + out_pad, 12)
    d_mom = torch.full((W, 8), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    d.process_device(src.ptr, src.stride, n, dst.ptr if mode & APPLY else None, dst.stride,
                     d_mom.data_ptr() if mode & MEASURE else None)
    torch.cuda.synchronize()
    want_out, want_mom = m.process(cap, bool(mode & APPLY), bool(mode & MEASURE))
    if in_place:
        src.check(want_out, what + " (in place)")
    else:
        src.check(None, what + ": the input")
        dst.check(want_out if mode & APPLY else None, what + ": the output")
    got_mom = d_mom.cpu().numpy()
    if mode & MEASURE:
        assert (got_mom == want_mom).all(), (what, got_mom, want_mom)
    else:
        assert (got_mom == -7).all(), what
    return want_mom


# 1. every length at which the kernel takes another path x W x the three modes: below one group, exactly one, head and tail
#    around whole groups, several workgroups per capture (the atomics), and a megabyte
@pytest.mark.parametrize("n", [2, 14, 16, 18, 4094, 4098, 65542, 1048586])
@pytest.mark.parametrize("W", [1, 3])
def test_lengths_and_modes(torch_dev, n, W):
    d, m = both(W)
    cap = reference(W, n)
    for mode, (in_res, out_res, in_pad, out_pad) in ((APPLY, (0, 0, 0, 0)), (MEASURE, (6, 0, 3, 0)), (BOTH, (10, 4, 5, 7)),
                                                     (BOTH, (3, 3, 1, 9))):
        run_case(torch_dev, d, m, cap, mode, in_res, out_res, in_pad, out_pad, f"n={n} W={W} mode={mode} residues {in_res},{out_res}")


# 2. every residue of the input against every residue of the output, odd strides, guard bytes around every row
@pytest.mark.parametrize("in_res", range(16))
def test_every_pair_of_residues(torch_dev, in_res):
    d, m = both(2, first_record=in_res)
    cap = reference(2, 274)
    for out_res in range(16):
        run_case(torch_dev, d, m, cap, BOTH if out_res & 1 else APPLY, in_res, out_res, 1 + 2 * (in_res % 3), 3 + 2 * (out_res % 4),
                 f"residues {in_res},{out_res}")


@pytest.mark.parametrize("n", [18, 4098, 65542])
def test_in_place(torch_dev, n):
    d, m = both(3, first_record=1)
    cap = reference(3, n, seed=4)
    for res in range(16):
        run_case(torch_dev, d, m, cap, BOTH if res % 3 else APPLY, res, res, 1 + res % 5, 0, f"n={n} residue {res}", in_place=True)


# 3. records at their limits and a matrix that clips, through the host path as well
def test_limits_and_clips():
    alt = np.empty(4096, dtype=np.int8)
    alt[0::4], alt[1::4], alt[2::4], alt[3::4] = 127, -128, -128, 127
    cap = np.stack([sm.lcg_captures(1, 4096, 9)[0], np.full(4096, -128, dtype=np.int8), np.full(4096, 127, dtype=np.int8), alt])
    d, m = api.Conditioner(4, device=0), cm.CalModel(4)
    for dc, mat in (((0, 0), (32767, 1, -1, -32767)), ((0, 0), (-32768, 0, 0, -32768)), ((32512, -32512), (16384, 16384, -16384, -16384)),
                    ((-32512, 32512), (1, 32767, 32767, -1)), ((32512, 32512), cm.IDENTITY), ((-32512, -32512), (32767, 1, 1, 32767))):
        d.set_correction(dc, mat)
        m.set_correction(dc, mat)
        for w in range(4):
            got_dc, got_m = d.correction(w)
            assert tuple(got_dc) == dc and tuple(got_m) == mat
        out, mom = d.process(cap)
        want_out, want_mom = m.process(cap)
        assert (out == want_out).all() and (mom == want_mom).all(), (dc, mat)
        assert mom[:, 6].sum() > 0 and (mom[:, 6] == want_mom[:, 6]).all(), "a record at its limit clips on these inputs"
    d.set_correction(None, None, 2)                        # one capture back to the identity
    m.set_correction(None, None, 2)
    out, none = d.process(cap, want_moments=False)
    assert none is None and (out == m.process(cap)[0]).all() and (out[2] == cap[2]).all()
    none, mom = d.process(cap, want_out=False)
    assert none is None and (mom == m.process(cap, want_out=False)[1]).all() and (mom[:, 6] == 0).all()


# 4. sums past 32 bits: a MiB of -128 has S_II = S_QQ = S_IQ = 2^33
def test_sums_past_32_bits(torch_dev):
    d, m = both(1, first_record=1)
    cap = np.full((1, 1 << 20), -128, dtype=np.int8)
    for mode in (MEASURE, BOTH):
        mom = run_case(torch_dev, d, m, cap, mode, 2, 2, 0, 0, f"1 MiB of -128, mode {mode}")
        assert [int(v) for v in mom[0]] == [1 << 19, -(1 << 26), -(1 << 26), 1 << 33, 1 << 33, 1 << 33, 0, 0]


# 5. the records of a call are those set before it, whatever still runs: ten calls with a setter change before each behind
#    one large call, then calls that alternate between two streams and read what the call before wrote
def test_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    W, n, big = 2, 65542, 1 << 25
    d, m = both(W)
    cap = reference(W, n, seed=5)
    d_big = torch.zeros((W, big), dtype=torch.int8, device=dev)
    d_in = torch.from_numpy(cap.copy()).to(dev)
    d_out = torch.zeros((10, W, n), dtype=torch.int8, device=dev)
    d_mom = torch.zeros((10, W, 8), dtype=torch.int64, device=dev)
    want = []
    torch.cuda.synchronize()
    d.process_device(d_big.data_ptr(), big, big, d_big.data_ptr(), big)
    for k in range(10):
        dc, mat = RECORDS[k % len(RECORDS)]
        dc = (dc[0] // 2 + k, dc[1] // 2 - k)
        d.set_correction(dc, mat, k % W)
        m.set_correction(dc, mat, k % W)
        d.process_device(d_in.data_ptr(), n, n, d_out[k].data_ptr(), n, d_mom[k].data_ptr())
        want.append(m.process(cap))
    torch.cuda.synchronize()
    got_out, got_mom = d_out.cpu().numpy(), d_mom.cpu().numpy()
    for k in range(10):
        assert (got_out[k] == want[k][0]).all() and (got_mom[k] == want[k][1]).all(), f"call {k}"
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    d_chain = torch.zeros((9, W, n), dtype=torch.int8, device=dev)
    d_chain[0].copy_(d_in)
    torch.cuda.synchronize()
    x = cap
    for k in range(1, 9):
        dc, mat = RECORDS[(k + 1) % len(RECORDS)]
        d.set_correction(dc, mat, k % W)
        m.set_correction(dc, mat, k % W)
        d.process_device(d_chain[k - 1].data_ptr(), n, n, d_chain[k].data_ptr(), n, None, streams[k & 1].cuda_stream)
        x = m.process(x, want_moments=False)[0]
    for s in streams:
        s.synchronize()
    assert (d_chain[8].cpu().numpy() == x).all(), "a call on another stream ran before the one it follows"


# 6. what needs a handle to be refused
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    d = api.Conditioner(3, device=0)
    buf = torch.zeros(4096, dtype=torch.int8, device=dev)
    mom = torch.zeros((3, 8), dtype=torch.int64, device=dev)
    p = buf.data_ptr()
    with pytest.raises(api.HrfdError, match="hrfd_cal_set_correction"):
        d.set_correction((0, 0), cm.IDENTITY, 3)
    with pytest.raises(api.HrfdError, match="hrfd_cal_get_correction"):
        d.correction(3)
    with pytest.raises(api.HrfdError, match="32769"):
        d.set_correction((0, 0), (16384, 0, 32767, 2), 0)
    with pytest.raises(api.HrfdError, match="in place"):
        d.process_device(p, 64, 32, p, 96)
    with pytest.raises(api.HrfdError, match="overlaps"):
        d.process_device(p, 64, 32, p + 16, 64)
    with pytest.raises(api.HrfdError, match="overlaps"):
        d.process_device(p + 100, 64, 32, p, 64)
    with pytest.raises(api.HrfdError, match="neither"):
        d.process_device(p, 64, 32, None, 0, None)
    dc, m = d.correction(0)
    assert tuple(dc) == (0, 0) and tuple(m) == cm.IDENTITY
    d.process_device(p, 64, 32, p, 64, mom.data_ptr())   # the handle still works
    torch.cuda.synchronize()
    assert (mom.cpu().numpy()[:, 0] == 16).all()


# 7. the closed loop on the device
def test_closed_loop_inject_measure_solve_apply_survey(torch_dev):
    """The recipe's clean capture through a conditioner set to the impairment, then a second conditioner: measure only, host
    solve, set, apply in place, Spectrum, find_stations.  The uncorrected survey holds the two stations, the spur at 0 Hz and
    the strong station's image; the corrected one exactly the two stations."""
    torch, dev = torch_dev
    R, L, F = cm.RECIPE_R, cm.RECIPE_L, cm.RECIPE_FRAMES
    clean = cm.recipe_clean()
    n = clean.size
    dc_inj, m_inj = cm.recipe_injection()
    want_imp, want_clips = cm.apply(clean, dc_inj, m_inj)
    d_cap = torch.from_numpy(clean[None, :]).to(dev)
    d_mom = torch.zeros((1, 8), dtype=torch.int64, device=dev)
    d_power = torch.zeros((1, 1 << L), dtype=torch.int64, device=dev)
    inject, fix = api.Conditioner(1, device=0), api.Conditioner(1, device=0)
    spec = api.Spectrum(1, R, L, device=0)
    inject.set_correction(dc_inj, m_inj)
    torch.cuda.synchronize()
    inject.process_device(d_cap.data_ptr(), n, n, d_cap.data_ptr(), n, d_mom.data_ptr())
    torch.cuda.synchronize()
    assert (d_cap.cpu().numpy()[0] == want_imp).all() and int(d_mom[0, 6]) == want_clips == 0

    def survey():
        spec.process_device(d_cap.data_ptr(), n, F, d_power.data_ptr())
        torch.cuda.synchronize()
        return api.find_stations(d_power.cpu().numpy().view(np.uint64), F, R, L, 200e3, 100e3, 10.0)

    raw = survey()
    fix.process_device(d_cap.data_ptr(), n, n, None, 0, d_mom.data_ptr())
    torch.cuda.synchronize()
    mom = d_mom.cpu().numpy()
    assert (mom[0] == cm.moments(want_imp)).all()
    dc, m, solved = api.cal_solve(api.cal_sum([mom])[0])
    assert solved and (list(dc), list(m)) == cm.solve(mom[0])[:2]
    fix.set_correction(dc, m)
    fix.process_device(d_cap.data_ptr(), n, n, d_cap.data_ptr(), n, d_mom.data_ptr())
    torch.cuda.synchronize()
    want_out, want_clips = cm.apply(want_imp, dc, m)
    assert (d_cap.cpu().numpy()[0] == want_out).all() and int(d_mom[0, 6]) == want_clips
    corrected = survey()
    print("solved", dc, m, "raw", raw, "corrected", corrected)
    assert len(raw) > 2, raw
    assert len(corrected) == 2, corrected
    for (w, off, _), want in zip(corrected, cm.RECIPE_OFFSETS_HZ):
        assert w == 0 and abs(off - want) <= 100e3, (off, want)


# 8. one workgroup per capture (the hook): wave and workgroup totals pass 32 bits before anything reaches the row, which is
#    then written by the plain store; and 3 workgroups for the same bytes, each with several steps of its own
def test_one_workgroup_sums_past_32_bits(torch_dev):
    from tests.hooks import HOOKS_ON
    if not HOOKS_ON:
        pytest.skip("debug_set_workgroups needs HRFD_DEBUG_HOOKS=1 (this run is the shipped state)")
    d, m = both(1, first_record=1)
    cap = np.full((1, (1 << 20) + 10), -128, dtype=np.int8)
    for wgs in (1, 3):
        d.debug_set_workgroups(wgs)
        for mode in (MEASURE, BOTH):
            mom = run_case(torch_dev, d, m, cap, mode, 6, 6, 0, 0, f"1 MiB of -128 in {wgs} workgroups, mode {mode}")
            assert [int(v) for v in mom[0][3:6]] == [(1 << 33) + 5 * (1 << 14)] * 3
    with pytest.raises(api.HrfdError, match="hrfd_cal_debug_set_workgroups"):
        d.debug_set_workgroups(0)
