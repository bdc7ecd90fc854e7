"""k_nco (hrfd_tx_kernels.hip: one oscillator per thread, 64 threads per workgroup) at its edges, against the CPU oracle's
Nco, bit for bit (compared as uint32): banks that do not fill, exactly fill and cross a workgroup, every channel at a
frequency of its own, calls of 1, 2 and 257 samples that continue the state, setters between the calls, and frequencies
that put the wrap compare on its boundary or take the wrap loops round two to four times.

SAFETY LIMIT: no test here may pass |f| > 4 fs.  The wrap loops subtract 2 pi from a float; from about 2^27 rad that no
longer changes the value and the kernel would never return.  (hrfd_nco_create / hrfd_nco_set_frequency refuse a step of
2^24 rad or more on the host -- tested below by calls that must fail and therefore launch nothing.)"""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api

pytestmark = pytest.mark.gpu

FS = 16777216.0                                            # 2^24: f = ratio * fs is exact in float for the ratios below
NEAR_HALF = 0.5 - 2.0 ** -25                               # f = 2^23 - 0.5: the step is the last float BELOW pi (0x40490FDA)
# f / fs, the telling ones first so that every bank of 19 channels or more has them all (a bank of one has +0.5):
#   +-0.5            the float step 0x40490FDB is just above pi: the wrap compare sits on its boundary
#   +-NEAR_HALF      the largest phase an accumulator can hold: the extreme table indices of runFast (see _reach)
#   +-0.75, +-1, +-2.5, +-4   two to four turns of the wrap loops
#   +-0.4999, +-1/8, +-1e-7, 0
RATIOS = [0.5, -0.5, NEAR_HALF, -NEAR_HALF, 0.75, -0.75, 1.0, -1.0, 2.5, -2.5, 4.0, -4.0, 0.4999, -0.4999, 0.125, -0.125,
          1e-7, -1e-7, 0.0]
COUNTS = (1, 2, 257)


def _ratio(c):
    if c < len(RATIOS):
        return RATIOS[c]
    return (((c * np.sqrt(2.0)) % 1.0) - 0.5) * 0.98          # the rest irrational, in (-0.49, 0.49)


def _freq(ratio):
    f = float(np.float32(ratio * FS))
    assert abs(f) <= 4 * FS, f                               # the safety limit
    return f


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _setters(C_):
    """(channel in the middle of a workgroup, the bank's last channel, the channel that is reset) -- outside RATIOS for
    every bank of 63 channels or more"""
    mid = 64 + 31 if C_ > 64 + 31 else C_ // 2
    return mid, C_ - 1, C_ // 3


def _reach(phases, turns):
    """From the ORACLE's phase sequence: the table index of Nco::runFast before its clamp, and the turns of the wrap loops.
    A phase handed out is an accumulator that has been wrapped, a float in [-P, P] with P = 0x40490FDA the last float below
    pi (0x40490FDB > pi is wrapped): (int16)(phase * 16384 / 2 pi) + 8192 truncates towards zero, so P gives
    8191 + 8192 = 16383 and -P gives -8191 + 8192 = 1.  The index is monotone in the phase, so [1, 16383] is all it can
    be: index 0 and the clamp's upper side (16384 -> 16383) are UNREACHABLE through the API, and max(0, min(16383, .))
    never changes a value.  What can be shown is that both extremes of the reachable interval ARE reached."""
    idx = np.trunc((phases.astype(np.float32) * np.float32(16384)).astype(np.float64) / (2 * np.pi)).astype(np.int64) + 8192
    P = np.array([0x40490FDA], dtype=np.uint32).view(np.float32)[0]
    assert float(P) < np.pi < float(np.nextafter(P, np.float32(4)))
    assert np.abs(phases).max() == P
    assert idx.min() == 1 and idx.max() == 16383, (idx.min(), idx.max())
    assert turns.max() >= 4 and (turns == 2).any() and (turns == 3).any(), np.unique(turns)


@pytest.mark.parametrize("fast", [True, False], ids=["runFast", "run"])
@pytest.mark.parametrize("C_", [1, 63, 64, 65, 130], ids=lambda c: "C%d" % c)
def test_nco_bank_sweep(oracle, C_, fast):
    g = api.Nco(FS, _freq(_ratio(0)), C_)
    os_ = [oracle.nco(FS, _freq(_ratio(c))) for c in range(C_)]
    tw = [oracle.nco(FS, _freq(_ratio(c))) for c in range(C_)]     # twins that only record the phase sequence
    for c in range(C_):
        g.set_frequency(_freq(_ratio(c)), channel=c)
    mid, last, rst = _setters(C_)
    phases, turns = [], []
    for call, n in enumerate(COUNTS):
        if call == 1:
            for c, r in ((mid, -0.3), (last, 1.75)):
                g.set_frequency(_freq(r), channel=c)
                os_[c].set_frequency(_freq(r))
                tw[c].set_frequency(_freq(r))
        if call == 2:
            g.reset(channel=rst)
            os_[rst].reset()
            tw[rst].reset()
        gi, gq = g.run(n, fast=fast)
        gi, gq = np.atleast_2d(gi), np.atleast_2d(gq)
        for c in range(C_):
            wi, wq = os_[c].run(n, fast)
            assert (_u32(gi[c]) == _u32(wi)).all() and (_u32(gq[c]) == _u32(wq)).all(), (C_, fast, call, n, c, _ratio(c))
            p, t = tw[c].phases(n)
            phases.append(p)
            turns.append(t)
    if C_ >= len(RATIOS):
        _reach(np.concatenate(phases), np.concatenate(turns))


def test_nco_refuses_a_step_that_would_never_wrap():
    """a frequency whose step is not finite, or 2^24 rad or more, is refused with HRFD_EINVAL by create and by
    set_frequency, on the host: these calls never reach a launch.  The accepted neighbour of the bound is only SET, never
    run.  A refused set_frequency changes nothing: the bank still runs its old frequencies."""
    L = _lib.load()
    h = C.c_void_p()
    bad = [(8000.0, float("nan")), (8000.0, float("inf")), (8000.0, float("-inf")), (0.0, 1000.0), (0.0, 0.0),
           (float("nan"), 1000.0), (1.0, 2670177.0), (1.0, -2670177.0), (1e-30, 1e30), (8000.0, 3.0e38)]
    for fs, f in bad:
        assert L.hrfd_nco_create(3, C.c_float(fs), C.c_float(f), -1, C.byref(h)) == -1, (fs, f)
        assert not h.value
    assert float(np.float32(2 * np.pi * 2670177.0)) >= 2.0 ** 24 > float(np.float32(2 * np.pi * 2670176.0))
    assert L.hrfd_nco_create(3, C.c_float(1.0), C.c_float(2670176.0), -1, C.byref(h)) == 0       # the last step below 2^24: accepted
    assert L.hrfd_nco_destroy(h) == 0
    g = api.Nco(8000.0, 1000.0, 3)
    for f in (float("nan"), float("inf"), float("-inf"), 8000.0 * 2670200.0, -3.0e38):
        for ch in (0, 2, api.ALL):
            assert L.hrfd_nco_set_frequency(g.h, ch, C.c_float(f)) == -1, (f, ch)
    assert L.hrfd_nco_set_frequency(g.h, 3, C.c_float(1000.0)) == -1                             # (no such channel)
    i, q = g.run(8, fast=False)
    assert (_u32(i[0]) == _u32(i[1])).all() and (_u32(i[0]) == _u32(i[2])).all()
    assert i[0, 0] == 1.0 and q[0, 0] == 0.0 and abs(float(q[0, 2]) - 1.0) < 1e-6                 # 1000 Hz at 8 kS/s: a quarter turn in two samples
