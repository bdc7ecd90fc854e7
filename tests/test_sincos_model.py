"""glibc's sinf / cosf restated in C (oracle/sincosf_model.h) against this host's libm on EVERY float with |x| < 120 --
the statement of tools/proofs/sincosf_glibc.c as a test -- and the two variants of the restatement against each other.
No GPU: what the device computes is held to these models by tests/test_gpu_sincos.py.

Measured (8 cores): the three full-range digest sets (libm, model 0, model 1: 3 x 2 246 049 792 floats) take 7.5 s of
wall time together; they are computed once per process (sincos_model.range_digest) and shared with the GPU tests."""
import ctypes as C

import numpy as np
import pytest

from tests import sincos_model as M


def _host_variant():
    from hackrfdiags_amd import _lib
    return int(_lib.load().hrfd_libm_variant())


def _differing(sign, src_a, src_b):
    """the floats of one sign on which two sources differ, found by digest and then by value: (sin list, cos list)"""
    da, db = M.range_digest(src_a, sign), M.range_digest(src_b, sign)
    sin_l, cos_l = [], []
    for k in np.nonzero(da != db)[0]:
        u = M.chunk_patterns(M.RANGES[sign][0] + int(k))
        sa, ca = M.eval(src_a, M.from_bits(u))
        sb, cb = M.eval(src_b, M.from_bits(u))
        assert (M.bits(sa) != M.bits(sb)).any() or (M.bits(ca) != M.bits(cb)).any(), ("digests differ, values do not", sign, int(k))
        sin_l += [int(v) for v in u[M.bits(sa) != M.bits(sb)]]
        cos_l += [int(v) for v in u[M.bits(ca) != M.bits(cb)]]
    return sin_l, cos_l


def test_chunks_tile_the_restated_range():
    assert M.POS == (0, 1071) and M.NEG == (2048, 1071)
    assert M.from_bits([M.TOP - 1])[0] < 120.0 and M.from_bits([M.TOP])[0] == 120.0
    u = M.chunk_patterns(1070)
    assert int(u[0]) == 1070 << 20 and int(u[-1]) == M.TOP - 1


def test_digest_is_the_sum_of_the_mix_and_refuses_what_leaves_the_pattern_space():
    """one chunk's digest recomputed in Python from eval; the mix takes the pattern in (two neighbours with swapped
    results change the sum); chunk ranges outside 0..4095 and unknown sources are refused"""
    def mix(u, s, c):
        with np.errstate(over="ignore"):
            z = ((s.astype(np.uint64) << np.uint64(32)) | c.astype(np.uint64)) + u.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))

    chunk = 0x3F4                                            # the chunk that begins at the pi / 4 threshold
    u = M.chunk_patterns(chunk)
    for src in (M.MODEL0, M.MODEL1, M.LIBM):
        sn, cs = M.eval(src, M.from_bits(u))
        with np.errstate(over="ignore"):
            want = int(mix(u, M.bits(sn), M.bits(cs)).sum(dtype=np.uint64))
        assert int(M.digest(src, chunk, 1)[0]) == want, src
    s, c = M.bits(sn).copy(), M.bits(cs).copy()
    assert s[7] != s[8]
    s[[7, 8]] = s[[8, 7]]
    with np.errstate(over="ignore"):
        assert int(mix(u, s, c).sum(dtype=np.uint64)) != want
    L = M._lib()
    out = (C.c_uint64 * 4)()
    for src, first, n in ((3, 0, 1), (-1, 0, 1), (0, 4096, 1), (0, 4095, 2), (0, 0, 4097), (0, 0xFFFFFFFF, 2)):
        assert L.orc_sincosf_digest(src, first, n, out) == -1, (src, first, n)
    assert L.orc_sincosf_digest(0, 4095, 1, out) == 0


@pytest.mark.parametrize("sign", ["pos", "neg"])
def test_model_of_the_hosts_variant_equals_libm_on_every_float(sign):
    """hrfd_libm_variant() names the build of glibc's sinf / cosf this host runs; the restatement of that build must
    give libm's floats on every chunk of the range (1071 chunks of 2^20 floats per sign).  On a host whose libm is
    neither build there is nothing to claim, and the device follows the FMA build (include/hrfd.h)."""
    v = _host_variant()
    if v not in (0, 1):
        pytest.skip("this host's libm is neither build of glibc's sinf / cosf (hrfd_libm_variant() == -1)")
    got, want = M.range_digest(v, sign), M.range_digest(M.LIBM, sign)
    if not (got == want).all():
        sin_l, cos_l = _differing(sign, v, M.LIBM)
        pytest.fail("model %d differs from libm on sinf of %s and cosf of %s" %
                    (v, ["0x%08X" % p for p in sin_l[:8]], ["0x%08X" % p for p in cos_l[:8]]))


def test_the_two_variants_differ_on_exactly_the_34_committed_floats():
    sin_l, cos_l = [], []
    for sign in ("pos", "neg"):
        s, c = _differing(sign, M.MODEL0, M.MODEL1)
        sin_l += s
        cos_l += c
    assert len(sin_l) == 12 and len(cos_l) == 22
    assert tuple(sin_l) == M.FMA_DIFFERS_SIN
    assert tuple(cos_l) == M.FMA_DIFFERS_COS
    assert (np.abs(M.from_bits(sin_l + cos_l)) > 17.0).all()


def test_the_other_variant_differs_from_libm_on_the_committed_floats_only():
    """the proof program's second line: the variant the host does NOT run misses libm on the 34 floats and nowhere else"""
    v = _host_variant()
    if v not in (0, 1):
        pytest.skip("this host's libm is neither build of glibc's sinf / cosf")
    sin_l, cos_l = [], []
    for sign in ("pos", "neg"):
        s, c = _differing(sign, 1 - v, M.LIBM)
        sin_l += s
        cos_l += c
    assert tuple(sin_l) == M.FMA_DIFFERS_SIN and tuple(cos_l) == M.FMA_DIFFERS_COS


def test_model_outside_the_range_and_special_values():
    """what the GPU test's edge cases lean on: denormals pass through sinf unchanged, cosf is 1 below 2^-12, +-0 keep
    their sign, and outside |x| < 120 the models are the double functions rounded (NaN for NaN and infinities)"""
    u = np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x80000001, 0x807FFFFF, 0x397FFFFF], dtype=np.uint32)
    for src in (M.MODEL0, M.MODEL1, M.LIBM):
        sn, cs = M.eval(src, M.from_bits(u))
        assert (M.bits(sn) == u).all(), src
        assert (M.bits(cs) == 0x3F800000).all(), src
    x = np.array([120.0, 1e6, np.finfo(np.float32).max, np.inf, -np.inf, np.nan], dtype=np.float32)
    for src in (M.MODEL0, M.MODEL1):
        sn, cs = M.eval(src, x)
        assert np.isnan(sn[3:]).all() and np.isnan(cs[3:]).all()
        assert np.isfinite(sn[:3]).all() and np.isfinite(cs[:3]).all()
