"""The DEVICE's restatement of glibc's sinf / cosf (hrfd_tx_kernels.hip: glibc_sincosf_pair_v, glibc_sincosf_v) on every
float of the restated range |x| < 120, in BOTH variants (without / with fused multiply-adds) and both forms (the pair
function of every product caller; glibc_sinf and glibc_cosf called separately), against the same text in C
(oracle/sincosf_model.h) and, in the variant this host runs, against its libm directly.

The host probes its libm once (hrfd_libm_variant()), so the product only ever runs one of the two templates on a given
machine, and every product consumer but Nco::run quantises to int8 or int16 before anything is compared:
hrfd_debug_sincosf_digest / _eval (include/hrfd_debug.h, read-only, available without HRFD_DEBUG_HOOKS) select the
template themselves and return floats.  One digest call covers a whole sign of the range (1071 chunks of 2^20 bit
patterns, one workgroup each).

Cost: the host side (libm and two models over the whole range, computed once per process by sincos_model.range_digest)
takes 7.5 s on 8 CPU cores; each exhaustive case prints its two digest kernels' times (kernel_ms)."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import sincos_model as M

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1)
FORMS = (0, 1)
FORM_NAME = {0: "pair", 1: "one_sided"}
SIGN_BIT = 0x80000000


@pytest.fixture(scope="module")
def host():
    """{(source, sign): digests} of the three CPU sources, once per module; and the host's libm variant"""
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path cannot run (and there is no CPU fallback)")
    d = {(src, sign): M.range_digest(src, sign) for src in (M.MODEL0, M.MODEL1, M.LIBM) for sign in M.RANGES}
    return d, int(_lib.load().hrfd_libm_variant())


def _records(variant, form, chunk, source):
    """up to 8 (pattern, device bits, wanted bits) of the floats of a chunk on which the device differs from a source"""
    u = M.chunk_patterns(chunk)
    x = M.from_bits(u)
    gs, gc = api.debug_sincosf_eval(variant, form, x)
    ws, wc = M.eval(source, x)
    rec = []
    for name, g, w in (("sinf", M.bits(gs), M.bits(ws)), ("cosf", M.bits(gc), M.bits(wc))):
        for i in np.nonzero(g != w)[0][:8]:
            rec.append("%s(0x%08X): device 0x%08X, wanted 0x%08X" % (name, int(u[i]), int(g[i]), int(w[i])))
    return rec[:8]


@pytest.mark.parametrize("form", FORMS, ids=lambda f: FORM_NAME[f])
@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "variant%d" % v)
def test_device_equals_the_model_on_every_float_of_the_range(host, variant, form):
    digests, host_variant = host
    for sign, (first, n) in M.RANGES.items():
        got, ms = api.debug_sincosf_digest(variant, form, first, n, timed=True)
        print("digest kernel, variant %d, %s, %s floats: %.2f ms" % (variant, FORM_NAME[form], sign, ms))
        sources = [variant] + ([M.LIBM] if variant == host_variant else [])
        for src in sources:
            bad = np.nonzero(got != digests[(src, sign)])[0]
            if bad.size:
                chunk = first + int(bad[0])
                pytest.fail("variant %d, %s: %d chunks of the %s floats differ from %s; chunk %d (from 0x%08X): %s" %
                            (variant, FORM_NAME[form], bad.size, sign, {0: "model 0", 1: "model 1", 2: "libm"}[src], chunk,
                             chunk << 20, _records(variant, form, chunk, src) or "eval agrees: the DIGEST kernel is wrong"))


def test_digest_equals_the_sum_over_eval_and_refuses_chunks_outside_the_pattern_space():
    """the digest kernel against the eval kernel and the host's mix on single chunks (first and last of each sign of the
    range, and more chunks than one); chunk ranges that leave 0..4095 and unknown variants / forms return HRFD_EINVAL"""
    for variant, form, chunk in ((1, 0, 0), (0, 1, 1070), (1, 1, 2048), (0, 0, 3118), (1, 0, 0x3F4)):
        got = api.debug_sincosf_digest(variant, form, chunk, 1)
        assert int(got[0]) == int(M.digest(variant, chunk, 1)[0]), (variant, form, chunk)
    got = api.debug_sincosf_digest(1, 0, 1069, 2)
    assert (got == M.digest(M.MODEL1, 1069, 2)).all()
    L = _lib.load()
    out = (C.c_uint64 * 4)()
    for variant, form, first, n in ((0, 0, 4096, 1), (0, 0, 4095, 2), (0, 0, 0, 4097), (0, 0, 0xFFFFFFFF, 2), (0, 0, 0, 0),
                                    (2, 0, 0, 1), (-1, 0, 0, 1), (0, 2, 0, 1), (0, -1, 0, 1)):
        assert L.hrfd_debug_sincosf_digest(variant, form, first, n, out, None) == -1, (variant, form, first, n)
    assert L.hrfd_debug_sincosf_digest(0, 0, 0, 1, None, None) == -1
    one = (C.c_float * 1)(1.0)
    assert L.hrfd_debug_sincosf_eval(2, 0, one, 1, one, one) == -1
    assert L.hrfd_debug_sincosf_eval(0, 0, one, 0, one, one) == -1
    assert L.hrfd_debug_sincosf_eval(0, 0, None, 1, one, one) == -1


def test_variant_is_live_on_the_34_floats_where_the_two_builds_differ():
    """the only floats of the range on which the two templates may differ (tests/test_sincos_model.py derives the list):
    variant 0 and variant 1 differ exactly where the table says, and each gives its own model's bits -- a kernel that
    ignored `variant` (or the host's probe) cannot pass"""
    u = np.array(sorted(set(M.FMA_DIFFERS_SIN) | set(M.FMA_DIFFERS_COS)), dtype=np.uint32)
    assert len(M.FMA_DIFFERS_SIN) == 12 and len(M.FMA_DIFFERS_COS) == 22 and u.size == 34   # (no float is in both lists)
    x = M.from_bits(u)
    in_sin = np.isin(u, np.array(M.FMA_DIFFERS_SIN, dtype=np.uint32))
    in_cos = np.isin(u, np.array(M.FMA_DIFFERS_COS, dtype=np.uint32))
    for form in FORMS:
        s0, c0 = api.debug_sincosf_eval(0, form, x)
        s1, c1 = api.debug_sincosf_eval(1, form, x)
        assert ((M.bits(s0) != M.bits(s1)) == in_sin).all(), form
        assert ((M.bits(c0) != M.bits(c1)) == in_cos).all(), form
        for variant, (s, c) in ((0, (s0, c0)), (1, (s1, c1))):
            ws, wc = M.eval(variant, x)
            assert (M.bits(s) == M.bits(ws)).all() and (M.bits(c) == M.bits(wc)).all(), (variant, form)


def _edge_patterns():
    f32 = lambda v: int(np.array([v], dtype=np.float32).view(np.uint32)[0])
    u = [0x00000000,                                        # 0
         0x00000001, 0x007FFFFF, 0x00800000,                # the smallest and the largest denormal, the smallest normal
         0x397FFFFE, 0x397FFFFF, 0x39800000, 0x39800001,    # either side of 2^-12 (abstop12 == 0x398)
         0x3F3FFFFE, 0x3F3FFFFF, 0x3F400000, 0x3F400001,    # either side of the pi / 4 threshold (abstop12 == 0x3f4)
         M.TOP - 1]                                         # the last float below 120
    for k in range(1, 153):                                 # the float nearest k pi / 4 and 16 neighbours on either side
        c = f32(k * np.pi / 4)
        u += list(range(c - 16, c + 17))
    u = np.array(u, dtype=np.uint32)
    return np.concatenate([u, u | np.uint32(SIGN_BIT)])


def test_edges_by_value():
    """+-0, the denormals (sinf must hand the input back bit for bit: no flush to zero), both sides of the 2^-12 and the
    pi / 4 thresholds, the neighbourhood of every multiple of pi / 4 up to 152 (where the reduction's n changes and the
    polynomials change roles) and the last float below 120 -- both variants, both forms, bitwise against the model"""
    u = _edge_patterns()
    assert (np.abs(M.from_bits(u)) < 120.0).all() and u.size == 2 * (13 + 152 * 33)
    x = M.from_bits(u)
    tiny = (u & np.uint32(0x7FFFFFFF)) < np.uint32(0x39800000)
    assert tiny.sum() == 2 * 6
    for variant in VARIANTS:
        ws, wc = M.eval(variant, x)
        for form in FORMS:
            gs, gc = api.debug_sincosf_eval(variant, form, x)
            bad = np.nonzero((M.bits(gs) != M.bits(ws)) | (M.bits(gc) != M.bits(wc)))[0]
            assert bad.size == 0, (variant, form, [("0x%08X" % int(u[i]), "sin 0x%08X / 0x%08X" % (int(M.bits(gs)[i]), int(M.bits(ws)[i])),
                                                    "cos 0x%08X / 0x%08X" % (int(M.bits(gc)[i]), int(M.bits(wc)[i]))) for i in bad[:8]])
            assert (M.bits(gs)[tiny] == u[tiny]).all(), (variant, form)
            assert (M.bits(gc)[tiny] == 0x3F800000).all(), (variant, form)


def test_outside_the_restated_range():
    """|x| >= 120, infinities, NaN: the device rounds its own double sin / cos, so bit equality with glibc is not
    promised (no caller gets there: every phase is wrapped).  NaN and +-inf give NaN; a finite argument gives a float
    within one float ulp of (float)sin((double)x) on the host -- both sides are faithful double results rounded once."""
    x = np.array([120.0, 1e6, np.finfo(np.float32).max, -120.0, -1e6, -np.finfo(np.float32).max, 120.00001, 12345.678,
                  np.inf, -np.inf, np.nan], dtype=np.float32)
    fin = np.isfinite(x)
    ws, wc = M.eval(M.MODEL1, x)                             # outside the range the models ARE (float)sin((double)x), (float)cos((double)x)
    for variant in VARIANTS:
        for form in FORMS:
            gs, gc = api.debug_sincosf_eval(variant, form, x)
            assert np.isnan(gs[~fin]).all() and np.isnan(gc[~fin]).all(), (variant, form, gs, gc)
            for name, g, w in (("sin", gs, ws), ("cos", gc, wc)):
                err = np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float64))
                ulp = np.spacing(np.abs(w[fin])).astype(np.float64)
                print(name, "variant", variant, FORM_NAME[form], "error in ulps:", (err / ulp).tolist())
                assert np.isfinite(g[fin]).all() and (err <= ulp).all(), (name, variant, form, g[fin], w[fin])
