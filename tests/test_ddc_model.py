"""The DDC bank without a GPU: the default filters and their generator, the tables the library exports, the C ABI's
argument checks on a machine without a device, and the numpy model (tests/ddc_model.py) the GPU tests hold the kernel
to -- its properties, and the selectivity it gives together with the CPU oracle's receive chain."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import ddc_model as dm
from tools import ddc_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HRFD_EINVAL, HRFD_ENODEV = -1, -2


# ---- design
def test_design_tool_regenerates_the_committed_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ddc_design.py"), "--check"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", ["DDC_A2", "DDC_A4", "DDC_A8", "DDC_B"])
def test_default_filters_meet_their_specification(name):
    """quantised taps: ripple <= 0.1 dB over the passband, >= 60 dB in the stopband (zero-padded FFT), sum |h| <= 65535"""
    q = ddc_design.tables()[name]
    fs, fp, fst = ddc_design.SPECS[name]
    ripple, atten = ddc_design.response(q, fs, fp, fst)
    assert ripple <= 0.1 and atten >= 60.0, (ripple, atten)
    assert int(np.abs(q.astype(np.int64)).sum()) <= 65535
    assert q.size <= (64 if name != "DDC_B" else 256)
    assert abs(int(q.astype(np.int64).sum()) - 32768) <= q.size     # unity gain at DC


# ---- the library's tables
@pytest.mark.parametrize("name", ["DDC_COS", "DDC_A2", "DDC_A4", "DDC_A8", "DDC_B"])
def test_library_tables_equal_the_header(name):
    got = api.q15_table(name)
    want = ddc_design.tables()[name]
    assert got.dtype == np.int16 and got.size == want.size and (got == want).all()


def test_cos_table_is_rounded_cosine():
    assert (api.q15_table("DDC_COS") == np.round(32767 * np.cos(2 * np.pi * np.arange(4096) / 4096))).all()


def test_q15_table_reads_short_tables_unchanged():
    for name, n in (("HB1", 3), ("WBFM_D1", None), ("SSB_HILBERT", None)):
        t = api.q15_table(name)
        assert t.size == _lib.load().hrfd_q15_table(name.encode(), None, 0)
        assert n is None or t.size == n
    assert api.q15_table("NO_SUCH_TABLE").size == 0


# ---- the C ABI without a device
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _no_gpu(lib):
    if lib.hrfd_device_count() > 0:
        pytest.skip("checks the behaviour without a GPU")


def test_abi_refuses_bad_arguments_without_a_device(lib):
    h = C.c_void_p()
    assert lib.hrfd_ddc_create(1, 4, 3, -1, C.byref(h)) == HRFD_EINVAL
    assert b"decimation" in lib.hrfd_last_error()
    assert lib.hrfd_ddc_create(0, 4, 4, -1, C.byref(h)) == HRFD_EINVAL
    assert lib.hrfd_ddc_create(1, 0, 4, -1, C.byref(h)) == HRFD_EINVAL
    assert lib.hrfd_ddc_set_gain_shift(None, 0, 8) == HRFD_EINVAL
    assert b"0..7" in lib.hrfd_last_error()
    small = np.ones(4, dtype=np.int16)
    i16 = C.POINTER(C.c_int16)
    for stage, n in ((0, 65), (1, 257)):
        taps = np.ones(n, dtype=np.int16)
        assert lib.hrfd_ddc_set_filter(None, stage, taps.ctypes.data_as(i16), n) == HRFD_EINVAL
        assert b"taps" in lib.hrfd_last_error()
    heavy = np.full(3, 30000, dtype=np.int16)                    # sum |h| = 90000 > 65535
    for stage in (0, 1):
        assert lib.hrfd_ddc_set_filter(None, stage, heavy.ctypes.data_as(i16), 3) == HRFD_EINVAL
        assert b"65535" in lib.hrfd_last_error()
    assert lib.hrfd_ddc_set_filter(None, 2, small.ctypes.data_as(i16), 4) == HRFD_EINVAL


def test_valid_create_without_a_device_is_enodev(lib):
    _no_gpu(lib)
    h = C.c_void_p()
    for r in (1, 2, 4, 8):
        assert lib.hrfd_ddc_create(2, 8, r, -1, C.byref(h)) == HRFD_ENODEV
        assert not h.value


def test_ddc_step_and_tune_range():
    assert api.ddc_step(0, 4) == 0
    assert api.ddc_step(2_048_000, 4) == 1 << 30
    assert api.ddc_step(-2_048_000, 4) == 3 << 30
    assert api.ddc_step(100_000, 8) == dm.ddc_step(100_000, 8) == round(100_000 / 16_384_000 * 2 ** 32)


# ---- model properties
def _tone(f, R, n, amp=60, n0=0):
    t = (n0 + np.arange(n)) / (R * dm.FS_OUT)
    x = amp * np.exp(2j * np.pi * f * t)
    return np.stack([np.round(x.real), np.round(x.imag)], 1).astype(np.int8).reshape(1, -1)


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_model_moves_a_tone_at_plus_f_to_dc(R):
    f = 300_000.0
    m = dm.DdcModel(1, 1, R)
    m.set_tuning(0, 0, dm.ddc_step(f, R))
    out = m.process(_tone(f, R, R * 2048), 4096).reshape(-1, 2).astype(np.float64)
    tail = out[400:]
    assert abs(tail[:, 0].mean() - 60) <= 1.5 and abs(tail[:, 1].mean()) <= 1.5
    assert tail.std(axis=0).max() <= 1.0


def test_model_any_split_of_the_stream_gives_the_same_output():
    rng = np.random.default_rng(3)
    R, W, Cn = 4, 2, 3
    total = 6000
    cap = rng.integers(-128, 128, size=(W, R * total), dtype=np.int8)
    ref = dm.DdcModel(W, Cn, R)
    parts = [dm.DdcModel(W, Cn, R) for _ in range(2)]
    for m in [ref] + parts:
        m.set_tuning(0, 1, dm.ddc_step(123_456, R))
        m.set_tuning(1, 0, dm.ddc_step(-3_000_000, R))
        m.set_tuning(2, 1, 0x12345678)
        m.set_gain_shift(2, 3)
    whole = ref.process(cap, total)
    for m, cuts in zip(parts, ([2, 510, 1000, 1234, 2000, 1254], [4096, 1904])):
        got, o = [], 0
        for nb in cuts:
            got.append(m.process(cap[:, R * o:R * (o + nb)], nb))
            o += nb
        assert o == total
        assert (np.concatenate(got, axis=1) == whole).all()


def test_model_retune_is_phase_continuous():
    R, f1, f2 = 2, 100_000.0, -250_000.0
    m = dm.DdcModel(1, 1, R)
    m.set_tuning(0, 0, dm.ddc_step(f1, R))
    m.process(np.zeros((1, R * 1000), dtype=np.int8), 1000)
    n = m.N
    before = m.phase(0)
    m.set_tuning(0, 0, dm.ddc_step(f2, R))
    assert m.phase(0) == before                                   # continuous at the change point
    assert m.phase(0, n + 10) == (before + 10 * dm.ddc_step(f2, R)) & dm.MASK32
    assert m.phase(0, n - 3) == (before - 3 * dm.ddc_step(f2, R)) & dm.MASK32   # earlier samples: the new tuning


# ---- selectivity: model + CPU oracle rx
@pytest.fixture(scope="module")
def selectivity(oracle):
    cap, audio = dm.selectivity_capture(oracle)
    m = dm.DdcModel(1, 2, dm.SEL_R)
    for c, f in enumerate(dm.SEL_OFFSETS):
        m.set_tuning(c, 0, dm.ddc_step(f + 64_000, dm.SEL_R))
        m.set_gain_shift(c, dm.SEL_GAIN_SHIFT[c])
    streams = m.process(cap, dm.SEL_BLOCKS * 262144)
    pcm = [dm.oracle_rx_wbfm(oracle, streams[c]) for c in range(2)]
    return cap, audio, streams, pcm


def test_selectivity_two_wbfm_stations_400_khz_apart(selectivity):
    """The weak station (-10 dB) 400 kHz beside a strong one at R = 4, through the model and the oracle's WBFM chain.
    Measured with the model: own audio 0.976 / 0.989 (weak / strong station), the other station's audio 0.040 / 0.039
    (the two audio excerpts themselves correlate at 0.047 under the same delay search: that is the floor)."""
    _, audio, _, pcm = selectivity
    own = [dm.best_corr(audio[c], pcm[c]) for c in range(2)]
    other = [dm.best_corr(audio[1 - c], pcm[c]) for c in range(2)]
    print("own", own, "other", other)
    assert min(own) >= 0.85, own
    assert max(other) <= 0.05, other
