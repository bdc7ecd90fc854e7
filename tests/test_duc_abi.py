"""CPU-side checks of the DUC bank's C ABI (hrfd_duc_*): every argument error comes back as HRFD_EINVAL before any
device is touched, so these hold on a machine without a GPU too; the exported default filters are tools/duc_design.py's."""
import ctypes as C
import os

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "hackrfdiags_amd", "csrc")])
    return _lib.load()


def err(L):
    return L.hrfd_last_error().decode(errors="replace")


def i16(a):
    a = np.ascontiguousarray(a, dtype=np.int16)
    return a, a.ctypes.data_as(C.POINTER(C.c_int16))


def test_duc_symbols_are_exported(L):
    for name in ("create", "destroy", "reset", "set_tuning", "set_amplitude", "set_output_shift", "set_filter",
                 "get_phase", "get_clips", "process", "process_device", "transmit"):
        assert hasattr(L, "hrfd_duc_" + name), name


@pytest.mark.parametrize("W,Cn,R,what", [(1, 1, 3, "interpolation"), (1, 1, 16, "interpolation"),
                                          (1, 1, 0, "interpolation"), (1, 32769, 8, "channels"),
                                          (0, 4, 8, "n_captures"), (4, 0, 8, "n_channels")])
def test_create_refuses_bad_shapes(L, W, Cn, R, what):
    h = C.c_void_p(123)
    assert L.hrfd_duc_create(W, Cn, R, 0, C.byref(h)) == EINVAL
    assert not h.value, "the result is cleared on failure"
    assert what in err(L)
    assert L.hrfd_duc_create(1, 1, 8, 0, None) == EINVAL


def test_setters_refuse_bad_values_without_a_handle(L):
    assert L.hrfd_duc_set_amplitude(None, 0, 32769) == EINVAL and "0..32768" in err(L)
    assert L.hrfd_duc_set_amplitude(None, 0, 32768) == EINVAL and "handle" in err(L)
    assert L.hrfd_duc_set_output_shift(None, 0, 25) == EINVAL and "0..24" in err(L)
    assert L.hrfd_duc_set_output_shift(None, 0, 24) == EINVAL and "handle" in err(L)
    assert L.hrfd_duc_set_tuning(None, 0, 0, 1) == EINVAL
    assert L.hrfd_duc_reset(None) == EINVAL
    v = C.c_uint32()
    assert L.hrfd_duc_get_phase(None, 0, C.byref(v)) == EINVAL
    n = C.c_uint64()
    assert L.hrfd_duc_get_clips(None, 0, C.byref(n)) == EINVAL
    assert L.hrfd_duc_destroy(None) == 0


def test_set_filter_refuses_bad_tap_sets_without_a_handle(L):
    assert L.hrfd_duc_set_filter(None, 2, None, 0) == EINVAL and "stage" in err(L)
    t, p = i16(np.ones(65))
    assert L.hrfd_duc_set_filter(None, 0, p, 65) == EINVAL and "65 taps" in err(L)
    t, p = i16(np.ones(257))
    assert L.hrfd_duc_set_filter(None, 1, p, 257) == EINVAL and "257 taps" in err(L)
    t, p = i16([30000, 30000, 5536])                               # sum |h| = 65536
    assert L.hrfd_duc_set_filter(None, 1, p, 3) == EINVAL and "65535" in err(L)
    t, p = i16([30000, 30000, 5535])                               # at the bound: only the handle is missing
    assert L.hrfd_duc_set_filter(None, 1, p, 3) == EINVAL and "handle" in err(L)
    assert L.hrfd_duc_set_filter(None, 0, None, 3) == EINVAL and "tap array" in err(L)
    # stage A's bound is per polyphase branch of the handle's R: a set over 65535 in total is refused only by a handle
    t, p = i16([30000, 30000, 30000])
    assert L.hrfd_duc_set_filter(None, 0, p, 3) == EINVAL and "handle" in err(L)


def test_calls_refuse_bad_arguments_without_a_handle(L):
    buf = np.zeros(64, dtype=np.int8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.hrfd_duc_process(None, ptr, 4, ptr) == EINVAL and "NULL" in err(L)
    assert L.hrfd_duc_process_device(None, ptr, 4, 4, ptr, 32, None) == EINVAL
    assert L.hrfd_duc_transmit(None, None, ptr, 1, ptr, 1 << 20, None) == EINVAL
    assert L.hrfd_duc_transmit(None, ptr, ptr, 0, ptr, 1 << 20, None) == EINVAL and "n_per_channel" in err(L)
    assert L.hrfd_duc_transmit(None, ptr, ptr, 1 << 17, ptr, 1 << 20, None) == EINVAL and "n_per_channel" in err(L)


def test_create_without_a_gpu_is_enodev(L):
    if L.hrfd_device_count() > 0:
        pytest.skip("a GPU is visible: the handle is made on it (tests/test_gpu_duc*.py)")
    h = C.c_void_p()
    assert L.hrfd_duc_create(2, 4, 8, 0, C.byref(h)) == -2 and not h.value


@pytest.mark.parametrize("R", [2, 4, 8])
def test_default_filters_are_exported(L, R):
    from tools import duc_design
    want = duc_design.tables()[f"DUC_A{R}"]
    got = api.q15_table(f"DUC_A{R}")
    assert got.size == want.size and (got == want).all()
    assert (duc_design.branch_sums(got, R) <= 65535).all()
    assert abs(int(got.astype(np.int64).sum()) - R * 32768) <= R


def test_header_declares_the_duc_block():
    text = open(os.path.join(ROOT, "include", "hrfd.h")).read()
    for name in ("hrfd_duc_create", "hrfd_duc_transmit", "hrfd_duc_get_clips", '"DUC_A8"'):
        assert name in text, name
