"""Every refusal of the three banks (hrfd_ddc_*, hrfd_duc_*, hrfd_spec_*) that is decided before a device is needed,
through the raw C ABI: the return code, and an error text that starts with the public function's name.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

EINVAL, ENODEV = -1, -2
NULL = None
I16P = C.POINTER(C.c_int16)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def taps(values):
    a = np.ascontiguousarray(values, dtype=np.int16)
    return a, a.ctypes.data_as(I16P)


def refused(lib, name, *args, code=EINVAL):
    rc = getattr(lib, name)(*args)
    err = lib.hrfd_last_error().decode()
    assert rc == code, (name, args, rc, err)
    assert err.startswith(name), (name, args, err)


def creates(lib):
    """(function, arguments without the result pointer) of every create call that is refused for its arguments"""
    out = []
    for rate in (0, 3, 16):
        out += [("hrfd_ddc_create", (1, 1, rate, 0)), ("hrfd_duc_create", (1, 1, rate, 0)), ("hrfd_spec_create", (1, rate, 8, 0))]
    out += [("hrfd_ddc_create", (0, 1, 2, 0)), ("hrfd_ddc_create", (1, 0, 2, 0)),
            ("hrfd_duc_create", (0, 1, 2, 0)), ("hrfd_duc_create", (1, 0, 2, 0)), ("hrfd_spec_create", (0, 2, 8, 0)),
            ("hrfd_duc_create", (1, 32769, 2, 0)), ("hrfd_duc_create", (65537, 1, 2, 0)), ("hrfd_spec_create", (65537, 2, 8, 0)),
            ("hrfd_spec_create", (1, 2, 7, 0)), ("hrfd_spec_create", (1, 2, 14, 0))]
    return out


def test_create_refuses_bad_arguments_and_has_no_cpu_path(lib):
    for name, args in creates(lib):
        h = C.c_void_p(0x1234)
        refused(lib, name, *args, C.byref(h))
        if not (name == "hrfd_ddc_create" and 0 in args[:2]):   # the DDC's first check leaves *out alone
            assert h.value is None, (name, args)
    for name, args in (("hrfd_ddc_create", (1, 1, 2, 0)), ("hrfd_duc_create", (1, 1, 2, 0)), ("hrfd_spec_create", (1, 2, 8, 0))):
        refused(lib, name, *args, NULL)
        if lib.hrfd_device_count() == 0:
            h = C.c_void_p(0x1234)
            refused(lib, name, *args, C.byref(h), code=ENODEV)
            assert h.value is None, name


def test_every_entry_refuses_a_null_handle(lib):
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    u32, u64 = C.c_uint32(0), C.c_uint64(0)
    _, t = taps([1, 2])
    for name, args in [
            ("hrfd_ddc_reset", ()), ("hrfd_ddc_set_tuning", (0, 0, 0)), ("hrfd_ddc_set_gain_shift", (0, 0)),
            ("hrfd_ddc_set_filter", (0, t, 2)), ("hrfd_ddc_set_filter", (1, t, 2)), ("hrfd_ddc_get_phase", (0, C.byref(u32))),
            ("hrfd_ddc_process", (p, 2, p)), ("hrfd_ddc_process_device", (p, 4, 2, p, 2, NULL)),
            ("hrfd_duc_reset", ()), ("hrfd_duc_set_tuning", (0, 0, 0)), ("hrfd_duc_set_amplitude", (0, 0)),
            ("hrfd_duc_set_output_shift", (0, 0)), ("hrfd_duc_set_filter", (0, t, 2)), ("hrfd_duc_set_filter", (1, t, 2)),
            ("hrfd_duc_get_phase", (0, C.byref(u32))), ("hrfd_duc_get_clips", (0, C.byref(u64))),
            ("hrfd_duc_process", (p, 2, p)), ("hrfd_duc_process_device", (p, 2, 2, p, 4, NULL)),
            ("hrfd_spec_set_window", (NULL,)), ("hrfd_spec_set_band", (0, 0, 0, 1, 0)), ("hrfd_spec_clear_bands", ()),
            ("hrfd_spec_n_bands", (C.byref(u32),)), ("hrfd_spec_process", (p, 1, p, p, p)),
            ("hrfd_spec_process_device", (p, 512, 1, p, p, p, NULL))]:
        refused(lib, name, NULL, *args)


def test_set_filter_checks_its_taps_before_the_handle(lib):
    """a bad stage, too many taps and stage B's tap sum are refused with their own text, NULL handle or not; the DUC's stage
    A sum is per branch of the handle's R, so without a handle the refusal is the handle's"""
    _, one = taps([1])
    for bank in ("ddc", "duc"):
        name = f"hrfd_{bank}_set_filter"
        for stage in (-1, 2):
            refused(lib, name, NULL, stage, one, 1)
            assert "stage" in lib.hrfd_last_error().decode()
        for stage, n in ((0, 65), (1, 257)):
            keep, t = taps(np.zeros(n))
            refused(lib, name, NULL, stage, t, n)
            assert f"{n} taps" in lib.hrfd_last_error().decode()
        refused(lib, name, NULL, 1, NULL, 3)
        assert "3 taps" in lib.hrfd_last_error().decode()
        keep, t = taps([32767, -32768, 1])                      # 65536
        refused(lib, name, NULL, 1, t, 3)
        assert "65536" in lib.hrfd_last_error().decode()
        keep, t = taps([32767, -32768])                         # 65535: the refusal is the NULL handle's
        refused(lib, name, NULL, 1, t, 2)
        assert "NULL handle" in lib.hrfd_last_error().decode()
    keep, t = taps([32767, -32768, 1])
    refused(lib, "hrfd_ddc_set_filter", NULL, 0, t, 3)
    assert "65536" in lib.hrfd_last_error().decode()
    refused(lib, "hrfd_duc_set_filter", NULL, 0, t, 3)
    assert "NULL handle" in lib.hrfd_last_error().decode()


def test_setters_check_their_value_before_the_handle(lib):
    for name, args, word in (("hrfd_ddc_set_gain_shift", (0, 8), "8"), ("hrfd_duc_set_amplitude", (0, 32769), "32769"),
                             ("hrfd_duc_set_output_shift", (0, 25), "25"),
                             ("hrfd_spec_set_band", (0, 0, 0, 1, (1 << 44) + 1), "2^44")):
        refused(lib, name, NULL, *args)
        assert word in lib.hrfd_last_error().decode(), name
