"""Every refusal of the conditioner bank (hrfd_cal_*) that is decided before a device is needed, through the raw C ABI: the
return code, and an error text that starts with the public function's name and names what was wrong.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

EINVAL, ENODEV = -1, -2
NULL = None
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, name, *args, code=EINVAL, word=None):
    rc = getattr(lib, name)(*args)
    err = lib.hrfd_last_error().decode()
    assert rc == code, (name, args, rc, err)
    assert err.startswith(name), (name, args, err)
    if word is not None:
        assert word in err, (name, word, err)


def i32(values):
    a = np.ascontiguousarray(values, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def i16(values):
    a = np.ascontiguousarray(values, dtype=np.int16)
    return a, a.ctypes.data_as(C.POINTER(C.c_int16))


def test_create_refuses_bad_arguments_and_has_no_cpu_path(lib):
    for n in (0, 65537):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_cal_create", n, 0, C.byref(h), word="captures")
        assert h.value is None
    refused(lib, "hrfd_cal_create", 1, 0, NULL)
    if lib.hrfd_device_count() == 0:
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_cal_create", 1, 0, C.byref(h), code=ENODEV)
        assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    _, dc = i32([0, 0])
    _, m = i16([16384, 0, 0, 16384])
    for name, args in [("hrfd_cal_set_correction", (0, dc, m)), ("hrfd_cal_set_correction", (ALL, NULL, NULL)),
                       ("hrfd_cal_get_correction", (0, dc, m)), ("hrfd_cal_process", (p, 16, p, p)),
                       ("hrfd_cal_process_device", (p, 16, 16, p, 16, p, NULL))]:
        refused(lib, name, NULL, *args)
    assert lib.hrfd_cal_destroy(NULL) == 0
    refused(lib, "hrfd_cal_solve", NULL, dc, m)
    refused(lib, "hrfd_cal_solve", buf.ctypes.data_as(C.POINTER(C.c_int64)), NULL, m)
    refused(lib, "hrfd_cal_solve", buf.ctypes.data_as(C.POINTER(C.c_int64)), dc, NULL)


def test_set_correction_checks_its_record_before_the_handle(lib):
    """the row rule |m_a| + |m_b| <= 32768 on both rows and |dc| <= 32512, each with its own text, NULL handle or not"""
    _, dc0 = i32([0, 0])
    _, ident = i16([16384, 0, 0, 16384])
    for row, m in ((0, (32767, 2, 0, 0)), (0, (-32768, -1, 0, 0)), (0, (16385, -16384, 0, 0)), (1, (0, 0, 32767, 2)),
                   (1, (16384, 0, -32768, 1)), (1, (1, 0, 1, -32768))):
        keep, mp = i16(m)
        refused(lib, "hrfd_cal_set_correction", NULL, 0, dc0, mp, word=f"row {row}")
        assert "32769" in lib.hrfd_last_error().decode()
        refused(lib, "hrfd_cal_set_correction", NULL, 0, NULL, mp, word=f"row {row}")
    for dc in ((32513, 0), (0, -32513), (-(1 << 31), 0), (0, (1 << 31) - 1)):
        keep, dp = i32(dc)
        refused(lib, "hrfd_cal_set_correction", NULL, 0, dp, ident, word="dc")
        refused(lib, "hrfd_cal_set_correction", NULL, ALL, dp, NULL, word="dc")
    # the limits themselves pass the record check: the refusal left is the handle's
    for m in ((32767, 1, -1, -32767), (-32768, 0, 0, -32768)):
        keep, mp = i16(m)
        keep2, dp = i32((32512, -32512))
        refused(lib, "hrfd_cal_set_correction", NULL, 0, dp, mp, word="bad handle or capture")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(64, dtype=np.int64)
    a = buf.ctypes.data
    p, q = C.c_void_p(a), C.c_void_p(a + 256)
    for n in (0, 1, 3, 17, (1 << 30) + 2, 0xFFFFFFFE, 0xFFFFFFFF):
        refused(lib, "hrfd_cal_process", NULL, p, n, q, q, word="n_bytes")
        refused(lib, "hrfd_cal_process_device", NULL, p, 1 << 31, n, q, 1 << 31, q, NULL, word="n_bytes")
    refused(lib, "hrfd_cal_process", NULL, p, 16, NULL, NULL, word="neither")
    refused(lib, "hrfd_cal_process_device", NULL, p, 16, 16, NULL, 16, NULL, NULL, word="neither")
    refused(lib, "hrfd_cal_process_device", NULL, p, 14, 16, q, 16, NULL, NULL, word="strides")
    refused(lib, "hrfd_cal_process_device", NULL, p, 16, 16, q, 14, NULL, NULL, word="strides")
    refused(lib, "hrfd_cal_process_device", NULL, p, 16, 16, NULL, 0, C.c_void_p(a + 4), NULL, word="8-byte")
    # in place: the same address needs the same strides
    refused(lib, "hrfd_cal_process_device", NULL, p, 32, 16, p, 48, NULL, NULL, word="in place")
    refused(lib, "hrfd_cal_process_device", NULL, p, 48, 16, p, 32, q, NULL, word="in place")
    # with everything else in order the refusal left is the handle's, an output stride is not looked at without an output,
    # and 2^30 bytes are allowed
    refused(lib, "hrfd_cal_process_device", NULL, p, 32, 16, p, 32, NULL, NULL, word="NULL argument")
    refused(lib, "hrfd_cal_process_device", NULL, p, 16, 16, NULL, 0, q, NULL, word="NULL argument")
    refused(lib, "hrfd_cal_process_device", NULL, p, 1 << 30, 1 << 30, NULL, 0, q, NULL, word="NULL argument")


def test_the_workgroup_hook_is_inert_without_the_opt_in():
    """hrfd_cal_debug_set_workgroups changes how a launch is cut, so it answers HRFD_ESTATE in a process that did not start
    with HRFD_DEBUG_HOOKS=1, before it looks at its arguments; with the opt-in it refuses the NULL handle and a bad count"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from hackrfdiags_amd import _lib\n"
            "L = _lib.load()\n"
            "print(L.hrfd_cal_debug_set_workgroups(None, 1), L.hrfd_last_error().decode())\n" % root)
    env = {k: v for k, v in os.environ.items() if k != "HRFD_DEBUG_HOOKS"}
    off = subprocess.check_output([sys.executable, "-c", code], env=env, text=True)
    assert off.startswith("-4 hrfd_cal_debug_set_workgroups") and "HRFD_DEBUG_HOOKS" in off, off
    on = subprocess.check_output([sys.executable, "-c", code], env={**env, "HRFD_DEBUG_HOOKS": "1"}, text=True)
    assert on.startswith("-1 hrfd_cal_debug_set_workgroups"), on
