"""Every refusal of the tone bank (hrfd_tone_*) that is decided before a device is needed, through the raw C ABI: the return
code, and an error text that starts with the public function's name and names what was wrong.  No GPU.  What only a handle
can decide (a call before any tones are set, blocks that are no whole number of the handle's frames, a window entry of
-32768) is refused by the same plain-C++ checks tests/cpp/san_tone.cc runs on the CPU, and through a handle in
tests/test_gpu_tone.py."""
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


def u32(values):
    a = np.ascontiguousarray(values, dtype=np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def u8(values):
    a = np.ascontiguousarray(values, dtype=np.uint8)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_create_refuses_bad_arguments_and_has_no_cpu_path(lib):
    for n in (0, 65537):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_tone_create", n, 256, 0, C.byref(h), word="channels")
        assert h.value is None
    for L in (0, 64, 192, 129, 16384, 0x80000000):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_tone_create", 1, L, 0, C.byref(h), word="frame_len")
        assert h.value is None
    refused(lib, "hrfd_tone_create", 1, 256, 0, NULL)
    if lib.hrfd_device_count() == 0:
        for L in (128, 8192):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_tone_create", 1, L, 0, C.byref(h), code=ENODEV)
            assert h.value is None
            refused(lib, "hrfd_tone_create", 65536, L, 0, C.byref(h), code=ENODEV)


def test_every_entry_refuses_a_null_handle(lib):
    buf = np.zeros(4096, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    _, steps = u32([1, 2, 3])
    _, groups = u8([0, 1, 3])
    k = C.c_uint32(7)
    for name, args in [("hrfd_tone_set_tones", (steps, groups, 3)), ("hrfd_tone_set_tones", (steps, NULL, 1)),
                       ("hrfd_tone_n_tones", (C.byref(k),)), ("hrfd_tone_set_window", (NULL,)),
                       ("hrfd_tone_set_window", (buf.ctypes.data_as(C.POINTER(C.c_int16)),)),
                       ("hrfd_tone_set_threshold", (0, 1 << 20, 1 << 43)), ("hrfd_tone_set_threshold", (ALL, 0, 0)),
                       ("hrfd_tone_process", (p, NULL, 1, p, p, p, p, p)), ("hrfd_tone_process", (p, p, 1024, NULL, NULL, NULL, NULL, p)),
                       ("hrfd_tone_process_device", (p, 1024, NULL, 1, p, p, p, p, p, NULL)),
                       ("hrfd_tone_process_device", (p, 1024 * 1024 + 2, p, 1024, NULL, p, NULL, NULL, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_tone_destroy(NULL) == 0


def test_set_tones_checks_its_list_before_the_handle(lib):
    _, steps = u32(list(range(130)))
    refused(lib, "hrfd_tone_set_tones", NULL, steps, NULL, 0, word="tones")
    refused(lib, "hrfd_tone_set_tones", NULL, steps, NULL, 129, word="tones")
    refused(lib, "hrfd_tone_set_tones", NULL, NULL, NULL, 1, word="tones")
    for bad in (4, 5, 255):
        for where in (0, 127):
            g = [3] * 128
            g[where] = bad
            keep, groups = u8(g)
            refused(lib, "hrfd_tone_set_tones", NULL, steps, groups, 128, word=f"group {bad}")
    # the limits themselves pass the list check: the refusal left is the handle's
    keep, groups = u8([3] * 128)
    refused(lib, "hrfd_tone_set_tones", NULL, steps, groups, 128, word="NULL handle")


def test_set_threshold_checks_its_values_before_the_handle(lib):
    for group in (4, 5, 0xFFFFFFFE):
        refused(lib, "hrfd_tone_set_threshold", NULL, group, 0, 0, word="group")
    for ratio in ((1 << 20) + 1, 0xFFFFFFFF):
        refused(lib, "hrfd_tone_set_threshold", NULL, 0, ratio, 0, word="ratio_q8")
        refused(lib, "hrfd_tone_set_threshold", NULL, ALL, ratio, 0, word="ratio_q8")
    for energy in ((1 << 43) + 1, (1 << 64) - 1):
        refused(lib, "hrfd_tone_set_threshold", NULL, 3, 1 << 20, energy, word="min_energy")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(4096, dtype=np.int64)
    a = buf.ctypes.data
    p, q = C.c_void_p(a), C.c_void_p(a + 1024)
    for n in (0, 1025, 0xFFFFFFFF):
        refused(lib, "hrfd_tone_process", NULL, p, NULL, n, q, q, q, q, q, word="n_blocks")
        refused(lib, "hrfd_tone_process_device", NULL, p, 1 << 32, NULL, n, q, q, q, q, q, NULL, word="n_blocks")
    refused(lib, "hrfd_tone_process", NULL, p, p, 1, NULL, NULL, NULL, NULL, NULL, word="no output")
    refused(lib, "hrfd_tone_process_device", NULL, p, 1024, p, 1, NULL, NULL, NULL, NULL, NULL, NULL, word="no output")
    # odd or short strides
    for stride, n in ((1025, 1), (1022, 1), (0, 1), (2046, 2), (1024 * 1024 - 2, 1024), (1024 * 1024 + 1, 1024)):
        refused(lib, "hrfd_tone_process_device", NULL, p, stride, NULL, n, q, q, q, q, q, NULL, word="channel_stride_bytes")
    # an odd PCM address, misaligned power, energy and valid
    refused(lib, "hrfd_tone_process_device", NULL, C.c_void_p(a + 1), 1024, NULL, 1, q, q, q, q, q, NULL, word="even address")
    refused(lib, "hrfd_tone_process", NULL, C.c_void_p(a + 3), NULL, 1, q, q, q, q, q, word="even address")
    for off in (1, 2, 4, 7):
        refused(lib, "hrfd_tone_process_device", NULL, p, 1024, NULL, 1, C.c_void_p(a + 1024 + off), q, q, q, q, NULL, word="aligned")
        refused(lib, "hrfd_tone_process_device", NULL, p, 1024, NULL, 1, q, C.c_void_p(a + 1024 + off), q, q, q, NULL, word="aligned")
    for off in (1, 2, 3):
        refused(lib, "hrfd_tone_process_device", NULL, p, 1024, NULL, 1, q, q, C.c_void_p(a + 1024 + off), q, q, NULL, word="aligned")
    refused(lib, "hrfd_tone_process_device", NULL, NULL, 1024, NULL, 1, q, q, q, q, q, NULL, word="NULL argument")
    # with everything else in order the refusal left is the handle's: the limits themselves, a stride of exactly one row or
    # more, best and present at any address, any single output
    refused(lib, "hrfd_tone_process_device", NULL, C.c_void_p(a + 2), 1024 * 1024, p, 1024, q, q, C.c_void_p(a + 1028),
            C.c_void_p(a + 1025), C.c_void_p(a + 1027), NULL, word="NULL handle")
    for i in range(5):
        outs = [NULL] * 5
        outs[i] = q
        refused(lib, "hrfd_tone_process_device", NULL, p, 1026, NULL, 1, *outs, NULL, word="NULL handle")
        refused(lib, "hrfd_tone_process", NULL, p, NULL, 1, *outs, word="NULL handle")


def test_the_max_wgs_hook_is_inert_without_the_opt_in():
    """hrfd_tone_debug_set_max_wgs: HRFD_ESTATE naming HRFD_DEBUG_HOOKS in a process without the opt-in, whatever its
    arguments; HRFD_EINVAL for the NULL handle in one with it (child processes: the library reads the variable once)"""
    from tests.hooks import check_max_wgs_hook_refusals
    check_max_wgs_hook_refusals("hrfd_tone_debug_set_max_wgs")
