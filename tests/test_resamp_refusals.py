"""Every refusal of the resampler bank (hrfd_resamp_*) that is decided before a device is needed, through the raw C ABI: the
return code, and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on a
handle's L, M or d cannot be shown without a device: K = ceil(T / L) > 512, a branch sum of 65536, a short out_capacity,
HRFD_ESTATE before set_taps, and out against the rows of all channels are refused in tests/test_gpu_resamp.py, and by the same
plain-C++ checks in tests/cpp/san_resamp.cc.  n_in L >= 2^31 is a rule the kernel's 32-bit q relies on, but no call can break
it: n_in <= 524288 and L <= 512 give 2^28 at the most (san_resamp.cc calls the check itself)."""
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


def i16(values):
    a = np.ascontiguousarray(values, dtype=np.int16)
    return a, a.ctypes.data_as(C.POINTER(C.c_int16))


def test_create_refuses_bad_ratios_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_resamp_create", n, 1, 1, 0, C.byref(h), word="channels")
        assert h.value is None
    for L, M in ((0, 1), (1, 0), (513, 1), (1, 513), (0xFFFFFFFF, 1), (513, 512)):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_resamp_create", 1, L, M, 0, C.byref(h), word="1..512")
        assert h.value is None
    for L, M in ((2, 2), (6, 4), (4, 6), (512, 256), (441, 147), (9, 3)):
        refused(lib, "hrfd_resamp_create", 1, L, M, 0, C.byref(C.c_void_p()), word="lowest terms")
    for L, M in ((1, 9), (2, 17), (63, 512), (3, 25)):
        refused(lib, "hrfd_resamp_create", 1, L, M, 0, C.byref(C.c_void_p()), word="more than 8 x up")
    refused(lib, "hrfd_resamp_create", 1, 1, 1, 0, NULL)
    if lib.hrfd_device_count() == 0:
        for C_, L, M in ((1, 1, 1), (65536, 512, 511), (3, 1, 8), (3, 64, 511), (1, 441, 80)):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_resamp_create", C_, L, M, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    buf = np.zeros(4096, dtype=np.int64)
    p, q = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 16384)
    n = C.c_uint32(77)
    _, taps = i16([16384])
    for name, args in [("hrfd_resamp_set_taps", (taps, 1)), ("hrfd_resamp_reset", (ALL,)), ("hrfd_resamp_reset", (65535,)),
                       ("hrfd_resamp_out_count", (1, C.byref(n))), ("hrfd_resamp_out_count", (524288, C.byref(n))),
                       ("hrfd_resamp_process", (p, NULL, 100, q, 100, C.byref(n))), ("hrfd_resamp_process", (p, p, 512, q, 0, C.byref(n))),
                       ("hrfd_resamp_process_device", (p, 200, NULL, 100, q, 1200, 600, C.byref(n), NULL)),
                       ("hrfd_resamp_process_device", (p, 1030, p, 512, q, 6, 3, C.byref(n), NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert n.value == 77
    assert lib.hrfd_resamp_destroy(NULL) == 0


def test_set_taps_checks_its_list_before_the_handle(lib):
    keep, taps = i16([1] * 16385)
    refused(lib, "hrfd_resamp_set_taps", NULL, taps, 0, word="taps")
    refused(lib, "hrfd_resamp_set_taps", NULL, taps, 16385, word="taps")
    refused(lib, "hrfd_resamp_set_taps", NULL, taps, 0xFFFFFFFF, word="taps")
    refused(lib, "hrfd_resamp_set_taps", NULL, NULL, 1, word="taps")
    refused(lib, "hrfd_resamp_set_taps", NULL, taps, 16384, word="NULL handle")


def test_reset_and_out_count_check_their_values_before_the_handle(lib):
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_resamp_reset", NULL, channel, word="channel")
    n = C.c_uint32(0)
    for n_in in (0, 524289, 0xFFFFFFFF):
        refused(lib, "hrfd_resamp_out_count", NULL, n_in, C.byref(n), word="n_in")
    refused(lib, "hrfd_resamp_out_count", NULL, 1, NULL, word="NULL argument")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, q = C.c_void_p(a), C.c_void_p(a + 65536)
    n = C.c_uint32(0)
    r = C.byref(n)
    dev, host = "hrfd_resamp_process_device", "hrfd_resamp_process"
    for n_in in (0, 524289, 0xFFFFFFFF):
        refused(lib, host, NULL, p, NULL, n_in, q, 8, r, word="n_in")
        refused(lib, dev, NULL, p, 1 << 33, NULL, n_in, q, 16, 8, r, NULL, word="n_in")
    # n_pcm needs whole blocks
    for n_in in (1, 511, 513, 1000, 524287):
        refused(lib, host, NULL, p, p, n_in, q, 8, r, word="multiple of 512")
        refused(lib, dev, NULL, p, 2 * n_in, p, n_in, q, 16, 8, r, NULL, word="multiple of 512")
    refused(lib, dev, NULL, p, 1024, C.c_void_p(a + 2), 512, q, 16, 8, r, NULL, word="4-byte aligned")
    # odd or short strides, on the input and on the output
    for stride, n_in in ((201, 100), (198, 100), (0, 1), (1, 1), (2 * 524288 - 2, 524288)):
        refused(lib, dev, NULL, p, stride, NULL, n_in, q, 16, 8, r, NULL, word="channel_stride_bytes")
    for stride, cap in ((17, 8), (14, 8), (0, 1), (2 * 3145728 - 2, 3145728)):
        refused(lib, dev, NULL, p, 200, NULL, 100, q, stride, cap, r, NULL, word="out_stride_bytes")
    # odd addresses
    refused(lib, dev, NULL, C.c_void_p(a + 1), 200, NULL, 100, q, 16, 8, r, NULL, word="even address")
    refused(lib, host, NULL, C.c_void_p(a + 3), NULL, 100, q, 8, r, word="even address")
    refused(lib, dev, NULL, p, 200, NULL, 100, C.c_void_p(a + 65537), 16, 8, r, NULL, word="even address")
    refused(lib, host, NULL, p, NULL, 100, C.c_void_p(a + 65539), 8, r, word="even address")
    # NULLs
    refused(lib, dev, NULL, NULL, 200, NULL, 100, q, 16, 8, r, NULL, word="NULL argument")
    refused(lib, dev, NULL, p, 200, NULL, 100, NULL, 16, 8, r, NULL, word="NULL argument")
    refused(lib, dev, NULL, p, 200, NULL, 100, q, 16, 8, NULL, NULL, word="NULL argument")
    refused(lib, host, NULL, NULL, NULL, 100, q, 8, r, word="NULL argument")
    refused(lib, host, NULL, p, NULL, 100, NULL, 8, r, word="NULL argument")
    refused(lib, host, NULL, p, NULL, 100, q, 8, NULL, word="NULL argument")
    # out over the input: the same, its last two bytes, its first two bytes; in place is no option
    for n_in, cap, off in ((100, 100, 0), (100, 600, 198), (100, 600, -1198), (512, 85, 2), (1, 1, 0)):
        refused(lib, dev, NULL, C.c_void_p(a + 8192), 2 * n_in, NULL, n_in, C.c_void_p(a + 8192 + off), 2 * cap, cap, r, NULL,
                word="overlaps")
        refused(lib, host, NULL, C.c_void_p(a + 8192), NULL, n_in, C.c_void_p(a + 8192 + off), cap, r, word="overlaps")
    # with everything else in order the refusal left is the handle's: out directly behind and in front of the input, padded
    # strides, every even residue, the limits themselves
    for n_in, cap, off in ((100, 600, 200), (100, 600, -1200), (1, 1, 2), (1, 1, -2)):
        refused(lib, dev, NULL, C.c_void_p(a + 8192), 2 * n_in, NULL, n_in, C.c_void_p(a + 8192 + off), 2 * cap, cap, r, NULL,
                word="NULL handle")
    for res in range(0, 16, 2):
        refused(lib, dev, NULL, C.c_void_p(a + res), 1030, p, 512, C.c_void_p(a + 65536 + 14 - res), 6150, 3072, r, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 2 * 524288, NULL, 524288, C.c_void_p(a + (1 << 21)), 2, 0, r, NULL, word="NULL handle")
    assert n.value == 0


def test_the_max_wgs_hook_is_inert_without_the_opt_in():
    """hrfd_resamp_debug_set_max_wgs: HRFD_ESTATE naming HRFD_DEBUG_HOOKS in a process without the opt-in, whatever its
    arguments; HRFD_EINVAL for the NULL handle in one with it (child processes: the library reads the variable once)"""
    from tests.hooks import check_max_wgs_hook_refusals
    check_max_wgs_hook_refusals("hrfd_resamp_debug_set_max_wgs")
