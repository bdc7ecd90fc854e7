"""Every refusal of the HDLC bank (hrfd_hdlc_*) that is decided before a device is needed, through the raw C ABI: the return
code, and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on a handle
cannot be shown without a device: a channel number above the handle's count is refused in tests/test_gpu_hdlc.py, and by the
same plain-C++ check in tests/cpp/san_hdlc.cc.  The bank has no debug_set_max_wgs hook to refuse: k_hdlc is one workgroup per
channel, at most 65536 of them, so its launch is never cut."""
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


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_hdlc_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_hdlc_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_hdlc_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def buffers():
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    return buf, a, C.c_void_p(a + 1), C.c_void_p(a + 16384), C.c_void_p(a + 32768), C.c_void_p(a + 49152), C.c_void_p(a + 49156), C.c_void_p(a + 49160)


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    _keep, a, b, n, o, f, x, d = buffers()
    v = C.c_uint32(7)
    for name, args in [("hrfd_hdlc_set_limits", (1, 512)), ("hrfd_hdlc_set_limits", (1, 1)), ("hrfd_hdlc_set_limits", (1021, 1021)),
                       ("hrfd_hdlc_set_require_carrier", (0,)), ("hrfd_hdlc_set_require_carrier", (1,)),
                       ("hrfd_hdlc_reset", (ALL,)), ("hrfd_hdlc_reset", (65535,)),
                       ("hrfd_hdlc_max_out", (1, C.byref(v))), ("hrfd_hdlc_max_out", (1 << 20, C.byref(v))),
                       ("hrfd_hdlc_process", (b, n, 1, o, 4, f, x, d)), ("hrfd_hdlc_process", (b, n, 1 << 20, o, 1 << 19, f, NULL, d)),
                       ("hrfd_hdlc_process_device", (b, 1, n, 1, o, 4, 4, f, x, d, NULL)),
                       ("hrfd_hdlc_process_device", (b, 1229, n, 1229, o, 1 << 20, 1024, f, NULL, d, NULL)),
                       ("hrfd_hdlc_process_device", (b, 1 << 33, n, 1 << 20, o, 1 << 33, 1 << 19, f, x, d, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert v.value == 7
    assert lib.hrfd_hdlc_destroy(NULL) == 0


def test_the_setters_check_their_values_before_the_handle(lib):
    for P in (0, 1022, 0xFFFFFFFF):
        refused(lib, "hrfd_hdlc_set_limits", NULL, 1, P, word=f"max_payload {P}")
    for m, P in ((0, 512), (513, 512), (2, 1), (0xFFFFFFFF, 1021)):
        refused(lib, "hrfd_hdlc_set_limits", NULL, m, P, word=f"min_payload {m}")
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_hdlc_reset", NULL, channel, word="channel")


def test_max_out_checks_its_arguments_before_the_handle(lib):
    v = C.c_uint32(0)
    for max_bits in (0, (1 << 20) + 1, 0xFFFFFFFF):
        refused(lib, "hrfd_hdlc_max_out", NULL, max_bits, C.byref(v), word="max_bits")
        refused(lib, "hrfd_hdlc_debug_max_out", max_bits, 1, 512, C.byref(v), word="max_bits")
    refused(lib, "hrfd_hdlc_max_out", NULL, 1, NULL, word="result pointer")
    refused(lib, "hrfd_hdlc_debug_max_out", 1, 1, 512, NULL, word="result pointer")
    refused(lib, "hrfd_hdlc_debug_max_out", 1, 0, 512, C.byref(v), word="min_payload 0")
    refused(lib, "hrfd_hdlc_debug_max_out", 1, 1, 1022, C.byref(v), word="max_payload 1022")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    _keep, a, b, n, o, f, x, d = buffers()
    dev, host = "hrfd_hdlc_process_device", "hrfd_hdlc_process"
    for max_bits in (0, (1 << 20) + 1, 0xFFFFFFFF):
        refused(lib, host, NULL, b, n, max_bits, o, 64, f, x, d, word="max_bits")
        refused(lib, dev, NULL, b, 1 << 33, n, max_bits, o, 64, 64, f, x, d, NULL, word="max_bits")
    # a row of bits shorter than the call reads
    for stride, max_bits in ((0, 1), (99, 100), ((1 << 20) - 1, 1 << 20)):
        refused(lib, dev, NULL, b, stride, n, max_bits, o, 64, 64, f, x, d, NULL, word=f"bits_stride_bytes {stride} is below max_bits")
    # the row of records: a multiple of 4, at least 4; the stride a multiple of 4 that holds it
    for out_bytes in (0, 1, 2, 3, 6, 65):
        refused(lib, host, NULL, b, n, 8, o, out_bytes, f, x, d, word=f"out_bytes {out_bytes}")
        refused(lib, dev, NULL, b, 8, n, 8, o, 1024, out_bytes, f, x, d, NULL, word=f"out_bytes {out_bytes}")
    for stride in (0, 60, 66, 63):
        refused(lib, dev, NULL, b, 8, n, 8, o, stride, 64, f, x, d, NULL, word=f"out_stride_bytes {stride}")
    # addresses
    for off in (1, 2, 3):
        refused(lib, dev, NULL, b, 8, n, 8, C.c_void_p(a + 32768 + off), 64, 64, f, x, d, NULL, word="4-byte aligned address")
        refused(lib, host, NULL, b, n, 8, C.c_void_p(a + 32768 + off), 64, f, x, d, word="4-byte aligned address")
        bad = C.c_void_p(a + 50000 + off)
        for args in ((b, 8, bad, 8, o, 64, 64, f, x, d), (b, 8, n, 8, o, 64, 64, bad, x, d), (b, 8, n, 8, o, 64, 64, f, bad, d),
                     (b, 8, n, 8, o, 64, 64, f, x, bad)):
            refused(lib, dev, NULL, *args, NULL, word="must be 4-byte aligned")
        refused(lib, host, NULL, b, bad, 8, o, 64, f, x, d, word="must be 4-byte aligned")
    # what must be there: everything but n_bad
    for args in ((NULL, 8, n, 8, o, 64, 64, f, x, d), (b, 8, NULL, 8, o, 64, 64, f, x, d), (b, 8, n, 8, NULL, 64, 64, f, x, d),
                 (b, 8, n, 8, o, 64, 64, NULL, x, d), (b, 8, n, 8, o, 64, 64, f, x, NULL)):
        refused(lib, dev, NULL, *args, NULL, word="NULL argument")
    refused(lib, host, NULL, NULL, n, 8, o, 64, f, x, d, word="NULL argument")
    refused(lib, host, NULL, b, n, 8, o, 64, f, x, NULL, word="NULL argument")
    # with everything else in order the refusal left is the handle's: rows of bits at every residue with an odd stride, no
    # n_bad, the limits themselves
    for res in range(8):
        refused(lib, dev, NULL, C.c_void_p(a + res), 1231, n, 1229, o, 68, 64, f, NULL, d, NULL, word="NULL handle")
    refused(lib, dev, NULL, b, 1 << 20, n, 1 << 20, o, 4, 4, f, x, d, NULL, word="NULL handle")
