"""Every refusal of the HDLC framer bank (hrfd_hdlcgen_*, hrfd_hdlc_encode) that is decided before a device is needed, through
the raw C ABI: the return code, and an error text that starts with the public function's name and names the rule.  No GPU.
What depends on a handle cannot be shown without a device: a flag count out of range behind a real handle, a bound above
2^20 under the handle's flag counts, and rows of bits that overlap the records of a later channel are refused in
tests/test_gpu_hdlcgen.py, and by the same plain-C++ checks in tests/cpp/san_hdlcgen.cc.  The bank has no debug_set_max_wgs
hook to refuse: k_hdlcgen is one workgroup per channel, at most 65536 of them, so its launch is never cut."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

EINVAL, ENODEV = -1, -2
NULL = None


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
        refused(lib, "hrfd_hdlcgen_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_hdlcgen_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_hdlcgen_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def buffers():
    """records, n_frames, bits (misaligned), n_bits, n_sent, dropped: apart from one another in one block"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    return buf, a, C.c_void_p(a), C.c_void_p(a + 16384), C.c_void_p(a + 32769), C.c_void_p(a + 49152), C.c_void_p(a + 49156), C.c_void_p(a + 49160)


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    _keep, a, r, f, b, n, s, d = buffers()
    v = C.c_uint32(7)
    for name, args in [("hrfd_hdlcgen_set_flags", (12, 2, 3)), ("hrfd_hdlcgen_set_flags", (0, 1, 1)), ("hrfd_hdlcgen_set_flags", (255, 255, 255)),
                       ("hrfd_hdlcgen_max_bits", (1, 1, C.byref(v))), ("hrfd_hdlcgen_max_bits", (1, 1021, C.byref(v))),
                       ("hrfd_hdlcgen_max_bits", (64, 64 * 1021, C.byref(v))),
                       ("hrfd_hdlcgen_process", (r, 4, f, b, 1, n, s, d)), ("hrfd_hdlcgen_process", (r, 16384, f, b, 16000, n, NULL, NULL)),
                       ("hrfd_hdlcgen_process_device", (r, 4, 4, f, b, 1, 1, n, s, d, NULL)),
                       ("hrfd_hdlcgen_process_device", (r, 1036, 1032, f, b, 1231, 1229, n, NULL, NULL, NULL)),
                       ("hrfd_hdlcgen_process_device", (r, 1 << 33, 16384, f, b, 1 << 33, 16000, n, s, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert v.value == 7
    assert lib.hrfd_hdlcgen_destroy(NULL) == 0


def test_set_flags_checks_its_values_before_the_handle(lib):
    for lead in (256, 0xFFFFFFFF):
        refused(lib, "hrfd_hdlcgen_set_flags", NULL, lead, 2, 3, word=f"n_lead_flags {lead}")
    for between in (0, 256, 0xFFFFFFFF):
        refused(lib, "hrfd_hdlcgen_set_flags", NULL, 12, between, 3, word=f"n_between {between}")
    for tail in (0, 256, 0xFFFFFFFF):
        refused(lib, "hrfd_hdlcgen_set_flags", NULL, 12, 2, tail, word=f"n_tail_flags {tail}")


def test_max_bits_checks_its_arguments_before_the_handle(lib):
    v = C.c_uint32(7)
    refused(lib, "hrfd_hdlcgen_max_bits", NULL, 1, 1, NULL, word="result pointer")
    for n_frames, payload_bytes in ((0, 0), (0, 5), (2, 1), (1, 0), (1, 1022), (3, 3 * 1021 + 1), (0xFFFFFFFF, 0xFFFFFFFE), (1, 1 << 63)):
        refused(lib, "hrfd_hdlcgen_max_bits", NULL, n_frames, payload_bytes, C.byref(v), word="frames of")
    # more than a call's 2^20 bits under any flag counts: 107 frames of 1021 bytes are 1 050 825 bits and 107 flags
    refused(lib, "hrfd_hdlcgen_max_bits", NULL, 107, 107 * 1021, C.byref(v), word="more than one call")
    refused(lib, "hrfd_hdlcgen_max_bits", NULL, 65536, 65536, C.byref(v), word="more than one call")
    refused(lib, "hrfd_hdlcgen_max_bits", NULL, 0xFFFFFFFF, 1 << 40, C.byref(v), word="more than one call")
    assert v.value == 7


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    _keep, a, r, f, b, n, s, d = buffers()
    dev, host = "hrfd_hdlcgen_process_device", "hrfd_hdlcgen_process"
    for max_bits in (0, (1 << 20) + 1, 0xFFFFFFFF):
        refused(lib, host, NULL, r, 64, f, b, max_bits, n, s, d, word="max_bits")
        refused(lib, dev, NULL, r, 64, 64, f, b, 1 << 33, max_bits, n, s, d, NULL, word="max_bits")
    for in_bytes in (0, 1, 2, 3, 6, 65):
        refused(lib, host, NULL, r, in_bytes, f, b, 8, n, s, d, word=f"in_bytes {in_bytes}")
        refused(lib, dev, NULL, r, 1024, in_bytes, f, b, 8, 8, n, s, d, NULL, word=f"in_bytes {in_bytes}")
    for stride in (0, 60, 66, 63):
        refused(lib, dev, NULL, r, stride, 64, f, b, 8, 8, n, s, d, NULL, word=f"in_stride_bytes {stride}")
    # a row of bits shorter than the call may write
    for stride, max_bits in ((0, 1), (99, 100), ((1 << 20) - 1, 1 << 20)):
        refused(lib, dev, NULL, r, 64, 64, f, b, stride, max_bits, n, s, d, NULL, word=f"bits_stride_bytes {stride} is below max_bits")
    # addresses
    for off in (1, 2, 3):
        refused(lib, dev, NULL, C.c_void_p(a + off), 64, 64, f, b, 8, 8, n, s, d, NULL, word="4-byte aligned address")
        refused(lib, host, NULL, C.c_void_p(a + off), 64, f, b, 8, n, s, d, word="4-byte aligned address")
        bad = C.c_void_p(a + 50000 + off)
        for args in ((r, 64, 64, bad, b, 8, 8, n, s, d), (r, 64, 64, f, b, 8, 8, bad, s, d), (r, 64, 64, f, b, 8, 8, n, bad, d),
                     (r, 64, 64, f, b, 8, 8, n, s, bad)):
            refused(lib, dev, NULL, *args, NULL, word="must be 4-byte aligned")
        refused(lib, host, NULL, r, 64, bad, b, 8, n, s, d, word="must be 4-byte aligned")
    # what must be there: everything but n_sent and dropped
    for args in ((NULL, 64, 64, f, b, 8, 8, n, s, d), (r, 64, 64, NULL, b, 8, 8, n, s, d), (r, 64, 64, f, NULL, 8, 8, n, s, d),
                 (r, 64, 64, f, b, 8, 8, NULL, s, d)):
        refused(lib, dev, NULL, *args, NULL, word="NULL argument")
    refused(lib, host, NULL, NULL, 64, f, b, 8, n, s, d, word="NULL argument")
    refused(lib, host, NULL, r, 64, f, b, 8, NULL, s, d, word="NULL argument")
    # bits on the records, already with one channel
    for at in (a, a + 63, a - 7):
        refused(lib, dev, NULL, r, 64, 64, f, C.c_void_p(at), 8, 8, n, s, d, NULL, word="overlaps")
    # with everything else in order the refusal left is the handle's: rows of bits at every residue with an odd stride, that
    # touch the records without overlapping them, no n_sent, no dropped
    for res in range(8):
        refused(lib, dev, NULL, r, 68, 64, f, C.c_void_p(a + 32768 + res), 1231, 1229, n, NULL, NULL, NULL, word="NULL handle")
    refused(lib, dev, NULL, r, 64, 64, f, C.c_void_p(a + 64), 1 << 20, 1 << 20, n, s, d, NULL, word="NULL handle")
    refused(lib, dev, NULL, r, 64, 64, f, C.c_void_p(a - 8), 8, 8, n, s, d, NULL, word="NULL handle")


def test_the_host_framer_checks_everything_and_needs_no_handle(lib):
    _keep, a, r, f, b, n, s, d = buffers()
    name = "hrfd_hdlc_encode"
    for flags, word in (((256, 2, 3), "n_lead_flags 256"), ((12, 0, 3), "n_between 0"), ((12, 256, 3), "n_between 256"), ((12, 2, 0), "n_tail_flags 0"),
                        ((12, 2, 256), "n_tail_flags 256")):
        refused(lib, name, r, 64, 1, *flags, b, 100, n, s, d, word=word)
    for max_bits in (0, (1 << 20) + 1, 0xFFFFFFFF):
        refused(lib, name, r, 64, 1, 12, 2, 3, b, max_bits, n, s, d, word="max_bits")
    for in_bytes in (0, 2, 6, 65):
        refused(lib, name, r, in_bytes, 1, 12, 2, 3, b, 100, n, s, d, word=f"in_bytes {in_bytes}")
    refused(lib, name, C.c_void_p(a + 2), 64, 1, 12, 2, 3, b, 100, n, s, d, word="4-byte aligned address")
    refused(lib, name, r, 64, 1, 12, 2, 3, b, 100, C.c_void_p(a + 49153), s, d, word="must be 4-byte aligned")
    for args in ((NULL, 64, 1, 12, 2, 3, b, 100, n, s, d), (r, 64, 1, 12, 2, 3, NULL, 100, n, s, d), (r, 64, 1, 12, 2, 3, b, 100, NULL, s, d)):
        refused(lib, name, *args, word="NULL argument")
    # the bits on the records: the loop reads payload bytes while it writes bits.  Rows that touch are fine
    for at, max_bits in ((a, 100), (a + 63, 1), (a - 99, 100), (a - 7, 1 << 20)):
        refused(lib, name, r, 64, 1, 12, 2, 3, C.c_void_p(at), max_bits, n, s, d, word="overlaps")
    count = (C.c_uint32 * 3)(9, 9, 9)
    for at, max_bits in ((a + 64, 100), (a - 100, 100)):       # (a row of zeros holds no record: no byte is written)
        assert lib.hrfd_hdlc_encode(r, 64, 1, 12, 2, 3, C.c_void_p(at), max_bits, C.byref(count, 0), NULL, NULL) == 0 and count[0] == 0
    # in order: a row of zeros holds no record, so nothing is written and every frame asked for is dropped
    count = (C.c_uint32 * 3)(9, 9, 9)
    assert lib.hrfd_hdlc_encode(r, 64, 5, 0, 1, 1, b, 1, C.byref(count, 0), C.byref(count, 4), C.byref(count, 8)) == 0
    assert list(count) == [0, 0, 5]
    assert lib.hrfd_hdlc_encode(r, 64, 0, 255, 255, 255, b, 1 << 20, C.byref(count, 0), NULL, NULL) == 0 and list(count) == [0, 0, 5]
