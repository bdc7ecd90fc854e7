"""Every refusal of the AFSK bank (hrfd_afsk_*) that is decided before a device is needed, through the raw C ABI: the return
code, and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on a handle
cannot be shown without a device: a channel number above the handle's count, and a bits_stride below the bound of the
handle's own modem, are refused in tests/test_gpu_afsk.py, and by the same plain-C++ checks in tests/cpp/san_afsk.cc.  The
bank has no debug_set_max_wgs hook to refuse: k_afsk is one workgroup per channel, at most 65536 of them, so its launch is
never cut."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

EINVAL, ENODEV = -1, -2
NULL = None
ALL = 0xFFFFFFFF
MARK, SPACE, BAUD = 644245094, 1181116006, 644245094


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
        refused(lib, "hrfd_afsk_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_afsk_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_afsk_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    p, b, n, h = C.c_void_p(a), C.c_void_p(a + 16384), C.c_void_p(a + 32768), C.c_void_p(a + 40960)
    v = C.c_uint32(7)
    for name, args in [("hrfd_afsk_set_modem", (MARK, SPACE, BAUD, 8, 2, 1)), ("hrfd_afsk_set_modem", (1, 1 << 31, 1 << 31, 2, 1, 0)),
                       ("hrfd_afsk_set_modem", (1 << 31, 1, 1, 32, 8, -1)),
                       ("hrfd_afsk_set_carrier", (0,)), ("hrfd_afsk_set_carrier", ((1 << 64) - 1,)),
                       ("hrfd_afsk_reset", (ALL,)), ("hrfd_afsk_reset", (65535,)),
                       ("hrfd_afsk_max_bits", (1, C.byref(v))), ("hrfd_afsk_max_bits", (1024, C.byref(v))),
                       ("hrfd_afsk_process", (p, NULL, 1, b, n, h)), ("hrfd_afsk_process", (p, n, 4, NULL, NULL, h)),
                       ("hrfd_afsk_process", (p, NULL, 1024, b, n, NULL)),
                       ("hrfd_afsk_process_device", (p, 1024, NULL, 1, b, 2, n, h, NULL)),
                       ("hrfd_afsk_process_device", (p, 4100, n, 4, NULL, 0, NULL, h, NULL)),
                       ("hrfd_afsk_process_device", (p, 1 << 20, NULL, 1024, b, 1 << 20, n, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert v.value == 7
    assert lib.hrfd_afsk_destroy(NULL) == 0


def test_set_modem_checks_its_values_before_the_handle(lib):
    for W in (0, 1, 33, 0xFFFFFFFF):
        refused(lib, "hrfd_afsk_set_modem", NULL, MARK, SPACE, BAUD, W, 2, 1, word=f"window {W}")
    for A in (0, 9, 0xFFFFFFFF):
        refused(lib, "hrfd_afsk_set_modem", NULL, MARK, SPACE, BAUD, 8, A, 1, word=f"loop shift {A}")
    for step in (0, (1 << 31) + 1, 0xFFFFFFFF):
        refused(lib, "hrfd_afsk_set_modem", NULL, MARK, SPACE, step, 8, 2, 1, word=f"baud_step {step}")
        refused(lib, "hrfd_afsk_set_modem", NULL, step, SPACE, BAUD, 8, 2, 1, word=f"mark_step {step}")
        refused(lib, "hrfd_afsk_set_modem", NULL, MARK, step, BAUD, 8, 2, 1, word=f"space_step {step}")
    refused(lib, "hrfd_afsk_set_modem", NULL, MARK, SPACE, (1 << 31) + 1, 8, 2, 1, word="at most one bit per sample")
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_afsk_reset", NULL, channel, word="channel")


def test_max_bits_checks_its_arguments_before_the_handle(lib):
    v = C.c_uint32(0)
    for n_blocks in (0, 1025, 0xFFFFFFFF):
        refused(lib, "hrfd_afsk_max_bits", NULL, n_blocks, C.byref(v), word="n_blocks")
    refused(lib, "hrfd_afsk_max_bits", NULL, 1, NULL, word="result pointer")


def test_the_debug_entries_refuse_what_the_contract_refuses(lib):
    out = np.zeros(128, dtype=np.int16)
    o = out.ctypes.data_as(C.POINTER(C.c_int16))
    refused(lib, "hrfd_afsk_debug_taps", MARK, SPACE, 33, o, word="window 33")
    refused(lib, "hrfd_afsk_debug_taps", 0, SPACE, 8, o, word="mark_step 0")
    refused(lib, "hrfd_afsk_debug_taps", MARK, SPACE, 8, NULL, word="result pointer")
    m = np.array([MARK, SPACE, BAUD, 8, 9, 1], dtype=np.uint32)
    st = np.zeros(18, dtype=np.uint32)
    x = np.zeros(512, dtype=np.int16)
    hard = np.zeros(64, dtype=np.uint8)
    u32 = lambda a_: a_.ctypes.data_as(C.POINTER(C.c_uint32))
    refused(lib, "hrfd_afsk_debug_slow", u32(m), 0, C.c_void_p(x.ctypes.data), NULL, 1, u32(st), NULL, NULL, C.c_void_p(hard.ctypes.data),
            word="loop shift 9")
    m[4] = 2
    refused(lib, "hrfd_afsk_debug_slow", u32(m), 0, C.c_void_p(x.ctypes.data), NULL, 1, u32(st), NULL, NULL, NULL, word="no output")
    refused(lib, "hrfd_afsk_debug_slow", NULL, 0, C.c_void_p(x.ctypes.data), NULL, 1, u32(st), NULL, NULL, NULL, word="NULL argument")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, b, n, h = C.c_void_p(a + 65536), C.c_void_p(a + 131072), C.c_void_p(a), C.c_void_p(a + 32768)
    dev, host = "hrfd_afsk_process_device", "hrfd_afsk_process"
    for n_blocks in (0, 1025, 0xFFFFFFFF):
        refused(lib, host, NULL, p, NULL, n_blocks, b, n, h, word="n_blocks")
        refused(lib, dev, NULL, p, 1 << 33, NULL, n_blocks, b, 1 << 33, n, h, NULL, word="n_blocks")
    # at least one output; bits and n_bits go together
    refused(lib, host, NULL, p, NULL, 1, NULL, NULL, NULL, word="no output")
    refused(lib, dev, NULL, p, 1024, NULL, 1, NULL, 1024, NULL, NULL, NULL, word="no output")
    for hard in (h, NULL):
        refused(lib, host, NULL, p, NULL, 1, b, NULL, hard, word="bits and n_bits go together")
        refused(lib, host, NULL, p, NULL, 1, NULL, n, hard, word="bits and n_bits go together")
        refused(lib, dev, NULL, p, 1024, NULL, 1, b, 1024, NULL, hard, NULL, word="bits and n_bits go together")
        refused(lib, dev, NULL, p, 1024, NULL, 1, NULL, 1024, n, hard, NULL, word="bits and n_bits go together")
    # odd or short strides of the PCM
    for stride, n_blocks in ((1025, 1), (1022, 1), (0, 1), (1, 1), (1024 * 1024 - 2, 1024)):
        refused(lib, dev, NULL, p, stride, NULL, n_blocks, b, 1 << 20, n, h, NULL, word="channel_stride_bytes")
    # a row of bits below the bound of the slowest modem there is (baud_step 1, A = 8: 2^23 a sample) is too short for any;
    # the stride is not looked at without bits
    for n_blocks, low in ((1, 2), (512, 513), (1024, 1025)):
        refused(lib, dev, NULL, p, 1 << 20, NULL, n_blocks, b, low - 1, n, h, NULL, word=f"bits_stride_bytes {low - 1} is below")
        refused(lib, dev, NULL, p, 1 << 20, NULL, n_blocks, b, low, n, h, NULL, word="NULL handle")
        refused(lib, dev, NULL, p, 1 << 20, NULL, n_blocks, NULL, 0, NULL, h, NULL, word="NULL handle")
    # an odd address of the PCM; n_pcm and n_bits off a 4-byte boundary
    refused(lib, dev, NULL, C.c_void_p(a + 65537), 1024, NULL, 1, b, 1024, n, h, NULL, word="even address")
    refused(lib, host, NULL, C.c_void_p(a + 65539), NULL, 1, b, n, h, word="even address")
    for off in (1, 2, 3):
        refused(lib, dev, NULL, p, 1024, NULL, 1, b, 1024, C.c_void_p(a + off), h, NULL, word="n_pcm and n_bits must be 4-byte aligned")
        refused(lib, host, NULL, p, NULL, 1, b, C.c_void_p(a + off), h, word="n_pcm and n_bits must be 4-byte aligned")
        refused(lib, dev, NULL, p, 1024, C.c_void_p(a + 4096 + off), 1, b, 1024, n, h, NULL, word="n_pcm and n_bits must be 4-byte aligned")
        refused(lib, host, NULL, p, C.c_void_p(a + 4096 + off), 1, b, n, h, word="n_pcm and n_bits must be 4-byte aligned")
    # no input
    refused(lib, dev, NULL, NULL, 1024, NULL, 1, b, 1024, n, h, NULL, word="NULL argument")
    refused(lib, host, NULL, NULL, NULL, 1, b, n, h, word="NULL argument")
    # with everything else in order the refusal left is the handle's: every even residue of the PCM, bits and hard at odd
    # addresses (they are bytes), a padded stride, only hard, the limits themselves
    for res in range(0, 16, 2):
        refused(lib, dev, NULL, C.c_void_p(a + 65536 + res), 1030, n, 1, C.c_void_p(a + 131073), 77, C.c_void_p(a + 4096),
                C.c_void_p(a + 32769), NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1024, NULL, 1, NULL, 0, NULL, h, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1024 * 1024, NULL, 1024, b, 1 << 20, n, h, NULL, word="NULL handle")
