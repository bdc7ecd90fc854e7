"""Every refusal of the level bank (hrfd_level_*) that is decided before a device is needed, through the raw C ABI: the return
code, and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on a handle's
channel count cannot be shown without a device: a channel number above it, and out against the rows of all channels, are
refused in tests/test_gpu_level.py, and by the same plain-C++ checks in tests/cpp/san_level.cc.  The bank has no
debug_set_max_wgs hook to refuse: k_level is one workgroup per channel, at most 65536 of them, so its launch is never cut
(DESIGN.md 3.13)."""
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


def u16(values):
    a = np.ascontiguousarray(values, dtype=np.uint16)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint16))


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_level_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_level_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_level_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    p, q, g, k = C.c_void_p(a), C.c_void_p(a + 16384), C.c_void_p(a + 32768), C.c_void_p(a + 40960)
    _, one = u16([32768])
    _, most = u16([32768] * 64)
    for name, args in [("hrfd_level_set_weights", (one, 1)), ("hrfd_level_set_weights", (most, 64)),
                       ("hrfd_level_set", (0, 0, 16)), ("hrfd_level_set", (ALL, 32767, 32768)), ("hrfd_level_set", (65535, 8192, 64)),
                       ("hrfd_level_set_bypass", (0, 1)), ("hrfd_level_set_bypass", (ALL, 0)), ("hrfd_level_set_bypass", (65535, -1)),
                       ("hrfd_level_reset", (ALL,)), ("hrfd_level_reset", (65535,)),
                       ("hrfd_level_process", (p, NULL, 1, q, g, k)), ("hrfd_level_process", (p, g, 4, p, NULL, NULL)),
                       ("hrfd_level_process", (p, NULL, 1, NULL, NULL, k)),
                       ("hrfd_level_process_device", (p, 1024, NULL, 1, q, 1024, g, k, NULL)),
                       ("hrfd_level_process_device", (p, 4100, g, 4, p, 4100, NULL, NULL, NULL)),
                       ("hrfd_level_process_device", (p, 1024, NULL, 1, NULL, 0, g, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_level_destroy(NULL) == 0


def test_set_weights_checks_its_table_before_the_handle(lib):
    keep, w = u16([32768] * 65)
    refused(lib, "hrfd_level_set_weights", NULL, w, 0, word="1..64 weights")
    refused(lib, "hrfd_level_set_weights", NULL, w, 65, word="1..64 weights")
    refused(lib, "hrfd_level_set_weights", NULL, w, 0xFFFFFFFF, word="1..64 weights")
    refused(lib, "hrfd_level_set_weights", NULL, NULL, 1, word="weights")
    for first in (0, 32767, 32769, 65535):
        keep2, bad = u16([first] + [100] * 63)
        for n in (1, 64):
            refused(lib, "hrfd_level_set_weights", NULL, bad, n, word="w[0] must be 32768")
    for k in (1, 17, 63):
        for v in (32769, 65535):
            table = [32768] * 64
            table[k] = v
            keep3, bad = u16(table)
            refused(lib, "hrfd_level_set_weights", NULL, bad, 64, word=f"w[{k}] = {v}")
            refused(lib, "hrfd_level_set_weights", NULL, bad, k + 1, word=f"w[{k}] = {v}")
            if k > 1:
                refused(lib, "hrfd_level_set_weights", NULL, bad, k, word="NULL handle")      # the entry lies behind W


def test_setters_check_their_values_before_the_handle(lib):
    for target in (32768, 65536, 0xFFFFFFFF):
        refused(lib, "hrfd_level_set", NULL, 0, target, 64, word=f"target {target}")
    for floor in (0, 15, 32769, 0xFFFFFFFF):
        refused(lib, "hrfd_level_set", NULL, 0, 8192, floor, word=f"floor {floor}")
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_level_set", NULL, channel, 8192, 64, word="channel")
        refused(lib, "hrfd_level_set_bypass", NULL, channel, 1, word="channel")
        refused(lib, "hrfd_level_reset", NULL, channel, word="channel")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, q, g, k = C.c_void_p(a + 65536), C.c_void_p(a + 131072), C.c_void_p(a), C.c_void_p(a + 32768)
    dev, host = "hrfd_level_process_device", "hrfd_level_process"
    for n_blocks in (0, 1025, 0xFFFFFFFF):
        refused(lib, host, NULL, p, NULL, n_blocks, q, g, k, word="n_blocks")
        refused(lib, dev, NULL, p, 1 << 33, NULL, n_blocks, q, 1 << 33, g, k, NULL, word="n_blocks")
    # at least one output
    refused(lib, host, NULL, p, NULL, 1, NULL, NULL, NULL, word="no output")
    refused(lib, dev, NULL, p, 1024, NULL, 1, NULL, 1024, NULL, NULL, NULL, word="no output")
    # odd or short strides, on the input and on the output; out's stride does not matter without out
    for stride, n_blocks in ((1025, 1), (1022, 1), (0, 1), (1, 1), (1024 * 1024 - 2, 1024)):
        refused(lib, dev, NULL, p, stride, NULL, n_blocks, q, 1 << 20, g, k, NULL, word="channel_stride_bytes")
        refused(lib, dev, NULL, p, 1 << 20, NULL, n_blocks, q, stride, g, k, NULL, word="out_stride_bytes")
        refused(lib, dev, NULL, p, 1 << 20, NULL, n_blocks, NULL, stride, g, k, NULL, word="NULL handle")
    # odd addresses of the PCM, out and peak; n_pcm and gain at 2 modulo 4
    refused(lib, dev, NULL, C.c_void_p(a + 65537), 1024, NULL, 1, q, 1024, g, k, NULL, word="even addresses")
    refused(lib, host, NULL, C.c_void_p(a + 65539), NULL, 1, q, g, k, word="even addresses")
    refused(lib, dev, NULL, p, 1024, NULL, 1, C.c_void_p(a + 131073), 1024, g, k, NULL, word="even addresses")
    refused(lib, host, NULL, p, NULL, 1, C.c_void_p(a + 131075), g, k, word="even addresses")
    refused(lib, dev, NULL, p, 1024, NULL, 1, q, 1024, g, C.c_void_p(a + 32769), NULL, word="even addresses")
    refused(lib, host, NULL, p, NULL, 1, q, g, C.c_void_p(a + 32771), word="even addresses")
    for off in (1, 2, 3):
        refused(lib, dev, NULL, p, 1024, NULL, 1, q, 1024, C.c_void_p(a + off), C.c_void_p(a + 32770), NULL,
                word="4-byte aligned" if off == 2 else None)
        refused(lib, host, NULL, p, C.c_void_p(a + 4096 + off), 1, q, g, k, word="4-byte aligned" if off == 2 else None)
    refused(lib, dev, NULL, p, 1024, C.c_void_p(a + 4098), 1, q, 1024, g, k, NULL, word="4-byte aligned")
    # no input
    refused(lib, dev, NULL, NULL, 1024, NULL, 1, q, 1024, g, k, NULL, word="NULL argument")
    refused(lib, host, NULL, NULL, NULL, 1, q, g, k, word="NULL argument")
    # every overlap of out and the input other than exact in-place, with the reason: shifted by a sample either way, by a row
    # less a sample either way, the same address under another stride
    base = a + 65536
    for n_blocks, off in ((1, 2), (1, -2), (1, 1022), (1, -1022), (4, 4094), (4, -4094), (4, 512), (1024, 1024 * 1024 - 2)):
        refused(lib, dev, NULL, C.c_void_p(base), 1024 * n_blocks, NULL, n_blocks, C.c_void_p(base + off), 1024 * n_blocks, g, k, NULL,
                word="overlaps the input (in place means out at the input's own address and stride")
        refused(lib, host, NULL, C.c_void_p(base), NULL, n_blocks, C.c_void_p(base + off), g, k, word="overlaps the input (in place")
    for stride, out_stride in ((1024, 1026), (1030, 1024), (2048, 4096)):
        refused(lib, dev, NULL, p, stride, NULL, 1, p, out_stride, g, k, NULL, word="overlaps the input (in place")
    # with everything else in order the refusal left is the handle's: in place under the same stride, dense and padded; out
    # directly behind and in front of the input; every even residue; a meter call; the limits themselves
    for stride in (1024, 1026, 4096):
        refused(lib, dev, NULL, p, stride, NULL, 1, p, stride, g, k, NULL, word="NULL handle")
    refused(lib, host, NULL, p, NULL, 3, p, g, k, word="NULL handle")
    for off in (1024, -1024):
        refused(lib, dev, NULL, p, 1024, NULL, 1, C.c_void_p(base + off), 1024, g, k, NULL, word="NULL handle")
        refused(lib, host, NULL, p, NULL, 1, C.c_void_p(base + off), g, k, word="NULL handle")
    for res in range(0, 16, 2):
        refused(lib, dev, NULL, C.c_void_p(base + res), 1030, g, 1, C.c_void_p(a + 131072 + 14 - res), 1026, C.c_void_p(a + 4096),
                C.c_void_p(a + 32768 + res), NULL, word="NULL handle")
        refused(lib, dev, NULL, C.c_void_p(base + res), 1030, NULL, 1, C.c_void_p(base + res), 1030, NULL, NULL, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1024, NULL, 1, NULL, 0, NULL, k, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1024 * 1024, NULL, 1024, p, 1024 * 1024, g, k, NULL, word="NULL handle")
