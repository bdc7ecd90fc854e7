"""Every refusal of the audio bank (hrfd_audio_*) that is decided before a device is needed, through the raw C ABI: the
return code, and an error text that starts with the public function's name and names what was wrong.  No GPU.  A channel or
a bus is checked twice: against the largest any handle can have (65536 channels, 64 buses) before the handle is looked at,
which is what can be shown here, and against the handle's own sizes after it (tests/test_gpu_audio.py, and the same plain-C++
checks in tests/cpp/san_audio.cc); the overlap of d_out with the input likewise, for one channel here and for the handle's
rows there."""
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


def u32(values):
    a = np.ascontiguousarray(values, dtype=np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_audio_create", n, 1, 0, C.byref(h), word="channels")
        assert h.value is None
    for m in (0, 65, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_audio_create", 1, m, 0, C.byref(h), word="buses")
        assert h.value is None
    refused(lib, "hrfd_audio_create", 1, 1, 0, NULL)
    if lib.hrfd_device_count() == 0:
        for n, m in ((1, 1), (65536, 64)):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_audio_create", n, m, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    buf = np.zeros(4096, dtype=np.int64)
    p, q = C.c_void_p(buf.ctypes.data), C.c_void_p(buf.ctypes.data + 8192)
    _, taps = i16([16384])
    _, ch = u32([0, 65535])
    _, g = i16([32767, -32767])
    for name, args in [("hrfd_audio_set_taps", (taps, 1)), ("hrfd_audio_set_bus", (0, ch, g, 2)), ("hrfd_audio_set_bus", (63, NULL, NULL, 0)),
                       ("hrfd_audio_set_want", (0, 0)), ("hrfd_audio_set_want", (ALL, 127)), ("hrfd_audio_set_want", (65535, 254)),
                       ("hrfd_audio_set_want", (0, 255)), ("hrfd_audio_reset", (ALL,)), ("hrfd_audio_reset", (65535,)),
                       ("hrfd_audio_gate", (p, p, 128, 3, 1, q)), ("hrfd_audio_gate_device", (p, p, 8192, 0, 1024, q, NULL)),
                       ("hrfd_audio_process", (p, NULL, NULL, 1, q, q, q)), ("hrfd_audio_process", (p, p, p, 1, NULL, q, NULL)),
                       ("hrfd_audio_process_device", (p, 1024, NULL, NULL, 1, q, 1024, q, q, NULL)),
                       ("hrfd_audio_process_device", (p, 1026, p, p, 1, q, 1030, NULL, NULL, NULL)),
                       ("hrfd_audio_process_device", (p, 1024 * 1024, p, p, 1024, NULL, 0, q, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_audio_destroy(NULL) == 0


def test_set_taps_checks_its_list_before_the_handle(lib):
    keep, taps = i16([1] * 513)
    refused(lib, "hrfd_audio_set_taps", NULL, taps, 0, word="taps")
    refused(lib, "hrfd_audio_set_taps", NULL, taps, 513, word="taps")
    refused(lib, "hrfd_audio_set_taps", NULL, NULL, 1, word="taps")
    for h in ([32767, -32767, 2], [-32768, -32768], [128] * 512):
        assert sum(abs(v) for v in h) == 65536
        keep, taps = i16(h)
        refused(lib, "hrfd_audio_set_taps", NULL, taps, len(h), word="sum |h| = 65536")
    # the limits themselves pass the list check: the refusal left is the handle's
    for h in ([32767, -32767, 1], [128] * 511 + [127], [-32768, 32767]):
        keep, taps = i16(h)
        refused(lib, "hrfd_audio_set_taps", NULL, taps, len(h), word="NULL handle")


def test_set_bus_checks_its_list_before_the_handle(lib):
    keep_c, ch = u32([0] * 4097)
    keep_g, g = i16([1] * 4097)
    refused(lib, "hrfd_audio_set_bus", NULL, 64, ch, g, 1, word="bus 64")
    refused(lib, "hrfd_audio_set_bus", NULL, ALL, ch, g, 1, word="bus")
    refused(lib, "hrfd_audio_set_bus", NULL, 0, ch, g, 4097, word="4097")
    refused(lib, "hrfd_audio_set_bus", NULL, 0, NULL, g, 1, word="arrays")
    refused(lib, "hrfd_audio_set_bus", NULL, 0, ch, NULL, 1, word="arrays")
    for where in (0, 4095):
        gains = [32767] * 4096
        gains[where] = -32768
        keep_g2, g2 = i16(gains)
        refused(lib, "hrfd_audio_set_bus", NULL, 0, ch, g2, 4096, word=f"entry {where} has gain -32768")
        chans = [65535] * 4096
        chans[where] = 65536
        keep_c2, c2 = u32(chans)
        refused(lib, "hrfd_audio_set_bus", NULL, 0, c2, g, 4096, word=f"entry {where} names channel 65536")
    refused(lib, "hrfd_audio_set_bus", NULL, 63, ch, g, 4096, word="NULL handle")


def test_set_want_and_reset_check_their_values_before_the_handle(lib):
    for want in (128, 129, 200, 253, 256, 0xFFFFFFFF):
        refused(lib, "hrfd_audio_set_want", NULL, 0, want, word="want")
        refused(lib, "hrfd_audio_set_want", NULL, ALL, want, word="want")
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_audio_set_want", NULL, channel, 0, word="channel")
        refused(lib, "hrfd_audio_reset", NULL, channel, word="channel")


def test_gate_checks_sizes_before_the_handle(lib):
    buf = np.zeros(64, dtype=np.int64)
    p = C.c_void_p(buf.ctypes.data)
    for name, tail in (("hrfd_audio_gate", ()), ("hrfd_audio_gate_device", (NULL,))):
        for n in (0, 1025, 0xFFFFFFFF):
            refused(lib, name, NULL, p, p, 512, 0, n, p, *tail, word="n_blocks")
        for L in (0, 64, 127, 192, 384, 16384, 0x80000000):
            refused(lib, name, NULL, p, p, L, 0, 16, p, *tail, word="frame_len")
        for L, n in ((1024, 1), (1024, 3), (8192, 8), (8192, 1016), (4096, 1020)):
            refused(lib, name, NULL, p, p, L, 0, n, p, *tail, word="whole number of frames")
        for group in (4, 5, 0xFFFFFFFF):
            refused(lib, name, NULL, p, p, 128, group, 1, p, *tail, word="group")
        for args in ((NULL, p, p), (p, NULL, p), (p, p, NULL)):
            refused(lib, name, NULL, args[0], args[1], 128, 3, 1, args[2], *tail, word="NULL argument")
        refused(lib, name, NULL, p, p, 8192, 3, 1024, p, *tail, word="NULL handle")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, q = C.c_void_p(a), C.c_void_p(a + 65536)
    dev, host = "hrfd_audio_process_device", "hrfd_audio_process"
    for n in (0, 1025, 0xFFFFFFFF):
        refused(lib, host, NULL, p, NULL, NULL, n, q, q, q, word="n_blocks")
        refused(lib, dev, NULL, p, 1 << 32, NULL, NULL, n, q, 1 << 32, q, q, NULL, word="n_blocks")
    # both outputs NULL, with and without clips
    refused(lib, host, NULL, p, p, p, 1, NULL, NULL, q, word="no output")
    refused(lib, dev, NULL, p, 1024, p, p, 1, NULL, 1024, NULL, NULL, NULL, word="no output")
    # odd or short strides, on the input and on the output
    for stride, n in ((1025, 1), (1022, 1), (0, 1), (2046, 2), (1024 * 1024 - 2, 1024), (1024 * 1024 + 1, 1024)):
        refused(lib, dev, NULL, p, stride, NULL, NULL, n, q, 1024 * n, q, q, NULL, word="channel_stride_bytes")
        refused(lib, dev, NULL, p, 1024 * n, NULL, NULL, n, q, stride, q, q, NULL, word="out_stride_bytes")
    # odd addresses
    refused(lib, dev, NULL, C.c_void_p(a + 1), 1024, NULL, NULL, 1, q, 1024, q, q, NULL, word="even address")
    refused(lib, host, NULL, C.c_void_p(a + 3), NULL, NULL, 1, q, q, q, word="even address")
    refused(lib, dev, NULL, p, 1024, NULL, NULL, 1, C.c_void_p(a + 65537), 1024, q, q, NULL, word="even address")
    refused(lib, dev, NULL, p, 1024, NULL, NULL, 1, q, 1024, C.c_void_p(a + 65539), q, NULL, word="even address")
    for off in (1, 2, 3):
        refused(lib, dev, NULL, p, 1024, NULL, NULL, 1, q, 1024, q, C.c_void_p(a + 65536 + off), NULL, word="aligned")
    refused(lib, dev, NULL, NULL, 1024, NULL, NULL, 1, q, 1024, q, q, NULL, word="NULL argument")
    # d_out over the input: the same, the last two bytes, the first two bytes; in place is no option
    for n, off in ((1, 0), (1, 1022), (1, -1022), (4, 4094), (4, -4094), (4, 2)):
        refused(lib, dev, NULL, C.c_void_p(a + 8192), 1024 * n, NULL, NULL, n, C.c_void_p(a + 8192 + off), 1024 * n, q, q, NULL,
                word="overlaps")
        refused(lib, host, NULL, C.c_void_p(a + 8192), NULL, NULL, n, C.c_void_p(a + 8192 + off), q, q, word="overlaps")
    # with everything else in order the refusal left is the handle's: the limits themselves, out directly behind and in
    # front of the input, padded strides, every even residue, each output alone
    for n, off in ((1, 1024), (1, -1024), (4, 4096), (4, -4096)):
        refused(lib, dev, NULL, C.c_void_p(a + 8192), 1024 * n, NULL, NULL, n, C.c_void_p(a + 8192 + off), 1024 * n, q, q, NULL,
                word="NULL handle")
    refused(lib, dev, NULL, C.c_void_p(a + 2), 1024 * 1024 + 6, p, p, 1024, NULL, 0, C.c_void_p(a + 65538), C.c_void_p(a + 65540), NULL,
            word="NULL handle")
    refused(lib, dev, NULL, p, 1026, NULL, NULL, 1, q, 1030, NULL, NULL, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1026, NULL, NULL, 1, q, 1030, NULL, q, NULL, word="NULL handle")
    refused(lib, host, NULL, p, NULL, NULL, 1, NULL, q, NULL, word="NULL handle")


def test_the_max_wgs_hook_is_inert_without_the_opt_in():
    """hrfd_audio_debug_set_max_wgs: HRFD_ESTATE naming HRFD_DEBUG_HOOKS in a process without the opt-in, whatever its
    arguments; HRFD_EINVAL for the NULL handle in one with it (child processes: the library reads the variable once)"""
    from tests.hooks import check_max_wgs_hook_refusals
    check_max_wgs_hook_refusals("hrfd_audio_debug_set_max_wgs")
