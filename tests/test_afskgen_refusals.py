"""Every refusal of the AFSK generator bank (hrfd_afskgen_*) that is decided before a device is needed, through the raw C ABI:
the return code, and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on
a handle's state cannot be shown without a device: a channel number above the handle's, out against the rows of all channels,
and the rules of the queue against the clock and what is queued (a start before the time, an overlap, the fifth message, a
clock moved under a pending message) are refused in tests/test_gpu_afskgen.py, and by the same plain-C++ checks in
tests/cpp/san_afskgen.cc.  The bank has no debug_set_max_wgs hook to refuse: k_afskgen's grid is the channel count, so its
launch is never cut."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

EINVAL, ENODEV = -1, -2
NULL = None
ALL = 0xFFFFFFFF
APPEND = 0xFFFFFFFFFFFFFFFF
TOP = 1 << 31


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


def message(gap=0, n_bits=3, mark=1, space=1, baud=TOP, amp=0, flags=0, pad=0):
    """the eight uint32 the C side reads, and their pointer"""
    a = np.array([gap, n_bits, mark, space, baud, amp, flags, pad], dtype=np.uint32)
    return a, C.c_void_p(a.ctypes.data)


BITS = np.ones(8192, dtype=np.uint8)
bits = C.c_void_p(BITS.ctypes.data)


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_afskgen_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_afskgen_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_afskgen_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    p, q, k = C.c_void_p(a), C.c_void_p(a + 16384), C.c_void_p(a + 40961)
    v32, v64 = C.c_uint32(0), C.c_uint64(0)
    keep1, one = message()
    keep2, most = message(0xFFFFFFFF, 8192, TOP, TOP, TOP, 32767, 1)
    keep3, slow = message(0, 1, 1, 1, 3, 0, 0)                 # 1431655766 samples
    for name, args in [("hrfd_afskgen_queue", (0, one, bits, APPEND)), ("hrfd_afskgen_queue", (ALL, most, bits, 0)),
                       ("hrfd_afskgen_queue", (65535, slow, bits, (1 << 63) - 1)),
                       ("hrfd_afskgen_cut", (0,)), ("hrfd_afskgen_cut", (ALL,)), ("hrfd_afskgen_cut", (65535,)),
                       ("hrfd_afskgen_reset", ()),
                       ("hrfd_afskgen_set_time", (0,)), ("hrfd_afskgen_set_time", ((1 << 63) - 1,)),
                       ("hrfd_afskgen_time", (C.byref(v64),)),
                       ("hrfd_afskgen_pending", (0, C.byref(v32), C.byref(v64))), ("hrfd_afskgen_pending", (65535, NULL, C.byref(v64))),
                       ("hrfd_afskgen_pending", (0, C.byref(v32), NULL)),
                       ("hrfd_afskgen_get_clips", (0, C.byref(v64))), ("hrfd_afskgen_get_clips", (65535, C.byref(v64))),
                       ("hrfd_afskgen_process", (p, 1, q, k)), ("hrfd_afskgen_process", (p, 4, p, NULL)),
                       ("hrfd_afskgen_process", (NULL, 1024, q, NULL)),
                       ("hrfd_afskgen_process_device", (p, 1024, 1, q, 1024, k, NULL)),
                       ("hrfd_afskgen_process_device", (p, 4100, 4, p, 4100, NULL, NULL)),
                       ("hrfd_afskgen_process_device", (NULL, 0, 1, q, 1024, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_afskgen_destroy(NULL) == 0


def test_queue_checks_its_message_before_the_handle(lib):
    keep, one = message()
    refused(lib, "hrfd_afskgen_queue", NULL, 0, NULL, bits, APPEND, word="NULL argument (msg, bits)")
    refused(lib, "hrfd_afskgen_queue", NULL, 0, one, NULL, APPEND, word="NULL argument (msg, bits)")
    for n in (0, 8193, 0xFFFFFFFF):
        keep, m = message(n_bits=n)
        refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word="n_bits must be 1..8192")
    for name in ("mark", "space", "baud"):
        for v in (0, TOP + 1, 0xFFFFFFFF):
            keep, m = message(**{name: v})
            refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word=f"{name}_step must be 1..2^31")
    for amp in (32768, 65536, 0xFFFFFFFF):
        keep, m = message(amp=amp)
        refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word="amp above 32767")
    for flags in (2, 3, 0x80000000):
        keep, m = message(flags=flags)
        refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word="only bit 0 of flags")
    keep, m = message(pad=1)
    refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word="a pad of 0")
    # the length: below 2^31 samples
    for n_bits, baud in ((1, 1), (1, 2), (2, 4), (8192, 16384)):
        keep, m = message(n_bits=n_bits, baud=baud)
        refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word="samples (below 2^31)")
    keep, m = message(n_bits=8192, baud=16385)
    refused(lib, "hrfd_afskgen_queue", NULL, 0, m, bits, APPEND, word="NULL handle")
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_afskgen_queue", NULL, channel, one, bits, APPEND, word="channel")
    for start in (1 << 63, (1 << 64) - 2):
        refused(lib, "hrfd_afskgen_queue", NULL, 0, one, bits, start, word="below 2^63")


def test_setters_and_getters_check_their_values_before_the_handle(lib):
    v32, v64 = C.c_uint32(0), C.c_uint64(0)
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_afskgen_cut", NULL, channel, word="channel")
        refused(lib, "hrfd_afskgen_pending", NULL, channel, C.byref(v32), C.byref(v64), word="channel")
        refused(lib, "hrfd_afskgen_get_clips", NULL, channel, C.byref(v64), word="channel")
    refused(lib, "hrfd_afskgen_pending", NULL, ALL, C.byref(v32), C.byref(v64), word="one channel")
    refused(lib, "hrfd_afskgen_get_clips", NULL, ALL, C.byref(v64), word="one channel")
    refused(lib, "hrfd_afskgen_pending", NULL, 0, NULL, NULL, word="NULL results")
    refused(lib, "hrfd_afskgen_get_clips", NULL, 0, NULL, word="result pointer")
    refused(lib, "hrfd_afskgen_time", NULL, NULL, word="NULL result")
    for N in (1 << 63, (1 << 64) - 1):
        refused(lib, "hrfd_afskgen_set_time", NULL, N, word="below 2^63")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, q, k = C.c_void_p(a + 65536), C.c_void_p(a + 131072), C.c_void_p(a + 32769)
    dev, host = "hrfd_afskgen_process_device", "hrfd_afskgen_process"
    for n_blocks in (0, 1025, 0xFFFFFFFF):
        refused(lib, host, NULL, p, n_blocks, q, k, word="n_blocks")
        refused(lib, host, NULL, NULL, n_blocks, q, k, word="n_blocks")
        refused(lib, dev, NULL, p, 1 << 33, n_blocks, q, 1 << 33, k, NULL, word="n_blocks")
    # no output
    refused(lib, host, NULL, p, 1, NULL, k, word="NULL argument")
    refused(lib, dev, NULL, p, 1024, 1, NULL, 1024, k, NULL, word="NULL argument")
    refused(lib, dev, NULL, NULL, 1024, 1, NULL, 1024, NULL, NULL, word="NULL argument")
    # odd or short strides, on the input and on the output; the input's stride does not matter without an input
    for stride, n_blocks in ((1025, 1), (1022, 1), (0, 1), (1, 1), (1024 * 1024 - 2, 1024)):
        refused(lib, dev, NULL, p, stride, n_blocks, q, 1 << 20, k, NULL, word="channel_stride_bytes")
        refused(lib, dev, NULL, p, 1 << 20, n_blocks, q, stride, k, NULL, word="out_stride_bytes")
        refused(lib, dev, NULL, NULL, 1 << 20, n_blocks, q, stride, k, NULL, word="out_stride_bytes")
        refused(lib, dev, NULL, NULL, stride, n_blocks, q, 1 << 20, k, NULL, word="NULL handle")
    # odd addresses of the PCM and out (active is bytes: any address)
    refused(lib, dev, NULL, C.c_void_p(a + 65537), 1024, 1, q, 1024, k, NULL, word="even addresses")
    refused(lib, host, NULL, C.c_void_p(a + 65539), 1, q, k, word="even addresses")
    refused(lib, dev, NULL, p, 1024, 1, C.c_void_p(a + 131073), 1024, k, NULL, word="even addresses")
    refused(lib, host, NULL, p, 1, C.c_void_p(a + 131075), k, word="even addresses")
    refused(lib, host, NULL, NULL, 1, C.c_void_p(a + 131075), k, word="even addresses")
    # every overlap of out and the input other than exact in-place, with the reason
    base = a + 65536
    for n_blocks, off in ((1, 2), (1, -2), (1, 1022), (1, -1022), (4, 4094), (4, -4094), (4, 512), (1024, 1024 * 1024 - 2)):
        refused(lib, dev, NULL, C.c_void_p(base), 1024 * n_blocks, n_blocks, C.c_void_p(base + off), 1024 * n_blocks, k, NULL,
                word="overlaps the input (in place means out at the input's own address and stride")
        refused(lib, host, NULL, C.c_void_p(base), n_blocks, C.c_void_p(base + off), k, word="overlaps the input (in place")
    for stride, out_stride in ((1024, 1026), (1030, 1024), (2048, 4096)):
        refused(lib, dev, NULL, p, stride, 1, p, out_stride, k, NULL, word="overlaps the input (in place")
    # with everything else in order the refusal left is the handle's
    for stride in (1024, 1026, 4096):
        refused(lib, dev, NULL, p, stride, 1, p, stride, k, NULL, word="NULL handle")
    refused(lib, host, NULL, p, 3, p, k, word="NULL handle")
    for off in (1024, -1024):
        refused(lib, dev, NULL, p, 1024, 1, C.c_void_p(base + off), 1024, k, NULL, word="NULL handle")
        refused(lib, host, NULL, p, 1, C.c_void_p(base + off), k, word="NULL handle")
    for res in range(0, 16, 2):
        refused(lib, dev, NULL, C.c_void_p(base + res), 1030, 1, C.c_void_p(a + 131072 + 14 - res), 1026, k, NULL, word="NULL handle")
        refused(lib, dev, NULL, C.c_void_p(base + res), 1030, 1, C.c_void_p(base + res), 1030, NULL, NULL, word="NULL handle")
        refused(lib, dev, NULL, NULL, 0, 1, C.c_void_p(base + res), 1030, NULL, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1024 * 1024, 1024, p, 1024 * 1024, k, NULL, word="NULL handle")


def test_the_debug_entries_refuse_what_the_queue_refuses(lib):
    v64 = C.c_uint64(0)
    words = np.zeros(257, dtype=np.uint32)
    w = C.c_void_p(words.ctypes.data)
    refused(lib, "hrfd_afskgen_debug_length", 1, 1, NULL, word="NULL result")
    refused(lib, "hrfd_afskgen_debug_length", 0, 5, C.byref(v64), word="at least one bit")
    refused(lib, "hrfd_afskgen_debug_length", 1, 1, C.byref(v64), word="below 2^31")
    for n in (0, 8193):
        refused(lib, "hrfd_afskgen_debug_levels", bits, n, 1, w, word="1..8192 bits")
    refused(lib, "hrfd_afskgen_debug_levels", NULL, 1, 1, w, word="both arrays")
    out = np.zeros(512, dtype=np.int16)
    o = C.c_void_p(out.ctypes.data)
    keep, five = message()
    starts = np.array([0, 10, 20, 30, 40], dtype=np.uint64)
    s = C.c_void_p(starts.ctypes.data)
    refused(lib, "hrfd_afskgen_debug_slow", five, bits, s, NULL, 5, 0, NULL, 1, o, NULL, NULL, word="at most 4 messages")
    refused(lib, "hrfd_afskgen_debug_slow", five, bits, s, NULL, 1, 1 << 63, NULL, 1, o, NULL, NULL, word="below 2^63")
    refused(lib, "hrfd_afskgen_debug_slow", five, bits, s, NULL, 1, 0, NULL, 0, o, NULL, NULL, word="n_blocks")
    two = np.array([[0, 3, 1, 1, TOP, 0, 0, 0]] * 2, dtype=np.uint32)        # 6 samples each
    both_at = np.array([7, 12], dtype=np.uint64)
    refused(lib, "hrfd_afskgen_debug_slow", C.c_void_p(two.ctypes.data), bits, C.c_void_p(both_at.ctypes.data), NULL, 2, 0, NULL, 1, o, NULL,
            NULL, word="messages 0 and 1 overlap")
    both_at[1] = 13
    assert lib.hrfd_afskgen_debug_slow(C.c_void_p(two.ctypes.data), bits, C.c_void_p(both_at.ctypes.data), NULL, 2, 0, NULL, 1, o, NULL, NULL) == 0
