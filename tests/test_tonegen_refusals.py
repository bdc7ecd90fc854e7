"""Every refusal of the tone generator bank (hrfd_tonegen_*) that is decided before a device is needed, through the raw C ABI:
the return code, and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on
a handle's state cannot be shown without a device: a channel number above the handle's, out against the rows of all channels,
and the rules of the queue against the clock and what is queued (a start before the time, an overlap, a segment behind a
FOREVER one, the 33rd segment) are refused in tests/test_gpu_tonegen.py, and by the same plain-C++ checks in
tests/cpp/san_tonegen.cc.  The bank has no debug_set_max_wgs hook to refuse: k_tonegen's grid is at most 2^22 workgroups,
so its launch is never cut."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

EINVAL, ENODEV = -1, -2
NULL = None
ALL = 0xFFFFFFFF
FOREVER = 0xFFFFFFFF
APPEND = 0xFFFFFFFFFFFFFFFF


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


def segs(*rows):
    """(gap, length, step_a, step_b, amp_a, amp_b) rows as the array the C side reads, and its pointer"""
    a = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 6)
    return a, C.c_void_p(a.ctypes.data)


ONE = (0, 1, 0, 0, 0, 0)
MOST = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFF, 32767, 32767)


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_tonegen_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_tonegen_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_tonegen_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    p, q, k = C.c_void_p(a), C.c_void_p(a + 16384), C.c_void_p(a + 40961)
    v32, v64 = C.c_uint32(0), C.c_uint64(0)
    keep1, one = segs(ONE)
    keep2, most = segs(*([MOST] * 31 + [(0, FOREVER, 1, 2, 3, 4)]))
    for name, args in [("hrfd_tonegen_queue", (0, 0, one, 1, APPEND)), ("hrfd_tonegen_queue", (ALL, 1, most, 32, 0)),
                       ("hrfd_tonegen_queue", (65535, 1, one, 1, (1 << 63) - 1)),
                       ("hrfd_tonegen_cut", (0, 0)), ("hrfd_tonegen_cut", (ALL, 1)), ("hrfd_tonegen_cut", (65535, 1)),
                       ("hrfd_tonegen_reset", ()),
                       ("hrfd_tonegen_set_time", (0,)), ("hrfd_tonegen_set_time", ((1 << 63) - 1,)),
                       ("hrfd_tonegen_time", (C.byref(v64),)),
                       ("hrfd_tonegen_pending", (0, 0, C.byref(v32), C.byref(v64))), ("hrfd_tonegen_pending", (65535, 1, NULL, C.byref(v64))),
                       ("hrfd_tonegen_pending", (0, 1, C.byref(v32), NULL)),
                       ("hrfd_tonegen_get_clips", (0, C.byref(v64))), ("hrfd_tonegen_get_clips", (65535, C.byref(v64))),
                       ("hrfd_tonegen_process", (p, 1, q, k)), ("hrfd_tonegen_process", (p, 4, p, NULL)),
                       ("hrfd_tonegen_process", (NULL, 1024, q, NULL)),
                       ("hrfd_tonegen_process_device", (p, 1024, 1, q, 1024, k, NULL)),
                       ("hrfd_tonegen_process_device", (p, 4100, 4, p, 4100, NULL, NULL)),
                       ("hrfd_tonegen_process_device", (NULL, 0, 1, q, 1024, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_tonegen_destroy(NULL) == 0


def test_queue_checks_its_segments_before_the_handle(lib):
    keep, one = segs(ONE)
    refused(lib, "hrfd_tonegen_queue", NULL, 0, 2, one, 1, APPEND, word="track 2")
    refused(lib, "hrfd_tonegen_queue", NULL, 0, 0xFFFFFFFF, one, 1, APPEND, word="track")
    for n in (0, 33, 0xFFFFFFFF):
        refused(lib, "hrfd_tonegen_queue", NULL, 0, 0, one, n, APPEND, word="1..32 segments")
    refused(lib, "hrfd_tonegen_queue", NULL, 0, 0, NULL, 1, APPEND, word="segments")
    for amp in (32768, 65536, 0xFFFFFFFF):
        for at in (0, 5):
            for which in (4, 5):
                rows = [list(ONE) for _ in range(6)]
                rows[at][which] = amp
                keep2, bad = segs(*rows)
                refused(lib, "hrfd_tonegen_queue", NULL, 0, 0, bad, 6, APPEND, word=f"segment {at} has an amp above 32767")
                if at == 5:
                    refused(lib, "hrfd_tonegen_queue", NULL, 0, 0, bad, 5, APPEND, word="NULL handle")     # the entry lies behind n
    rows = [list(ONE) for _ in range(3)]
    rows[1][1] = 0
    keep3, bad = segs(*rows)
    refused(lib, "hrfd_tonegen_queue", NULL, 0, 1, bad, 3, 0, word="segment 1 has length 0")
    rows[1][1] = FOREVER
    keep4, bad = segs(*rows)
    refused(lib, "hrfd_tonegen_queue", NULL, 0, 1, bad, 3, 0, word="segment 2 lies behind a FOREVER segment")
    refused(lib, "hrfd_tonegen_queue", NULL, 0, 1, bad, 2, 0, word="NULL handle")                          # FOREVER as the last
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_tonegen_queue", NULL, channel, 0, one, 1, APPEND, word="channel")
    for start in (1 << 63, (1 << 64) - 2):
        refused(lib, "hrfd_tonegen_queue", NULL, 0, 0, one, 1, start, word="below 2^63")


def test_setters_and_getters_check_their_values_before_the_handle(lib):
    v32, v64 = C.c_uint32(0), C.c_uint64(0)
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_tonegen_cut", NULL, channel, 0, word="channel")
        refused(lib, "hrfd_tonegen_pending", NULL, channel, 0, C.byref(v32), C.byref(v64), word="channel")
        refused(lib, "hrfd_tonegen_get_clips", NULL, channel, C.byref(v64), word="channel")
    refused(lib, "hrfd_tonegen_pending", NULL, ALL, 0, C.byref(v32), C.byref(v64), word="one channel")
    refused(lib, "hrfd_tonegen_get_clips", NULL, ALL, C.byref(v64), word="one channel")
    for track in (2, 0xFFFFFFFF):
        refused(lib, "hrfd_tonegen_cut", NULL, 0, track, word=f"track {track}")
        refused(lib, "hrfd_tonegen_pending", NULL, 0, track, C.byref(v32), C.byref(v64), word=f"track {track}")
    refused(lib, "hrfd_tonegen_pending", NULL, 0, 0, NULL, NULL, word="NULL results")
    refused(lib, "hrfd_tonegen_get_clips", NULL, 0, NULL, word="result pointer")
    refused(lib, "hrfd_tonegen_time", NULL, NULL, word="NULL result")
    for N in (1 << 63, (1 << 64) - 1):
        refused(lib, "hrfd_tonegen_set_time", NULL, N, word="below 2^63")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, q, k = C.c_void_p(a + 65536), C.c_void_p(a + 131072), C.c_void_p(a + 32769)
    dev, host = "hrfd_tonegen_process_device", "hrfd_tonegen_process"
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
    # with everything else in order the refusal left is the handle's: in place under the same stride, dense and padded; out
    # directly behind and in front of the input; every even residue; generate only; the limits themselves
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
