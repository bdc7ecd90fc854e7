"""Every refusal of the DCS generator bank (hrfd_dcsgen_*) by its text, through the raw C ABI: the return code, and an error
text that starts with the public function's name and names the rule.  No GPU.  What a call's arguments decide on their own is
refused in front of the handle, so a NULL handle shows it; the rules of the queue against the clock and what is queued (a
start before the time, an overlap, a segment behind a FOREVER one, the ninth segment, a time at or above 2^63) are the
plain-C++ checks of hrfd_dcsgen.h, which hrfd_dcsgen_debug_edit runs on a queue given by value exactly as hrfd_dcsgen_queue
runs them on the handle's.  A channel number above the handle's and out against the rows of all channels need a handle:
tests/test_gpu_dcsgen.py.  The bank has no debug_set_max_wgs hook to refuse: k_dcsgen's grid is at most 2^22 workgroups."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api

EINVAL, ENODEV = -1, -2
NULL = None
ALL = 0xFFFFFFFF
FOREVER = 0xFFFFFFFF
APPEND = 0xFFFFFFFFFFFFFFFF
NO_END = 0xFFFFFFFFFFFFFFFF


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
    """(gap, length, tail, word, amp) rows as the array the C side reads, and its pointer"""
    a = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 5)
    return a, C.c_void_p(a.ctypes.data)


ONE = (0, 1, 0, 0, 0)
MOST = (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFE, 0x7FFFFF, 32767)


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_dcsgen_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_dcsgen_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_dcsgen_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    p, q, k = C.c_void_p(a), C.c_void_p(a + 16384), C.c_void_p(a + 40961)
    v32, v64 = C.c_uint32(0), C.c_uint64(0)
    keep1, one = segs(ONE)
    keep2, most = segs(*([MOST] * 7 + [(0, FOREVER, 1440, 1, 2)]))
    taps = np.array([32767, -32768], dtype=np.int16)
    most_taps = np.full(512, 127, dtype=np.int16)
    for name, args in [("hrfd_dcsgen_set_taps", (C.c_void_p(taps.ctypes.data), 2)),
                       ("hrfd_dcsgen_set_taps", (C.c_void_p(most_taps.ctypes.data), 512)),
                       ("hrfd_dcsgen_queue", (0, one, 1, APPEND)), ("hrfd_dcsgen_queue", (ALL, most, 8, 0)),
                       ("hrfd_dcsgen_queue", (65535, one, 1, (1 << 63) - 1)),
                       ("hrfd_dcsgen_cut", (0, 0)), ("hrfd_dcsgen_cut", (ALL, 1)), ("hrfd_dcsgen_cut", (65535, 1)),
                       ("hrfd_dcsgen_reset", ()),
                       ("hrfd_dcsgen_set_time", (0,)), ("hrfd_dcsgen_set_time", ((1 << 63) - 1,)),
                       ("hrfd_dcsgen_time", (C.byref(v64),)),
                       ("hrfd_dcsgen_pending", (0, C.byref(v32), C.byref(v64))), ("hrfd_dcsgen_pending", (65535, NULL, C.byref(v64))),
                       ("hrfd_dcsgen_pending", (0, C.byref(v32), NULL)),
                       ("hrfd_dcsgen_get_clips", (0, C.byref(v64))), ("hrfd_dcsgen_get_clips", (65535, C.byref(v64))),
                       ("hrfd_dcsgen_process", (p, 1, q, k)), ("hrfd_dcsgen_process", (p, 4, p, NULL)),
                       ("hrfd_dcsgen_process", (NULL, 1024, q, NULL)),
                       ("hrfd_dcsgen_process_device", (p, 1024, 1, q, 1024, k, NULL)),
                       ("hrfd_dcsgen_process_device", (p, 4100, 4, p, 4100, NULL, NULL)),
                       ("hrfd_dcsgen_process_device", (NULL, 0, 1, q, 1024, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_dcsgen_destroy(NULL) == 0


def test_set_taps_checks_its_taps_before_the_handle(lib):
    t = np.zeros(600, dtype=np.int16)
    tp = C.c_void_p(t.ctypes.data)
    for n in (0, 513, 0xFFFFFFFF):
        refused(lib, "hrfd_dcsgen_set_taps", NULL, tp, n, word="1..512 taps")
    refused(lib, "hrfd_dcsgen_set_taps", NULL, NULL, 1, word="taps")
    t[:2] = (32767, -32767)
    refused(lib, "hrfd_dcsgen_set_taps", NULL, tp, 2, word="NULL handle")          # sum |h| = 65534
    t[2] = 2
    refused(lib, "hrfd_dcsgen_set_taps", NULL, tp, 3, word="sum |h| = 65536 > 65535")
    t[2] = 1
    refused(lib, "hrfd_dcsgen_set_taps", NULL, tp, 3, word="NULL handle")          # 65535 itself


def test_queue_checks_its_segments_before_the_handle(lib):
    keep, one = segs(ONE)
    for n in (0, 9, 0xFFFFFFFF):
        refused(lib, "hrfd_dcsgen_queue", NULL, 0, one, n, APPEND, word="1..8 segments")
    refused(lib, "hrfd_dcsgen_queue", NULL, 0, NULL, 1, APPEND, word="segments")
    for amp in (32768, 65536, 0xFFFFFFFF):
        for at in (0, 5):
            rows = [list(ONE) for _ in range(6)]
            rows[at][4] = amp
            keep2, bad = segs(*rows)
            refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 6, APPEND, word=f"segment {at} has an amp above 32767")
            if at == 5:
                refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 5, APPEND, word="NULL handle")     # the entry lies behind n
    for word in (1 << 23, 0xFFFFFFFF):
        rows = [list(ONE) for _ in range(3)]
        rows[2][3] = word
        keep3, bad = segs(*rows)
        refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 3, 0, word=f"segment 2 has the word 0x{word:x}")
    rows = [list(ONE) for _ in range(3)]
    rows[1][1] = 0
    keep4, bad = segs(*rows)
    refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 3, 0, word="segment 1 has length 0")
    rows[1][1] = 1
    rows[1][2] = 0xFFFFFFFF
    keep5, bad = segs(*rows)
    refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 3, 0, word="segment 1 has a tail of 2^32-1")
    rows[1][2] = 0
    rows[1][1] = FOREVER
    keep6, bad = segs(*rows)
    refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 3, 0, word="segment 2 lies behind a FOREVER segment")
    refused(lib, "hrfd_dcsgen_queue", NULL, 0, bad, 2, 0, word="NULL handle")                      # FOREVER as the last
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_dcsgen_queue", NULL, channel, one, 1, APPEND, word="channel")
    for start in (1 << 63, (1 << 64) - 2):
        refused(lib, "hrfd_dcsgen_queue", NULL, 0, one, 1, start, word="below 2^63")


def edit_refused(lib, queue, N, new, start, word):
    q = np.zeros((8, 6), dtype=np.uint64)
    if queue:
        q[:len(queue)] = np.array(queue, dtype=np.uint64)
    before = q.copy()
    n = C.c_uint32(len(queue))
    keep, a = segs(*new)
    refused(lib, "hrfd_dcsgen_debug_edit", C.c_void_p(q.ctypes.data), C.byref(n), N, 0, a, len(new), start, word=word)
    assert n.value == len(queue) and (q == before).all()   # refused whole: the queue is as it was


def test_the_queue_rules_refuse_by_their_texts(lib):
    w = api.dcs_word(0o023)
    held = [[1000, 2000, 2100, w, 5, 100]]                  # S, S + L, E
    edit_refused(lib, held, 500, [ONE], 499, "start 499 lies before the stream time 500")
    edit_refused(lib, held, 500, [(0, 10, 0, w, 5)], 2099, "the segments at 1000 and 2099 would overlap")
    edit_refused(lib, held, 500, [(0, 501, 0, w, 5)], 500, "the segments at 500 and 1000 would overlap")
    edit_refused(lib, held, 500, [(0, 400, 101, w, 5)], 500, "would overlap")           # its tail overlaps, not its code
    forever = [[1000, NO_END, NO_END, w, 5, 1440]]
    edit_refused(lib, forever, 500, [ONE], APPEND, "nothing can be appended behind a FOREVER segment")
    edit_refused(lib, forever, 500, [ONE], 5000, "would lie behind the FOREVER segment at 1000")
    edit_refused(lib, held, 500, [(0, FOREVER, 0, w, 5)], 600, "would lie behind the FOREVER segment at 600")
    eight = [[1000 + 10 * i, 1005 + 10 * i, 1010 + 10 * i, w, 5, 5] for i in range(8)]
    edit_refused(lib, eight, 1010 + 510, [ONE], APPEND, "9 segments that have not ended on one channel (at most 8)")
    edit_refused(lib, eight[:4], 500, [ONE] * 5, APPEND, "9 segments that have not ended")
    top = (1 << 63) - 10
    edit_refused(lib, [], top, [(0, 10, 0, w, 5)], APPEND, "segment 0 would lie at or above stream time 2^63")
    edit_refused(lib, [], top, [(0, 5, 5, w, 5)], top, "segment 0 would lie at or above stream time 2^63")
    edit_refused(lib, [], top, [(0, 4, 5, w, 5), (0, 1, 0, w, 5)], top, "segment 1 would lie at or above stream time 2^63")
    edit_refused(lib, [], top, [(10, 1, 0, w, 5)], top, "segment 0 would lie")
    edit_refused(lib, [], 0, [ONE], 1 << 63, "below 2^63")
    # the limits themselves are taken
    q = np.zeros((8, 6), dtype=np.uint64)
    q[:8] = np.array(eight, dtype=np.uint64)
    n = C.c_uint32(8)
    keep, a = segs(ONE)
    assert lib.hrfd_dcsgen_debug_edit(C.c_void_p(q.ctypes.data), C.byref(n), 1010 + 511, 0, a, 1, APPEND) == 0 and n.value == 8
    n = C.c_uint32(0)
    keep, a = segs((0, 4, 5, w, 5))
    assert lib.hrfd_dcsgen_debug_edit(C.c_void_p(q.ctypes.data), C.byref(n), top, 0, a, 1, top) == 0
    assert n.value == 1 and int(q[0, 2]) == (1 << 63) - 1


def test_setters_and_getters_check_their_values_before_the_handle(lib):
    v32, v64 = C.c_uint32(0), C.c_uint64(0)
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_dcsgen_cut", NULL, channel, 0, word="channel")
        refused(lib, "hrfd_dcsgen_pending", NULL, channel, C.byref(v32), C.byref(v64), word="channel")
        refused(lib, "hrfd_dcsgen_get_clips", NULL, channel, C.byref(v64), word="channel")
    refused(lib, "hrfd_dcsgen_pending", NULL, ALL, C.byref(v32), C.byref(v64), word="one channel")
    refused(lib, "hrfd_dcsgen_get_clips", NULL, ALL, C.byref(v64), word="one channel")
    refused(lib, "hrfd_dcsgen_pending", NULL, 0, NULL, NULL, word="NULL results")
    refused(lib, "hrfd_dcsgen_get_clips", NULL, 0, NULL, word="result pointer")
    refused(lib, "hrfd_dcsgen_time", NULL, NULL, word="NULL result")
    for N in (1 << 63, (1 << 64) - 1):
        refused(lib, "hrfd_dcsgen_set_time", NULL, N, word="below 2^63")


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    """gen_check_call's rules and texts, unchanged, under this bank's names"""
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, q, k = C.c_void_p(a + 65536), C.c_void_p(a + 131072), C.c_void_p(a + 32769)
    dev, host = "hrfd_dcsgen_process_device", "hrfd_dcsgen_process"
    for n_blocks in (0, 1025, 0xFFFFFFFF):
        refused(lib, host, NULL, p, n_blocks, q, k, word="n_blocks must be 1..1024")
        refused(lib, host, NULL, NULL, n_blocks, q, k, word="n_blocks")
        refused(lib, dev, NULL, p, 1 << 33, n_blocks, q, 1 << 33, k, NULL, word="n_blocks")
    refused(lib, host, NULL, p, 1, NULL, k, word="NULL argument (out)")
    refused(lib, dev, NULL, p, 1024, 1, NULL, 1024, k, NULL, word="NULL argument")
    refused(lib, dev, NULL, NULL, 1024, 1, NULL, 1024, NULL, NULL, word="NULL argument")
    for stride, n_blocks in ((1025, 1), (1022, 1), (0, 1), (1, 1), (1024 * 1024 - 2, 1024)):
        refused(lib, dev, NULL, p, stride, n_blocks, q, 1 << 20, k, NULL, word="channel_stride_bytes")
        refused(lib, dev, NULL, p, 1 << 20, n_blocks, q, stride, k, NULL, word="out_stride_bytes")
        refused(lib, dev, NULL, NULL, 1 << 20, n_blocks, q, stride, k, NULL, word="out_stride_bytes")
        refused(lib, dev, NULL, NULL, stride, n_blocks, q, 1 << 20, k, NULL, word="NULL handle")
    refused(lib, dev, NULL, C.c_void_p(a + 65537), 1024, 1, q, 1024, k, NULL, word="even addresses")
    refused(lib, host, NULL, C.c_void_p(a + 65539), 1, q, k, word="even addresses")
    refused(lib, dev, NULL, p, 1024, 1, C.c_void_p(a + 131073), 1024, k, NULL, word="even addresses")
    refused(lib, host, NULL, NULL, 1, C.c_void_p(a + 131075), k, word="even addresses")
    base = a + 65536
    for n_blocks, off in ((1, 2), (1, -2), (1, 1022), (1, -1022), (4, 4094), (4, -4094), (4, 512), (1024, 1024 * 1024 - 2)):
        refused(lib, dev, NULL, C.c_void_p(base), 1024 * n_blocks, n_blocks, C.c_void_p(base + off), 1024 * n_blocks, k, NULL,
                word="overlaps the input (in place means out at the input's own address and stride")
        refused(lib, host, NULL, C.c_void_p(base), n_blocks, C.c_void_p(base + off), k, word="overlaps the input (in place")
    for stride, out_stride in ((1024, 1026), (1030, 1024), (2048, 4096)):
        refused(lib, dev, NULL, p, stride, 1, p, out_stride, k, NULL, word="overlaps the input (in place")
    for stride in (1024, 1026, 4096):
        refused(lib, dev, NULL, p, stride, 1, p, stride, k, NULL, word="NULL handle")
    for off in (1024, -1024):
        refused(lib, dev, NULL, p, 1024, 1, C.c_void_p(base + off), 1024, k, NULL, word="NULL handle")
    for res in range(0, 16, 2):
        refused(lib, dev, NULL, C.c_void_p(base + res), 1030, 1, C.c_void_p(a + 131072 + 14 - res), 1026, k, NULL, word="NULL handle")
        refused(lib, dev, NULL, NULL, 0, 1, C.c_void_p(base + res), 1030, NULL, NULL, word="NULL handle")
    refused(lib, dev, NULL, p, 1024 * 1024, 1024, p, 1024 * 1024, k, NULL, word="NULL handle")


def test_the_debug_entries_refuse_what_is_out_of_order(lib):
    out = np.zeros(512, dtype=np.int16)
    taps = np.array([16384], dtype=np.int16)
    tp, op = C.c_void_p(taps.ctypes.data), C.c_void_p(out.ctypes.data)
    bad = np.array([[10, 5, 20, 0, 0, 0]], dtype=np.uint64)                     # S + L in front of S
    refused(lib, "hrfd_dcsgen_debug_slow", tp, 1, C.c_void_p(bad.ctypes.data), 1, 0, NULL, 1, op, NULL, NULL, word="out of order")
    refused(lib, "hrfd_dcsgen_debug_slow", tp, 1, NULL, 9, 0, NULL, 1, op, NULL, NULL, word="at most 8")
    refused(lib, "hrfd_dcsgen_debug_slow", tp, 0, NULL, 0, 0, NULL, 1, op, NULL, NULL, word="1..512 taps")
    refused(lib, "hrfd_dcsgen_debug_slow", tp, 1, NULL, 0, (1 << 63) - 512, NULL, 2, op, NULL, NULL, word="below 2^63")
    n = C.c_uint32(0)
    refused(lib, "hrfd_dcsgen_debug_edit", NULL, C.byref(n), 0, 3, NULL, 0, 0, word="op 3")
    refused(lib, "hrfd_dcsgen_debug_edit", NULL, NULL, 0, 1, NULL, 0, 0, word="NULL argument")
