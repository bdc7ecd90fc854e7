"""Every refusal of the three host transports (hrfd_ingest_*, hrfd_fanout_*, hrfd_play_*) that is decided before a device
is needed, through the raw C ABI as tests/test_cal_refusals.py does for the conditioner: the return code, and an error
text that is there.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib

OK, EINVAL, ENODEV, ESTATE = 0, -1, -2, -4
NULL = None
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def refused(lib, name, *args, code=EINVAL, named=True):
    rc = getattr(lib, name)(*args)
    err = lib.hrfd_last_error().decode()
    assert rc == code, (name, args, rc, err)
    assert err, name
    if named:
        assert err.startswith(name), (name, err)


def test_every_ingest_entry_refuses_a_null_handle(lib):
    p, n = C.c_void_p(0x1234), C.c_uint64(77)
    refused(lib, "hrfd_ingest_create", NULL, 21504, 2, 2, C.byref(p))
    assert p.value == 0x1234                                # nothing was created, nothing written
    assert lib.hrfd_ingest_destroy(NULL) == OK
    refused(lib, "hrfd_ingest_acquire", NULL, C.byref(p))
    refused(lib, "hrfd_ingest_submit", NULL, 0)
    refused(lib, "hrfd_ingest_collect", NULL, C.byref(p), C.byref(p), C.byref(p), C.byref(p))
    refused(lib, "hrfd_ingest_collect", NULL, NULL, NULL, NULL, NULL)
    refused(lib, "hrfd_ingest_replayed", NULL, C.byref(n))
    assert p.value == 0x1234 and n.value == 77


def test_every_fanout_entry_refuses_a_null_handle(lib):
    buf = np.zeros(64, dtype=np.int64)
    p, u = C.c_void_p(buf.ctypes.data), C.c_uint32(77)
    out = C.c_void_p(0x1234)
    assert lib.hrfd_fanout_destroy(NULL) == OK
    refused(lib, "hrfd_fanout_shards", NULL, C.byref(u))
    for ch in (0, ALL):
        refused(lib, "hrfd_fanout_set_mode", NULL, ch, 3, named=False)
        refused(lib, "hrfd_fanout_set_gain", NULL, ch, 3, C.c_float(1.0), named=False)
        refused(lib, "hrfd_fanout_set_threshold", NULL, ch, -30, named=False)
    refused(lib, "hrfd_fanout_scatter", NULL, 0, p, 21504, 2, NULL)
    refused(lib, "hrfd_fanout_input", NULL, 0, 21504, 2, C.byref(out), C.byref(u), C.byref(u))
    refused(lib, "hrfd_fanout_process", NULL, 0)
    refused(lib, "hrfd_fanout_collect", NULL, 0, p, p, C.byref(u))
    refused(lib, "hrfd_fanout_collect", NULL, 0, NULL, NULL, NULL)
    assert out.value == 0x1234 and u.value == 77


def test_every_play_entry_refuses_a_null_handle(lib):
    buf = np.zeros(64, dtype=np.int8)
    p, u = C.c_void_p(buf.ctypes.data), C.c_uint32(77)
    assert lib.hrfd_play_destroy(NULL) == OK
    refused(lib, "hrfd_play_load", NULL, p, 64)
    refused(lib, "hrfd_play_load_file", NULL, b"/nonexistent.iq")
    refused(lib, "hrfd_play_set_position", NULL, 0, 0)
    refused(lib, "hrfd_play_set_position", NULL, ALL, 0)
    refused(lib, "hrfd_play_get_position", NULL, 0, C.byref(u))
    refused(lib, "hrfd_play_get_device", NULL, p, 64, 64, NULL)
    refused(lib, "hrfd_play_get", NULL, p, 64)
    assert u.value == 77 and (buf == 0).all()


def test_fanout_create_checks_its_arguments_before_it_looks_for_a_device(lib):
    devs = (C.c_int * 4)(0, 0, 0, 0)
    h = C.c_void_p(0x1234)
    refused(lib, "hrfd_fanout_create", 4, devs, 4, NULL)                 # no result pointer
    refused(lib, "hrfd_fanout_create", 4, NULL, 4, C.byref(h))          # no device list
    refused(lib, "hrfd_fanout_create", 4, devs, 0, C.byref(h))          # no shard
    refused(lib, "hrfd_fanout_create", 0, devs, 1, C.byref(h))          # a shard without a channel
    refused(lib, "hrfd_fanout_create", 3, devs, 4, C.byref(h))
    assert h.value == 0x1234
    if lib.hrfd_device_count() > 0:
        pytest.skip("a device is visible: HRFD_ENODEV cannot be seen here")
    refused(lib, "hrfd_fanout_create", 4, devs, 4, C.byref(h), code=ENODEV)
    assert h.value is None


def test_play_create_refuses_no_channels_and_has_no_cpu_path(lib):
    h = C.c_void_p(0x1234)
    refused(lib, "hrfd_play_create", 0, 0, C.byref(h))
    refused(lib, "hrfd_play_create", 1, 0, NULL)
    assert h.value == 0x1234
    if lib.hrfd_device_count() > 0:
        pytest.skip("a device is visible: HRFD_ENODEV cannot be seen here")
    refused(lib, "hrfd_play_create", 1, 0, C.byref(h), code=ENODEV)
    assert h.value is None


def test_fanout_channel_range_edges(lib):
    first, count = C.c_uint32(77), C.c_uint32(77)
    f, c = C.byref(first), C.byref(count)
    refused(lib, "hrfd_fanout_channel_range", 8, 0, 0, f, c)
    refused(lib, "hrfd_fanout_channel_range", 8, 2, 2, f, c)
    refused(lib, "hrfd_fanout_channel_range", 8, 2, ALL, f, c)
    refused(lib, "hrfd_fanout_channel_range", 8, 2, 0, NULL, c)
    refused(lib, "hrfd_fanout_channel_range", 8, 2, 0, f, NULL)
    assert first.value == 77 and count.value == 77

    def rng(n, g, s):
        assert lib.hrfd_fanout_channel_range(n, g, s, f, c) == OK
        return first.value, count.value

    # the rule stated a second time: sizes floor(n / G), the first n mod G shards one more, contiguous from 0
    for n, g in [(0, 1), (0, 3), (1, 1), (2, 5), (5, 5), (6, 5), (9, 4), (ALL, 1), (ALL, 7), (ALL, ALL), (ALL - 1, ALL)]:
        base, extra = divmod(n, g)
        for s in sorted(s for s in {0, 1, extra - 1, extra, extra + 1, g - 2, g - 1} if 0 <= s < g):
            want = (s * base + min(s, extra), base + (1 if s < extra else 0))
            assert rng(n, g, s) == want, (n, g, s)
        lo, cnt = rng(n, g, g - 1)
        assert lo + cnt == n
