"""Every refusal of the DCS bank (hrfd_dcs_*) that is decided before a device is needed, through the raw C ABI: the return code,
and an error text that starts with the public function's name and names the rule.  No GPU.  What depends on a handle's channel
count cannot be shown without a device: a channel number above it is refused in tests/test_gpu_dcs.py, which also shows a
handle working on behind its refusals.  Here the state that must survive a refusal is the slow entry's: a refused
hrfd_dcs_debug_slow leaves the state it was given untouched, and the next call goes on from it."""
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


def arr(values, dtype):
    a = np.ascontiguousarray(values, dtype=dtype)
    return a, C.c_void_p(a.ctypes.data)


def test_create_refuses_bad_sizes_and_has_no_cpu_path(lib):
    for n in (0, 65537, 0xFFFFFFFF):
        h = C.c_void_p(0x1234)
        refused(lib, "hrfd_dcs_create", n, 0, C.byref(h), word="channels")
        assert h.value is None
    refused(lib, "hrfd_dcs_create", 1, 0, NULL, word="result pointer")
    if lib.hrfd_device_count() == 0:
        for n in (1, 3, 65536):
            h = C.c_void_p(0x1234)
            refused(lib, "hrfd_dcs_create", n, 0, C.byref(h), code=ENODEV)
            assert h.value is None


def test_every_entry_refuses_a_null_handle(lib):
    """a NULL handle behind arguments that are in order, the limits among them"""
    buf = np.zeros(1 << 13, dtype=np.int64)
    a = buf.ctypes.data
    p, h, b, q, n = C.c_void_p(a), C.c_void_p(a + 16386), C.c_void_p(a + 32769), C.c_void_p(a + 40963), C.c_void_p(a + 49152)
    keep1, one = arr([16384], np.int16)
    keep2, most = arr([127] * 512, np.int16)
    keep3, codes = arr([0o023, 0o754, 0o777, 0], np.uint16)
    keep4, inv = arr([0, 1, 0, 7], np.uint8)
    keep5, grp = arr([0, 3, 1, 2], np.uint8)
    v = C.c_uint32(0)
    for name, args in [("hrfd_dcs_set_taps", (one, 1)), ("hrfd_dcs_set_taps", (most, 512)),
                       ("hrfd_dcs_set_codes", (codes, inv, grp, 4)), ("hrfd_dcs_set_codes", (codes, NULL, NULL, 4)),
                       ("hrfd_dcs_set_codes", (NULL, NULL, NULL, 0)), ("hrfd_dcs_n_codes", (C.byref(v),)),
                       ("hrfd_dcs_set_min_hits", (0, 1)), ("hrfd_dcs_set_min_hits", (3, 512)), ("hrfd_dcs_set_min_hits", (ALL, 128)),
                       ("hrfd_dcs_reset", (ALL,)), ("hrfd_dcs_reset", (65535,)),
                       ("hrfd_dcs_process", (p, NULL, 1, h, b, q)), ("hrfd_dcs_process", (p, n, 1024, NULL, NULL, q)),
                       ("hrfd_dcs_process", (p, NULL, 1, h, NULL, NULL)),
                       ("hrfd_dcs_process_device", (p, 1024, NULL, 1, h, b, q, NULL)),
                       ("hrfd_dcs_process_device", (p, 4098, n, 4, NULL, b, NULL, NULL)),
                       ("hrfd_dcs_process_device", (p, 1 << 20, NULL, 1024, h, NULL, NULL, NULL))]:
        refused(lib, name, NULL, *args, word="NULL handle")
    assert lib.hrfd_dcs_destroy(NULL) == 0


def test_set_taps_checks_its_list_before_the_handle(lib):
    keep, t = arr([1] * 513, np.int16)
    for n in (0, 513, 0xFFFFFFFF):
        refused(lib, "hrfd_dcs_set_taps", NULL, t, n, word="1..512 taps")
    refused(lib, "hrfd_dcs_set_taps", NULL, NULL, 1, word="taps")
    keep2, big = arr([32767, -32767, 2], np.int16)
    refused(lib, "hrfd_dcs_set_taps", NULL, big, 3, word="sum |h| = 65536 > 65535")
    refused(lib, "hrfd_dcs_set_taps", NULL, big, 2, word="NULL handle")                # 65534
    keep3, edge = arr([-32768, 32767], np.int16)
    refused(lib, "hrfd_dcs_set_taps", NULL, edge, 2, word="NULL handle")               # 65535


def test_set_codes_checks_its_list_before_the_handle(lib):
    keep, many = arr(list(range(129)), np.uint16)
    refused(lib, "hrfd_dcs_set_codes", NULL, many, NULL, NULL, 129, word="at most 128")
    refused(lib, "hrfd_dcs_set_codes", NULL, many, NULL, NULL, 0xFFFFFFFF, word="at most 128")
    refused(lib, "hrfd_dcs_set_codes", NULL, NULL, NULL, NULL, 1, word="their array")
    for code in (512, 0o1000, 65535):
        keep2, c = arr([0o023, code], np.uint16)
        refused(lib, "hrfd_dcs_set_codes", NULL, c, NULL, NULL, 2, word=f"entry 1 has code {code}")
        refused(lib, "hrfd_dcs_set_codes", NULL, c, NULL, NULL, 1, word="NULL handle")   # the entry lies behind K
    keep3, c = arr([0o023, 0o754, 0o411], np.uint16)
    for g in (4, 255):
        keep4, grp = arr([0, 3, g], np.uint8)
        refused(lib, "hrfd_dcs_set_codes", NULL, c, NULL, grp, 3, word=f"entry 2 has group {g}")
    # aliases: the same code twice, the three of a kind, a code against the inverted form of its complement's
    for codes, inv, text in (([0o023, 0o023], None, "entries 0 (D023N) and 1 (D023N)"),
                             ([0o754, 0o023, 0o114, 0o766], None, "entries 1 (D023N) and 3 (D766N)"),
                             ([0o023, 0o047], [0, 1], "entries 0 (D023N) and 1 (D047I)"),
                             ([0o375, 0o131, 0o340], [0, 0, 1], "entries 0 (D375N) and 2 (D340I)")):
        keep5, c = arr(codes, np.uint16)
        keep6, i = arr(inv, np.uint8) if inv is not None else (None, NULL)
        refused(lib, "hrfd_dcs_set_codes", NULL, c, i, NULL, len(codes), word=text)
        refused(lib, "hrfd_dcs_set_codes", NULL, c, i, NULL, len(codes), word="are aliases: both have the canonical word 0x")
    keep7, c = arr([0o023, 0o047], np.uint16)
    refused(lib, "hrfd_dcs_set_codes", NULL, c, NULL, NULL, 2, word="NULL handle")     # D023N and D047N are no aliases


def test_setters_check_their_values_before_the_handle(lib):
    for group in (4, 0xFFFFFFFE):
        refused(lib, "hrfd_dcs_set_min_hits", NULL, group, 128, word=f"group {group}")
    for n in (0, 513, 0xFFFFFFFF):
        refused(lib, "hrfd_dcs_set_min_hits", NULL, 0, n, word=f"min_hits {n}")
    for channel in (65536, 0xFFFFFFFE):
        refused(lib, "hrfd_dcs_reset", NULL, channel, word="channel")
    refused(lib, "hrfd_dcs_n_codes", NULL, NULL, word="NULL result")
    w = C.c_uint32(0)
    refused(lib, "hrfd_dcs_code_word", 512, 0, C.byref(w), C.byref(w), word="code 512")
    refused(lib, "hrfd_dcs_code_word", 0o023, 0, NULL, NULL, word="NULL result")
    assert lib.hrfd_dcs_code_word(0o023, 0, C.byref(w), NULL) == 0 and w.value == 0x763813
    assert lib.hrfd_dcs_code_word(0o023, 1, NULL, C.byref(w)) == 0 and w.value != 0x763813


def test_process_checks_sizes_and_addresses_before_the_handle(lib):
    buf = np.zeros(1 << 15, dtype=np.int64)
    a = buf.ctypes.data
    p, h, b, q, n = C.c_void_p(a + 65536), C.c_void_p(a), C.c_void_p(a + 16385), C.c_void_p(a + 32771), C.c_void_p(a + 49152)
    dev, host = "hrfd_dcs_process_device", "hrfd_dcs_process"
    for n_blocks in (0, 1025, 0xFFFFFFFF):
        refused(lib, host, NULL, p, NULL, n_blocks, h, b, q, word="n_blocks")
        refused(lib, dev, NULL, p, 1 << 33, NULL, n_blocks, h, b, q, NULL, word="n_blocks")
    refused(lib, host, NULL, p, NULL, 1, NULL, NULL, NULL, word="no output")
    refused(lib, dev, NULL, p, 1024, NULL, 1, NULL, NULL, NULL, NULL, word="no output")
    for stride, n_blocks in ((1025, 1), (1022, 1), (0, 1), (1, 1), (1024 * 1024 - 2, 1024)):
        refused(lib, dev, NULL, p, stride, NULL, n_blocks, h, b, q, NULL, word="channel_stride_bytes")
    refused(lib, dev, NULL, C.c_void_p(a + 65537), 1024, NULL, 1, h, b, q, NULL, word="even addresses")
    refused(lib, host, NULL, C.c_void_p(a + 65539), NULL, 1, h, b, q, word="even addresses")
    refused(lib, dev, NULL, p, 1024, NULL, 1, C.c_void_p(a + 1), b, q, NULL, word="even addresses")
    refused(lib, host, NULL, p, NULL, 1, C.c_void_p(a + 3), b, q, word="even addresses")
    for off in (1, 2, 3):
        refused(lib, dev, NULL, p, 1024, C.c_void_p(a + 49152 + off), 1, h, b, q, NULL, word="4-byte aligned" if off == 2 else None)
        refused(lib, host, NULL, p, C.c_void_p(a + 49152 + off), 1, h, b, q, word="4-byte aligned" if off == 2 else None)
    refused(lib, dev, NULL, NULL, 1024, NULL, 1, h, b, q, NULL, word="NULL argument")
    refused(lib, host, NULL, NULL, NULL, 1, h, b, q, word="NULL argument")
    # with everything else in order the refusal left is the handle's: every even residue of the PCM and of hits, best and
    # present at any address, each output alone, the limits themselves
    for res in range(0, 16, 2):
        refused(lib, dev, NULL, C.c_void_p(a + 65536 + res), 1030, n, 1, C.c_void_p(a + 14 - res), b, q, NULL, word="NULL handle")
    for outs in ((h, NULL, NULL), (NULL, b, NULL), (NULL, NULL, q)):
        refused(lib, dev, NULL, p, 1024, NULL, 1, *outs, NULL, word="NULL handle")
        refused(lib, host, NULL, p, NULL, 1, *outs, word="NULL handle")
    refused(lib, dev, NULL, p, 1024 * 1024, NULL, 1024, h, b, q, NULL, word="NULL handle")


def test_a_refused_slow_call_leaves_the_state_and_the_next_call_goes_on(lib):
    """hrfd_dcs_debug_slow checks like the bank's own entries, under its own name, and touches nothing it was given until every
    check has passed"""
    rng = np.random.default_rng(1)
    keep0, taps = arr([16384], np.int16)
    keep1, codes = arr([0o754, 0o023], np.uint16)
    keep2, alias = arr([0o754, 0o023, 0o340], np.uint16)
    keep3, mh = arr([128] * 4, np.uint32)
    keep4, bad_mh = arr([128, 0, 128, 128], np.uint32)
    pcm = rng.integers(-3000, 3000, size=1024).astype(np.int16)
    pp = C.c_void_p(pcm.ctypes.data)

    def state_after(first_refusals):
        state = np.zeros(300, dtype=np.uint32)
        sp = C.c_void_p(state.ctypes.data)
        hits, best, present = np.zeros((1, 2), dtype=np.uint16), np.zeros((1, 4), dtype=np.uint8), np.zeros((1, 4), dtype=np.uint8)
        o = [C.c_void_p(x.ctypes.data) for x in (hits, best, present)]
        assert lib.hrfd_dcs_debug_slow(taps, 1, codes, NULL, NULL, 2, mh, pp, NULL, 1, sp, *o) == 0
        before = state.copy()
        if first_refusals:
            name = "hrfd_dcs_debug_slow"
            refused(lib, name, taps, 0, codes, NULL, NULL, 2, mh, pp, NULL, 1, sp, *o, word="1..512 taps")
            refused(lib, name, taps, 1, alias, NULL, NULL, 3, mh, pp, NULL, 1, sp, *o, word="entries 1 (D023N) and 2 (D340N)")
            refused(lib, name, taps, 1, codes, NULL, NULL, 2, bad_mh, pp, NULL, 1, sp, *o, word="min_hits 0")
            refused(lib, name, taps, 1, codes, NULL, NULL, 2, NULL, pp, NULL, 1, sp, *o, word="NULL argument")
            refused(lib, name, taps, 1, codes, NULL, NULL, 2, mh, pp, NULL, 0, sp, *o, word="n_blocks")
            refused(lib, name, taps, 1, codes, NULL, NULL, 2, mh, pp, NULL, 1, sp, NULL, NULL, NULL, word="no output")
            refused(lib, name, taps, 1, codes, NULL, NULL, 2, mh, pp, NULL, 1, NULL, *o, word="NULL argument")
            assert (state == before).all() and before.any()
        assert lib.hrfd_dcs_debug_slow(taps, 1, codes, NULL, NULL, 2, mh, C.c_void_p(pcm.ctypes.data + 1024), NULL, 1, sp, *o) == 0
        return state, hits.copy()

    (s0, h0), (s1, h1) = state_after(False), state_after(True)
    assert (s0 == s1).all() and (h0 == h1).all()
