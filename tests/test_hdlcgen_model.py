"""The HDLC framer bank's law on the CPU: tests/hdlcgen_model.py (the run / scan restatement) against api.hdlc_encode (the
per-bit loop) bit for bit, back through both decoders (api.hdlc_frames, tests/hdlc_model.py), the bound, the fit / drop rule
at its edges, the C text of hackrfdiags_amd/csrc/hrfd_hdlcgen.h through the built library's host entry hrfd_hdlc_encode, and
the AX.25 helpers.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import hdlc_model
from tests import hdlcgen_model as M

EDGES = M.edge_payloads()
RANDOM = M.random_payloads(7, 24) + M.random_payloads(8, 40, 1, 40)
FLAGS = [(12, 2, 3), (0, 1, 1), (255, 255, 255), (1, 7, 2)]


def c_encode(row, in_bytes, n_frames, lead, between, tail, max_bits, guard=64):
    """hrfd_hdlc_encode into a row between guard bytes -> (bits, n_sent, dropped); nothing outside [0, n_bits) is written"""
    row = np.ascontiguousarray(row, dtype=np.uint8)
    buf = np.full(max_bits + 2 * guard, 0xA5, dtype=np.uint8)
    n_bits, n_sent, dropped = C.c_uint32(99), C.c_uint32(99), C.c_uint32(99)
    rc = _lib.load().hrfd_hdlc_encode(C.c_void_p(row.ctypes.data), in_bytes, n_frames, lead, between, tail,
                                      C.c_void_p(buf.ctypes.data + guard), max_bits, C.byref(n_bits), C.byref(n_sent), C.byref(dropped))
    assert rc == 0, _lib.load().hrfd_last_error().decode()
    n = n_bits.value
    assert (buf[:guard] == 0xA5).all() and (buf[guard + n:] == 0xA5).all(), "a byte outside the row's n_bits was written"
    return buf[guard:guard + n].copy(), n_sent.value, dropped.value


def test_the_search_found_what_it_names():
    p = dict(EDGES)["fifth one is the last bit"]
    f = api.hdlc_encode([p], 0, 1, 1)
    assert f[-14:].tolist() == [1, 1, 1, 1, 1, 0] + M.FLAG.tolist() and M.fcs(p) >> 11 == 31
    q = dict(EDGES)["run into the check sequence"]
    assert q[-1] >> 5 == 7 and M.fcs(q) & 7 == 7
    assert M.fcs(b"123456789") == 0x906E == api.crc16_x25(b"123456789")


@pytest.mark.parametrize("name,payload", EDGES, ids=[n for n, _ in EDGES])
def test_model_equals_hdlc_encode_on_the_edge_payloads(name, payload):
    for lead, between, tail in FLAGS[:2]:
        bits, sent, dropped = M.encode([payload], lead, between, tail)
        assert (sent, dropped) == (1, 0)
        assert np.array_equal(bits, api.hdlc_encode([payload], lead, between, tail))
    assert M.frame_bits(payload).size <= 8 * (len(payload) + 2) + 8 * (len(payload) + 2) // 5


def test_model_equals_hdlc_encode_on_random_payloads():
    for p in RANDOM + [b"\x01", bytes(range(256)) * 3 + bytes(253)]:
        assert np.array_equal(M.encode([p])[0], api.hdlc_encode([p]))
    for lead, between, tail in FLAGS:
        batch = RANDOM[24:40] + [p for _, p in EDGES[10:]]
        assert np.array_equal(M.encode(batch, lead, between, tail)[0], api.hdlc_encode(batch, lead, between, tail))


def test_both_decoders_give_the_payloads_back():
    batch = [p for _, p in EDGES] + RANDOM[:6]
    bits, sent, _ = M.encode(batch, 2, 1, 2)
    assert sent == len(batch)
    assert api.hdlc_frames(bits) == batch
    frames, n_frames, n_bad, dropped, _ = hdlc_model.HdlcModel(1, 1, 1021).process([bits])
    assert [p for _, p, _ in frames[0]] == batch and (n_frames[0], n_bad[0], dropped[0]) == (len(batch), 0, 0)


def test_the_bound_is_met_by_ff_payloads_and_never_passed():
    """0xFF 0xFF has the check sequence 0xFFFF: a frame of 32 ones, 6 stuffed zeros = floor(32 / 5), so one such frame, and two
    (12 = floor(64 / 5)), meet the bound exactly.  Other all-0xFF payloads have zeros in their check sequence, so equality
    cannot hold for them: their length is asserted exactly instead, from the one run of the payload and a walk of the
    sixteen bits of the check sequence, and it stays below the bound, as everything does"""
    assert M.fcs(b"\xff\xff") == 0xFFFF
    for k in (1, 2):
        assert M.encode([b"\xff\xff"] * k)[0].size == M.bound(k, 2 * k) == api.hdlcgen_max_bits(k, 2 * k)
    for lead, between, tail in FLAGS:
        assert M.encode([b"\xff\xff"], lead, between, tail)[0].size == M.bound(1, 2, lead, between, tail)
    for n in (1, 7, 8, 63, 64, 65, 255, 256, 257, 1021):
        # the exact length: the payload is one run of 8 n ones with floor(8 n / 5) zeros in it; what is left of the run, 8 n % 5
        # ones, goes on into the sixteen bits of the check sequence, which are walked here
        c, ones, in_fcs = M.fcs(b"\xff" * n), 8 * n % 5, 0
        for k in range(16):
            ones = ones + 1 if (c >> k) & 1 else 0
            if ones == 5:
                in_fcs, ones = in_fcs + 1, 0
        got = M.encode([b"\xff" * n])[0].size
        assert got == 8 * (n + 2) + 8 * n // 5 + in_fcs + 8 * (12 + 3)
        assert got == api.hdlc_encode([b"\xff" * n]).size and got <= M.bound(1, n)
    for batch in ([p for _, p in EDGES], RANDOM[:10], RANDOM[24:]):
        assert M.encode(batch)[0].size <= M.bound(len(batch), sum(map(len, batch)))


def test_fit_and_drop_at_the_exact_length():
    batch = [b"\xff" * 9, b"hello", b"\x00\xf8\x1f", b"\xff" * 300]
    for lead, between, tail in FLAGS:
        full, _, _ = M.encode(batch, lead, between, tail)
        for k in range(1, len(batch) + 1):
            exact = M.encode(batch[:k], lead, between, tail)[0].size
            assert np.array_equal(M.encode(batch[:k], lead, between, tail)[0], api.hdlc_encode(batch[:k], lead, between, tail))
            for max_bits, sent in ((exact - 1, k - 1), (exact, k), (exact + 1, k)):
                bits, n_sent, dropped = M.encode(batch, lead, between, tail, max_bits)
                assert (n_sent, dropped) == (sent, len(batch) - sent), (k, max_bits)
                want = api.hdlc_encode(batch[:sent], lead, between, tail) if sent else np.zeros(0, dtype=np.uint8)
                assert np.array_equal(bits, want) and bits.size <= max_bits
        assert M.encode(batch, lead, between, tail, 1)[0].size == 0


def test_the_walk_ends_at_a_malformed_record():
    good = [b"abc", b"\xff" * 5, b"xyz1"]
    row = M.record_row(good, fcs_field=0xBEEF, end_bit=12345)      # end_bit and fcs are ignored
    assert np.array_equal(M.row_bits(row, row.size, 3)[0], api.hdlc_encode(good))
    for bad in (b"", b"\x55" * 1022):
        row = M.record_row([good[0], bad, good[2]])
        bits, sent, dropped = M.row_bits(row, row.size, 3)
        assert (sent, dropped) == (1, 2) and np.array_equal(bits, api.hdlc_encode(good[:1]))
    row = M.record_row(good)
    for cut, sent in ((row.size - 4, 2), (12 + 16 + 4, 2), (12 + 12, 1), (12 + 4, 1), (8, 0), (4, 0)):
        bits, n_sent, dropped = M.row_bits(row, cut, 3)
        assert (n_sent, dropped) == (sent, 3 - sent), cut
    assert M.row_bits(row, row.size, 0) [1:] == (0, 0) and M.row_bits(row, row.size, 5)[1:] == (3, 2)


# ---- the C text through the built library
def test_hrfd_hdlc_encode_equals_the_model():
    lib = _lib.load()
    assert hasattr(lib, "hrfd_hdlc_encode"), "the library has no host framer"
    for name, p in EDGES:
        row = M.record_row([p])
        for lead, between, tail in FLAGS[:2]:
            want, _, _ = M.encode([p], lead, between, tail)
            got, sent, dropped = c_encode(row, row.size, 1, lead, between, tail, want.size)
            assert np.array_equal(got, want) and (sent, dropped) == (1, 0), name
    for lead, between, tail in FLAGS:
        batch = RANDOM[:4] + RANDOM[24:40] + [p for _, p in EDGES[10:]]
        row = M.record_row(batch)
        want, _, _ = M.encode(batch, lead, between, tail)
        got, sent, dropped = c_encode(row, row.size, len(batch), lead, between, tail, M.bound(len(batch), sum(map(len, batch)), lead, between, tail))
        assert np.array_equal(got, want) and (sent, dropped) == (len(batch), 0)
        assert np.array_equal(api.hdlc_encode_c(batch, lead, between, tail), want)


def test_hrfd_hdlc_encode_fits_drops_and_walks_like_the_model():
    batch = [b"\xff" * 9, b"hello", b"\x00\xf8\x1f", b"\xff" * 300]
    row = M.record_row(batch)
    for lead, between, tail in FLAGS:
        for k in range(1, len(batch) + 1):
            exact = M.encode(batch[:k], lead, between, tail)[0].size
            for max_bits in (exact - 1, exact, exact + 1):
                want = M.encode(batch, lead, between, tail, max_bits)
                got = c_encode(row, row.size, len(batch), lead, between, tail, max_bits)
                assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (k, max_bits)
        assert c_encode(row, row.size, len(batch), lead, between, tail, 1) [1:] == (0, 4)
    good = [b"abc", b"\xff" * 5, b"xyz1"]
    for bad in (b"", b"\x55" * 1022):
        row = M.record_row([good[0], bad, good[2]])
        got = c_encode(row, row.size, 3, 12, 2, 3, 4096)
        assert got[1:] == (1, 2) and np.array_equal(got[0], api.hdlc_encode(good[:1]))
    row = M.record_row(good, fcs_field=0xBEEF, end_bit=12345)
    for cut in (row.size, row.size - 4, 12 + 16 + 4, 12 + 12, 12 + 4, 8, 4):
        for n_frames in (0, 1, 3, 5):
            want = M.row_bits(row, cut, n_frames)
            got = c_encode(row[:cut].copy(), cut, n_frames, 12, 2, 3, 4096)        # a copy of exactly in_bytes bytes
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (cut, n_frames)
    out, (sent, dropped) = api.hdlc_encode_c(batch, max_bits=200, want_counts=True)
    assert (sent, dropped) == M.encode(batch, max_bits=200)[1:] and np.array_equal(out, M.encode(batch, max_bits=200)[0])
    assert api.hdlc_encode_c([]).size == 0


# ---- AX.25
def test_ax25_helpers_match_a_hand_written_ui_frame_and_round_trip():
    want = bytes([0x82, 0xA0, 0xA4, 0xA6, 0x40, 0x40, 0x60,            # APRS  -0
                  0x9C, 0x60, 0x86, 0x82, 0x98, 0x98, 0x62,            # N0CALL-1
                  0xAE, 0x92, 0x88, 0x8A, 0x62, 0x40, 0x65,            # WIDE1 -2, the last address
                  0x03, 0xF0]) + b">hi"
    assert api.ax25_ui_frame("APRS", "n0call-1", b">hi", path=["WIDE1-2"]) == want
    assert api.ax25_address("APRS", 0) == want[:7] and api.ax25_address("WIDE1", 2, last=True) == want[14:21]
    got = api.ax25_parse(want)
    assert got == {"dest": ("APRS", 0), "src": ("N0CALL", 1), "path": [("WIDE1", 2)], "control": 3, "pid": 0xF0, "info": b">hi"}
    for dest, src, path, pid, info in ((("CQ", 0), ("A1A", 15), [], 0xF0, b""), ("BEACON-3", "DL1ABC-7", ["RELAY", ("WIDE2", 2)], 0xCF, bytes(range(256))),
                                       ("X", "Y", ["D%d-%d" % (i, i) for i in range(8)], 0, b"\x7e\xff")):
        f = api.ax25_ui_frame(dest, src, info, path, pid)
        g = api.ax25_parse(f)
        assert api.ax25_ui_frame(g["dest"], g["src"], g["info"], g["path"], g["pid"]) == f and g["control"] == 3 and g["info"] == info
        assert api.hdlc_frames(api.hdlc_encode_c([f])) == [f]
    for call, ssid in (("", 0), ("TOOLONG", 0), ("AB-C", 0), ("OK", 16), ("OK", -1)):
        with pytest.raises(ValueError):
            api.ax25_address(call, ssid)
    with pytest.raises(ValueError):
        api.ax25_ui_frame("A", "B", b"", path=["C"] * 9)
    with pytest.raises(ValueError):
        api.ax25_ui_frame("A", "B", bytes(1021))
    for bad in (want[:13], want[:21], want[:21] + b"\x13\xf0", bytes([0x83]) + want[1:]):
        with pytest.raises(ValueError):
            api.ax25_parse(bad)
