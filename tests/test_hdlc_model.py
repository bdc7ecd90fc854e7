"""The HDLC bank's law without a GPU: tests/hdlc_model.py (written from the contract) against the slow loop of
hackrfdiags_amd/csrc/hrfd_hdlc.h through hrfd_hdlc_debug_slow, against api.hdlc_frames over the joined stream (frames of at
most P bytes, carrier ignored) however the stream is cut, and on the cases the contract names: the row bound on back-to-back
minimal frames, over-long frames, maximal stuffing, a shared zero between flags, and the carrier dropped on a data bit and
on a closing flag's last bit."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import hdlc_model as hm


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class Slow:
    """one channel through hrfd_hdlc_debug_slow, the state carried from call to call"""

    def __init__(self, lib, m=1, P=512, require_carrier=False):
        self.lib, self.lim = lib, np.array([m, P, 1 if require_carrier else 0], dtype=np.uint32)
        self.state = np.zeros(260, dtype=np.uint32)

    def process(self, row, out_bytes):
        row = np.ascontiguousarray(row, dtype=np.uint8)
        out = np.full(out_bytes + 8, 0xA5, dtype=np.uint8)
        counts = np.zeros(3, dtype=np.uint32)
        p = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.lib.hrfd_hdlc_debug_slow(p(self.lim), p(row) if row.size else None, row.size, p(self.state), p(out), out_bytes, p(counts))
        assert rc == 0, self.lib.hrfd_last_error().decode()
        assert (out[out_bytes:] == 0xA5).all()
        return out[:out_bytes], counts


def both(lib, stream, cuts, m=1, P=512, require_carrier=False, out_bytes=None):
    """the stream cut at `cuts` through the model and the slow loop: counts first, then the rows, call by call.  Returns the
    good frames of the whole stream as (absolute end bit, payload)"""
    model, slow = hm.HdlcModel(1, m, P, require_carrier), Slow(lib, m, P, require_carrier)
    frames = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        ob = out_bytes if out_bytes is not None else hm.max_out(max(b - a, 1), m, P)
        want, n_frames, n_bad, dropped, outs = model.process([stream[a:b]], ob)
        got, counts = slow.process(stream[a:b], ob)
        assert counts.tolist() == [n_frames[0], n_bad[0], dropped[0]], (a, b)
        assert got[:len(outs[0])].tobytes() == outs[0], (a, b)
        assert (got[len(outs[0]):] == 0xA5).all(), "bytes behind the last record were written"
        assert api.Hdlc.parse(got, counts[0]) == want[0]
        if out_bytes is None:
            assert dropped[0] == 0
        frames += [(a + e, p) for e, p, _ in want[0]]
    return frames


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_slow_loop_and_hdlc_frames_agree_however_the_stream_is_cut(lib, seed):
    rng = np.random.default_rng(seed)
    P = (24, 64, 40)[seed - 1]
    m = (1, 3, 2)[seed - 1]
    stream = hm.mixed_stream(rng, 160, P=P)
    want = hm.reference_frames(stream, m, P)
    assert len(want) >= 20 and len(api.hdlc_frames(stream, m)) > len(want)         # some are over-long
    one = both(lib, stream, [0, len(stream)], m, P)
    assert [p for _, p in one] == want
    for k in (1, 7, 60):
        cut = both(lib, stream, hm.random_cuts(rng, len(stream), k), m, P)
        assert cut == one, f"{k} cuts"
    # every closing bit is a zero behind six ones
    for e, _ in one:
        assert (stream[e - 6:e] & 1).all() and not stream[e] & 1


@pytest.mark.parametrize("m", [1, 2, 5])
def test_max_out_never_drops_back_to_back_minimal_frames(lib, m):
    """50 frames of m bytes that share their flags: a closing bit every 8 (m + 3) bits where nothing is stuffed, the densest a
    stream can be (the payloads hold no five ones); the row of max_out holds them all, in one call and with a frame carried
    into the call"""
    P = 512
    stream = np.array(hm.shared_flag_frames([bytes([2 * i + 2] * m) for i in range(50)]), dtype=np.uint8)
    assert len(stream) <= 8 + 50 * (8 * (m + 3) + 3)           # (a check sequence may be stuffed)
    v = C.c_uint32(0)
    for max_bits in (1, 8 * (m + 3), 8 * (m + 3) + 1, len(stream), hm.MAX_BITS):
        assert lib.hrfd_hdlc_debug_max_out(max_bits, m, P, C.byref(v)) == 0 and v.value == hm.max_out(max_bits, m, P)
        assert v.value == api.hdlc_max_out(max_bits, m, P) and v.value % 4 == 0
    frames = both(lib, stream, [0, len(stream)], m, P)
    assert [p for _, p in frames] == [bytes([2 * i + 2] * m) for i in range(50)]
    # the first call ends one bit in front of a closing bit: the second closes a frame with its first bit
    ends = [e for e, _ in frames]
    assert min(np.diff(ends)) >= 8 * (m + 3) and (np.diff(ends) == 8 * (m + 3)).sum() >= 25
    for first in (ends[0], ends[3], 9):
        assert both(lib, stream, [0, first, len(stream)], m, P) == frames
    # and a row one record short drops exactly the last
    size = 8 + ((m + 3) & ~3)
    model = hm.HdlcModel(1, m, P)
    got = model.process([stream], 49 * size)
    assert (got[1][0], got[3][0]) == (49, 1)
    slow_out, counts = Slow(lib, m, P).process(stream, 49 * size)
    assert counts.tolist() == [49, 0, 1] and slow_out.tobytes() == got[4][0]


def test_over_long_frames_at_P_and_P_plus_1(lib):
    for P in (1, 5, 1021):
        ok, long = bytes(range(1, P + 1))[:P] if P < 256 else bytes([7] * P), bytes([9] * (P + 1))
        stream = np.array(hm.FLAG + hm.frame_bits(ok) + hm.FLAG + hm.frame_bits(long) + hm.FLAG + hm.frame_bits(ok[:1]) + hm.FLAG, dtype=np.uint8)
        frames = both(lib, stream, [0, len(stream)], 1, P)
        assert [p for _, p in frames] == [ok, ok[:1]]
        assert api.hdlc_frames(stream, 1) == [ok, long, ok[:1]]
        assert both(lib, stream, [0, len(stream) // 2, len(stream)], 1, P) == frames


def test_a_payload_of_all_ones_is_stuffed_the_most(lib):
    p = bytes([255] * 40)
    body = hm.frame_bits(p)
    assert len(body) >= 8 * 40 + 64            # a zero behind every five ones
    stream = np.array(hm.FLAG + body + hm.FLAG, dtype=np.uint8)
    for cuts in ([0, len(stream)], [0, 13, len(stream)], list(range(0, len(stream), 5)) + [len(stream)]):
        assert [q for _, q in both(lib, stream, cuts)] == [p]


def test_a_flag_that_shares_its_zero_with_the_next(lib):
    p, q = b"one", b"another"
    stream = np.array([0] + [1, 1, 1, 1, 1, 1, 0] * 3 + hm.frame_bits(p) + [0] + [1, 1, 1, 1, 1, 1, 0] * 2 + hm.frame_bits(q) + hm.FLAG,
                      dtype=np.uint8)
    frames = both(lib, stream, [0, len(stream)])
    assert [f for _, f in frames] == [p, q] == api.hdlc_frames(stream)
    for cut in range(1, len(stream)):
        assert both(lib, stream, [0, cut, len(stream)]) == frames


def test_n_bad_counts_a_frame_with_one_flipped_bit(lib):
    body = hm.frame_bits(b"link quality")
    body[20] ^= 1
    stream = np.array(hm.FLAG + body + hm.FLAG + hm.frame_bits(b"fine") + hm.FLAG, dtype=np.uint8)
    model = hm.HdlcModel(1)
    frames, n_frames, n_bad, dropped, _ = model.process([stream])
    assert ([p for _, p, _ in frames[0]], n_frames[0], n_bad[0], dropped[0]) == ([b"fine"], 1, 1, 0)
    assert [p for _, p in both(lib, stream, [0, 30, len(stream)])] == [b"fine"]


def test_require_carrier_on_a_data_bit_and_on_a_closing_flags_last_bit(lib):
    a, b, c = b"first", b"second", b"third"
    parts = [hm.FLAG, hm.frame_bits(a), hm.FLAG, hm.frame_bits(b), hm.FLAG, hm.frame_bits(c), hm.FLAG]
    stream = np.array(sum(parts, []), dtype=np.uint8) | hm.CARRIER
    end_a = len(parts[0]) + len(parts[1]) + 7                  # a's closing flag's last bit
    data_b = end_a + 1 + 11                                    # a data bit of b
    every = [p for _, p in both(lib, stream, [0, len(stream)], require_carrier=True)]
    assert every == [a, b, c]
    s = stream.copy()
    s[data_b] &= ~np.uint8(hm.CARRIER)
    assert [p for _, p in both(lib, s, [0, len(s)], require_carrier=True)] == [a, c]
    assert [p for _, p in both(lib, s, [0, len(s)], require_carrier=False)] == [a, b, c]
    s = stream.copy()
    s[end_a] &= ~np.uint8(hm.CARRIER)
    # the flag's last bit without carrier: the frame it closes is lost, the one it opens is not
    assert [p for _, p in both(lib, s, [0, len(s)], require_carrier=True)] == [b, c]
    for cut in (end_a, end_a + 1, data_b):
        assert [p for _, p in both(lib, s, [0, cut, len(s)], require_carrier=True)] == [b, c]
    # no carrier at all: nothing, with the flag on; everything with it off
    s = stream & ~np.uint8(hm.CARRIER)
    assert both(lib, s, [0, len(s)], require_carrier=True) == []
    assert [p for _, p in both(lib, s, [0, len(s)])] == [a, b, c]


def test_the_debug_entry_refuses_what_the_contract_refuses(lib):
    p = lambda a: C.c_void_p(a.ctypes.data)
    st, out, cnt, row = np.zeros(260, dtype=np.uint32), np.zeros(16, dtype=np.uint8), np.zeros(3, dtype=np.uint32), np.zeros(8, dtype=np.uint8)
    for lim, word in (([0, 512, 0], "min_payload 0"), ([1, 1022, 0], "max_payload 1022"), ([6, 5, 0], "min_payload 6")):
        lim = np.array(lim, dtype=np.uint32)
        assert lib.hrfd_hdlc_debug_slow(p(lim), p(row), 8, p(st), p(out), 16, p(cnt)) == -1
        assert word in lib.hrfd_last_error().decode()
    lim = np.array([1, 512, 0], dtype=np.uint32)
    assert lib.hrfd_hdlc_debug_slow(p(lim), p(row), 8, p(st), p(out), 6, p(cnt)) == -1 and "out_bytes 6" in lib.hrfd_last_error().decode()
    assert lib.hrfd_hdlc_debug_slow(p(lim), p(row), (1 << 20) + 1, p(st), p(out), 16, p(cnt)) == -1
    assert lib.hrfd_hdlc_debug_slow(p(lim), None, 8, p(st), p(out), 16, p(cnt)) == -1 and "NULL" in lib.hrfd_last_error().decode()
    st[0] = 8
    assert lib.hrfd_hdlc_debug_slow(p(lim), p(row), 8, p(st), p(out), 16, p(cnt)) == -1 and "no call leaves" in lib.hrfd_last_error().decode()
