"""The law of the HDLC framer bank (hrfd_hdlcgen_*, include/hrfd.h) restated in numpy, and the payloads the suites frame.

A frame is framed without a loop over its bits, by the run / scan formulation the kernel uses: a data bit's place in its run
of ones comes from a running maximum of "index of the last zero", a one whose place is a multiple of five is followed by a
stuffed zero, and an exclusive sum of those marks gives every data bit its place in the output.  The check sequence comes
from a byte table.  api.hdlc_encode, the per-bit loop, is what tests/test_hdlcgen_model.py holds this against."""
import numpy as np

MAX_PAYLOAD = 1021
MAX_BITS = 1 << 20
FLAG = np.array([0, 1, 1, 1, 1, 1, 1, 0], dtype=np.uint8)


def _crc_table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = (t >> 1) ^ (0x8408 * (t & 1))
    return t


CRC_TABLE = _crc_table()


def fcs(payload: bytes) -> int:
    crc = 0xFFFF
    for b in payload:
        crc = (crc >> 8) ^ int(CRC_TABLE[(crc ^ b) & 255])
    return crc ^ 0xFFFF


def frame_bits(payload: bytes) -> np.ndarray:
    """the bits of one frame between its flags: payload and check sequence LSB first, stuffed"""
    c = fcs(payload)
    d = np.unpackbits(np.frombuffer(bytes(payload) + bytes([c & 255, c >> 8]), dtype=np.uint8), bitorder="little")
    i = np.arange(d.size)
    last_zero = np.maximum.accumulate(np.where(d == 0, i, -1))     # in front of the frame's first bit: a zero at -1
    place = i - last_zero                                          # of a one in its run: 1, 2, ..
    mark = (d == 1) & (place % 5 == 0)
    at = i + np.cumsum(mark) - mark                                # exclusive sum
    out = np.zeros(d.size + int(mark.sum()), dtype=np.uint8)
    out[at] = d
    return out


def record_row(payloads, fcs_field: int = 0, end_bit: int = 0) -> np.ndarray:
    """payloads -> a row of records; a payload may be any bytes here (the malformed ones of the suites as well)"""
    out = bytearray()
    for p in payloads:
        p = bytes(p)
        out += int(end_bit).to_bytes(4, "little") + (len(p) & 0xFFFF).to_bytes(2, "little") + int(fcs_field).to_bytes(2, "little")
        out += p + b"\0" * (-len(p) & 3)
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def walk(row: np.ndarray, in_bytes: int, n_frames: int):
    """the payloads of the records the walk of a row reaches before it ends"""
    row = np.asarray(row, dtype=np.uint8)
    out, at = [], 0
    for _ in range(int(n_frames)):
        if in_bytes - at < 8:
            break
        n = int(row[at + 4]) | (int(row[at + 5]) << 8)
        size = 8 + ((n + 3) & ~3)
        if n == 0 or n > MAX_PAYLOAD or size > in_bytes - at:
            break
        out.append(row[at + 8:at + 8 + n].tobytes())
        at += size
    return out


def row_bits(row, in_bytes: int, n_frames: int, lead: int = 12, between: int = 2, tail: int = 3, max_bits: int = MAX_BITS):
    """one channel -> (bits, n_sent, dropped)"""
    parts, cur, sent = [], 0, 0
    for p in walk(row, in_bytes, n_frames):
        f = frame_bits(p)
        pre = lead if sent == 0 else between
        if cur + 8 * pre + f.size + 8 * tail > max_bits:
            break
        parts += [np.tile(FLAG, pre), f]
        cur += 8 * pre + f.size
        sent += 1
    if sent:
        parts.append(np.tile(FLAG, tail))
    bits = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return bits, sent, int(n_frames) - sent


def encode(payloads, lead: int = 12, between: int = 2, tail: int = 3, max_bits: int = MAX_BITS):
    row = record_row(payloads)
    return row_bits(row, row.size, len(payloads), lead, between, tail, max_bits)


def bound(n_frames: int, payload_bytes: int, lead: int = 12, between: int = 2, tail: int = 3) -> int:
    D = 8 * (payload_bytes + 2 * n_frames)
    return D + D // 5 + 8 * (lead + (n_frames - 1) * between + tail)


# ---- the payloads both suites frame
def _bits_to_bytes(bits):
    return np.packbits(np.array(bits, dtype=np.uint8), bitorder="little").tobytes()


def _search(rng, want, tries=200000):
    """a random payload of 2..9 bytes for which want(payload) holds; deterministic under the suites' seed"""
    for _ in range(tries):
        p = rng.integers(0, 256, int(rng.integers(2, 10)), dtype=np.uint8).tobytes()
        if want(p):
            return p
    raise AssertionError("no payload found")


def _fifth_one_is_last_bit(p):
    """the frame's last data bit is the fifth one of its run: its stuffed zero stands directly in front of the closing flag"""
    f = frame_bits(p)
    return f[-1] == 0 and f[-6:-1].all() and (f.size < 7 or f[-7] == 0) and fcs(p) >> 11 == 31


def _run_enters_fcs(p):
    """a run of ones that begins in the payload and goes on into the check sequence, across the stuffing point"""
    return p[-1] >> 5 == 7 and fcs(p) & 7 == 7


def edge_payloads(seed: int = 2025):
    """[(name, payload)]: what the issue lists.  Runs across lane (8 bits), wave (512) and tile (2048) boundaries; runs of
    4..11 ones that end at every bit of a lane; the two searched ones; zeros; one byte"""
    rng = np.random.default_rng(seed)
    out = [(f"ff x {n}", b"\xff" * n) for n in (1, 7, 8, 63, 64, 65, 255, 256, 257, 1021)]
    for run in (4, 5, 6, 9, 10, 11):
        bits = []
        for end in range(8):                                   # the run's last one is bit `end` of a byte
            lead_zeros = (end + 1 - run) % 8
            bits += [0] * 8 + [0] * lead_zeros + [1] * run + [0] * (7 - end)
        assert len(bits) % 8 == 0
        out.append((f"runs of {run}", _bits_to_bytes(bits)))
    out.append(("fifth one is the last bit", _search(rng, _fifth_one_is_last_bit)))
    out.append(("run into the check sequence", _search(rng, _run_enters_fcs)))
    out.append(("zeros", b"\0" * 40))
    out.append(("one byte", b"\x7e"))
    return out


def random_payloads(seed: int, count: int, lo: int = 1, hi: int = MAX_PAYLOAD):
    """random bytes, every other one mostly ones so that stuffing is dense"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(lo, hi + 1))
        p = rng.integers(0, 256, n, dtype=np.uint8)
        if k & 1:
            p |= rng.integers(0, 256, n, dtype=np.uint8)
            p |= rng.integers(0, 256, n, dtype=np.uint8)
        out.append(p.tobytes())
    return out
