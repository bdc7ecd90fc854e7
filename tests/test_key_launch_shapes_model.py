"""The arithmetic tests/test_gpu_key_launch_shapes.py and tests/test_gpu_hdlcgen_launch_shapes.py rest on, restated from the
source as plain functions and checked without a device: where k_duc<R, true> puts the boundary between the dwords it reads and
the dwords it zeroes (OFF, delta, p_lo, p_hi of hackrfdiags_amd/csrc/hrfd_duc.hip, all functions of the tap counts), how
ddc_store_zeros (hrfd_ddc.hip) splits a row's bytes into a head, 16-byte stores and a tail, and which tile of 256 lanes a byte
of a frame falls into in k_hdlcgen (hrfd_hdlcgen.hip).  The tap lists, key rows, store sweeps and payloads of the GPU files are
built here, so that this file states what each of them reaches: OFF = 0 and the largest OFF of every rate, both values of
delta, every combination of (key in the tile in front, key in the tile) the masking tells apart; every row residue modulo 16
under every class of store; payloads of 1, 2, 3 and 4 tiles whose check sequence lies across a tile edge, a run of ones
carried from tile to tile, the most bits `ob` holds in LDS, a row that no further frame fits.  The GPU files import all of it
and assert the same figures next to their calls, so that a constant that moves in the library fails an assertion there
instead of leaving a test that no longer reaches its path."""
import numpy as np

from tests import hdlcgen_model as M

_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


# ================================================================ the keyed DUC
TILE = 1024                                # kBankTile: k_duc's and k_ddc's
DUC_MAX_TA, DUC_MAX_TB, DUC_H = 64, 256, 318
RATES = (1, 2, 4, 8)


def duc_geometry(TA, TB, R):
    """(LA, LB, OFF, delta) of k_duc: the look-back of stage A in channel samples and of stage B, the even number of samples
    the u rails hold in front of the tile, and where stage B's window of v index 0 starts in them"""
    LA = (TA - 1) // R if TA > 0 else 0
    LB = TB - 1 if TB > 0 else 0
    OFF = (LA + LB + 1) & ~1
    return LA, LB, OFF, OFF - LA - LB


def duc_read_range(TA, TB, R, on_prev, on_cur):
    """(p_lo, p_hi, nud): the u dwords the keyed kernel reads of the nud it fills; the others are zeros"""
    OFF = duc_geometry(TA, TB, R)[2]
    return (0 if on_prev else OFF // 2), ((OFF + TILE) // 2 if on_cur else OFF // 2), (OFF + TILE + 16) // 2


def duc_tap_pairs(R):
    """test_gpu_duc.test_random_taps_every_shift_and_amplitude's tap counts.  (3 R + 1, 5) has LA + LB = 3 + 4, so delta = 1,
    at every rate (others, like (2, 146) from R = 2 on, at some): no further pair is needed"""
    return [(1, 1), (2, 146), (64, 256), (0, 37), (33, 0), (0, 0), (7, 255), (3 * R + 1, 5), (64, 2)]


def duc_unit(row, t, k):
    """what k_duc<R, true> does with unit (channel, tile t) under the channel's key row at key block 2^k: "skip", or the
    (on_prev, on_cur) its masking is built from.  Tile 0 has no tile in front: its look-back is the history, masked already"""
    block = lambda m: int(row[m >> k]) != 0
    on_cur = block(TILE * t)
    on_prev = t == 0 or block(TILE * (t - 1))
    return "skip" if t >= 1 and not on_cur and not on_prev else (on_prev, on_cur)


K1_W, K1_C, K1_K, K1_M = 2, 5, 10, 3 * TILE + 77
K1_CAPS = [1, 0, 1, 0, 1]
K1_KEY = np.array([[1, 0, 0, 0x80],        # on -> off, off -> off, off -> on (the remainder)
                   [0, 0, 0, 0],           # tile 0 off: computed over the history alone, the rest skipped
                   [2, 1, 255, 7],         # always
                   [0, 1, 0, 0],           # with channel 1: capture 0 is idle in tile 3
                   [1, 1, 0, 0]], dtype=np.uint8)
K1_KEY.setflags(write=False)
K2_M, K2_BEHIND = TILE + 300, 700
K2_KEY = np.array([[1, 0], [0, 0], [0, 1], [1, 1], [0, 0]], dtype=np.uint8)      # channels 0, 1 and 4 end the call keyed off
K5_W, K5_C, K5_R, K5_M, K5_ON = 16, 64, 8, 2 * TILE + 77, 8


def k5_key(seed):
    """[64, 3]: 8 of the 64 channels have a random key in which every one of them is on somewhere, the others are off"""
    rng = np.random.default_rng(seed)
    key = np.zeros((K5_C, -(-K5_M // TILE)), dtype=np.uint8)
    on = np.sort(rng.choice(K5_C, size=K5_ON, replace=False))
    for c in on:
        while not key[c].any():
            key[c] = rng.integers(0, 2, size=key.shape[1]) * rng.integers(1, 256, size=key.shape[1])
    return key, on


def test_duc_tap_pairs_reach_every_boundary_of_the_masking():
    assert duc_geometry(64, 256, 1) == (63, 255, 318, 0) and DUC_H == 318
    assert duc_geometry(0, 0, 8) == (0, 0, 0, 0) and duc_geometry(1, 1, 4) == (0, 0, 0, 0)
    assert duc_geometry(4, 5, 1) == (3, 4, 8, 1) and duc_geometry(0, 37, 2) == (0, 36, 36, 0) and duc_geometry(33, 0, 2) == (16, 0, 16, 0)
    for R in RATES:
        geo = {p: duc_geometry(*p, R) for p in duc_tap_pairs(R)}
        offs = [g[2] for g in geo.values()]
        largest = max(duc_geometry(ta, tb, R)[2] for ta in range(DUC_MAX_TA + 1) for tb in range(DUC_MAX_TB + 1))
        assert min(offs) == 0 and max(offs) == largest == geo[(64, 256)][2] == ((63 // R + 255 + 1) & ~1)
        assert {g[3] for g in geo.values()} == {0, 1} and geo[(3 * R + 1, 5)][3] == 1
        assert any(ta == 0 and tb > 0 for ta, tb in geo) and any(tb == 0 and ta > 0 for ta, tb in geo)
        assert all(g[2] % 2 == 0 and g[2] <= DUC_H and g[3] in (0, 1) for g in geo.values())
        # the boundary between read and zeroed dwords moves with the taps: as many places as there are OFFs
        assert len({duc_read_range(*p, R, False, True)[0] for p in geo}) == len(set(offs)) >= 7
        for p in geo:
            lo, hi, nud = duc_read_range(*p, R, True, True)
            assert (lo, nud - hi) == (0, 8)                    # the 16 samples behind the tile are never read under a key
            assert duc_read_range(*p, R, False, False)[0] == duc_read_range(*p, R, False, False)[1]
    assert [duc_geometry(64, 256, R)[2] for R in RATES] == [318, 286, 270, 262]


def test_k1_key_rows_reach_every_case_of_the_masking():
    tiles = -(-K1_M // TILE)
    assert tiles == 4 == K1_KEY.shape[1] and K1_M % TILE == 77 and K1_KEY.shape[0] == K1_C == len(K1_CAPS)
    units = {(c, t): duc_unit(K1_KEY[c], t, K1_K) for c in range(K1_C) for t in range(tiles)}
    assert [units[0, t] for t in range(4)] == [(True, True), (True, False), "skip", (False, True)]
    assert [units[1, t] for t in range(4)] == [(True, False), "skip", "skip", "skip"]
    assert {units[2, t] for t in range(4)} == {(True, True)}
    assert set(units.values()) == {"skip", (True, True), (True, False), (False, True)}
    assert units[0, 3] == (False, True)                        # the remainder of 77 samples behind an idle tile
    assert sum(v == "skip" for v in units.values()) == 1 + 3 + 0 + 1 + 1
    # two channels of capture 0 are idle in tile 3, and they are all it has: that workgroup skips every unit it loops over
    on_zero = [c for c in range(K1_C) if K1_CAPS[c] == 0]
    assert on_zero == [1, 3] and all(units[c, 3] == "skip" for c in on_zero) and not all(units[c, 2] == "skip" for c in on_zero)


def test_k2_and_k5_shapes():
    assert K2_KEY.shape == (K1_C, -(-K2_M // TILE)) and [int(r[-1]) for r in K2_KEY] == [0, 0, 1, 1, 0]
    # the history the call stores is 18 samples of the first key block and 300 of the last: masked sample by sample
    assert duc_geometry(64, 256, 1)[2] == DUC_H and K2_M - DUC_H == TILE - 18 and K2_BEHIND < TILE
    key, on = k5_key(5)
    assert key.shape == (64, 3) and len(on) == 8 and sorted(np.flatnonzero(key.any(axis=1)).tolist()) == on.tolist()
    units = [duc_unit(key[c], t, 10) for c in range(K5_C) for t in range(3)]
    assert units.count("skip") >= 2 * 56 and {(True, True), (True, False), (False, True)} & set(units)
    assert K5_W * K5_C == 1024 and K5_C % K5_W == 0


# ================================================================ the keyed DDC's zero store
def ddc_zero_split(residue, n):
    """(head, n16, tail) of ddc_store_zeros for n bytes at an address of `residue` modulo 16"""
    head = min(-residue & 15, n)
    n16 = (n - head) >> 4
    return head, n16, n - head - 16 * n16


def zero_classes(residue, n):
    """the names of the store's shapes that (residue, n) is an instance of"""
    head, n16, tail = ddc_zero_split(residue, n)
    out = set()
    if head == n:
        out.add("ends in the head")
    if n16 == 0 and tail > 0:
        out.add("no 16-byte store, a tail")
    if tail == 0 and n16 > 0:
        out.add("16-byte stores, no tail")
    if head == 0:
        out.add("no head")
    if head > 0 and n16 > 0 and tail > 0:
        out.add("all three")
    return out


ZERO_CLASSES = {"ends in the head", "no 16-byte store, a tail", "16-byte stores, no tail", "no head", "all three"}
R1_C = 16
R1_M = (1, 2, 7, 8, 9, 15, 16, 17, 24, 1023)                   # outputs of the short tile: 2 M bytes to zero


_SHORT = {"ends in the head", "no 16-byte store, a tail", "no head"}
_LONG = {"16-byte stores, no tail", "all three", "no head"}
# bytes to zero -> the classes the 16 residues give it.  Up to 14 bytes a store ends in the head or has no 16-byte store; 16
# bytes do not fit behind a head; from 32 bytes on there always is a 16-byte store
R1_CLASSES = {2: _SHORT, 4: _SHORT, 14: _SHORT, 16: {"16-byte stores, no tail", "no 16-byte store, a tail", "no head"},
              18: _LONG | {"no 16-byte store, a tail"}, 30: _LONG | {"no 16-byte store, a tail"}, 32: _LONG, 34: _LONG, 48: _LONG,
              2046: _LONG}


def r1_pad(ob):
    """rows ob + pad bytes apart with ob + pad = 1 modulo 16: channel c's row starts at residue (first row's + c) % 16"""
    return (1 - ob) % 16 + 16


def r1_on_channel(i):
    """the one channel that is keyed on in the i-th single-tile call"""
    return (5 * i + 2) % R1_C


def r1_reach(M, first_residue, on=None):
    """{(residue, classes)} the zero store of a short tile of M outputs meets on 16 channels, all but `on` keyed off"""
    return {((first_residue + c) % 16, frozenset(zero_classes((first_residue + c) % 16, 2 * M))) for c in range(R1_C) if c != on}


def test_ddc_zero_split_restates_the_store():
    assert ddc_zero_split(0, 16) == (0, 1, 0) and ddc_zero_split(1, 2) == (2, 0, 0) and ddc_zero_split(1, 15) == (15, 0, 0)
    assert ddc_zero_split(8, 14) == (8, 0, 6) and ddc_zero_split(3, 2046) == (13, 127, 1) and ddc_zero_split(15, 34) == (1, 2, 1)
    assert ddc_zero_split(0, 2) == (0, 0, 2) and ddc_zero_split(12, 4) == (4, 0, 0) and ddc_zero_split(12, 36) == (4, 2, 0)
    for residue in range(16):
        for n in range(0, 2049, 2):
            head, n16, tail = ddc_zero_split(residue, n)
            assert head + 16 * n16 + tail == n and 0 <= head < 16 and 0 <= tail < 16
            assert (residue + head) % 16 == 0 or (head == n and n16 == tail == 0)


def test_r1_sweep_reaches_every_residue_under_every_class():
    assert all((ob + r1_pad(ob)) % 16 == 1 and r1_pad(ob) >= 16 for ob in range(2, 4200, 2))
    assert len({r1_on_channel(i) for i in range(len(R1_M))}) == len(R1_M)      # another channel in every call
    for first in range(16):                                    # wherever the allocation puts the first row
        single, second = set(), set()
        for i, m in enumerate(R1_M):
            single |= {(2 * m, r, cl) for r, cl in r1_reach(m, first, r1_on_channel(i))}
            second |= {(2 * m, r, cl) for r, cl in r1_reach(m, first)}
        for name in ZERO_CLASSES:
            # the second tiles: every class at every residue that can hold it under these lengths.  No head only at residue
            # 0, a head not at residue 0, and one that the shortest store (2 bytes) ends in is not 1 byte long either; no
            # tail behind 16-byte stores needs a head of n modulo 16: 0, 2 or 14 bytes for the lengths 16 .. 48
            got = {r for _, r, cl in second if name in cl}
            want = {"no head": {0}, "ends in the head": set(range(1, 15)), "all three": set(range(1, 16)),
                    "16-byte stores, no tail": {0, 2, 14}}.get(name, set(range(16)))
            assert got == want, (first, name, sorted(got))
            # the single tiles leave one channel out per call: every class still, at all of its residues but one at most
            alone = {r for _, r, cl in single if name in cl}
            assert alone <= want and len(alone) >= max(1, len(want) - 1), (first, name, sorted(alone))
        assert {r for _, r, _ in single} == set(range(16))
        assert {r for _, r, _ in second} == set(range(16)) and len(second) == 16 * len(R1_M)
        assert len(single) == 15 * len(R1_M)
    # the classes by the length alone
    assert sorted(R1_CLASSES) == [2 * m for m in R1_M]
    for n, classes in R1_CLASSES.items():
        assert set().union(*(zero_classes(r, n) for r in range(16))) == classes, n
    assert zero_classes(1, 2) == {"ends in the head"} and zero_classes(1, 30) == {"no 16-byte store, a tail"}
    assert "ends in the head" in zero_classes(2, 14) and "ends in the head" not in zero_classes(3, 14)
    assert {n for n in (2 * m for m in R1_M) if "16-byte stores, no tail" in zero_classes(0, n)} == {16, 32, 48}


# ================================================================ the keyed receive: key blocks against rx blocks
R2_BLOCK_BYTES, R2_BLOCKS = 2 * 1536, 4


def test_r2_key_blocks_straddle_rx_blocks():
    M_out = R2_BLOCK_BYTES // 2 * R2_BLOCKS
    assert M_out == 6 * TILE
    rx_edges = {1536 * b for b in range(1, R2_BLOCKS)}
    for k, n_keys in ((10, 6), (12, 2)):
        key_edges = {j << k for j in range(1, -(-M_out // (1 << k)))}
        assert -(-M_out // (1 << k)) == n_keys
        assert key_edges - rx_edges and rx_edges - key_edges, "edges of each kind that are not the other's"
        straddle = [j for j in range(n_keys) if any(j << k < e < min((j + 1) << k, M_out) for e in rx_edges)]
        assert straddle, k
    assert (1 << 17) == 512 * 256                              # the only block the own suite uses: one rx block of 512 PCM samples


# ================================================================ the framer
HDLCGEN_LANES = 256                        # kHdlcgenThreads: one data byte a lane, 2048 data bits a tile
HDLCGEN_MAX_FRAME = 9820                   # kHdlcgenMaxFrame
HDLCGEN_MAX_FLAGS = 255
F1_N = (253, 254, 255, 256, 509, 510, 511, 512, 765, 766, 767, 768, 1019, 1020, 1021)


def tiles(n):
    """the tiles k_hdlcgen takes for a payload of n bytes: its n + 2 data bytes, 256 a tile"""
    return -(-(n + 2) // HDLCGEN_LANES)


def fcs_lanes(n):
    """[(tile, lane)] of the check sequence's two bytes"""
    return [divmod(n, HDLCGEN_LANES), divmod(n + 1, HDLCGEN_LANES)]


def data_bits(payload):
    c = M.fcs(payload)
    return np.unpackbits(np.frombuffer(bytes(payload) + bytes([c & 255, c >> 8]), dtype=np.uint8), bitorder="little")


def run_across(payload, edge):
    """(first bit, length) of the run of ones in the frame's data bits that holds the last bit in front of byte `edge` and
    the first bit of it, or None"""
    d = data_bits(payload)
    at = 8 * edge
    if at >= d.size or not (d[at - 1] and d[at]):
        return None
    lo, hi = at - 1, at
    while lo > 0 and d[lo - 1]:
        lo -= 1
    while hi + 1 < d.size and d[hi + 1]:
        hi += 1
    return lo, hi - lo + 1


def f1_edge(n):
    """the tile edge (a byte index) the crossing payload of n bytes crosses: the last one that has a data byte behind it"""
    return HDLCGEN_LANES * ((n + 1) // HDLCGEN_LANES) if n + 2 > HDLCGEN_LANES else None


def crossing_payload(n):
    """n random bytes with a run of 7..11 ones across f1_edge(n).  Where the edge has two payload bytes on either side the run
    is written into zeros; where the check sequence lies at the edge (n = 255, 256, 511, 512, 767, 768) payloads are drawn
    until their check sequence completes such a run.  n = 253 and 254 are one tile: there the run ends the payload"""
    def make():
        rng = np.random.default_rng(1000 + n)
        edge = f1_edge(n)
        for _ in range(100000):
            p = rng.integers(0, 256, n, dtype=np.uint8)
            length = int(rng.integers(7, 12))
            if edge is None:
                bits = np.unpackbits(p, bitorder="little")
                bits[-length - 1:] = [0] + [1] * length
                return np.packbits(bits, bitorder="little").tobytes()
            front = int(rng.integers(1, length))               # ones in front of the edge
            if edge + 2 <= n:
                bits = np.unpackbits(p, bitorder="little")
                bits[8 * (edge - 2):8 * (edge + 2)] = 0
                bits[8 * edge - front:8 * edge - front + length] = 1
                return np.packbits(bits, bitorder="little").tobytes()
            if edge - 1 < n:                                   # the byte in front of the edge is the payload's: ones at its top
                p[edge - 1] = (0xFF << (8 - min(front, 7))) & 0xFF
            got = run_across(p.tobytes(), edge)
            if got is not None and 7 <= got[1] <= 11:
                return p.tobytes()
        raise AssertionError(f"no payload of {n} bytes found")
    return once(("crossing", n), make)


def f1_payloads():
    """per n of F1_N: (plain, dense in ones, crossing)"""
    return once("f1", lambda: [M.random_payloads(300 + n, 2, n, n) + [crossing_payload(n)] for n in F1_N])


def f1_items():
    return [p for three in f1_payloads() for p in three]


F2_FLAGS = ((255, 255, 255), (0, 255, 1))
FF = b"\xff" * M.MAX_PAYLOAD


def f2_rows():
    return once("f2", lambda: [[FF, FF], [FF], [M.random_payloads(77, 1, 1021, 1021)[0], FF]])


F3_FRAMES = (106, 130, 4000)


def f3_rows():
    """a row that all 106 frames of 1021 bytes fit, one of 130 that fills max_bits = 2^20, one of 4000 one-byte frames"""
    return once("f3", lambda: [M.random_payloads(31, 106, 1021, 1021), M.random_payloads(32, 130, 1021, 1021),
                               [bytes([b]) for b in np.random.default_rng(33).integers(0, 256, 4000).tolist()]])


def f3_want():
    return once("f3 want", lambda: [M.encode(p) for p in f3_rows()])


def test_hdlcgen_tiles_and_the_check_sequence_across_tile_edges():
    assert [tiles(n) for n in (1, 254, 255, 510, 511, 766, 767, 1021)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert sorted({tiles(n) for n in F1_N}) == [1, 2, 3, 4] and tiles(M.MAX_PAYLOAD) == 4
    for t in range(3):
        assert fcs_lanes(256 * t + 255) == [(t, 255), (t + 1, 0)] and 256 * t + 255 in F1_N
        assert fcs_lanes(256 * t + 254) == [(t, 254), (t, 255)] and fcs_lanes(256 * t + 256) == [(t + 1, 0), (t + 1, 1)]
    assert [f1_edge(n) for n in F1_N] == [None, None, 256, 256, 256, 256, 512, 512, 512, 512, 768, 768, 768, 768, 768]
    # the per-byte CRC term at every distance 1..1021 from the check sequence, the levels 2^8 and 2^9 among them
    assert max(F1_N) == 1021 and (1021 >> 9) & 1 and (300 >> 8) & 1


def test_f1_payloads_carry_a_run_across_every_tile_edge():
    per = f1_payloads()
    assert len(per) == len(F1_N) and all(len(p) == n for n, three in zip(F1_N, per) for p in three)
    crossed = set()
    for n, (plain, dense, crossing) in zip(F1_N, per):
        assert plain != dense and 0 < np.unpackbits(np.frombuffer(plain, dtype=np.uint8)).mean() < 0.6 < np.unpackbits(np.frombuffer(dense, dtype=np.uint8)).mean() < 1
        edge = f1_edge(n)
        if edge is None:
            d = data_bits(crossing)[:8 * n]
            tail_run = int(np.argmin(d[::-1]))                 # the ones that end the payload
            assert 7 <= tail_run <= 11 and tiles(n) == 1
            continue
        first, length = run_across(crossing, edge)
        assert 7 <= length <= 11 and first < 8 * edge <= first + length - 1 < 8 * (edge + 2), (n, first, length)
        crossed.add(edge)
        # a run of 7 or more is stuffed at least once, and the run the next tile starts behind is not zero
        assert M.frame_bits(crossing).size > 8 * (n + 2)
    assert crossed == {256, 512, 768}
    # the three payloads of a length differ in their check sequences, and none of them is all ones
    assert all(len({M.fcs(p) for p in three}) == 3 and b"\xff" * 64 not in b"".join(three) for three in per)


def test_f2_fills_ob_and_f3_fills_the_row():
    assert M.frame_bits(FF).size == 9819 <= HDLCGEN_MAX_FRAME
    for flags in F2_FLAGS:
        lead, between, tail = flags
        want = [M.encode(p, *flags) for p in f2_rows()]
        assert [w[1] for w in want] == [2, 1, 2]
        assert want[0][0].size == 8 * (lead + between + tail) + 2 * 9819 and want[1][0].size == 8 * (lead + tail) + 9819
    assert M.encode(f2_rows()[0], 255, 255, 255)[0].size == 25758
    # ob holds the flags in front of a frame and the frame: 255 flags and the longest frame there is
    assert 8 * HDLCGEN_MAX_FLAGS + M.frame_bits(FF).size == 2040 + 9819 <= 8 * HDLCGEN_MAX_FLAGS + HDLCGEN_MAX_FRAME
    assert M.frame_bits(f2_rows()[2][0]).size < 9000               # the random frame in front of the longest one
    # F3
    assert M.bound(106, 106 * 1021) <= M.MAX_BITS < M.bound(107, 107 * 1021)
    (b0, s0, d0), (b1, s1, d1), (b2, s2, d2) = f3_want()
    assert (s0, d0) == (106, 0) and s1 + d1 == 130 and d1 > 0 and s1 > 106 and (s2, d2) == (4000, 0)
    between, tail = 2, 3
    assert M.MAX_BITS - HDLCGEN_MAX_FRAME - 8 * (between + tail) < b1.size <= M.MAX_BITS
    nxt = M.frame_bits(f3_rows()[1][s1]).size
    assert b1.size - 8 * tail + 8 * between + nxt + 8 * tail > M.MAX_BITS      # the frame that was dropped did not fit
    assert b2.size > 4000 * (24 + 16) and 130 * (8 + 1024) == 134160
