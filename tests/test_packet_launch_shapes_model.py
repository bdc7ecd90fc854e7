"""The dispatch arithmetic tests/test_gpu_packet_launch_shapes.py rests on, restated from the source as plain functions and
checked without a device: how afskgen_stage cuts the dirty (slot, channel) entries into uploads (hackrfdiags_amd/csrc/
hrfd_afskgen.hip), which bits of a row k_hdlc classes as flags and how many of them a tile of 2048 holds (the contract's rule;
hrfd_hdlc.hip closes them 256 a round), and what a window gives k_afsk for its tap packing (hrfd_afsk.hip).  AfskgenDirty
restates the host's bookkeeping that decides which entries are dirty at a launch: the slot a message takes, what a cut and an
ended message touch.  The streams of the GPU file's section H are built here, so that this file states, against
tests/hdlc_model.py, what each of them reaches: more than 256 flags in a tile, 293 flags in a tile, an end_bit above 65535
in a row of 70 000 bits, a carried frame of exactly cap bits, resets that change what the call behind them gives.  The GPU file imports all of it and asserts the same figures next to its calls, so that a
constant that moves in the library fails an assertion there instead of leaving a test that no longer reaches its path."""
import numpy as np

from tests import afskgen_model as gm
from tests import hdlc_model as hm

AFSKGEN_STAGE_SLOTS = 256                  # kAfskgenStageSlots
AFSKGEN_SLOTS = 4                          # kAfskgenMaxMessages
AFSKGEN_RAMP = 64
HDLC_TILE = 2048                           # kHdlcTile
HDLC_ROUND = 256                           # kHdlcThreads: the flags one round of step 4 closes
HDLC_MAX_FLAGS = HDLC_TILE // 7 + 2        # kHdlcMaxFlags
HDLC_MAX_BITS = 1 << 20
SHARED = [1, 1, 1, 1, 1, 1, 0]             # a flag that shares its first zero with the bit in front of it
ALL = 0xFFFFFFFF
MANY = 1300


# ------------------------------------------------------------------ the three restatements
def afskgen_runs(dirty):
    """[(first id, count, what)] of afskgen_stage over dirty = {slot * C + c: 1 (the slot) | 2 (the slot and its levels)}:
    the ids sorted; a run ends at 256 entries, at a gap, or where `what` changes"""
    ids = sorted(dirty)
    runs, i = [], 0
    while i < len(ids):
        what, j = dirty[ids[i]], i + 1
        while j < len(ids) and j - i < AFSKGEN_STAGE_SLOTS and ids[j] == ids[j - 1] + 1 and dirty[ids[j]] == what:
            j += 1
        runs.append((ids[i], j - i, what))
        i = j
    return runs


def hdlc_flags_per_tile(bits):
    """the flag-class bits of a call's row in each of its tiles of 2048, from a zero state: a zero behind exactly six ones,
    the run saturating at 7"""
    counts = [0] * (-(-len(bits) // HDLC_TILE))
    ones = 0
    for j, byte in enumerate(np.asarray(bits, dtype=np.uint8).tolist()):
        if byte & 1:
            ones = min(7, ones + 1)
        else:
            if ones == 6:
                counts[j // HDLC_TILE] += 1
            ones = 0
    return counts


def afsk_window(W):
    """(par, lead, J) of k_afsk: the parity of a lane's window start, the dwords from there to the lane's own, the tap pairs"""
    par = (W - 1) & 1
    return par, (W - 1 + par) // 2, W // 2 + 1


def afsk_window_setting(W):
    """(loop_shift, nrzi) of the GPU file's window test: both values of each meet both parities of W"""
    i = W - 2
    return (1, 8)[(i >> 1) & 1], bool((i >> 2) & 1)


def touching_kinds(runs):
    """the pairs of neighbouring runs (the second starts where the first ends) that need different things"""
    return [(a, b) for a, b in zip(runs, runs[1:]) if a[0] + a[1] == b[0] and a[2] != b[2]]


class AfskgenDirty:
    """the host side of hrfd_afskgen.hip as far as it decides the dirty entries of a launch: a message takes the lowest slot
    no message of its channel holds (afskgen_insert) and dirties it with its levels; a cut dirties the slot of every message
    the channel holds; a message that has ended at the clock dirties its slot when the next setter or launch drops it.
    Queues hold (start, end, slot).  No refusals: it takes the calls the GPU file makes, which the numpy model has accepted"""

    def __init__(self, C):
        self.C, self.N = C, 0
        self.q = [[] for _ in range(C)]
        self.dirty = {}

    def _selected(self, channel):
        return range(self.C) if channel == ALL else [channel]

    def _touch(self, c, slot, what):
        i = slot * self.C + c
        self.dirty[i] = max(self.dirty.get(i, 0), what)

    def _drop_ended(self):
        for c in range(self.C):
            for _, end, slot in self.q[c]:
                if end <= self.N:
                    self._touch(c, slot, 1)
            self.q[c] = [m for m in self.q[c] if m[1] > self.N]

    def queue(self, channel, n_bits, baud_step, start=gm.APPEND, gap=0):
        L = gm.length(n_bits, baud_step)
        laid = []
        for c in self._selected(channel):
            left = [m for m in self.q[c] if m[1] > self.N]
            at = (left[-1][1] if left else self.N) if start == gm.APPEND else start
            laid.append(at + gap)
        self._drop_ended()
        for c, s in zip(self._selected(channel), laid):
            used = {m[2] for m in self.q[c]}
            slot = min(set(range(AFSKGEN_SLOTS + 1)) - used)
            assert slot < AFSKGEN_SLOTS
            self.q[c] = sorted(self.q[c] + [(s, s + L, slot)])
            self._touch(c, slot, 2)

    def cut(self, channel=ALL):
        self._drop_ended()
        for c in self._selected(channel):
            for _, _, slot in self.q[c]:
                self._touch(c, slot, 1)
            self.q[c] = [(s, min(e, self.N + AFSKGEN_RAMP), slot) for s, e, slot in self.q[c] if s <= self.N]

    def launch(self, n_blocks):
        """the entries afskgen_stage finds at this call, which then are clean; the clock moves on"""
        self._drop_ended()
        dirty, self.dirty = self.dirty, {}
        self.N += 512 * n_blocks
        return dirty

    def pending(self, c):
        left = [m for m in self.q[c] if m[1] > self.N]
        return len(left), (left[-1][1] if left else self.N)


# ------------------------------------------------------------------ section G1: what is set in front of each of its four calls
G1_BLOCKS = 2
G1_BAUD_STEP = gm.step(1200)               # api.AfskGen.queue's default baud, which every message of G1 keeps
G1_ODD_TONES = (0x5A5A5A5B, 0x13579BDF, G1_BAUD_STEP)
# name: (bits, seed of the bits, what queue takes besides); all at 1200 baud, so `first` is 401 samples and `second` 1847
G1_MESSAGES = {"first": (60, 1, dict(amplitude=20000)), "second": (277, 2, dict(amplitude=12000, nrzi=False)),
               "third": (300, 3, dict(amplitude=32767, steps=G1_ODD_TONES)), "fourth": (150, 4, dict(amplitude=9000))}


def g1_ops(i):
    """[("queue", channel, message, start, gap) | ("cut", channel)] in front of call i.  `first` sounds at [100, 501) and has
    ended when call 1 is set up, `second` at [551, 2398): on the odd channels the cut ends it at 1088, and `third` follows it
    there on the slot `first` held; on the even channels `third` waits for `second` on a slot of its own"""
    if i == 0:
        return [("queue", ALL, "first", 100, 0), ("queue", ALL, "second", gm.APPEND, 50)]
    if i == 1:
        return [("cut", c) for c in range(1, MANY, 2)] + [("queue", c, "third", gm.APPEND, 10) for c in range(0, MANY, 3)]
    if i == 2:
        return [("queue", c, "fourth", gm.APPEND, 100 + c % 7) for c in (255, 256, 257, 1299)]
    return [("cut", ALL)]


def g1_apply(handles, shadow, i):
    """g1_ops(i) on every handle of `handles` (api.AfskGen's calls) and on the AfskgenDirty `shadow`"""
    for op in g1_ops(i):
        if op[0] == "cut":
            for h in handles:
                h.cut(op[1])
            shadow.cut(op[1])
        else:
            _, channel, name, start, gap = op
            n_bits, seed, kw = G1_MESSAGES[name]
            bits = np.random.default_rng(seed).integers(0, 2, size=n_bits, dtype=np.uint8)
            for h in handles:
                h.queue(channel, bits, start=start, gap=gap, **kw)
            assert kw.get("steps", G1_ODD_TONES)[2] == G1_BAUD_STEP
            shadow.queue(channel, n_bits, G1_BAUD_STEP, start, gap)


def g1_dirty():
    """the dirty entries of the four calls, by the shadow alone"""
    def make():
        shadow, out = AfskgenDirty(MANY), []
        for i in range(4):
            g1_apply((), shadow, i)
            out.append(shadow.launch(G1_BLOCKS))
        return out
    return once("g1", make)


# ------------------------------------------------------------------ the streams of section H, each made once
_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


H1_A, H1_B, H1_OPEN = b"round1", b"rounds", b"carried in"


def bits_of(parts):
    x = np.array(parts, dtype=np.uint8)
    x.setflags(write=False)
    return x


def h1_row(broken=False):
    """a frame, 262 flags that share their zeros, a second frame: 265 flags in 1987 bits, all in tile 0.  broken: the first
    frame's check sequence is wrong"""
    fcs = hm.crc16_x25(H1_A) ^ 0x0100 if broken else None
    return once(("h1", broken), lambda: bits_of(hm.FLAG + hm.frame_bits(H1_A, fcs) + hm.FLAG + SHARED * 262 + hm.frame_bits(H1_B) + hm.FLAG))


def h1_open():
    """the call in front of h1_row that leaves a whole frame open: the row's first flag closes it"""
    return once("h1 open", lambda: bits_of(hm.FLAG + hm.frame_bits(H1_OPEN)))


H2_FRAME = b"behind seven hundred flags"


def h2_row(s):
    return once(("h2", s), lambda: bits_of([0] * s + [0] + SHARED * 700 + hm.frame_bits(H2_FRAME) + hm.FLAG))


H3_P = 24


def h3_rows(C, n, seed=7):
    """C streams of n bits out of hm.mixed_stream (frames of up to 26 bytes, noise, runs of ones, flipped bits), built as
    the HDLC bank's own suite builds its streams"""
    def make():
        rng = np.random.default_rng(seed)
        rows = []
        for _ in range(C):
            parts, have = [], 0
            while have < n:
                parts.append(hm.mixed_stream(rng, 12, P=H3_P))
                have += len(parts[-1])
            rows.append(np.concatenate(parts)[:n])
        x = np.stack(rows)
        x.setflags(write=False)
        return x
    return once(("h3", C, n, seed), make)


def h3_frames(C, n):
    """the model's frames over h3_rows(C, n) in one call, per channel"""
    return once(("h3 frames", C, n), lambda: hm.HdlcModel(C, 1, H3_P).process(list(h3_rows(C, n)))[0])


H5_BITS = 2049                             # a tile and a bit
H5_RESET = (0, 1023, 1024, 1025, 1299)


def h5_payload(c):
    return b"across the cut %4d" % c


def h5_rows():
    """1300 rows of 2 x 2049 bits out of 40 streams, each at an offset of its own.  On the channels that are reset between
    the two calls a good frame lies across the cut, about 100 of its bits in front of it: carried, it closes as a record in
    the second call; behind a reset nothing is open when its closing flag comes"""
    def make():
        pool = h3_rows(40, 9000)
        rows = [pool[c % 40, 53 * (c // 40):][:2 * H5_BITS] for c in range(MANY)]
        for c in H5_RESET:
            frame = bits_of(hm.FLAG + hm.frame_bits(h5_payload(c)) + hm.FLAG) | hm.CARRIER
            at = H5_BITS - 100 - c % 7
            row = rows[c].copy()
            row[at:at + len(frame)] = frame
            row.setflags(write=False)
            rows[c] = row
        return rows
    return once("h5", make)


def h5_counts():
    """d_n_bits of the second call: 0, 1, 2048, 2049 and above max_bits = 2049; the reset channels take their whole rows"""
    counts = np.random.default_rng(5).choice(np.array([0, 1, 2048, 2049, 2050, 0xFFFFFFFF], dtype=np.uint32), size=MANY)
    counts[list(H5_RESET)] = H5_BITS
    return counts


def h5_second_call(reset):
    """the second call's frames on the channels of H5_RESET, by the model: behind a reset of them, or without it"""
    def make():
        rows = [h5_rows()[c] for c in H5_RESET]
        m = hm.HdlcModel(len(rows), 1, H3_P)
        m.process([r[:H5_BITS] for r in rows])
        if reset:
            m.reset()
        return m.process([r[H5_BITS:] for r in rows])[0]
    return once(("h5 second", reset), make)


H4_P = 1021
H4_CAP = 8 * (H4_P + 2) + 7
H4_CUTS = range(-20, 5)                    # around the bit in front of the long frame's closing zero


def h4_row(n_bytes):
    """(the row, the index of the long frame's closing zero)"""
    def make():
        long = np.random.default_rng(n_bytes).integers(0, 256, size=n_bytes, dtype=np.uint8).tobytes()
        head = hm.FLAG + hm.frame_bits(long) + hm.FLAG
        return bits_of(head + hm.frame_bits(b"next") + hm.FLAG), len(head) - 1, long
    return once(("h4", n_bytes), make)


def payloads(frames):
    return [p for _, p, _ in frames]


def model_frames(row, P=512):
    return hm.HdlcModel(1, 1, P).process([row])


# ------------------------------------------------------------------ afskgen_stage
def test_afskgen_runs_cut_at_256_at_gaps_and_where_the_need_changes():
    assert afskgen_runs({}) == []
    assert afskgen_runs({i: 2 for i in range(65)}) == [(0, 65, 2)]                             # the most the bank's own suite has
    assert afskgen_runs({i: 1 for i in range(256)}) == [(0, 256, 1)]
    assert afskgen_runs({i: 1 for i in range(257)}) == [(0, 256, 1), (256, 1, 1)]
    assert afskgen_runs({5: 1, 6: 1, 8: 1}) == [(5, 2, 1), (8, 1, 1)]                          # a gap
    assert afskgen_runs({5: 1, 6: 2, 7: 2, 8: 1}) == [(5, 1, 1), (6, 2, 2), (8, 1, 1)]        # the need changes
    assert touching_kinds(afskgen_runs({5: 1, 6: 2, 7: 2, 9: 1})) == [((5, 1, 1), (6, 2, 2))]
    # every id is in exactly one run, with what it needs
    rng = np.random.default_rng(1)
    dirty = {int(i): int(rng.integers(1, 3)) for i in rng.choice(5200, size=3000, replace=False)}
    covered = {i: what for first, count, what in afskgen_runs(dirty) for i in range(first, first + count)}
    assert covered == dirty and max(count for _, count, _ in afskgen_runs(dirty)) <= AFSKGEN_STAGE_SLOTS


def test_afskgen_two_messages_on_1300_channels_go_up_in_eleven_uploads():
    """section G1's first call: the ids are slot * 1300 + c, so slots 0 and 1 of every channel are 0..2599 without a gap"""
    dirty = g1_dirty()[0]
    assert dirty == {i: 2 for i in range(2 * MANY)}
    runs = afskgen_runs(dirty)
    assert runs == [(256 * k, 256, 2) for k in range(10)] + [(2560, 40, 2)]
    assert [r for r in runs if r[0] < MANY < r[0] + r[1]] == [(1280, 256, 2)]                  # one run crosses from slot 0 to slot 1


def test_afskgen_later_calls_of_g1_break_runs_where_the_need_changes():
    _, second, third, fourth = g1_dirty()
    # call 1: `first` has ended on every channel (its slot is emptied: 1), and `third` takes that slot on every channel
    # divisible by 3 (2); the cut `second` on slot 1 of the odd channels (1)
    want = {c: 2 if c % 3 == 0 else 1 for c in range(MANY)}
    want.update({MANY + c: 1 for c in range(1, MANY, 2)})
    assert second == want
    runs = afskgen_runs(second)
    assert runs[:4] == [(0, 1, 2), (1, 2, 1), (3, 1, 2), (4, 2, 1)] and len(touching_kinds(runs)) == 2 * len(range(0, MANY, 3)) - 2
    assert (MANY - 1) % 3 == 0 and (MANY - 1, 1, 2) in runs                                    # slot 0 of the last channel, with levels
    # a run that took its need from its last entry would leave `third` without its levels: 256..511 ends on a 1
    assert second[511] == 1 and {second[c] for c in range(256, 512)} == {1, 2}
    # call 2: the cut `second` has ended; `fourth` on the lowest free slot of its four channels
    want = {MANY + c: 1 for c in range(1, MANY, 2)}
    want.update({MANY + 255: 2, 256: 2, 257: 2, MANY + 1299: 2})
    assert third == want and (256, 2, 2) in afskgen_runs(third)
    # call 3: cut(ALL) touches whatever is held, levels stay: `second` has ended on the even channels as well
    assert set(fourth.values()) == {1} and {MANY + c for c in range(0, MANY, 2)} <= set(fourth)
    assert (MANY + 254, 3, 1) in afskgen_runs(fourth)                                          # 254 and 256 ended, 255 held `fourth`


def test_afskgen_dirty_takes_the_lowest_free_slot_and_a_cut_touches_what_is_held():
    t = AfskgenDirty(3)
    t.queue(ALL, 60, gm.step(1200), start=100)                 # [100, 501) on slot 0
    t.queue(1, 600, gm.step(1200))                             # [501, 4502) on slot 1 of channel 1
    assert t.pending(1) == (2, 4502) and t.launch(2) == {0: 2, 1: 2, 2: 2, 4: 2}
    t.cut(1)                                                   # drops the ended first message everywhere, shortens the second
    assert t.dirty == {0: 1, 1: 1, 2: 1, 4: 1} and t.pending(1) == (1, 1024 + 64) and t.pending(0) == (0, 1024)
    t.queue(1, 8, gm.step(1200))                               # slot 0 is free again
    assert t.dirty == {0: 1, 1: 2, 2: 1, 4: 1} and t.pending(1) == (2, 1088 + 54)


# ------------------------------------------------------------------ k_hdlc's flags
def test_hdlc_flags_are_zeros_behind_exactly_six_ones():
    assert hdlc_flags_per_tile([]) == [] and hdlc_flags_per_tile(hm.FLAG) == [1]
    assert hdlc_flags_per_tile([1] * 6 + [0]) == [1] and hdlc_flags_per_tile([1] * 7 + [0]) == [0] and hdlc_flags_per_tile([1] * 5 + [0]) == [0]
    assert hdlc_flags_per_tile([0] + SHARED * 3) == [3]
    assert hdlc_flags_per_tile([0] * 2047 + hm.FLAG) == [0, 1]                                 # the flag is where its last bit lies
    assert hdlc_flags_per_tile(np.array(hm.FLAG, dtype=np.uint8) | 0xFE) == [1]               # only bit 0 counts
    assert HDLC_MAX_FLAGS == 294 and -(-HDLC_TILE // 7) == 293


def test_h1_holds_more_flags_than_one_round_closes():
    row = h1_row()
    assert len(row) == 1987 and hdlc_flags_per_tile(row) == [265] and 265 > HDLC_ROUND
    frames, n_frames, n_bad, _, _ = model_frames(row)
    assert payloads(frames[0]) == [H1_A, H1_B] and n_bad[0] == 0
    assert frames[0][0][0] < 7 * HDLC_ROUND and frames[0][1][0] == len(row) - 1                # the second closes as flag 264
    assert len(H1_A) == len(H1_B)                              # equal records: a row that holds one holds either
    broken = h1_row(broken=True)
    assert len(broken) <= HDLC_TILE and hdlc_flags_per_tile(broken) == [265]
    frames, _, n_bad, _, _ = model_frames(broken)
    assert payloads(frames[0]) == [H1_B] and n_bad[0] == 1
    m = hm.HdlcModel(1)
    assert m.process([h1_open()])[0] == [[]] and m.ch[0].in_frame and len(m.ch[0].bits) == 8 * (len(H1_OPEN) + 2)
    assert payloads(m.process([row])[0][0]) == [H1_OPEN, H1_A, H1_B]


def test_h2_fills_tiles_with_293_flags():
    most = {s: max(hdlc_flags_per_tile(h2_row(s))) for s in range(7)}
    assert {s for s, v in most.items() if v == 293} == {0, 4, 5, 6} and set(most.values()) == {292, 293}
    for s in range(7):
        per_tile = hdlc_flags_per_tile(h2_row(s))
        assert len(h2_row(s)) > 2 * HDLC_TILE and sum(per_tile) == 701 and min(per_tile[:2]) >= 291 and max(per_tile) < HDLC_MAX_FLAGS
        assert payloads(model_frames(h2_row(s))[0][0]) == [H2_FRAME]


def test_h3_rows_of_70000_bits_close_frames_above_16_bits():
    """(the row of 2^20 bits is the same recipe; the GPU file asserts its reach from the model next to its call)"""
    assert h3_rows(2, 70000).shape == (2, 70000) and 70000 > 34 * HDLC_TILE
    for frames in h3_frames(2, 70000):
        assert frames[-1][0] > 65535 and sum(1 for e, _, _ in frames if e > 65535) > 5 and frames[0][0] < 65536


def test_h5_resets_change_what_the_second_call_gives():
    """every one of the five reset channels carries a good frame across the cut: without the reset (or with one the
    kernel does not see) the second call has a record more, its first"""
    rows = h5_rows()
    assert len(rows) == MANY and all(len(r) == 2 * H5_BITS for r in rows) and h5_counts()[list(H5_RESET)].tolist() == [H5_BITS] * 5
    carried, fresh = h5_second_call(reset=False), h5_second_call(reset=True)
    for i, c in enumerate(H5_RESET):
        assert payloads(carried[i])[0] == h5_payload(c) and carried[i][0][0] < 120
        assert h5_payload(c) not in payloads(fresh[i]) and carried[i][1:] == fresh[i]
    assert {1023, 1024, 1025} <= set(H5_RESET)                 # both sides of 1024


def test_h4_carries_a_frame_of_exactly_cap_bits():
    row, z, long = h4_row(H4_P)
    assert row[z] == 0 and row[z - 6:z].all() and H4_CAP == 8191
    assert payloads(model_frames(row, H4_P)[0][0]) == [long, b"next"]
    m = hm.HdlcModel(1, 1, H4_P)
    m.process([row[:z]])                                       # the cut one bit in front of the closing zero
    assert m.ch[0].in_frame and len(m.ch[0].bits) == H4_CAP
    over, z1, _ = h4_row(H4_P + 1)
    assert payloads(model_frames(over, H4_P)[0][0]) == [b"next"]
    m = hm.HdlcModel(1, 1, H4_P)
    alive = [m.process([over[j:j + 1]]) and m.ch[0].in_frame for j in range(z1)]
    died = alive.index(False, 8)                               # the one byte too many: cap bits are in, and the next kept bit kills it
    assert z1 + min(H4_CUTS) <= died < z1 and len(m.ch[0].bits) == H4_CAP and not any(alive[died:])
    assert min(H4_CUTS) == -20 and max(H4_CUTS) == 4 and z + min(H4_CUTS) > 0 and z1 + max(H4_CUTS) < len(over)


# ------------------------------------------------------------------ k_afsk's windows
def test_afsk_windows_give_both_parities_every_lead_and_every_pair_count():
    got = {W: afsk_window(W) for W in range(2, 33)}
    assert got[2] == (1, 1, 2) and got[7] == (0, 3, 4) and got[8] == (1, 4, 5) and got[32] == (1, 16, 17)
    assert {p for p, _, _ in got.values()} == {0, 1}
    leads = [lead for _, lead, _ in got.values()]
    pairs = [J for _, _, J in got.values()]
    assert sorted(set(leads)) == list(range(1, 17)) and sorted(set(pairs)) == list(range(2, 18))
    assert [v for v in range(1, 17) if leads.count(v) < 2] == [16] and [v for v in range(2, 18) if pairs.count(v) < 2] == [17]
    # the device has run five of them; the others have tap packings and window starts of their own
    assert len(set(got.values()) - {got[W] for W in (2, 7, 8, 27, 32)}) == 26


def test_afsk_window_settings_meet_both_parities():
    met = {(afsk_window(W)[0],) + afsk_window_setting(W) for W in range(2, 33)}
    assert met == {(p, A, nrzi) for p in (0, 1) for A in (1, 8) for nrzi in (False, True)}
