"""Walks over the commutator positions of the any-length receive chain (k_rx_ragged): builders of call
sequences and their inputs.  Plain Python / numpy: no GPU, no ctypes.  tests/test_ragged_walks_model.py holds the CPU
oracle to the compiled reference on them, tests/test_gpu_ragged_sweep.py the device to the oracle.

A walk is a list of calls (block_bytes, n_blocks, events); the events are applied in front of the call:
    ("mode", m)  ("gain", m, g)  ("reset", m)  ("threshold", t)   the setters of the handle (inner API: ("reset",))
    ("reduce",)          the call goes through reduce_sample_rate: the front end alone (n_blocks == 1)
    ("loud", bits)       bits[channel][block]: the block carries a signal above the squelch threshold (else all do)
Every builder keeps the books of where each block starts, in Walk.blocks, from the count formulas of 3.2b alone:
    held' = (held + n) % 8      256 kS/s samples of a block = (held + n) // 8      per stage floor((phase + cnt) / M)
with the reference's gate on top (Squelch.cc:227-273, SignalTracker.cc:104-146: a block passes when it or its
predecessor carried a signal).  Nothing here is measured on the code under test."""
from collections import namedtuple

import numpy as np

from hackrfdiags_amd import synth

NONE, AM, FM, WBFM, LSB, USB = range(6)
MODES = (AM, FM, WBFM, LSB, USB)
FULL_BYTES = synth.BLOCK_BYTES

SWEEP_CLASSES = (9, 15, 31, 33, 127, 129, 255, 257, 1001, 6001)      # IQ samples per block
SWEEP_CHUNKS = (1, 100, 1, 1, 153)                                   # blocks per call: 256 blocks of a class
GATED_LENGTHS = (9, 33, 129, 257, 1001, 2049)
GATED_CHANNELS = 8
GATED_THRESHOLD = -30
GATED_TURN = 1001
GATED_SEED = 7                                                       # + mode: every mode a walk of its own
INNER_CLASSES = (1, 2, 3, 5, 7, 9, 31, 33, 65, 701, 16383)           # 256 kS/s samples per call
INNER_MAX_SAMPLES = 16384

# One record per block and channel.  position: phase_sweep: IQ samples so far mod 256; inner_sweep: samples since the last
# reset mod 32; held: the front end's position (0..7); dpos: 256 kS/s samples the ACTIVE demodulator has taken, mod 32 (its
# three commutators: dpos % 4, dpos // 4 % 4, dpos // 16); n256: 256 kS/s samples the block completes; n_pcm: PCM samples it
# yields; cls: index of the block's length class, -1 for the extra calls
Block = namedtuple("Block", "call block channel samples position held dpos n256 allowed n_pcm cls mode")

_KIND = {AM: 0, FM: 1, WBFM: 2, LSB: 3, USB: 3}
_STAGES = (4, 4, 2)                                                  # every demodulator: 256 -> 64 -> 16 -> 8 kS/s


def pcm_capacity(block_bytes):
    return (block_bytes + 511) // 512


def iq256_capacity(block_bytes):
    return 2 * ((block_bytes // 2 + 7) // 8)


def demod_pcm_capacity(nbytes):
    return (nbytes + 63) // 64


class Walk(list):
    def __init__(self, n_channels=1):
        super().__init__()
        self.n_channels = n_channels
        self.blocks = []

    def total_bytes(self):
        return sum(bb * nb for bb, nb, _ in self)


class _Chain:
    """the positions of one channel's chain"""

    def __init__(self):
        self.held = 0
        self.total = 0
        self.mode = NONE
        self.tracking = False
        self.phase = [[0, 0, 0] for _ in range(4)]

    def dpos(self):
        if self.mode == NONE:
            return 0
        p = self.phase[_KIND[self.mode]]
        return p[0] + 4 * p[1] + 16 * p[2]

    def reset(self, mode):
        self.phase[_KIND[mode]] = [0, 0, 0]

    def front(self, n):
        n256 = (self.held + n) // 8
        self.held = (self.held + n) % 8
        self.total += n
        return n256

    def demod(self, cnt):
        p = self.phase[_KIND[self.mode]]
        for s, m in enumerate(_STAGES):
            p[s], cnt = (p[s] + cnt) % m, (p[s] + cnt) // m
        return cnt

    def block(self, n, loud):
        """one block of acceptIqData -> (n256, allowed, n_pcm)"""
        n256 = self.front(n)
        present = bool(loud) and n256 > 0                  # a call that completes no sample has magnitude 0
        allowed = present or self.tracking
        self.tracking = present
        n_pcm = self.demod(n256) if (allowed and self.mode != NONE) else 0
        return n256, allowed, n_pcm


def _add(walk, chains, samples, n_blocks=1, events=(), cls=-1, loud=None):
    """append one call and its bookkeeping; chains: one _Chain per channel"""
    reduce = any(e[0] == "reduce" for e in events)
    for e in events:
        for ch in chains:
            if e[0] == "mode":
                ch.mode = e[1]
            elif e[0] == "reset":
                ch.reset(e[1])
    if loud is not None:
        events = tuple(events) + (("loud", tuple(tuple(int(v) for v in row) for row in loud)),)
    call = len(walk)
    walk.append((2 * samples, n_blocks, tuple(events)))
    for c, ch in enumerate(chains):
        for b in range(n_blocks):
            pos, held, dpos = ch.total % 256, ch.held, ch.dpos()
            if reduce:
                n256, allowed, n_pcm = ch.front(samples), False, 0
            else:
                n256, allowed, n_pcm = ch.block(samples, True if loud is None else loud[c][b])
            walk.blocks.append(Block(call, b, c, samples, pos, held, dpos, n256, allowed, n_pcm, cls, ch.mode))


def phase_sweep(mode):
    """A plain stream (one bookkeeping for all channels: none is gated) that starts every length class from every one of
    the 256 positions: 256 consecutive blocks of an odd class visit them all.  Calls of 100 and 153 blocks (the kernel's
    block loop) with single-block calls between them (the round trip through RagState).  Then a call that completes no
    sample, full blocks from positions 255 and 1, and even classes that keep the front end's position where it is."""
    w = Walk()
    ch = [_Chain()]
    first = (("mode", mode),)
    for k, n in enumerate(SWEEP_CLASSES):
        for nb in SWEEP_CHUNKS:
            _add(w, ch, n, nb, first, cls=k)
            first = ()
    assert ch[0].total % 256 == 0 and ch[0].held == 0
    _add(w, ch, 3)                                         # 6 bytes: no 256 kS/s sample, no PCM, magnitude 0
    _add(w, ch, 252)
    assert ch[0].total % 256 == 255
    _add(w, ch, FULL_BYTES // 2)                           # 7 pending + 131072: 16384 samples, 512 PCM -- every array full
    _add(w, ch, 2)
    assert ch[0].total % 256 == 1
    _add(w, ch, FULL_BYTES // 2)
    _add(w, ch, 256, 3)                                    # on the 512-byte grid by length, at position 1
    _add(w, ch, 1000, 32)                                  # held stays 1, the demodulator walks its 32 positions
    _add(w, ch, 256, 1)
    return w


def gated_walk(mode, seed, n_calls=260):
    """GATED_CHANNELS channels, each with its own loud / quiet pattern under GATED_THRESHOLD: the front end's position is
    shared, every channel's demodulator stands somewhere else.  On the way: a gain change, a mode excursion and back, a
    reset of the active demodulator, a reset of an inactive one followed by a passage in that mode, a call that completes
    no sample, and reduce_sample_rate calls of uneven length (front end only)."""
    rng = np.random.default_rng(seed)
    other = FM if mode == WBFM else WBFM
    C = GATED_CHANNELS
    w = Walk(C)
    chains = [_Chain() for _ in range(C)]
    # A channel changes between loud and quiet only at a block of GATED_TURN samples or more: the front end's pipeline
    # carries 14 samples of the block before into the first outputs of a block, and only a long block's mean magnitude
    # is its own.  Channel 0 turns rarely ... channel 7 at nearly every chance.
    p_turn = [0.2 + 0.1 * c for c in range(C)]
    state = rng.random(C) < 0.5
    script = {0: (("mode", mode), ("threshold", GATED_THRESHOLD)),
              30: (("gain", mode, 1234.5),),
              60: (("mode", other),), 85: (("mode", mode),),
              110: (("reset", mode),),
              150: (("reset", other),), 153: (("mode", other),), 175: (("mode", mode),),
              210: (("reset", mode), ("gain", mode, 321.0))}
    for i in range(n_calls):
        events = script.get(i, ())
        n = int(GATED_LENGTHS[rng.integers(0, len(GATED_LENGTHS))])
        nb = int((1, 1, 2, 3)[rng.integers(0, 4)])
        turn = rng.random(C) < np.array(p_turn)
        if i % 13 == 7:
            _add(w, chains, int(rng.integers(9, 700)), 1, events + (("reduce",),), loud=state[:, None])
        elif i == 100:
            if chains[0].held > 4:                         # make room for three samples that complete nothing
                _add(w, chains, 8 - chains[0].held, 1, loud=state[:, None])
            _add(w, chains, 3, 1, events, loud=state[:, None])
            assert w.blocks[-1].n256 == 0
        else:
            if n >= GATED_TURN:
                state = state ^ turn
            _add(w, chains, n, nb, events, loud=np.repeat(state[:, None], nb, axis=1))
    return w


def inner_sweep(mode):
    """The inner API (X::acceptIqData on the 256 kS/s stream): every class from every one of the 32 positions, two resets
    at non-zero positions (a reset clears the commutators), and at the end 16384 samples from position 15: 512 PCM
    samples, the row's capacity."""
    w = Walk()
    ch = [_Chain()]
    ch[0].mode = mode

    def call(n, events=(), cls=-1):
        c = ch[0]
        if events:
            c.reset(mode)
            c.total = 0
        pos = c.total % 32
        assert pos == c.dpos()
        c.total += n
        w.append((2 * n, 1, tuple(events)))
        w.blocks.append(Block(len(w) - 1, 0, 0, n, pos, 0, pos, n, True, c.demod(n), cls, mode))

    for k, n in enumerate(INNER_CLASSES):
        if n % 2 == 0:
            for _ in range(16):
                call(n, cls=k)
            call(1)                                        # an odd call: the even class reaches the odd positions too
            for _ in range(16):
                call(n, cls=k)
            assert ch[0].total % 32 != 0
            call(7, (("reset",),))                         # reset at a non-zero position
            call(25)
        else:
            for _ in range(32):
                call(n, cls=k)
    call(5)
    call(9, (("reset",),))
    call(6)
    assert ch[0].total % 32 == 15
    call(INNER_MAX_SAMPLES)
    return w


# ---------------------------------------------------------------- inputs
def _stream(kind, seed, nbytes):
    blocks = (nbytes + FULL_BYTES - 1) // FULL_BYTES
    if kind == "fullscale":
        # stretches of full-scale DC of either sign and of full-scale noise (bytes 127 / -128), 3000 bytes each
        noise = np.where(synth.make_input("lcg", seed, blocks) < 0, -128, 127).astype(np.int8)
        parts = (synth.make_input("dc_pos", 0, blocks), synth.make_input("dc_neg", 0, blocks), noise)
        which = (np.arange(blocks * FULL_BYTES) // 3000) % 3
        return np.choose(which, parts).astype(np.int8)[:nbytes]
    return synth.make_input(kind, seed, blocks)[:nbytes]


def sweep_inputs(walk, seed, kinds=("fmtone", "lcg", "fullscale")):
    """int8 [len(kinds), walk.total_bytes()]"""
    n = walk.total_bytes()
    return np.stack([_stream(k, seed + i, n) for i, k in enumerate(kinds)])


def gated_inputs(walk, seed):
    """int8 [channels, total bytes]: an FM signal far above the threshold in the loud blocks, noise of a bit or two in
    the quiet ones (the tail block the tracker lets through is not silence)"""
    n = walk.total_bytes()
    rows = []
    for c in range(walk.n_channels):
        loud = _stream("fmtone", seed + c, n)
        row = _stream("lcg", seed + 100 + c, n) // 64
        off = 0
        for bb, nb, events in walk:
            bits = next((e[1] for e in events if e[0] == "loud"), None)
            for b in range(nb):
                if bits is None or bits[c][b]:
                    row[off:off + bb] = loud[off:off + bb]
                off += bb
        rows.append(row)
    return np.stack(rows)


def inner_inputs(walk, seed, channels=3):
    n = walk.total_bytes()
    return np.stack([_stream(("fmtone", "lcg", "fullscale")[c % 3], seed + c, n) for c in range(channels)])


# ---------------------------------------------------------------- a checker (the oracle or the compiled reference) over a walk
def fs4_mix(dec):
    """upconvertByFsOver4 (IqDataProcessor.cc:771-815) over one call's decimatedData: the rotation by the index within
    the call, int8 negation wrapping"""
    d = np.array(dec, dtype=np.int8).reshape(-1, 2)
    out = d.copy()
    neg = (0 - d.astype(np.int16)).astype(np.int8)
    out[1::4, 0], out[1::4, 1] = neg[1::4, 1], d[1::4, 0]
    out[2::4, 0], out[2::4, 1] = neg[2::4, 0], neg[2::4, 1]
    out[3::4, 0], out[3::4, 1] = d[3::4, 1], neg[3::4, 0]
    return out.reshape(-1)


class ChainOfParts:
    """The outer API put together from a checker's own parts: its IqDataProcessor kept in mode NONE as the front end
    (the 256 kS/s stream, the magnitude) and its four demodulator objects of the inner API behind it, which can be reset
    one by one -- the compiled reference has no entry that resets a demodulator behind its IqDataProcessor.  The gate
    is not computed here: `gates` yields, block by block, whether the demodulator runs (the oracle's `allowed`)."""

    def __init__(self, checker, gates):
        self.front = checker.rx()
        self.front.set_mode(NONE)
        self.demods = {AM: checker.demod(AM), FM: checker.demod(FM), WBFM: checker.demod(WBFM), LSB: checker.demod(LSB)}
        self.demods[USB] = self.demods[LSB]                # one SsbDemodulator, like Radio.cc:179-197
        self.gates = iter(gates)
        self.mode = NONE

    def set_mode(self, mode):
        self.mode = mode
        if mode in (LSB, USB):
            self.demods[LSB].set_sideband(mode == LSB)

    def set_gain(self, mode, gain):
        self.demods[mode].set_gain(gain)

    def set_threshold(self, threshold):
        pass

    def reset_demod(self, mode):
        self.demods[mode].reset()

    def reduce_sample_rate(self, x):
        return self.front.reduce_sample_rate(x)

    def process(self, x):
        _, mag, _, dump = self.front.process(x)
        allowed = next(self.gates)
        pcm = self.demods[self.mode].process(dump) if (allowed and self.mode != NONE) else np.zeros(0, np.int16)
        return pcm, mag, allowed, dump


def replay_outer(h, walk, row, channel, mixes=True, resets=True):
    """one channel of a walk through an object with the outer API of tests/reflib.py, one block per call like the
    reference -> per block (pcm, magnitude, allowed, iq256 bytes); a reduce_sample_rate call gives (None, None, None,
    bytes).  mixes: reduce_sample_rate of `h` returns the stream behind the Fs/4 mix (the oracle; the reference's
    decimatedData is in front of it).  resets=False: the walk without its reset events"""
    out = []
    off = 0
    for bb, nb, events in walk:
        reduce = False
        for e in events:
            if e[0] == "mode":
                h.set_mode(e[1])
            elif e[0] == "gain":
                h.set_gain(e[1], e[2])
            elif e[0] == "reset" and resets:
                h.reset_demod(e[1])
            elif e[0] == "threshold":
                h.set_threshold(e[1])
            elif e[0] == "reduce":
                reduce = True
        for b in range(nb):
            x = row[off:off + bb]
            off += bb
            if reduce:
                n, dec = h.reduce_sample_rate(x)
                out.append((None, None, None, dec if mixes else fs4_mix(dec)))
            else:
                out.append(h.process(x))
    return out


def replay_inner(d, walk, row):
    out = []
    off = 0
    for nbytes, _, events in walk:
        if events:
            d.reset()
        out.append(d.process(row[off:off + nbytes]))
        off += nbytes
    return out
