"""numpy model of the DCS bank (hrfd_dcs_*, include/hrfd.h): int64 arithmetic, the contract rule by rule, every sample of a
call at once.  The model carries what the handle carries: the taps, the code list with its groups and thresholds, and per
channel the last 512 inputs and the last 1312 slicer bits.  The GPU tests compare the library with it bit for bit;
tests/test_dcs_model.py compares it with the library's own slow loop (hrfd_dcs_debug_slow).  The signal sources of both
suites are here too."""
from __future__ import annotations

import numpy as np

BLOCK = 512
ALL = 0xFFFFFFFF
MAX_TAPS = 512
MAX_CODES = 128
MAX_BLOCKS = 1024
GROUPS = 4
NO_BEST = 255
WORD_BITS = 23
MASK = (1 << WORD_BITS) - 1
GENERATOR = 0xC75
DELAY = [(1250 * k) // 21 for k in range(WORD_BITS)]        # D[k]: 0 .. 1309
BIT_HIST = 1312                                             # slicer bits kept: whole dwords over D[22] = 1309
STATE_DW = 300
DEFAULT_MIN_HITS = 128


def polymod(v: int) -> int:
    """the remainder of v(x) modulo g, bit i = x^i"""
    while v.bit_length() >= GENERATOR.bit_length():
        v ^= GENERATOR << (v.bit_length() - GENERATOR.bit_length())
    return v


def word(code: int, inverted: bool = False) -> int:
    data = 0x800 | int(code)
    w = polymod(data << 11) << 12 | data
    return w ^ MASK if inverted else w


def rot23(w: int, r: int) -> int:
    return ((w >> r) | (w << (WORD_BITS - r))) & MASK


def canonical(w: int) -> int:
    return min(rot23(int(w), r) for r in range(WORD_BITS))


def masked(pcm, n_pcm=None) -> np.ndarray:
    """x int64 [C, n_blocks, 512]: the samples, zero where the position in its block is >= min(n_pcm, 512)"""
    x = np.asarray(pcm).astype(np.int64)
    x = x.reshape(1, -1, BLOCK) if x.ndim == 1 else x.reshape(x.shape[0], -1, BLOCK)
    if n_pcm is not None:
        lim = np.minimum(np.asarray(n_pcm, dtype=np.int64).reshape(x.shape[0], x.shape[1]), BLOCK)
        x = np.where(np.arange(BLOCK)[None, None, :] < lim[:, :, None], x, 0)
    return x


# ---- the signal sources
def levels(code: int, n: int, amplitude: int, t0: int = 0, inverted: bool = False, ppm: float = 0.0) -> np.ndarray:
    """the NRZ row of a code from stream time t0 on, int64: bit floor(21 t / 1250) mod 23 of the word, bit 0 first; ppm: a
    transmitter clock that fast (0 is api.dcs_levels)"""
    w = word(code, inverted)
    t = np.arange(t0, t0 + n, dtype=np.int64)
    if ppm:
        k = np.floor(t * (21.0 / 1250.0) * (1.0 + ppm * 1e-6)).astype(np.int64)
    else:
        k = t * 21 // 1250
    return np.where((w >> (k % WORD_BITS)) & 1, amplitude, -amplitude).astype(np.int64)


def white(rng, n: int, rms: float) -> np.ndarray:
    return np.round(rng.normal(0.0, rms, size=n)).astype(np.int64)


def to_pcm(x) -> np.ndarray:
    return np.clip(np.asarray(x), -32768, 32767).astype(np.int16)


class DcsModel:
    def __init__(self, n_channels: int):
        self.C = int(n_channels)
        assert 1 <= self.C <= 65536
        self.taps = np.array([16384], dtype=np.int64)
        self.canon = np.zeros(0, dtype=np.int64)            # in list order
        self.group = np.zeros(0, dtype=np.int64)
        self.min_hits = np.full(GROUPS, DEFAULT_MIN_HITS, dtype=np.int64)
        self.reset()

    def reset(self, channel: int = ALL):
        if channel == ALL:
            self.x_hist = np.zeros((self.C, BLOCK), dtype=np.int64)       # the newest last
            self.s_hist = np.zeros((self.C, BIT_HIST), dtype=np.int64)
        else:
            self.x_hist[channel] = 0
            self.s_hist[channel] = 0

    def set_taps(self, taps):
        h = np.asarray(taps, dtype=np.int64).ravel().copy()
        assert 1 <= h.size <= MAX_TAPS and np.abs(h).sum() <= 65535 and np.abs(h).max() <= 32768
        self.taps = h
        self.reset()

    def set_codes(self, codes, inverted=None, groups=None):
        codes = [int(c) for c in np.asarray(codes).ravel()]
        K = len(codes)
        inv = [False] * K if inverted is None else [bool(v) for v in np.asarray(inverted).ravel()]
        grp = [0] * K if groups is None else [int(v) for v in np.asarray(groups).ravel()]
        assert K <= MAX_CODES and len(inv) == K and len(grp) == K and all(0 <= c <= 0o777 for c in codes) and all(0 <= g < GROUPS for g in grp)
        canon = [canonical(word(c, i)) for c, i in zip(codes, inv)]
        assert len(set(canon)) == K, "two entries are aliases"
        self.canon = np.array(canon, dtype=np.int64)
        self.group = np.array(grp, dtype=np.int64)

    def set_min_hits(self, group: int = ALL, n: int = DEFAULT_MIN_HITS):
        assert 1 <= n <= BLOCK
        self.min_hits[slice(None) if group == ALL else group] = n

    def state(self) -> np.ndarray:
        """uint32 [C, 300]: every channel's state as the library lays it out"""
        st = np.zeros((self.C, STATE_DW), dtype=np.uint32)
        x = (self.x_hist & 0xFFFF).astype(np.uint32)
        st[:, :BLOCK // 2] = x[:, 0::2] | (x[:, 1::2] << 16)
        s = self.s_hist.astype(np.uint32).reshape(self.C, BIT_HIST // 32, 32)
        st[:, BLOCK // 2:BLOCK // 2 + BIT_HIST // 32] = (s << np.arange(32, dtype=np.uint32)[None, None, :]).sum(axis=2, dtype=np.uint64).astype(np.uint32)
        return st

    def canonical_words(self, pcm, n_pcm=None):
        """c int64 [C, n] of a call and the slicer bits s [C, n], the state left as it was"""
        return self._words(masked(np.asarray(pcm).reshape(self.C, -1), n_pcm).reshape(self.C, -1))[:2]

    def _words(self, x):
        C, n = x.shape
        X = np.concatenate([self.x_hist, x], axis=1)
        acc = np.stack([np.convolve(X[c], self.taps)[BLOCK:BLOCK + n] for c in range(C)])
        assert np.abs(acc).max(initial=0) < 1 << 31
        s = (acc > 0).astype(np.int64)
        S = np.concatenate([self.s_hist, s], axis=1)
        w = np.zeros((C, n), dtype=np.int64)
        for k, d in enumerate(DELAY):
            w |= S[:, BIT_HIST - d:BIT_HIST - d + n] << (WORD_BITS - 1 - k)
        c = w.copy()
        for r in range(1, WORD_BITS):
            c = np.minimum(c, ((w >> r) | (w << (WORD_BITS - r))) & MASK)
        return c, s, X, S

    def process(self, pcm, n_pcm=None):
        """pcm [C, n_blocks, 512], n_pcm [C, n_blocks] or None -> (hits uint16 [C, n_blocks, K], best uint8 [C, n_blocks, 4],
        present uint8 [C, n_blocks, 4])"""
        x = masked(np.asarray(pcm).reshape(self.C, -1), n_pcm)
        C, B = x.shape[0], x.shape[1]
        assert C == self.C and 1 <= B <= MAX_BLOCKS
        c, s, X, S = self._words(x.reshape(C, -1))
        K = self.canon.size
        hits = np.zeros((C, B, K), dtype=np.int64)
        if K:
            order = np.argsort(self.canon)
            at = np.minimum(np.searchsorted(self.canon[order], c), K - 1)
            hit = self.canon[order][at] == c
            cell = (np.arange(C * B).reshape(C, B, 1) * K + order[at].reshape(C, B, BLOCK))[hit.reshape(C, B, BLOCK)]
            hits = np.bincount(cell, minlength=C * B * K).reshape(C, B, K)
        best = np.full((C, B, GROUPS), NO_BEST, dtype=np.int64)
        present = np.zeros((C, B, GROUPS), dtype=np.int64)
        for g in range(GROUPS):
            mine = np.flatnonzero(self.group == g)
            if mine.size:
                pick = hits[:, :, mine].argmax(axis=2)      # the first of the largest: the lowest index
                best[:, :, g] = mine[pick]
                present[:, :, g] = np.take_along_axis(hits[:, :, mine], pick[:, :, None], axis=2)[:, :, 0] >= self.min_hits[g]
        self.x_hist = X[:, -BLOCK:]
        self.s_hist = S[:, -BIT_HIST:]
        return hits.astype(np.uint16), best.astype(np.uint8), present.astype(np.uint8)


# ---- the closed loop: a DCS code under a 1 kHz tone on each of two WBFM stations, through the modulator, the DUC, the DDC,
# the receive chain and the DCS bank (tests/test_dcs_model.py on the models and the CPU oracle, tests/test_gpu_dcs.py on the
# device).  tests/tone_model.py's loop with another audio
LOOP_CODES = ((0o754, False), (0o023, True))                # station 0 sends D754N, station 1 D023I
LOOP_BLOCKS = 16
LOOP_DCS_AMP, LOOP_TONE_HZ, LOOP_TONE_AMP = 2000, 1000.0, 5000.0


def loop_audio():
    """[2][8192] int16: each station's code as NRZ levels under the tone"""
    n = LOOP_BLOCKS * BLOCK
    tone = LOOP_TONE_AMP * np.sin(2 * np.pi * LOOP_TONE_HZ * np.arange(n) / 8000.0)
    return [np.round(levels(code, n, LOOP_DCS_AMP, 0, inv) + tone).astype(np.int16) for code, inv in LOOP_CODES]


def loop_model():
    """both codes listed, low-pass taps of 255: channel c must find entry c (DcsModel and api.Dcs take the same calls)"""
    from hackrfdiags_amd import api
    m = DcsModel(2)
    m.set_taps(api.dcs_lowpass_taps())
    m.set_codes([c for c, _ in LOOP_CODES], [i for _, i in LOOP_CODES])
    return m


def loop_check(hits, best, present):
    """The receive chain passes 134.4 bit/s NRZ (the CPU oracle showed 503 to 508 hits of 512 from block 3 on, and none of
    the other station's code): from block 4 on, where a word's 1820 samples of reach lie wholly inside the stream whatever
    the chain's delay, every block has its station's code present as the best of its group."""
    for c in range(2):
        assert present[c, 4:, 0].all() and (best[c, 4:, 0] == c).all(), (c, hits[c].tolist())
