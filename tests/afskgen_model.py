"""numpy model of the AFSK generator bank (hrfd_afskgen_*, include/hrfd.h at "AFSK generator bank"): written from the
contract's text, with Python integers for every stream time and the phase as a cumulative sum of the per-sample steps from
the message's first sample.  It takes the calls of api.AfskGen (a refusal raises ValueError).  The GPU tests compare the
library with it bit for bit; tests/test_afskgen_model.py compares it with the library's slow loop, with the tone generator's
model and with the AFSK bank's model in a closed loop."""
from __future__ import annotations

import numpy as np

from hackrfdiags_amd import api
from tests.ddc_model import COS

BLOCK = 512
MAX_MESSAGES = 4
MAX_BITS = 8192
MAX_BLOCKS = 1024
MAX_AMP = 32767
MAX_STEP = 1 << 31
RAMP = 64
APPEND = (1 << 64) - 1
MAX_TIME = 1 << 63
MASK32 = (1 << 32) - 1
ALL = 0xFFFFFFFF
ODD_STEP = 0x01234567                       # a baud step whose bit edges fall on every residue


def step(hz):
    return int(round(float(hz) / 8000 * 2.0 ** 32))


def levels(bits, nrzi):
    """l[i] of the contract: uint8 of 0 / 1"""
    d = np.asarray(bits).astype(np.int64).ravel() & 1
    if not nrzi:
        return d.astype(np.uint8)
    return ((1 + np.cumsum(1 - d)) & 1).astype(np.uint8)      # every 0 turns the level over, from mark


def pack_levels(lv):
    """bit i & 31 of word i >> 5 = l[i]"""
    pad = np.zeros((-len(lv)) % 32, dtype=np.uint8)
    return np.packbits(np.concatenate([lv, pad]), bitorder="little").view(np.uint32)


def length(n_bits, baud_step):
    """L = ceil(n_bits 2^32 / baud_step); ValueError from 2^31 on"""
    L = -((-(n_bits << 32)) // baud_step)
    if L >= 1 << 31:
        raise ValueError(f"{n_bits} bits at baud_step {baud_step} are {L} samples (below 2^31)")
    return L


class Message:
    """one queued message: it sounds at stream times start <= n < end; end lies in front of start + L behind a cut"""

    def __init__(self, start, end, mark_step, space_step, baud_step, amp, lv):
        self.start, self.end, self.mark_step, self.space_step, self.baud_step, self.amp, self.lv = \
            start, end, mark_step, space_step, baud_step, amp, lv

    def span(self, lo, hi):
        """g int64 of the stream times max(lo, start) .. min(hi, end) - 1 and the first of them; None where there is none"""
        a, b = max(lo, self.start), min(hi, self.end)
        if a >= b:
            return None, a
        k = np.arange(b - self.start, dtype=np.int64)        # from the message's first sample: theta is a running sum
        bit = (k * self.baud_step) >> 32                     # k < 2^31 and the step <= 2^31: below 2^62
        st = np.where(self.lv[bit] != 0, self.mark_step, self.space_step).astype(np.int64)
        theta = (np.cumsum(st) - st) & MASK32                # exclusive: theta(0) = 0; the sum stays below 2^62
        k, theta = k[a - self.start:], theta[a - self.start:]
        i = ((theta + (1 << 19)) >> 20) & 4095
        s = COS[(i - 1024) & 4095].astype(np.int64)
        v = (self.amp * s + (1 << 14)) >> 15
        e = np.minimum(np.minimum(k + 1, (self.end - self.start) - k), RAMP)      # E - n = (E - S) - k, below 2^31
        return (v * e + 32) >> 6, a


class AfskGenModel:
    def __init__(self, n_channels: int):
        self.C = int(n_channels)
        self.reset()

    n = property(lambda self: self.C)

    def _selected(self, channel):
        if channel == ALL:
            return range(self.C)
        if not 0 <= channel < self.C:
            raise ValueError(f"channel {channel}")
        return [channel]

    def _lay_out(self, q, gap, L, start):
        left = [m for m in q if m.end > self.N]
        if start == APPEND:
            at = left[-1].end if left else self.N
        else:
            if start < self.N:
                raise ValueError(f"start {start} lies before the stream time {self.N}")
            at = start
        s, e = at + gap, at + gap + L
        if at >= MAX_TIME or s >= MAX_TIME or e >= MAX_TIME:
            raise ValueError("the message would lie at or above stream time 2^63")
        for m in left:
            if m.start < e and s < m.end:
                raise ValueError(f"the messages at {min(m.start, s)} and {max(m.start, s)} would overlap")
        if len(left) >= MAX_MESSAGES:
            raise ValueError(f"{len(left) + 1} messages that have not ended on the channel (at most {MAX_MESSAGES})")
        return s, e

    def queue(self, channel, bits, mark_hz=1200, space_hz=2200, baud=1200, amplitude=8000, nrzi=True, start=APPEND, gap=0, steps=None):
        d = np.asarray(bits).ravel()
        m, s, r = (int(v) for v in steps) if steps is not None else (step(mark_hz), step(space_hz), step(baud))
        if not 1 <= d.size <= MAX_BITS:
            raise ValueError(f"n_bits must be 1..{MAX_BITS}")
        for name, v in (("mark_step", m), ("space_step", s), ("baud_step", r)):
            if not 1 <= v <= MAX_STEP:
                raise ValueError(f"{name} must be 1..2^31")
        if not 0 <= amplitude <= MAX_AMP:
            raise ValueError(f"amp above {MAX_AMP}")
        L = length(d.size, r)
        if start != APPEND and start >= MAX_TIME:
            raise ValueError(f"stream time {start} (below 2^63)")
        chans = self._selected(channel)
        laid = [self._lay_out(self.q[c], int(gap), L, start) for c in chans]       # refused whole
        lv = levels(d, nrzi)
        for c, (a, e) in zip(chans, laid):
            self.q[c] = sorted([x for x in self.q[c] if x.end > self.N] + [Message(a, e, m, s, r, int(amplitude), lv)], key=lambda x: x.start)

    def send(self, channel, payloads, **modem):
        self.queue(channel, api.hdlc_encode(payloads), **modem)

    def cut(self, channel=ALL):
        for c in self._selected(channel):
            q = [m for m in self.q[c] if m.start <= self.N < m.end]
            for m in q:
                m.end = min(m.end, self.N + RAMP)
            self.q[c] = q

    def reset(self):
        self.N = 0
        self.q = [[] for _ in range(self.C)]
        self._clips = [0] * self.C

    def set_time(self, N):
        if not 0 <= N < MAX_TIME:
            raise ValueError(f"stream time {N} (below 2^63)")
        if any(m.end > self.N for q in self.q for m in q):
            raise ValueError("a channel holds a message that has not ended")
        self.N = int(N)

    def time(self):
        return self.N

    def pending(self, channel):
        left = [m for m in self.q[channel] if m.end > self.N]
        return len(left), (left[-1].end if left else self.N)

    def clips(self, channel):
        return self._clips[channel]

    def process(self, pcm, n_blocks=None, want_active=False):
        """pcm int16 [C, n_blocks x 512] (any shape with C rows) or None with n_blocks -> out int16 [C, n_blocks, 512], or
        (out, active uint8 [C, n_blocks]) with want_active"""
        C = self.C
        x = np.zeros((C, BLOCK * int(n_blocks)), dtype=np.int64) if pcm is None else np.asarray(pcm).reshape(C, -1).astype(np.int64)
        n = x.shape[1]
        n_blocks = n // BLOCK
        assert n == n_blocks * BLOCK and 1 <= n_blocks <= MAX_BLOCKS and self.N + n <= MAX_TIME
        lo, hi = self.N, self.N + n
        active = np.zeros((C, n_blocks), dtype=np.uint8)
        y = x.copy()
        for c in range(C):
            q = self.q[c] = [m for m in self.q[c] if m.end > lo]       # what has ended leaves the queue
            for m in q:
                g, a = m.span(lo, hi)
                if g is None:
                    continue
                y[c, a - lo:a - lo + g.size] += g
                active[c, (a - lo) // BLOCK:(a - lo + g.size - 1) // BLOCK + 1] = 1
        out = np.clip(y, -32768, 32767)
        for c in range(C):
            self._clips[c] += int((out[c] != y[c]).sum())
        self.N = hi
        out = out.astype(np.int16).reshape(C, n_blocks, BLOCK)
        return (out, active) if want_active else out


# ---- the signals of the closed loops: tests/afsk_model.py's cases with this bank in place of afsk_signal
LOOP_LEVELS = ((300, 0.0), (8000, 0.0), (32767, 0.0), (8000, 500.0))      # (amplitude, sigma)
LOOP_SEEDS = tuple(range(1, 21))


def loop_case(modem, amplitude, sigma, seed, bank=None):
    """(payloads, pcm int16 [n_blocks, 512]): two frames of 40 random bytes on the modem's tones through `bank` (one channel;
    AfskGenModel unless given: api.AfskGen takes the same calls), 0..299 samples of silence in front, 100 behind, Gaussian
    noise of sigma over everything"""
    from tests import afsk_model as am
    rng = np.random.default_rng(seed)
    payloads = am.random_payloads(rng, 2)
    silence = int(rng.integers(0, 300))
    g = AfskGenModel(1) if bank is None else bank
    g.send(0, payloads, mark_hz=modem["mark_hz"], space_hz=modem["space_hz"], baud=modem["baud"], amplitude=amplitude, start=g.time() + silence)
    n_blocks = -(-(g.pending(0)[1] - g.time() + 100) // BLOCK)
    pcm = g.process(None, n_blocks).reshape(-1).astype(np.int64)
    if sigma:
        pcm = pcm + np.rint(rng.normal(0.0, sigma, size=pcm.size)).astype(np.int64)
    return payloads, np.clip(pcm, -32768, 32767).astype(np.int16).reshape(n_blocks, BLOCK)
