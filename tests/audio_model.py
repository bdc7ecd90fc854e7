"""numpy model of the audio bank (hrfd_audio_*, include/hrfd.h): int64 arithmetic, the contract line by line.  The model
carries what the handle carries: the taps, the last T - 1 values of x and the last gate of every channel, the wanted tones and
the bus lists.  The GPU tests compare the library with it bit for bit; tests/test_audio_model.py compares it with a
sample-by-sample restatement in Python integers."""
from __future__ import annotations

import numpy as np

BLOCK = 512
GROUPS = 4
ANY_TONE = 254
NO_TONE = 255
ALL = 0xFFFFFFFF
MASK32 = (1 << 32) - 1
UNITY = 32768
RAMP_STEP = 512


def sat16(v):
    return np.clip(v, -32768, 32767)


def envelope(p, q):
    """e int64 [..., 512] for gates p (the block before) and q (this block), arrays of 0 / 1 of one shape"""
    p = np.asarray(p, dtype=np.int64)[..., None]
    q = np.asarray(q, dtype=np.int64)[..., None]
    ramp = RAMP_STEP * (np.arange(BLOCK, dtype=np.int64) + 1)
    up, down = np.minimum(UNITY, ramp), np.maximum(0, UNITY - ramp)
    return np.where(p == q, UNITY * q, np.where(q == 1, up, down))


class AudioModel:
    def __init__(self, n_channels: int, n_buses: int = 1):
        self.C, self.M = int(n_channels), int(n_buses)
        self.taps = np.array([16384], dtype=np.int64)
        self.hist = np.zeros((self.C, 0), dtype=np.int64)       # the last T - 1 values of x, the newest last
        self.prev = np.zeros(self.C, dtype=np.int64)
        self.want = np.full(self.C, NO_TONE, dtype=np.int64)
        self.bus = [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)) for _ in range(self.M)]

    def set_taps(self, taps):
        self.taps = np.asarray(taps, dtype=np.int64).ravel().copy()
        assert 1 <= self.taps.size <= 512 and np.abs(self.taps).sum() <= 65535
        self.hist = np.zeros((self.C, self.taps.size - 1), dtype=np.int64)
        self.prev[:] = 0

    def set_bus(self, bus: int, channels=(), gains=()):
        ch, g = np.asarray(channels, dtype=np.int64).ravel(), np.asarray(gains, dtype=np.int64).ravel()
        assert ch.size == g.size <= 4096 and (ch < self.C).all() and (np.abs(g) <= 32767).all()
        self.bus[bus] = (ch.copy(), g.copy())

    def set_want(self, want: int, channel: int = ALL):
        if channel == ALL:
            self.want[:] = want
        else:
            self.want[channel] = want

    def reset(self, channel: int = ALL):
        if channel == ALL:
            self.hist[:] = 0
            self.prev[:] = 0
        else:
            self.hist[channel] = 0
            self.prev[channel] = 0

    def gate(self, best, present, frame_len: int, group: int) -> np.ndarray:
        """best, present [C, F, 4] -> open uint8 [C, n_blocks]"""
        L = int(frame_len)
        b = np.asarray(best).reshape(self.C, -1, GROUPS)[:, :, group].astype(np.int64)
        p = np.asarray(present).reshape(self.C, -1, GROUPS)[:, :, group] != 0
        want = self.want[:, None]
        match = p & ((want == ANY_TONE) | (b == want))          # [C, F]
        n_blocks = match.shape[1] * L // BLOCK
        if L <= BLOCK:
            hit = match.reshape(self.C, n_blocks, BLOCK // L).any(axis=2)
        else:
            hit = match[:, np.arange(n_blocks) * BLOCK // L]
        return (hit | (want == NO_TONE)).astype(np.uint8)

    def process(self, pcm, n_pcm=None, open=None):
        """pcm int16 [C, n_blocks x 512] (any shape with C rows), n_pcm and open [C, n_blocks] or None -> (out int16
        [C, n_blocks, 512], mix int16 [M, n_blocks, 512], clips uint32 [M])"""
        C, T = self.C, self.taps.size
        x = np.asarray(pcm).reshape(C, -1).astype(np.int64)
        n_blocks = x.shape[1] // BLOCK
        assert x.shape[1] == n_blocks * BLOCK and n_blocks >= 1
        # 1. input
        if n_pcm is not None:
            lim = np.minimum(np.asarray(n_pcm).reshape(C, n_blocks).astype(np.int64) & MASK32, BLOCK)
            taken = np.arange(BLOCK)[None, None, :] < lim[:, :, None]
            x = np.where(taken.reshape(C, -1), x, 0)
        # 2. voice filter: |acc| <= 65535 * 32768, exact in int64 as in int32
        xx = np.concatenate([self.hist, x], axis=1)
        N = x.shape[1]
        acc = np.zeros((C, N), dtype=np.int64)
        for k in range(T):
            acc += self.taps[k] * xx[:, T - 1 - k:T - 1 - k + N]
        assert np.abs(acc).max() < (1 << 31) - (1 << 14)
        y = sat16((acc + (1 << 13)) >> 14)
        self.hist = xx[:, N:].copy()
        # 3. gate
        q = np.ones((C, n_blocks), dtype=np.int64) if open is None else (np.asarray(open).reshape(C, n_blocks) != 0).astype(np.int64)
        p = np.concatenate([self.prev[:, None], q[:, :-1]], axis=1)
        self.prev = q[:, -1].copy()
        z = (y.reshape(C, n_blocks, BLOCK) * envelope(p, q) + (1 << 14)) >> 15
        # 5. buses
        mix = np.zeros((self.M, n_blocks, BLOCK), dtype=np.int64)
        clips = np.zeros(self.M, dtype=np.uint32)
        for m, (ch, g) in enumerate(self.bus):
            if ch.size == 0:
                continue
            s = np.zeros((n_blocks, BLOCK), dtype=np.int64)
            for lo in range(0, ch.size, 256):                   # bounded temporaries
                s += (g[lo:lo + 256, None, None] * z[ch[lo:lo + 256]]).sum(axis=0)
            r = (s + (1 << 11)) >> 12
            mix[m] = sat16(r)
            clips[m] = np.count_nonzero(mix[m] != r)
        return z.astype(np.int16), mix.astype(np.int16), clips
