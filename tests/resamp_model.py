"""numpy model of the resampler bank (hrfd_resamp_*, include/hrfd.h): int64 arithmetic, the contract line by line, vectorised
per branch.  The model carries what the handle carries: the taps, the last K - 1 values of x of every channel and the phase d.
The GPU tests compare the library with it bit for bit; tests/test_resamp_model.py compares it with slow_channel, an
output-by-output restatement in Python integers."""
from __future__ import annotations

from math import gcd

import numpy as np

BLOCK = 512
ALL = 0xFFFFFFFF
MAX_RATIO = 512
MAX_TAPS = 16384
MAX_BRANCH = 512
MAX_IN = 524288


def out_count(n_in: int, L: int, M: int, d: int) -> int:
    return 0 if n_in * L <= d else -((d - n_in * L) // M)


def masked(pcm, n_pcm=None) -> np.ndarray:
    """x int64 [C, n_in]: the samples, zero where the position in a block of 512 is >= min(n_pcm, 512)"""
    x = np.asarray(pcm).astype(np.int64)
    x = x.reshape(1, -1) if x.ndim == 1 else x.reshape(x.shape[0], -1)
    if n_pcm is not None:
        C, n = x.shape
        assert n % BLOCK == 0
        lim = np.minimum(np.asarray(n_pcm, dtype=np.int64).reshape(C, n // BLOCK), BLOCK)
        x = np.where(np.arange(BLOCK)[None, None, :] < lim[:, :, None], x.reshape(C, -1, BLOCK), 0).reshape(C, n)
    return x


def slow_channel(x, hist, taps, L: int, M: int, d: int):
    """one channel in Python integers: x the call's (masked) samples, hist the samples before them (any length, the newest
    last; zeros in front of it) -> (y, the next d)"""
    x, hist, h = [int(v) for v in x], [int(v) for v in hist], [int(v) for v in taps]
    T = len(h)
    K = -(-T // L)

    def at(s):
        if s >= 0:
            return x[s]
        return hist[len(hist) + s] if len(hist) + s >= 0 else 0

    y = []
    for j in range(out_count(len(x), L, M, d)):
        q = d + j * M
        i, p = divmod(q, L)
        acc = 0
        for k in range(K):
            if p + k * L < T:
                acc += h[p + k * L] * at(i - k)
                assert -(1 << 31) <= acc < (1 << 31) - (1 << 13)
        y.append(max(-32768, min(32767, (acc + (1 << 13)) >> 14)))
    return y, d + len(y) * M - len(x) * L


class ResampModel:
    def __init__(self, n_channels: int, up: int, down: int):
        self.C, self.L, self.M = int(n_channels), int(up), int(down)
        assert 1 <= self.C <= 65536 and 1 <= self.L <= MAX_RATIO and 1 <= self.M <= MAX_RATIO
        assert gcd(self.L, self.M) == 1 and self.M <= 8 * self.L
        self.taps = np.array([16384], dtype=np.int64) if self.L == 1 and self.M == 1 else None
        self.branch = None if self.taps is None else self.taps.reshape(1, 1)        # [L, K]: branch p, tap k = h[p + k L]
        self.K = 1
        self.hist = np.zeros((self.C, 0), dtype=np.int64)       # the last K - 1 values of x, the newest last
        self.d = 0

    def set_taps(self, taps):
        h = np.asarray(taps, dtype=np.int64).ravel().copy()
        K = -(-h.size // self.L)
        assert 1 <= h.size <= MAX_TAPS and K <= MAX_BRANCH
        padded = np.zeros(K * self.L, dtype=np.int64)
        padded[:h.size] = h
        assert np.abs(padded.reshape(K, self.L)).sum(axis=0).max() <= 65535
        self.taps, self.K = h, K
        self.branch = padded.reshape(K, self.L).T.copy()
        self.hist = np.zeros((self.C, K - 1), dtype=np.int64)
        self.d = 0

    def reset(self, channel: int = ALL):
        if channel == ALL:
            self.hist[:] = 0
            self.d = 0
        else:
            self.hist[channel] = 0

    def out_count(self, n_in: int) -> int:
        return out_count(int(n_in), self.L, self.M, self.d)

    def process(self, pcm, n_pcm=None) -> np.ndarray:
        """pcm [C, n_in], n_pcm [C, n_in / 512] or None -> out int16 [C, n_out]"""
        assert self.taps is not None, "no taps yet"
        x = masked(np.asarray(pcm).reshape(self.C, -1), n_pcm)
        n_in = x.shape[1]
        assert 1 <= n_in <= MAX_IN and n_in * self.L < (1 << 31)
        L, M, K = self.L, self.M, self.K
        n_out = self.out_count(n_in)
        xx = np.concatenate([self.hist, x], axis=1)             # sample s sits at K - 1 + s
        q = self.d + np.arange(n_out, dtype=np.int64) * M
        i, p = q // L, q % L
        acc = np.zeros((self.C, n_out), dtype=np.int64)
        k = np.arange(K, dtype=np.int64)
        for branch in np.unique(p):
            sel = np.flatnonzero(p == branch)
            for a in range(0, sel.size, 8192):                  # bounded gathers: [C, 8192, K]
                part = sel[a:a + 8192]
                win = xx[:, (K - 1 + i[part])[:, None] - k[None, :]]
                acc[:, part] = win @ self.branch[branch]
        assert np.abs(acc).max(initial=0) <= 65535 * 32768
        self.hist = xx[:, xx.shape[1] - (K - 1):] if K > 1 else self.hist
        self.d += n_out * M - n_in * L
        assert 0 <= self.d < M
        return np.clip((acc + (1 << 13)) >> 14, -32768, 32767).astype(np.int16)
