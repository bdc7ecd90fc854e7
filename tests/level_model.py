"""numpy model of the level bank (hrfd_level_*, include/hrfd.h): int64 arithmetic, the contract rule by rule, every frame of a
call at once.  The model carries what the handle carries: the release weights, every channel's target, floor and bypass, and
the last 64 peaks of every channel.  The GPU tests compare the library with it bit for bit; tests/test_level_model.py compares
it with slow_channel, a sample-by-sample restatement in Python integers."""
from __future__ import annotations

import numpy as np

BLOCK = 512
FRAME = 64
FRAMES_PER_BLOCK = BLOCK // FRAME
ALL = 0xFFFFFFFF
MAX_WEIGHTS = 64
HIST = 64
MAX_BLOCKS = 1024
UNITY = 32768
DEFAULT_TARGET = 8192
DEFAULT_FLOOR = 64
MAX_GAIN = (32767 << 12) // 16                 # 8388352


def default_weights() -> np.ndarray:
    k = np.arange(MAX_WEIGHTS, dtype=np.int64)
    return np.where(k < 8, UNITY, (UNITY * (MAX_WEIGHTS - k)) // 56)


def masked(pcm, n_pcm=None) -> np.ndarray:
    """x int64 [C, n_blocks, 512]: the samples, zero where the position in its block is >= min(n_pcm, 512)"""
    x = np.asarray(pcm).astype(np.int64)
    x = x.reshape(1, -1, BLOCK) if x.ndim == 1 else x.reshape(x.shape[0], -1, BLOCK)
    if n_pcm is not None:
        lim = np.minimum(np.asarray(n_pcm, dtype=np.int64).reshape(x.shape[0], x.shape[1]), BLOCK)
        x = np.where(np.arange(BLOCK)[None, None, :] < lim[:, :, None], x, 0)
    return x


def slow_channel(x, hist, w, target: int, floor: int):
    """one channel in Python integers: x the call's (masked) samples, whole frames; hist its last 64 peaks, the newest last
    -> (y, g, p, the next hist).  Asserts the bounds the contract states on the way."""
    x, p_all, w = [int(v) for v in x], [int(v) for v in hist], [int(v) for v in w]
    assert len(p_all) == HIST and len(x) % FRAME == 0 and w[0] == UNITY

    def gain(i):                                            # of the frame whose peak is p_all[i]
        E = max([floor] + [(p_all[i - k] * w[k] + (1 << 14)) >> 15 for k in range(len(w))])
        assert E >= p_all[i]
        g = (target << 12) // E
        assert g <= MAX_GAIN and g * E <= target << 12
        return g

    y, gains, peaks = [], [], []
    g_prev = gain(HIST - 1)
    for f in range(len(x) // FRAME):
        frame = x[FRAME * f:FRAME * (f + 1)]
        p_all.append(max(abs(v) for v in frame))
        g = gain(len(p_all) - 1)
        for n, v in enumerate(frame):
            gs = g if g <= g_prev else g_prev + (((g - g_prev) * (n + 1)) >> 6)
            assert g_prev <= gs <= g or gs == g
            assert abs(v * gs) <= target << 12 < 1 << 27
            y.append((v * gs + (1 << 11)) >> 12)
            assert abs(y[-1]) <= target
        gains.append(g)
        peaks.append(p_all[-1])
        g_prev = g
    return y, gains, peaks, p_all[-HIST:]


class LevelModel:
    def __init__(self, n_channels: int):
        self.C = int(n_channels)
        assert 1 <= self.C <= 65536
        self.w = default_weights()
        self.target = np.full(self.C, DEFAULT_TARGET, dtype=np.int64)
        self.floor = np.full(self.C, DEFAULT_FLOOR, dtype=np.int64)
        self.bypass = np.zeros(self.C, dtype=bool)
        self.hist = np.zeros((self.C, HIST), dtype=np.int64)    # the last 64 peaks, the newest last
        self.max_product = 0                                    # the largest |x gs| of the last call

    def set_weights(self, w):
        w = np.asarray(w, dtype=np.int64).ravel().copy()
        assert 1 <= w.size <= MAX_WEIGHTS and w[0] == UNITY and w.min() >= 0 and w.max() <= UNITY
        self.w = w

    def set(self, target: int, floor: int, channel: int = ALL):
        assert 0 <= target <= 32767 and 16 <= floor <= 32768
        sel = slice(None) if channel == ALL else channel
        self.target[sel] = target
        self.floor[sel] = floor

    def set_bypass(self, on: bool, channel: int = ALL):
        self.bypass[slice(None) if channel == ALL else channel] = bool(on)

    def reset(self, channel: int = ALL):
        self.hist[slice(None) if channel == ALL else channel] = 0

    def envelope(self, pcm, n_pcm=None):
        """(p, E, g) int64 [C, 8 n_blocks] of a call, the state left as it was: what a test picks its frames by"""
        x = masked(np.asarray(pcm).reshape(self.C, -1), n_pcm)
        p, E, g = self._frames(x)
        return p, E[:, 1:], g[:, 1:]

    def _frames(self, x):
        """p [C, F]; E, g [C, F + 1]: those of the frame in front of the call first"""
        C, F = self.C, x.shape[1] * FRAMES_PER_BLOCK
        p = np.abs(x).reshape(C, F, FRAME).max(axis=2)
        P = np.concatenate([self.hist, p], axis=1)              # frame f sits at 64 + f
        E = np.broadcast_to(self.floor[:, None], (C, F + 1)).copy()
        for k in range(self.w.size):                            # frames -1 .. F-1 sit at 63 .. 63 + F
            E = np.maximum(E, (P[:, HIST - 1 - k:HIST + F - k] * self.w[k] + (1 << 14)) >> 15)
        return p, E, (self.target[:, None] << 12) // E

    def process(self, pcm, n_pcm=None):
        """pcm [C, n_blocks, 512], n_pcm [C, n_blocks] or None -> (out int16 [C, n_blocks, 512], gain uint32 [C, 8 n_blocks],
        peak uint16 [C, 8 n_blocks])"""
        x = masked(np.asarray(pcm).reshape(self.C, -1), n_pcm)
        C, B = x.shape[0], x.shape[1]
        assert C == self.C and 1 <= B <= MAX_BLOCKS
        F = B * FRAMES_PER_BLOCK
        p, E, g = self._frames(x)
        assert (E[:, 1:] >= p).all() and g.max() <= MAX_GAIN
        g_prev, g_now = g[:, :-1, None], g[:, 1:, None]
        ramp = g_prev + (((g_now - g_prev) * (np.arange(FRAME, dtype=np.int64) + 1)[None, None, :]) >> 6)
        gs = np.where(g_now <= g_prev, g_now, ramp)
        xf = x.reshape(C, F, FRAME)
        prod = xf * gs
        self.max_product = int(np.abs(prod).max())
        assert (np.abs(prod) <= (self.target[:, None, None] << 12)).all()
        y = (prod + (1 << 11)) >> 12
        assert (np.abs(y) <= self.target[:, None, None]).all()
        y = np.where(self.bypass[:, None, None], xf, y)
        self.hist = np.concatenate([self.hist, p], axis=1)[:, -HIST:]
        return y.reshape(C, B, BLOCK).astype(np.int16), g[:, 1:].astype(np.uint32), p.astype(np.uint16)
