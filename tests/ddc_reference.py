"""A second restatement of the DDC bank's contract (include/hrfd.h, "DDC bank"), written from the header's text and
decomposed differently from tests/ddc_model.py, so that the two can check each other:

  - every capture is kept as one whole stream from N = 0 (zeros before it); nothing is carried per call;
  - a call recomputes theta(n) for every sample of the stream with the tuning current at that call (samples before
    N_ref included), mixes the whole stream, runs stage A as a full convolution (np.convolve, int64) followed by sat16
    and the decimation at m R + R - 1, stage B as a full convolution, then the gain step, and slices out the call's
    outputs;
  - a reset starts new streams.

Recomputing everything per call is quadratic in the stream's length: this is for short CPU tests."""
from __future__ import annotations

import numpy as np

MASK32 = (1 << 32) - 1
# COS[i] = round(32767 cos(2 pi i / 4096))
COS = np.array([int(round(32767.0 * np.cos(2.0 * np.pi * i / 4096.0))) for i in range(4096)], dtype=np.int64)


def sat(x, lo, hi):
    return np.minimum(np.maximum(x, lo), hi)


def mixer(i: np.ndarray, q: np.ndarray, theta: np.ndarray):
    """k = ((theta + 2^19) >> 20) & 4095, c = COS[k], s = COS[(k - 1024) & 4095];
    yI = (I c + Q s + 128) >> 8, yQ = (Q c - I s + 128) >> 8"""
    k = ((theta + (1 << 19)) >> 20) & 4095
    c, s = COS[k], COS[(k - 1024) & 4095]
    return (i * c + q * s + 128) >> 8, (q * c - i * s + 128) >> 8


def fir_full(h: np.ndarray, x: np.ndarray) -> np.ndarray:
    """sat16((sum_k h[k] x[n - k] + 2^14) >> 15) for every n of x, x zero before its start"""
    acc = np.convolve(x.astype(np.int64), h.astype(np.int64))[:x.size]
    return sat((acc + (1 << 14)) >> 15, -32768, 32767)


class DdcReference:
    def __init__(self, n_captures: int, n_channels: int, decimation: int, taps_a, taps_b):
        self.W, self.C, self.R = n_captures, n_channels, decimation
        self.hA = np.asarray(taps_a, dtype=np.int64)
        self.hB = np.asarray(taps_b, dtype=np.int64)
        self.rec = [dict(capture=0, step=0, theta_ref=0, n_ref=0, g=0) for _ in range(n_channels)]
        self.reset()

    def reset(self):
        self.streams = [np.zeros((0, 2), dtype=np.int64) for _ in range(self.W)]
        self.N = 0
        for r in self.rec:
            r["theta_ref"], r["n_ref"] = 0, 0

    def theta(self, c: int, n):
        r = self.rec[c]
        return (r["theta_ref"] + (n - r["n_ref"]) * r["step"]) & MASK32

    def set_tuning(self, c: int, capture: int, step: int):
        r = self.rec[c]
        r["theta_ref"], r["n_ref"] = self.theta(c, self.N), self.N
        r["capture"], r["step"] = capture, step & MASK32

    def set_gain_shift(self, c: int, g: int):
        self.rec[c]["g"] = g

    def set_filter(self, stage: int, taps):
        if stage == 0:
            self.hA = np.asarray(taps, dtype=np.int64)
        else:
            self.hB = np.asarray(taps, dtype=np.int64)

    def process(self, captures: np.ndarray, out_bytes: int) -> np.ndarray:
        R, M = self.R, out_bytes // 2
        cap = np.asarray(captures, dtype=np.int8).reshape(self.W, R * M, 2).astype(np.int64)
        self.streams = [np.concatenate([s, cap[w]]) for w, s in enumerate(self.streams)]
        m0 = self.N // R
        self.N += R * M
        n = np.arange(self.N, dtype=np.int64)
        out = np.empty((self.C, M, 2), dtype=np.int64)
        for c, r in enumerate(self.rec):
            x = self.streams[r["capture"]]
            y = mixer(x[:, 0], x[:, 1], self.theta(c, n))
            g = r["g"]
            rnd = (1 << (6 - g)) if g < 7 else 0
            for rail in range(2):
                a = fir_full(self.hA, y[rail]) if self.hA.size else y[rail]
                a = a[R - 1::R]
                b = fir_full(self.hB, a) if self.hB.size else a
                out[c, :, rail] = sat((b[m0:] + rnd) >> (7 - g), -128, 127)
        return out.reshape(self.C, 2 * M).astype(np.int8)


def float_ddc(x: np.ndarray, theta: np.ndarray, h_a, h_b, decimation: int, g: int) -> np.ndarray:
    """The same operation in float64 over one whole stream (int IQ [n, 2] from N = 0, theta uint32 [n]): the exact
    rotation by e^{-j 2 pi theta / 2^32} at the table's amplitude 32767 / 256, taps / 32768, no intermediate rounding
    or saturation; returns the complex outputs in int8 units, before the final rounding, for every output of the
    stream"""
    z = (x[:, 0] + 1j * x[:, 1]) * np.exp(-2j * np.pi * theta.astype(np.float64) / 2.0 ** 32) * (32767.0 / 256.0)
    h_a = np.asarray(h_a, dtype=np.float64) / 32768.0
    h_b = np.asarray(h_b, dtype=np.float64) / 32768.0
    a = np.convolve(z, h_a)[:z.size] if h_a.size else z
    a = a[decimation - 1::decimation]
    b = np.convolve(a, h_b)[:a.size] if h_b.size else a
    return b / 2.0 ** (7 - g)
