"""Two statements of the DUC contract written apart from tests/duc_model.py, to hold the model itself:

(a) DucWhole: integer arithmetic over the WHOLE stream of every channel since create / reset, with the interpolation
    written as an explicit zero-stuffing and np.convolve, and each channel's phase as the running sum of the steps in
    force at every wideband sample (retunes change the step from their counter on).  A call recomputes everything
    from the first sample with the filters, amplitudes and shifts of that call and keeps its own last R M outputs.
(b) float_sums: the same chain in float64 with no rounding (the mixer at the table's own angles), and the bound on
    |S_int - S_float| that the rounding steps allow."""
from __future__ import annotations

import numpy as np

from tests.ddc_model import COS, MASK32

H = 318


def q15(acc):
    return np.clip((acc + (1 << 14)) >> 15, -32768, 32767)


class DucWhole:
    def __init__(self, W, C, R, hA, hB):
        self.W, self.C, self.R = W, C, R
        self.hA, self.hB = np.asarray(hA, dtype=np.int64), np.asarray(hB, dtype=np.int64)
        self.capture = np.zeros(C, dtype=np.int64)
        self.amp = np.full(C, 32768, dtype=np.int64)
        self.shift = np.full(W, 8, dtype=np.int64)
        self.cur_step = np.zeros(C, dtype=np.int64)
        self.reset()

    def reset(self):
        self.x = [np.zeros((0, 2), dtype=np.int64) for _ in range(self.C)]
        self.changes = [[(0, int(s))] for s in self.cur_step]   # (counter, step) per channel
        self.N = 0
        self.clips = np.zeros(self.W, dtype=np.int64)

    def set_tuning(self, c, w, step):
        self.capture[c] = w
        self.cur_step[c] = step & MASK32
        self.changes[c].append((self.N, int(step) & MASK32))

    def theta(self, c, n_total):
        """theta(n) = sum of the steps in force at 0 .. n - 1 (theta(0) = 0), n = 0 .. n_total - 1"""
        st = np.zeros(n_total, dtype=np.int64)
        for n0, s in self.changes[c]:
            st[n0:] = s
        return np.concatenate([[0], np.cumsum(st[:-1]) & MASK32]) & MASK32 if n_total else st

    def channel_out(self, c):
        R, x = self.R, self.x[c]
        L = x.shape[0]
        rails = []
        for rail in range(2):
            u = x[:, rail] << 8
            b = u if self.hB.size == 0 else q15(np.convolve(u, self.hB)[:L])
            v = (b * int(self.amp[c]) + (1 << 14)) >> 15
            if self.hA.size == 0:
                a = np.repeat(v, R)
            else:
                z = np.zeros(L * R, dtype=np.int64)
                z[::R] = v
                a = q15(np.convolve(z, self.hA)[:L * R])
            rails.append(a)
        th = self.theta(c, L * R)
        k = ((th + (1 << 19)) >> 20) & 4095
        co, si = COS[k], COS[(k - 1024) & 4095]
        return (rails[0] * co - rails[1] * si + (1 << 14)) >> 15, (rails[1] * co + rails[0] * si + (1 << 14)) >> 15

    def process(self, ch, in_bytes):
        R, M = self.R, in_bytes // 2
        ch = np.asarray(ch, dtype=np.int8).reshape(self.C, M, 2).astype(np.int64)
        for c in range(self.C):
            self.x[c] = np.concatenate([self.x[c], ch[c]])
        L = self.x[0].shape[0]
        S = np.zeros((self.W, 2, R * M), dtype=np.int64)
        for c in range(self.C):
            yI, yQ = self.channel_out(c)
            S[self.capture[c], 0] += yI[R * (L - M):]
            S[self.capture[c], 1] += yQ[R * (L - M):]
        out = np.zeros((self.W, R * M, 2), dtype=np.int64)
        for w in range(self.W):
            s = int(self.shift[w])
            y = (S[w] + ((1 << (s - 1)) if s else 0)) >> s
            o = np.clip(y, -128, 127)
            self.clips[w] += int((o != y).sum())
            out[w] = o.T
        self.N += R * M
        return out.reshape(self.W, -1).astype(np.int8), S


def float_sums(x, R, hA, hB, amp, theta):
    """one channel, whole stream from silence: (S_float I, Q) without any rounding; theta int [L R] the phases"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 2)
    L = x.shape[0]
    out = []
    for rail in range(2):
        u = x[:, rail] * 256.0
        b = u if len(hB) == 0 else np.convolve(u, np.asarray(hB, dtype=np.float64))[:L] / 32768.0
        v = b * amp / 32768.0
        if len(hA) == 0:
            a = np.repeat(v, R)
        else:
            z = np.zeros(L * R)
            z[::R] = v
            a = np.convolve(z, np.asarray(hA, dtype=np.float64))[:L * R] / 32768.0
        out.append(a)
    k = ((np.asarray(theta, dtype=np.int64) + (1 << 19)) >> 20) & 4095
    co, si = COS[k] / 32768.0, COS[(k - 1024) & 4095] / 32768.0
    return out[0] * co - out[1] * si, out[1] * co + out[0] * si


def error_budget(R, hA, hB, amp):
    """|S_int - S_float| per channel, from the rounding steps: each (acc + 2^14) >> 15 is off by at most 1/2 (in
    [-1/2, 1/2)), and every later stage scales what came in by its gain in sum |h| / 32768 (no saturation)"""
    hA = np.abs(np.asarray(hA, dtype=np.float64))
    gA = max(hA[p::R].sum() for p in range(R)) / 32768.0 if hA.size else 1.0
    e_b = 0.5 if len(hB) else 0.0
    e_v = e_b * amp / 32768.0 + 0.5
    e_a = e_v * gA + (0.5 if hA.size else 0.0)
    return e_a * (2 * 32767 / 32768.0) + 0.5 + 1e-9
