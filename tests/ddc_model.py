"""numpy model of the DDC bank (hrfd_ddc_*, include/hrfd.h): int64 arithmetic, the contract line by line, state
carried across calls like the handle.  The GPU tests compare the library with it bit for bit."""
from __future__ import annotations

import numpy as np

FS_OUT = 2_048_000
MASK32 = (1 << 32) - 1


def cos_table() -> np.ndarray:
    return np.round(32767.0 * np.cos(2.0 * np.pi * np.arange(4096) / 4096.0)).astype(np.int64)


COS = cos_table()


def ddc_step(offset_hz: float, decimation: int) -> int:
    """step = round(f / (R * 2 048 000) * 2^32) mod 2^32"""
    return int(round(offset_hz / (decimation * FS_OUT) * 2.0 ** 32)) & MASK32


def history_len(decimation: int) -> int:
    return 255 * decimation + 63


def sat(x: np.ndarray, bits: int) -> np.ndarray:
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return np.clip(x, lo, hi)


def mix(iq: np.ndarray, theta: np.ndarray):
    """iq int [n, 2], theta uint32 as int64 [n] -> (yI, yQ) int64: multiplication by e^{-j theta}"""
    k = ((theta + (1 << 19)) >> 20) & 4095
    c = COS[k]
    s = COS[(k - 1024) & 4095]
    i, q = iq[:, 0].astype(np.int64), iq[:, 1].astype(np.int64)
    return (i * c + q * s + 128) >> 8, (q * c - i * s + 128) >> 8


def fir_acc(h: np.ndarray, x: np.ndarray, n_out: int, first_end: int, step: int) -> np.ndarray:
    """acc[m] = sum_k h[k] x[e_m - k], e_m = first_end + m * step (indices into x)"""
    h = np.asarray(h, dtype=np.int64)
    ends = first_end + step * np.arange(n_out)
    acc = np.zeros(n_out, dtype=np.int64)
    for k in range(h.size):
        acc += h[k] * x[ends - k]
    return acc


def q15(acc: np.ndarray) -> np.ndarray:
    """sat16((acc + 2^14) >> 15)"""
    return sat((acc + (1 << 14)) >> 15, 16)


def fir_q15(h: np.ndarray, x: np.ndarray, n_out: int, first_end: int, step: int) -> np.ndarray:
    """out[m] = sat16((sum_k h[k] x[e_m - k] + 2^14) >> 15), e_m = first_end + m * step (indices into x)"""
    return q15(fir_acc(h, x, n_out, first_end, step))


def default_taps(decimation: int):
    from tools import ddc_design
    t = ddc_design.tables()
    a = {1: np.zeros(0, dtype=np.int64), 2: t["DDC_A2"], 4: t["DDC_A4"], 8: t["DDC_A8"]}[decimation]
    return np.asarray(a, dtype=np.int64), np.asarray(t["DDC_B"], dtype=np.int64)


class DdcModel:
    """The handle: n_captures histories, n_channels channel records, one counter N."""

    def __init__(self, n_captures: int, n_channels: int, decimation: int):
        assert decimation in (1, 2, 4, 8)
        self.W, self.C, self.R = n_captures, n_channels, decimation
        self.H = history_len(decimation)
        self.hA, self.hB = default_taps(decimation)
        self.capture = np.zeros(self.C, dtype=np.int64)
        self.step = np.zeros(self.C, dtype=np.int64)
        self.g = np.zeros(self.C, dtype=np.int64)
        self.reset()

    def reset(self):
        """history 0, N = 0, every theta_ref = N_ref = 0; captures, steps, gain shifts and filters stay"""
        self.N = 0
        self.hist = np.zeros((self.W, self.H, 2), dtype=np.int64)
        self.theta_ref = np.zeros(self.C, dtype=np.int64)
        self.n_ref = np.zeros(self.C, dtype=np.int64)

    def phase(self, c: int, n: int | None = None) -> int:
        """theta(n) = theta_ref + (n - N_ref) * step mod 2^32 (n defaults to the counter N)"""
        n = self.N if n is None else n
        return (int(self.theta_ref[c]) + (n - int(self.n_ref[c])) * int(self.step[c])) & MASK32

    def set_tuning(self, c: int, capture: int, step: int):
        self.theta_ref[c] = self.phase(c)
        self.n_ref[c] = self.N
        self.capture[c] = capture
        self.step[c] = step & MASK32

    def set_gain_shift(self, c: int, g: int):
        assert 0 <= g <= 7
        self.g[c] = g

    def set_filter(self, stage: int, taps):
        taps = np.asarray(taps, dtype=np.int64)
        assert taps.size <= (64 if stage == 0 else 256) and np.abs(taps).sum() <= 65535
        if stage == 0:
            self.hA = taps
        else:
            self.hB = taps

    def seek(self, N: int, hist: np.ndarray):
        """move the counter to N with the H input samples in front of it (int [W, H, 2] or int8 [W, 2 H]): the
        phase is absolute, so the next call computes what a handle that ran up to N computes"""
        self.N = int(N)
        self.hist = np.asarray(hist).reshape(self.W, self.H, 2).astype(np.int64)

    def process(self, captures: np.ndarray, out_bytes: int, stages: bool = False):
        """captures int8 [W, R * out_bytes] -> int8 [C, out_bytes]; stages=True also returns a dict of int64
        [C, 2, n] arrays (rail 0 = I, 1 = Q): "accA" stage A's sums sum_k hA[k] y[..] (before rounding and sat16),
        "a" a16, both for the a16 indices -255 .. M - 1 of the call (stage B's look-back first; with T_A = 0 "accA"
        is None), "accB" stage B's sums (None with T_B = 0) and "b" b16 for the call's M outputs"""
        R, H, M = self.R, self.H, out_bytes // 2
        cap = np.asarray(captures, dtype=np.int8).reshape(self.W, R * M, 2).astype(np.int64)
        stream = np.concatenate([self.hist, cap], axis=1)           # [W, H + R M, 2]: index H + j = local sample j
        out = np.zeros((self.C, M, 2), dtype=np.int64)
        n_abs = self.N - H + np.arange(H + R * M, dtype=np.int64)     # absolute sample index of every stream entry
        st = {"accA": None if self.hA.size == 0 else np.zeros((self.C, 2, M + 255), dtype=np.int64),
              "a": np.zeros((self.C, 2, M + 255), dtype=np.int64),
              "accB": None if self.hB.size == 0 else np.zeros((self.C, 2, M), dtype=np.int64),
              "b": np.zeros((self.C, 2, M), dtype=np.int64)}
        for c in range(self.C):
            theta = (int(self.theta_ref[c]) + (n_abs - int(self.n_ref[c])) * int(self.step[c])) & MASK32
            y = mix(stream[int(self.capture[c])], theta)
            # stage A: a[m] = sum_k hA[k] y[m R + R - 1 - k]; entries of the stream before 0 are never reached
            first = H + R - 1 - 255 * R                                # a16 index -255 (stage B's deepest look-back)
            for rail in range(2):
                if self.hA.size == 0:
                    a = y[rail][first::R][:M + 255]
                else:
                    acc = fir_acc(self.hA, y[rail], M + 255, first, R)
                    a = q15(acc)
                    st["accA"][c, rail] = acc
                # stage B at 2.048 MS/s; a16 index m lives at position m + 255
                if self.hB.size == 0:
                    b = a[255:]
                else:
                    acc = fir_acc(self.hB, a, M, 255, 1)
                    b = q15(acc)
                    st["accB"][c, rail] = acc
                st["a"][c, rail], st["b"][c, rail] = a, b
                g = int(self.g[c])
                r = (1 << (6 - g)) if g < 7 else 0
                out[c, :, rail] = sat((b + r) >> (7 - g), 8)
        self.hist = stream[:, -H:].copy()
        self.N += R * M
        out = out.reshape(self.C, 2 * M).astype(np.int8)
        return (out, st) if stages else out


# ---- the selectivity scenario (tests/test_ddc_model.py on the model, tests/test_gpu_ddc.py on the device)
SEL_R = 4
SEL_OFFSETS = (-200_000.0, 200_000.0)      # station, interferer: 400 kHz apart
SEL_LEVELS = (25.0, 25.0 * 10 ** 0.5)      # the interferer 10 dB stronger
SEL_GAIN_SHIFT = (2, 0)
SEL_BLOCKS = 16                            # 16 x 64 ms: 8192 PCM samples per station
SEL_AUDIO = (9000, 25000)                  # where each station's audio starts in count.raw (mutual correlation 0.047)


def count_raw() -> np.ndarray:
    import os
    return np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "count.raw"), dtype="<i2")


def selectivity_capture(oracle):
    """(capture int8 [1, R * 16 * 262144], audio [2][8192]): two WBFM stations from count.raw (the oracle's
    modulator), upsampled in float to R x 2.048 MS/s, shifted to their offsets and rounded to int8"""
    pcm = count_raw()
    n_pcm = SEL_BLOCKS * 512
    audio = [pcm[o:o + n_pcm] for o in SEL_AUDIO]
    n_out = SEL_BLOCKS * 262144 // 2
    n_in = SEL_R * n_out
    total = np.zeros(n_in, dtype=np.complex128)
    t = np.arange(n_in) / (SEL_R * FS_OUT)
    for a, f, lev in zip(audio, SEL_OFFSETS, SEL_LEVELS):
        iq = oracle.wbfmmod().process(a).astype(np.float64).reshape(-1, 2)
        x = iq[:, 0] + 1j * iq[:, 1]
        x = x / np.sqrt(np.mean(np.abs(x) ** 2))
        spec = np.fft.fft(x)
        up = np.zeros(n_in, dtype=np.complex128)               # band-limited upsampling: zero-padded spectrum
        h = n_out // 2
        up[:h], up[-h:] = spec[:h], spec[-h:]
        up = np.fft.ifft(up) * SEL_R
        total += lev * up * np.exp(2j * np.pi * f * t)
    cap = np.empty((n_in, 2), dtype=np.int8)
    cap[:, 0] = np.clip(np.round(total.real), -128, 127)
    cap[:, 1] = np.clip(np.round(total.imag), -128, 127)
    return cap.reshape(1, -1), audio


def best_corr(a: np.ndarray, b: np.ndarray, n: int = 7000, delays: int = 400) -> float:
    """best absolute correlation over a delay search (tests/golden/make_golden_count.py)"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    if b.std() == 0:
        return 0.0
    return max(abs(np.corrcoef(a[:n], b[d:n + d])[0, 1]) for d in range(0, delays))


def oracle_rx_wbfm(oracle, stream: np.ndarray, block_bytes: int = 262144) -> np.ndarray:
    """one channel's int8 stream through the CPU oracle's receive chain in WBFM, block by block -> PCM"""
    from tests.reflib import WBFM
    rx = oracle.rx()
    rx.set_mode(WBFM)
    out = [rx.process(stream[o:o + block_bytes])[0] for o in range(0, stream.size, block_bytes)]
    return np.concatenate(out)
