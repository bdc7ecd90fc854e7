"""numpy model of the DUC bank (hrfd_duc_*, include/hrfd.h): int64 arithmetic, the contract line by line, state
carried across calls like the handle.  The GPU tests compare the library with it bit for bit."""
from __future__ import annotations

import numpy as np

from tests.ddc_model import COS, MASK32, fir_acc, q15, sat

FS_CH = 2_048_000
H = 318                                    # channel samples of history: stage B's 255 behind stage A's 63


def duc_step(offset_hz: float, interpolation: int) -> int:
    """step = round(f / (R * 2 048 000) * 2^32) mod 2^32 puts the channel's DC at +f"""
    return int(round(offset_hz / (interpolation * FS_CH) * 2.0 ** 32)) & MASK32


def default_taps(interpolation: int):
    from tools import ddc_design, duc_design
    a = np.zeros(0, dtype=np.int64) if interpolation == 1 else duc_design.tables()[f"DUC_A{interpolation}"]
    return np.asarray(a, dtype=np.int64), np.asarray(ddc_design.tables()["DDC_B"], dtype=np.int64)


def branch_ok(taps, R: int) -> bool:
    a = np.abs(np.asarray(taps, dtype=np.int64))
    return all(a[p::R].sum() <= 65535 for p in range(R))


def mix_up(aI: np.ndarray, aQ: np.ndarray, theta: np.ndarray):
    """multiplication by e^{+j theta}: (yI, yQ) int64, and the int32 bound of the products checked"""
    k = ((theta + (1 << 19)) >> 20) & 4095
    c = COS[k]
    s = COS[(k - 1024) & 4095]
    pI = aI * c - aQ * s + (1 << 14)
    pQ = aQ * c + aI * s + (1 << 14)
    assert np.abs(pI).max(initial=0) < 2 ** 31 and np.abs(pQ).max(initial=0) < 2 ** 31
    return pI >> 15, pQ >> 15


class DucModel:
    """The handle: n_channels histories and records, n_captures shifts and clip counters, one counter N."""

    def __init__(self, n_captures: int, n_channels: int, interpolation: int):
        assert interpolation in (1, 2, 4, 8) and 0 < n_channels <= 32768
        self.W, self.C, self.R = n_captures, n_channels, interpolation
        self.hA, self.hB = default_taps(interpolation)
        self.capture = np.zeros(self.C, dtype=np.int64)
        self.step = np.zeros(self.C, dtype=np.int64)
        self.amp = np.full(self.C, 32768, dtype=np.int64)
        self.shift = np.full(self.W, 8, dtype=np.int64)
        self.reset()

    def reset(self):
        """history 0, N = 0, every theta_ref = N_ref = 0, clip counters 0; the rest stays"""
        self.N = 0
        self.hist = np.zeros((self.C, H, 2), dtype=np.int64)
        self.theta_ref = np.zeros(self.C, dtype=np.int64)
        self.n_ref = np.zeros(self.C, dtype=np.int64)
        self.clips = np.zeros(self.W, dtype=np.int64)

    def phase(self, c: int, n: int | None = None) -> int:
        n = self.N if n is None else n
        return (int(self.theta_ref[c]) + (n - int(self.n_ref[c])) * int(self.step[c])) & MASK32

    def set_tuning(self, c: int, capture: int, step: int):
        self.theta_ref[c] = self.phase(c)
        self.n_ref[c] = self.N
        self.capture[c] = capture
        self.step[c] = step & MASK32

    def set_amplitude(self, c: int, a: int):
        assert 0 <= a <= 32768
        self.amp[c] = a

    def set_output_shift(self, w: int, s: int):
        assert 0 <= s <= 24
        self.shift[w] = s

    def set_filter(self, stage: int, taps):
        taps = np.asarray(taps, dtype=np.int64)
        if stage == 0:
            assert taps.size <= 64 and branch_ok(taps, self.R)
            self.hA = taps
        else:
            assert taps.size <= 256 and np.abs(taps).sum() <= 65535
            self.hB = taps

    def seek(self, N: int, hist: np.ndarray):
        """move the counter to N (a multiple of R) with the H channel samples in front of it (int [C, H, 2] or int8
        [C, 2 H]): the phase is absolute, so the next call computes what a handle that ran up to N computes"""
        assert N % self.R == 0
        self.N = int(N)
        self.hist = np.asarray(hist).reshape(self.C, H, 2).astype(np.int64)

    def process(self, channels: np.ndarray, in_bytes: int, stages: bool = False):
        """channels int8 [C, in_bytes] -> int8 [W, R * in_bytes]; stages=True also returns a dict of int64 arrays, rail 0 =
        I, 1 = Q: "accB" [C, 2, M + LA] stage B's sums (None with T_B = 0), "b" and "v" [C, 2, M + LA] for the channel
        positions -LA .. M - 1 (LA = (T_A - 1) // R, stage A's look-back), "accA" [C, 2, R M] stage A's sums (None with
        T_A = 0), "a" [C, 2, R M], "y" [C, 2, R M] the mixer's output and "S" [W, 2, R M] the sums"""
        R, M = self.R, in_bytes // 2
        TA, TB = self.hA.size, self.hB.size
        LA = (TA - 1) // R if TA else 0
        x = np.asarray(channels, dtype=np.int8).reshape(self.C, M, 2).astype(np.int64)
        stream = np.concatenate([self.hist, x], axis=1)               # [C, H + M, 2]: index H + j = local sample j
        n_abs = self.N + np.arange(R * M, dtype=np.int64)
        S = np.zeros((self.W, 2, R * M), dtype=np.int64)
        st = {"accB": None if TB == 0 else np.zeros((self.C, 2, M + LA), dtype=np.int64),
              "b": np.zeros((self.C, 2, M + LA), dtype=np.int64), "v": np.zeros((self.C, 2, M + LA), dtype=np.int64),
              "accA": None if TA == 0 else np.zeros((self.C, 2, R * M), dtype=np.int64),
              "a": np.zeros((self.C, 2, R * M), dtype=np.int64), "y": np.zeros((self.C, 2, R * M), dtype=np.int64)}
        for c in range(self.C):
            a = []
            for rail in range(2):
                u = stream[c, :, rail] << 8
                # stage B for the positions -LA .. M - 1 (stream index H - LA ..)
                if TB == 0:
                    b = u[H - LA:]
                else:
                    acc = fir_acc(self.hB, u, M + LA, H - LA, 1)
                    b = q15(acc)
                    st["accB"][c, rail] = acc
                v = (b * int(self.amp[c]) + (1 << 14)) >> 15
                st["b"][c, rail], st["v"][c, rail] = b, v
                # stage A: a[m R + p] = sum_j hA[p + j R] v[m - j]; v index i is position i - LA
                if TA == 0:
                    ar = np.repeat(v[LA:], R)
                else:
                    acc = np.zeros(R * M, dtype=np.int64)
                    for p in range(R):
                        for j, k in enumerate(range(p, TA, R)):
                            acc[p::R] += self.hA[k] * v[LA - j:LA - j + M]
                    ar = q15(acc)
                    st["accA"][c, rail] = acc
                st["a"][c, rail] = ar
                a.append(ar)
            theta = (int(self.theta_ref[c]) + (n_abs - int(self.n_ref[c])) * int(self.step[c])) & MASK32
            yI, yQ = mix_up(a[0], a[1], theta)
            st["y"][c, 0], st["y"][c, 1] = yI, yQ
            w = int(self.capture[c])
            S[w, 0] += yI
            S[w, 1] += yQ
        out = np.zeros((self.W, R * M, 2), dtype=np.int64)
        for w in range(self.W):
            s = int(self.shift[w])
            r = (1 << (s - 1)) if s else 0
            for rail in range(2):
                y = (S[w, rail] + r) >> s
                o = sat(y, 8)
                self.clips[w] += int((o != y).sum())
                out[w, :, rail] = o
        st["S"] = S
        self.hist = stream[:, -H:].copy()
        self.N += R * M
        out = out.reshape(self.W, 2 * R * M).astype(np.int8)
        return (out, st) if stages else out


# ---- the closed loop: WBFM stations from count.raw through the modulator, the DUC, the DDC and the receive chain
# (tests/test_duc_model.py on the models and the CPU oracle, tests/test_gpu_duc.py on the device)
def loop_stations(oracle):
    """(channel streams int8 [2, 16 x 262144], audio [2][8192], amplitudes [2]): the DDC selectivity test's two stations
    (count.raw excerpts, 400 kHz apart, the second 10 dB stronger) through the oracle's WBFM modulator; A puts each at
    the selectivity test's int8 RMS level after the DUC (output shift 8: unity)"""
    from tests import ddc_model as dm
    pcm = dm.count_raw()
    n_pcm = dm.SEL_BLOCKS * 512
    audio = [pcm[o:o + n_pcm] for o in dm.SEL_AUDIO]
    streams = np.stack([oracle.wbfmmod().process(a) for a in audio])
    rms = np.sqrt(np.mean(streams.astype(np.float64) ** 2) * 2)
    amps = [int(round(32768 * lev / rms)) for lev in dm.SEL_LEVELS]
    return streams, audio, amps


def loop_duc(streams, amps):
    """the DUC model at the selectivity test's R and offsets -> one capture int8 [1, R x 16 x 262144]"""
    from tests import ddc_model as dm
    m = DucModel(1, 2, dm.SEL_R)
    for c, f in enumerate(dm.SEL_OFFSETS):
        m.set_tuning(c, 0, duc_step(f, dm.SEL_R))
        m.set_amplitude(c, amps[c])
    return m.process(streams, streams.shape[1]), m
