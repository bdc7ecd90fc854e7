"""numpy model of the tone bank (hrfd_tone_*, include/hrfd.h): int64 arithmetic, the contract line by line.  A call is a pure
function of its input and the settings, so the model carries none but the settings.  The GPU tests compare the library with
it bit for bit; tests/test_tone_model.py compares it with a sample-by-sample restatement in Python integers."""
from __future__ import annotations

import numpy as np

from tests.ddc_model import COS

FS = 8000
BLOCK = 512
GROUPS = 4
NO_BEST = 255
MASK32 = (1 << 32) - 1


def tone_step(f_hz: float) -> int:
    """step = round(f / 8000 * 2^32) mod 2^32"""
    return int(round(float(f_hz) / FS * 2.0 ** 32)) & MASK32


def default_window(L: int) -> np.ndarray:
    n = np.arange(L, dtype=np.float64)
    return np.floor(32767.0 * 0.5 * (1.0 - np.cos(2.0 * np.pi * n / L)) + 0.5).astype(np.int64)


def tone_table(steps, L: int):
    """(c, s) int64 [K, L]: theta = step n mod 2^32, i = ((theta + 2^19) >> 20) & 4095, c = COS[i], s = COS[(i - 1024) & 4095]"""
    st = np.asarray(steps, dtype=np.int64).reshape(-1, 1)
    theta = (st * np.arange(L, dtype=np.int64)[None, :]) & MASK32
    i = ((theta + (1 << 19)) >> 20) & 4095
    return COS[i], COS[(i - 1024) & 4095]


class ToneModel:
    def __init__(self, n_channels: int, frame_len: int):
        self.C, self.L = int(n_channels), int(frame_len)
        self.steps = np.zeros(0, dtype=np.int64)
        self.groups = np.zeros(0, dtype=np.int64)
        self.window = default_window(self.L)
        self.ratio_q8 = [16 * self.L] * GROUPS
        self.min_energy = [256 * self.L] * GROUPS

    def set_tones(self, steps, groups=None):
        self.steps = np.asarray([int(s) & MASK32 for s in steps], dtype=np.int64)
        self.groups = np.zeros(self.steps.size, dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)

    def set_window(self, w=None):
        self.window = default_window(self.L) if w is None else np.asarray(w, dtype=np.int64).copy()

    def set_threshold(self, group, ratio_q8: int, min_energy: int):
        for g in range(GROUPS):
            if group in (g, MASK32):
                self.ratio_q8[g], self.min_energy[g] = int(ratio_q8), int(min_energy)

    def process(self, pcm, n_pcm=None):
        """pcm int16 [C, n_blocks x 512] (any shape with C rows), n_pcm [C, n_blocks] or None -> (power uint64 [C, F, K],
        energy uint64 [C, F], valid uint32 [C, F], best uint8 [C, F, 4], present uint8 [C, F, 4])"""
        C, L, K = self.C, self.L, self.steps.size
        x = np.asarray(pcm).reshape(C, -1).astype(np.int64)
        n_blocks = x.shape[1] // BLOCK
        assert x.shape[1] == n_blocks * BLOCK and (n_blocks * BLOCK) % L == 0 and K > 0
        F = n_blocks * BLOCK // L
        if n_pcm is None:
            taken = np.ones((C, n_blocks, BLOCK), dtype=bool)
        else:
            lim = np.minimum(np.asarray(n_pcm).reshape(C, n_blocks).astype(np.int64) & MASK32, BLOCK)
            taken = np.arange(BLOCK)[None, None, :] < lim[:, :, None]
        taken = taken.reshape(C, F, L)
        x = np.where(taken, x.reshape(C, F, L), 0)
        valid = taken.sum(axis=2)
        u = (x * self.window[None, None, :] + (1 << 14)) >> 15
        c, s = tone_table(self.steps, L)
        I = u @ c.T                                             # exact: |I| < 2^43
        Q = u @ s.T
        Ir, Qr = (I + (1 << 14)) >> 15, (Q + (1 << 14)) >> 15
        P = (Ir * Ir + Qr * Qr).astype(np.uint64)               # < 2^57
        E = (u * u).sum(axis=2).astype(np.uint64)
        best = np.full((C, F, GROUPS), NO_BEST, dtype=np.uint8)
        present = np.zeros((C, F, GROUPS), dtype=np.uint8)
        for g in range(GROUPS):
            idx = np.flatnonzero(self.groups == g)
            if idx.size == 0:
                continue
            b = idx[np.argmax(P[:, :, idx], axis=2)]            # argmax: the first of equal maxima
            Pb = np.take_along_axis(P, b[:, :, None], axis=2)[:, :, 0]
            best[:, :, g] = b
            # E T < 2^63: Python-int exact in uint64 as well
            limit = (E * np.uint64(self.ratio_q8[g])) >> np.uint64(8)
            present[:, :, g] = (valid == L) & (E >= np.uint64(self.min_energy[g])) & (Pb >= limit)
        return P, E, valid.astype(np.uint32), best, present


# ---- the closed loop: DTMF digits over two WBFM stations through the modulator, the DUC, the DDC, the receive chain and the
# tone bank (tests/test_tone_model.py on the models and the CPU oracle, tests/test_gpu_tone.py on the device)
LOOP_L = 256
LOOP_KEYS = ("1234567890*#ABCD", "D#9C9B63A2580*14")      # one digit per 64 ms block, 16 blocks
LOOP_TONE_AMP = 5000.0
LOOP_PILOT_HZ, LOOP_PILOT_AMP = 1000.0, 2500.0             # on station 0 only
DTMF_LOW_HZ = (697.0, 770.0, 852.0, 941.0)
DTMF_HIGH_HZ = (1209.0, 1336.0, 1477.0, 1633.0)
DTMF_KEYS = "123A456B789C*0#D"


def loop_audio():
    """[2][8192] int16: each station's digits, phase-continuous sines switched at the block boundaries; the pilot under
    station 0"""
    t = np.arange(BLOCK) / FS
    out = []
    for c, keys in enumerate(LOOP_KEYS):
        x = np.zeros(16 * BLOCK)
        for k, key in enumerate(keys[:16]):
            r, col = divmod(DTMF_KEYS.index(key), 4)
            x[k * BLOCK:(k + 1) * BLOCK] = LOOP_TONE_AMP * (np.sin(2 * np.pi * DTMF_LOW_HZ[r] * t) + np.sin(2 * np.pi * DTMF_HIGH_HZ[col] * t))
        if c == 0:
            x += LOOP_PILOT_AMP * np.sin(2 * np.pi * LOOP_PILOT_HZ * np.arange(x.size) / FS)
        out.append(np.round(x).astype(np.int16))
    return out


def loop_streams(oracle, audio):
    """duc_model.loop_stations with this audio: (channel streams int8 [2, 16 x 262144], amplitudes [2])"""
    from tests import ddc_model as dm
    streams = np.stack([oracle.wbfmmod().process(a) for a in audio])
    rms = np.sqrt(np.mean(streams.astype(np.float64) ** 2) * 2)
    return streams, [int(round(32768 * lev / rms)) for lev in dm.SEL_LEVELS]


def loop_settings(bank):
    """rows in group 0, columns in 1, the pilot in 2: a quarter of the frame's energy for a row and a column, a twentieth
    for the pilot (ToneModel and api.Tones take the same calls)"""
    from hackrfdiags_amd import api
    steps = [tone_step(f) for f in DTMF_LOW_HZ + DTMF_HIGH_HZ + (LOOP_PILOT_HZ,)]
    groups = [0] * 4 + [1] * 4 + [2]
    w = default_window(LOOP_L)
    return steps, groups, [(0, api.tone_threshold(w, 0.25)), (1, api.tone_threshold(w, 0.25)), (2, api.tone_threshold(w, 0.05))]


def loop_model():
    m = ToneModel(2, LOOP_L)
    steps, groups, th = loop_settings(m)
    m.set_tones(steps, groups)
    for g, r in th:
        m.set_threshold(g, r, 256 * LOOP_L)
    return m


def loop_check(best, present):
    """The receive chain delays the audio by less than one frame, so the second frame of every block lies wholly inside
    the block's digit: there the row, the column and the pilot's presence must be the ones sent."""
    for c, keys in enumerate(LOOP_KEYS):
        for k, key in enumerate(keys[:16]):
            f = 2 * k + 1
            r, col = divmod(DTMF_KEYS.index(key), 4)
            assert (best[c, f, 0], best[c, f, 1]) == (r, 4 + col), (c, k, key, best[c, f])
            assert present[c, f, 0] == 1 and present[c, f, 1] == 1, (c, k, key, present[c, f])
            assert best[c, f, 2] == 8 and present[c, f, 2] == (1 if c == 0 else 0), (c, k, present[c, f])
