"""The tone bank's numpy model (tests/tone_model.py) without a GPU: against a sample-by-sample restatement of include/hrfd.h
in Python integers, and as a detector: every CTCSS tone under noise, every DTMF digit, noise and silence, and the closed loop
modulator -> DUC -> DDC -> receive chain -> tones on the models and the CPU oracle, which fixes the audio the device test
(tests/test_gpu_tone.py) sends through the same chain."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import tone_model as tm
from tests.ddc_model import COS

M32 = (1 << 32) - 1


def slow(pcm, n_pcm, L, window, steps, groups, ratio_q8, min_energy):
    """one channel, Python integers only: lists of per-frame (power [K], energy, valid, best [4], present [4])"""
    cos = [int(v) for v in COS]
    n_blocks = len(pcm) // 512
    out = []
    for f in range(512 * n_blocks // L):
        u, valid = [], 0
        for n in range(L):
            j = f * L + n
            b, pos = j // 512, j % 512
            lim = 512 if n_pcm is None else min(int(n_pcm[b]) & M32, 512)
            x = int(pcm[j]) if pos < lim else 0
            valid += pos < lim
            u.append((x * int(window[n]) + (1 << 14)) >> 15)
        E = sum(v * v for v in u)
        P = []
        for step in steps:
            I = Q = 0
            for n in range(L):
                theta = (int(step) * n) & M32
                i = ((theta + (1 << 19)) >> 20) & 4095
                I += u[n] * cos[i]
                Q += u[n] * cos[(i - 1024) & 4095]
            assert abs(I) < 1 << 43 and abs(Q) < 1 << 43
            Ir, Qr = (I + (1 << 14)) >> 15, (Q + (1 << 14)) >> 15
            P.append(Ir * Ir + Qr * Qr)
        best, present = [], []
        for g in range(4):
            mine = [k for k in range(len(steps)) if groups[k] == g]
            if not mine:
                best.append(255)
                present.append(0)
                continue
            top = max(P[k] for k in mine)
            b = min(k for k in mine if P[k] == top)
            best.append(b)
            present.append(int(valid == L and E >= min_energy[g] and P[b] >= ((E * ratio_q8[g]) >> 8)))
        out.append((P, E, valid, best, present))
    return out


def agree(m, pcm, n_pcm, what):
    P, E, V, B, Pr = m.process(pcm, n_pcm)
    for c in range(m.C):
        want = slow(pcm[c], None if n_pcm is None else n_pcm[c], m.L, m.window, m.steps, m.groups, m.ratio_q8, m.min_energy)
        for f, (p, e, v, b, pr) in enumerate(want):
            assert [int(x) for x in P[c, f]] == p and int(E[c, f]) == e and int(V[c, f]) == v, (what, c, f)
            assert [int(x) for x in B[c, f]] == b and [int(x) for x in Pr[c, f]] == pr, (what, c, f)
    return P, E, V, B, Pr


# 1. the model against the slow restatement
@pytest.mark.parametrize("L", [128, 256])
def test_model_equals_the_contract_sample_by_sample(L):
    rng = np.random.default_rng(L)
    m = tm.ToneModel(2, L)
    m.set_tones([tm.tone_step(697.0), tm.tone_step(1209.0), tm.tone_step(1000.0)], [0, 1, 1])
    pcm = rng.integers(-32768, 32768, size=(2, 1024), dtype=np.int16)
    agree(m, pcm, None, "random")
    n_pcm = np.array([[0, 513], [255, 0xFFFFFFFF]], dtype=np.uint32)
    P, E, V, B, Pr = agree(m, pcm, n_pcm, "n_pcm")
    assert V[0].sum() == 512 and V[1].sum() == 255 + 512
    m.set_threshold(1, 40, 0)
    m.set_threshold(0, 1, 1 << 43)
    agree(m, pcm, np.array([[512, 1], [2, 511]], dtype=np.uint32), "thresholds")
    # the extremes: a flat window of 32767, full-scale input of either sign, steps 0, 1, 2^31
    m.set_window(np.full(L, 32767))
    m.set_tones([0, 1, 1 << 31], [0, 0, 2])
    for v in (-32768, 32767):
        P, E, V, B, Pr = agree(m, np.full((2, 512), v, dtype=np.int16), None, f"all {v}")
        assert int(E[0, 0]) == L * ((v * 32767 + (1 << 14)) >> 15) ** 2
    m.set_tones([M32, 5, 5], [3, 1, 1])
    P, E, V, B, Pr = agree(m, pcm, None, "ties")
    assert (B[:, :, 1] == 1).all() and (B[:, :, 0] == 255).all() and (Pr[:, :, 0] == 0).all()


def noise(rng, n, rms):
    """differenced Gaussian noise of the given rms: what an FM discriminator leaves, rising with frequency"""
    g = rng.standard_normal(n + 1)
    return np.diff(g) * (rms / np.sqrt(2.0))


def to_pcm(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


# 2. every CTCSS tone, amplitude 1500 under noise of rms 4000: 0.066 of the energy
def test_every_ctcss_tone_is_decoded_under_noise():
    L = 4096
    rng = np.random.default_rng(1)
    t = np.arange(L) / tm.FS
    pcm = np.stack([to_pcm(1500.0 * np.sin(2 * np.pi * f * t + 0.3 * k) + noise(rng, L, 4000.0)) for k, f in enumerate(api.CTCSS_HZ)])
    m = tm.ToneModel(len(api.CTCSS_HZ), L)
    m.set_tones([tm.tone_step(f) for f in api.CTCSS_HZ], [2] * len(api.CTCSS_HZ))
    P, E, V, B, Pr = m.process(pcm)
    frac = api.tone_fraction(P, E, m.window)
    margins, fracs = [], []
    for k in range(len(api.CTCSS_HZ)):
        assert B[k, 0, 2] == k, (k, B[k, 0])
        row = np.sort(P[k, 0].astype(np.float64))
        margins.append(row[-1] / row[-2])
        fracs.append(frac[k, 0, k])
    print("smallest margin", min(margins), "fractions", min(fracs), max(fracs))
    assert min(margins) >= 2.0, margins
    assert 0.05 <= min(fracs) and max(fracs) <= 0.09, fracs
    assert (B[:, 0, 0] == 255).all() and (Pr[:, 0, :2] == 0).all()


def dtmf_pcm(rng, key_row, key_col, n, amp=6000.0, rms=600.0):
    t = np.arange(n) / tm.FS
    x = amp * (np.sin(2 * np.pi * api.DTMF_LOW_HZ[key_row] * t + 1.0) + np.sin(2 * np.pi * api.DTMF_HIGH_HZ[key_col] * t + 2.0))
    return to_pcm(x + noise(rng, n, rms))


def dtmf_model(C, L):
    m = tm.ToneModel(C, L)
    m.set_tones([tm.tone_step(f) for f in api.DTMF_LOW_HZ + api.DTMF_HIGH_HZ], [0] * 4 + [1] * 4)
    r = api.tone_threshold(m.window, 0.25)
    m.set_threshold(tm.MASK32, r, 256 * L)
    return m


# 3. every DTMF digit at three frame lengths
@pytest.mark.parametrize("L", [128, 256, 512])
def test_every_dtmf_digit_is_decoded(L):
    rng = np.random.default_rng(2)
    keys = [(r, c) for r in range(4) for c in range(4)]
    pcm = np.stack([dtmf_pcm(rng, r, c, 512) for r, c in keys])
    m = dtmf_model(16, L)
    P, E, V, B, Pr = m.process(pcm)
    frac = api.tone_fraction(P, E, m.window)
    smallest = 1.0
    for i, (r, c) in enumerate(keys):
        for f in range(512 // L):
            assert (B[i, f, 0], B[i, f, 1]) == (r, 4 + c), (i, f, B[i, f])
            assert Pr[i, f, 0] == 1 and Pr[i, f, 1] == 1, (i, f)
            assert api.dtmf_digit(B[i, f, 0], B[i, f, 1] - 4) == "123A456B789C*0#D"[i]
            smallest = min(smallest, frac[i, f, r], frac[i, f, 4 + c])
    print("smallest fraction per tone", smallest)
    assert smallest > 0.25


# 4. noise alone, silence, and a frame with one squelched block
def test_noise_and_silence_are_never_present():
    rng = np.random.default_rng(3)
    for L in (128, 256, 512, 4096):
        n = max(L, 512) * 2
        pcm = np.stack([to_pcm(noise(rng, n, 4000.0)), to_pcm(noise(rng, n, 600.0)), np.zeros(n, dtype=np.int16)])
        for m in (dtmf_model(3, L), tm.ToneModel(3, L)):
            if m.steps.size == 0:
                m.set_tones([tm.tone_step(f) for f in api.CTCSS_HZ], [2] * len(api.CTCSS_HZ))
            P, E, V, B, Pr = m.process(pcm)
            assert (Pr == 0).all(), (L, Pr)
            assert (V == L).all() and (E[2] == 0).all() and (P[2] == 0).all()
            print("L", L, "tones", m.steps.size, "largest noise fraction", api.tone_fraction(P, E, m.window).max())
    # a digit that would be present, with one block squelched: every frame that touches the block is short
    L = 1024
    pcm = dtmf_pcm(rng, 1, 2, 2048)[None, :]
    m = dtmf_model(1, L)
    assert (m.process(pcm)[4][0, :, :2] == 1).all()
    P, E, V, B, Pr = m.process(pcm, np.array([[512, 0, 512, 512]], dtype=np.uint32))
    assert list(V[0]) == [512, 1024] and list(Pr[0, 0]) == [0, 0, 0, 0] and list(Pr[0, 1, :2]) == [1, 1]


def test_helpers():
    assert api.tone_step(1000.0) == tm.tone_step(1000.0) == 1 << 29
    assert api.tone_step(-1000.0) == (1 << 32) - (1 << 29)
    assert len(api.CTCSS_HZ) == 50 and api.CTCSS_HZ[0] == 67.0 and api.CTCSS_HZ[-1] == 254.1 and sorted(api.CTCSS_HZ) == list(api.CTCSS_HZ)
    for L in (128, 4096):
        w = api.tone_default_window(L)
        assert (w == tm.default_window(L)).all()
        assert abs(api.tone_gain(w) - L / 3.0) < 0.01 * L                  # Hann: S1 = L / 2, S2 = 3 L / 8
        assert abs(api.tone_threshold(w, 0.1875) - 16 * L) <= 0.01 * 16 * L  # the default ratio is about 0.19 of the energy
    assert api.dtmf_digit(0, 0) == "1" and api.dtmf_digit(3, 1) == "0" and api.dtmf_digit(2, 3) == "C"


# 5. the closed loop on the models and the CPU oracle: the amplitudes of tone_model.loop_audio pass here before the device
#    test runs the same chain
def test_closed_loop_dtmf_over_two_wbfm_stations(oracle):
    from tests import ddc_model as dm
    from tests import duc_model as um
    audio = tm.loop_audio()
    streams, amps = tm.loop_streams(oracle, audio)
    cap, duc = um.loop_duc(streams, amps)
    assert duc.clips[0] == 0
    d = dm.DdcModel(1, 2, dm.SEL_R)
    for c, f in enumerate(dm.SEL_OFFSETS):
        d.set_tuning(c, 0, dm.ddc_step(f + 64_000, dm.SEL_R))
        d.set_gain_shift(c, dm.SEL_GAIN_SHIFT[c])
    rx_in = d.process(cap, dm.SEL_BLOCKS * 262144)
    pcm = np.stack([dm.oracle_rx_wbfm(oracle, rx_in[c]) for c in range(2)])
    m = tm.loop_model()
    P, E, V, B, Pr = m.process(pcm)
    frac = api.tone_fraction(P, E, m.window)
    print("fractions of the decoded frames: rows", frac[:, 1::2, :4].max(axis=2).min(), "columns", frac[:, 1::2, 4:8].max(axis=2).min(),
          "pilot", frac[0, 1::2, 8].min(), "against", frac[1, 1::2, 8].max())
    tm.loop_check(B, Pr)
