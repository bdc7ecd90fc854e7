"""The spectrum bank's model (tests/spec_model.py) against its independent restatement (tests/spec_reference.py), bit for
bit, and against float64 within a budget derived from the contract's roundings; find_stations on synthetic captures."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import spec_model as sm
from tests import spec_reference as sr


def adversarial(L, kind, n_frames, seed):
    N = 1 << L
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(-128, 128, size=(1, 2 * N * n_frames)).astype(np.int8), None
    if kind == "min_min":
        return np.full((1, 2 * N * n_frames), -128, dtype=np.int8), np.full(N, -32768, dtype=np.int16)
    if kind == "alternation":
        x = np.empty((n_frames * N, 2), dtype=np.int8)
        x[0::2], x[1::2] = 127, -128
        return x.reshape(1, -1), np.full(N, 32767, dtype=np.int16)
    if kind == "fs4":
        t = np.arange(n_frames * N)
        x = np.stack([np.round(127 * np.cos(np.pi * t / 2)), np.round(127 * np.sin(np.pi * t / 2))], axis=1)
        return x.astype(np.int8).reshape(1, -1), None
    w = rng.integers(-32768, 32768, size=N).astype(np.int16)                     # "window": random with -32768 and 0
    w[::3] = -32768
    w[1::3] = 0
    return sm.lcg_captures(1, 2 * N * n_frames, seed), w


@pytest.mark.parametrize("L", range(sm.MIN_L, sm.MAX_L + 1))
@pytest.mark.parametrize("kind", ["random", "min_min", "alternation", "fs4", "window"])
def test_model_equals_restatement(L, kind):
    N = 1 << L
    n_frames = 1 if L > 10 else 3
    x, w = adversarial(L, kind, n_frames, 10 * L)
    m = sm.SpecModel(1, 8, L)
    if w is not None:
        m.set_window(w)
    band_list = [(0, N - 5, 11, 1000), (0, N // 2 - 2, 5, 0), (0, 0, N, 1 << 20), (0, 17, 1, 1 << 44)]
    for b, rec in enumerate(band_list):
        m.set_band(b, *rec)
    power, bp, pr = m.process(x, n_frames)
    _, p_ref = sr.spectrum(x, 1, L, n_frames, None if w is None else w)
    assert [int(v) for v in power[0]] == p_ref[0]
    want = sr.bands(p_ref, N, band_list, n_frames)
    assert [(int(a), int(b)) for a, b in zip(bp, pr)] == want
    if kind == "min_min":
        assert m.stage_max == [1 << 29] * (L + 1) and int(power[0, 0]) == n_frames << 29


def test_tables_equal_the_restatement():
    for L in range(sm.MIN_L, sm.MAX_L + 1):
        c, s = sr._tables(1 << L)
        assert (sm.cos_sin(L)[0] == c).all() and (sm.cos_sin(L)[1] == s).all() and (sm.hann(L) == sr.hann(1 << L)).all()


def test_no_bands_many_frames_and_pure_function():
    m = sm.SpecModel(2, 1, 8)
    x = sm.lcg_captures(2, 512 * 300, 4)
    power, bp, pr = m.process(x, 300)
    assert bp.size == 0 and pr.size == 0
    again = m.process(x, 300)[0]
    assert (power == again).all(), "no history: the same input gives the same output"
    halves = m.process(x[:, :512 * 150], 150)[0] + m.process(x[:, 512 * 150:], 150)[0]
    assert (power == halves).all(), "the sum over frames splits"
    _, p_ref = sr.spectrum(x, 2, 8, 300)
    assert [[int(v) for v in row] for row in power] == p_ref


def budget(L, M):
    """Per component, in LSB, against float64 np.fft.fft(u) / N with u the exact x w / 256, M the largest complex magnitude
    behind the window.  Worst case: errors never grow through a stage (a halved sum of two errors is at most the larger,
    a rotation keeps the magnitude), so they add: the window's rounded shift (0.5 per rail: 0.5 sqrt 2 as a complex
    magnitude), and per stage the halving's rounding (0.5 sqrt 2), the rotation's rounded shift (0.5 sqrt 2), the
    twiddle's quantisation (each of c, s within 0.5 of 32767 cos / sin: M 0.5 sqrt 2 / 32767) and its scale (32767 / 32768:
    M / 32768).  rms: the roundings as independent errors whose variance halves with every later halving, so at most
    twice one stage's (1/16 for the halvings, 1/12 for the rotation's shift, half the squared twiddle term per
    component), plus 0.25 for the bias: a halving rounds up or down by 0.25 on average, and as the stages alternate the
    direction no path collects more than one stage's."""
    tw = M * (0.5 * np.sqrt(2) / 32767 + 1 / 32768)
    worst = 0.5 * np.sqrt(2) + L * (np.sqrt(2) + tw)
    rms = np.sqrt(2 * (1 / 16 + 1 / 12 + tw * tw / 2)) + 0.25
    return worst, rms


@pytest.mark.parametrize("L", [8, 10, 11, 13])
@pytest.mark.parametrize("kind", ["random", "min_min", "alternation", "fs4"])
def test_model_against_float64_within_the_derived_budget(L, kind):
    x, w = adversarial(L, kind, 1, 99 + L)
    m = sm.SpecModel(1, 8, L)
    if w is not None:
        m.set_window(w)
    re, im = m.transform(x.reshape(1, 1, 1 << L, 2))
    X = np.empty((1 << L,), dtype=np.complex128)
    X[m.rev] = re[0, 0] + 1j * im[0, 0]
    F = sr.float_spectrum(x, 1, L, 1, m.window)[0, 0]
    err = np.concatenate([(X - F).real, (X - F).imag])
    worst, rms = budget(L, np.sqrt(m.stage_max[0]))
    print(f"L={L} {kind}: max {np.abs(err).max():.2f} (budget {worst:.1f}), rms {np.sqrt(np.mean(err ** 2)):.2f} (budget {rms:.2f})")
    assert np.abs(err).max() <= worst and np.sqrt(np.mean(err ** 2)) <= rms


def synthetic_fm_capture(seed=3):
    """R = 8, L = 13, 32 frames: three FM stations (75 kHz deviation, 1-3 kHz tones) of amplitude 4 / 1.5 / 0.6 LSB over
    0.3 LSB rms noise per rail, rounded to int8"""
    R, L, nf = 8, 13, 32
    n = nf << L
    fs = R * sm.FS_CH
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    x = rng.normal(0, 0.3, n) + 1j * rng.normal(0, 0.3, n)
    stations = [(-2_400_000.0, 4.0, 1000.0), (1_000_000.0, 1.5, 2000.0), (6_200_000.0, 0.6, 3000.0)]
    for f, amp, tone in stations:
        x += amp * np.exp(1j * (2 * np.pi * f * t + 75_000.0 / tone * np.sin(2 * np.pi * tone * t)))
    cap = np.stack([np.round(x.real), np.round(x.imag)], axis=1).clip(-128, 127).astype(np.int8).reshape(1, -1)
    return cap, [s[0] for s in stations], R, L, nf


def test_find_stations_on_synthetic_fm():
    """The 6 dB rule finds the three stations and nothing else.  What the alternating rounding of the halvings is for: with
    every stage rounding up, the +0.25 mean of (v + 1) >> 1 adds up over the stages to about 600 power units per frame in
    the 200 kHz around DC (noise alone on the input: floor 74, DC 591), 9.4 dB over the floor, and DC is reported as
    a station.  With the odd stages rounding down the same capture has a floor of 57 per frame and 61 at DC; the stations'
    band sums are 98 173 / 13 894 / 2 258 per frame: 32.4 / 23.9 / 16.0 dB."""
    cap, offsets, R, L, nf = synthetic_fm_capture()
    power = sm.SpecModel(1, R, L).process(cap, nf)[0]
    raster = 200_000.0
    found = api.find_stations(power, nf, R, L, 200_000.0, raster, 6.0)
    print(found)
    assert len(found) == 3, found
    for (w, off, bp), want in zip(found, offsets):
        assert w == 0 and abs(off - want) <= raster and bp > 0


def test_host_helpers():
    assert api.spec_bin_hz(8, 13) == 2000.0
    off = api.spec_offsets_hz(8, 13)
    assert off[0] == 0 and off[1] == 2000.0 and off[-1] == -2000.0 and off[4096] == -8_192_000.0
    # full scale from the model: a tone of amplitude 127 on a bin centre under the default window
    L, k = 10, 37
    t = np.arange(1 << L)
    x = np.stack([np.round(127 * np.cos(2 * np.pi * k * t / (1 << L))), np.round(127 * np.sin(2 * np.pi * k * t / (1 << L)))], axis=1)
    power = sm.SpecModel(1, 1, L).process(x.astype(np.int8).reshape(1, -1), 1)[0]
    db = api.spec_dbfs(power, 1)
    assert power[0].argmax() == k and abs(db[0, k]) < 0.05, db[0, k]
    assert api.spec_threshold(0.0, 1) == int(round(api.SPEC_FULL_SCALE_POWER))
    assert abs(api.spec_dbfs(api.spec_threshold(-30.0, 4) / 4.0, 1) + 30.0) < 0.01
