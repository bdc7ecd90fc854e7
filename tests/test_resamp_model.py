"""The numpy model of the resampler bank (tests/resamp_model.py) against an output-by-output restatement in Python integers,
its independence of how a stream is cut into calls, the count law, the promise of api.resample_taps measured on its taps, and
a sine through 6/1 and back through 1/6.  No GPU."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import resamp_model as rm

RATIOS = [(6, 1), (1, 6), (3, 2), (2, 3), (7, 8), (441, 80), (80, 441), (5, 1), (1, 1)]
CUTS = [1, 1, 2, 3, 1, 5, 64, 1, 100, 511, 11]


def taps_for(L, K, seed):
    T = L * K - 1 if L * K > 1 else 1
    return np.random.default_rng(seed).integers(-(65535 // K), 65535 // K + 1, size=T).astype(np.int16)


@pytest.mark.parametrize("L,M", RATIOS)
def test_model_equals_the_integer_loop(L, M):
    taps = taps_for(L, 7, L * 1000 + M)
    x = np.random.default_rng(1).integers(-32768, 32768, size=(2, 200), dtype=np.int16)
    m = rm.ResampModel(2, L, M)
    m.set_taps(taps)
    first = m.process(x[:, :90])
    second = m.process(x[:, 90:])
    for c in range(2):
        y, d = rm.slow_channel(x[c, :90], [], taps, L, M, 0)
        assert first[c].tolist() == y
        y2, d2 = rm.slow_channel(x[c, 90:], x[c, :90], taps, L, M, d)
        assert second[c].tolist() == y2 and d2 == m.d


def test_model_masks_behind_n_pcm_like_the_integer_loop():
    L, M = 3, 2
    taps = taps_for(L, 100, 5)
    x = np.random.default_rng(2).integers(-32768, 32768, size=(2, 1024), dtype=np.int16)
    n_pcm = np.array([[512, 7], [0, 0xFFFFFFFF]], dtype=np.uint32)
    m = rm.ResampModel(2, L, M)
    m.set_taps(taps)
    got = m.process(x, n_pcm)
    nxt = m.process(x[:, :50])
    xm = rm.masked(x, n_pcm)
    assert (xm[0, 512 + 7:] == 0).all() and (xm[1, :512] == 0).all() and (xm[0, :519] == x[0, :519]).all() and (xm[1, 512:] == x[1, 512:]).all()
    for c in range(2):
        y, d = rm.slow_channel(xm[c], [], taps, L, M, 0)
        assert got[c].tolist() == y
        assert nxt[c].tolist() == rm.slow_channel(x[c, :50], xm[c], taps, L, M, d)[0]


@pytest.mark.parametrize("L,M", RATIOS)
def test_one_call_equals_the_same_samples_cut_into_calls(L, M):
    n = 700
    cuts = CUTS + ([n - sum(CUTS)] if n > sum(CUTS) else [])
    taps = taps_for(L, 30, L + M)
    x = np.random.default_rng(3).integers(-32768, 32768, size=(3, n), dtype=np.int16)
    whole, parts = rm.ResampModel(3, L, M), rm.ResampModel(3, L, M)
    for m in (whole, parts):
        m.set_taps(taps)
    out = whole.process(x)
    assert out.shape[1] == -(-n * L // M)
    at, got, empty = 0, [], 0
    for k in cuts:
        count = parts.out_count(k)
        y = parts.process(x[:, at:at + k])
        assert y.shape[1] == count                         # out_count against the produced count
        empty += count == 0
        got.append(y)
        at += k
    assert (np.concatenate(got, axis=1) == out).all() and parts.d == whole.d
    if L == 1 and M > 1 or 2 * L <= M:
        assert empty > 0                                   # calls without output were among them


def test_out_count_and_phase_law():
    for L, M in RATIOS + [(147, 160), (1, 8), (512, 1)]:
        for d in sorted({0, 1, M // 2, M - 1}):
            if d >= M:
                continue
            for n in (1, 2, 3, 5, 8, 511, 512, 513, 524288):
                count = rm.out_count(n, L, M, d)
                js = [j for j in range(max(0, count - 2), count + 2) if d + j * M < n * L]      # the outputs whose i lies inside the call
                assert count == (js[-1] + 1 if js else 0)
                assert 0 <= d + count * M - n * L < M


# the helper's promise with 8 kS/s as the lower rate: +-0.05 dB up to 3.4 kHz, 60 dB down from 4.6 kHz on
@pytest.mark.parametrize("L,M,K", [(6, 1, 40), (1, 6, 240), (441, 80, 36), (80, 441, 200)])
def test_resample_taps_keep_their_promise(L, M, K):
    h = api.resample_taps(L, M, K)
    T = h.size
    assert h.dtype == np.int16 and T % 2 == 1 and T in (L * K, L * K - 1) and (h == h[::-1]).all()
    rate = 8000.0 * max(L, M)                              # the prototype rate
    N = 1 << 20
    H = np.abs(np.fft.rfft(h.astype(np.float64), N)) / (16384.0 * L)
    f = np.arange(H.size) * rate / N
    passband = 20 * np.log10(H[f <= 3400.0])
    stopband = 20 * np.log10(np.maximum(H[f >= 4600.0], 1e-12))
    branch = np.zeros(-(-T // L) * L, dtype=np.int64)
    branch[:T] = h
    worst = int(np.abs(branch.reshape(-1, L)).sum(axis=0).max())
    print(f"{L}/{M} K={K}: T={T} pass {passband.min():+.4f}..{passband.max():+.4f} dB, stop {stopband.max():.1f} dB, branch sum {worst}")
    assert np.abs(passband).max() <= 0.05
    assert stopband.max() <= -60.0
    assert worst <= 65535
    rm.ResampModel(1, L, M).set_taps(h)                    # and the model takes them


def test_resample_taps_refuses_what_no_handle_takes():
    for args in ((0, 1, 8), (1, 513, 8), (6, 1, 0), (6, 1, 513), (512, 1, 64), (1, 1, 1), (1, 1, 2)):
        with pytest.raises(ValueError):
            api.resample_taps(*args)


def test_a_sine_through_6_1_and_1_6_comes_back_delayed():
    """x: a 1 kHz sine at 8 kS/s, rounded to int16.  Up by 6 with T1 = 239 taps (a delay of 119 samples at 48 kS/s), down by 6
    with T2 = 243 taps (121 samples): 240 samples at 48 kS/s, 40 at 8 kS/s, a whole number.

    1. The two roundings.  Let u = sum h1 x, the first stage's sum before its rounding, in units of 2^-14.  The first stage
       gives y1 with |2^14 y1 - u| <= 2^13 (no saturation: |u| stays far below 2^29).  The second stage sums h2 over y1 where
       the unrounded cascade U = sum h2 u (units of 2^-28) sums it over u: the difference is at most 2^13 sum |h2|, and its
       own rounding adds at most 2^27.  So |2^28 y2 - U| <= 2^27 + 2^13 sum |h2|, about 1.5 LSB.  U is exact in int64.
    2. Itself, delayed.  Both filters are symmetric, so the cascade delays every component by exactly 40 samples and scales
       it by a real gain.  x has period 8 and odd symmetry: a 1 kHz and a 3 kHz component (the latter from its rounding,
       below 1 LSB), both inside the band where resample_taps promises +-0.05 dB per filter.  The images the first stage
       leaves at 8 k +- 1 kHz, .. are 60 dB down and meet 60 dB more in the second: below 10^-6 of the amplitude each, five of
       them per component.  So |y2[n] - x[n - 40]| <= the bound of 1. + A ((10^(0.05/20))^2 - 1) + 10 A 10^-6 + 1: the last
       1 LSB covers the 3 kHz component at twice its size."""
    A, n = 20000, 1024
    x = np.floor(A * np.sin(2 * np.pi * np.arange(n) / 8) + 0.5).astype(np.int16)[None, :]
    h1, h2 = api.resample_taps(6, 1, 40), api.resample_taps(1, 6, 243)
    assert h1.size == 239 and h2.size == 243
    up, down = rm.ResampModel(1, 6, 1), rm.ResampModel(1, 1, 6)
    up.set_taps(h1)
    down.set_taps(h2)
    y1 = up.process(x)
    y2 = down.process(y1)
    assert y1.shape == (1, 6 * n) and y2.shape == (1, n)
    # 1. against the unrounded cascade in integers
    z = np.zeros(6 * n, dtype=np.int64)
    z[::6] = x[0]
    u = np.convolve(z, h1.astype(np.int64))[:6 * n]
    U = np.convolve(u, h2.astype(np.int64))[:6 * n:6]
    bound = (1 << 27) + (1 << 13) * int(np.abs(h2.astype(np.int64)).sum())
    err = np.abs((y2[0].astype(np.int64) << 28) - U)
    print(f"two roundings: worst {err.max() / 2.0 ** 28:.3f} LSB, bound {bound / 2.0 ** 28:.3f} LSB")
    assert err.max() <= bound
    # 2. against the input, 40 samples late (behind the 2 x 40 samples in which the filters fill)
    tol = bound / 2.0 ** 28 + A * ((10 ** (0.05 / 20)) ** 2 - 1) + 10 * A * 1e-6 + 1
    late = np.abs(y2[0, 120:].astype(np.int64) - x[0, 80:n - 40])
    print(f"itself delayed: worst {late.max()} LSB, bound {tol:.1f} LSB")
    assert late.max() <= tol
