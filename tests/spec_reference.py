"""An independent statement of the spectrum bank's contract, structured differently from tests/spec_model.py, plus float64.

The transform is recursive: one decimation-in-frequency stage splits a block into its even outputs (the transform of the
halved sums) and its odd outputs (the transform of the halved, rotated differences), so the results come out in natural
order with no in-place stages and no bit-reversal table.  Plain Python integers for the butterflies' roundings (floor
division and math.floor instead of shifts), band sums from a cumulative sum."""
import math

import numpy as np


def _tables(N):
    c = [int(math.floor(32767 * math.cos(2 * math.pi * k / N) + 0.5)) for k in range(N // 2)]
    s = [int(math.floor(32767 * math.sin(2 * math.pi * k / N) + 0.5)) for k in range(N // 2)]
    return c, s


def hann(N):
    return [int(math.floor(32767 * 0.5 * (1 - math.cos(2 * math.pi * n / N)) + 0.5)) for n in range(N)]


def _dif(re, im, c, s, N):
    """natural-order outputs of the halving DIF transform of one block (numpy int64 columns, any leading shape)"""
    n = re.shape[-1]
    if n == 1:
        return re, im
    h = n // 2
    step = N // n
    cc = np.array([c[j * step] for j in range(h)], dtype=np.int64)
    ss = np.array([s[j * step] for j in range(h)], dtype=np.int64)
    a_re, a_im, b_re, b_im = re[..., :h], im[..., :h], re[..., h:], im[..., h:]
    up = 1 if (N // n).bit_length() % 2 == 1 else 0                  # blocks of N, N / 4, N / 16, ..: halves round up
    e_re, e_im = np.floor_divide(a_re + b_re + up, 2), np.floor_divide(a_im + b_im + up, 2)
    d_re, d_im = np.floor_divide(a_re - b_re + up, 2), np.floor_divide(a_im - b_im + up, 2)
    o_re = np.floor_divide(d_re * cc + d_im * ss + 16384, 32768)
    o_im = np.floor_divide(d_im * cc - d_re * ss + 16384, 32768)
    even = _dif(e_re, e_im, c, s, N)
    odd = _dif(o_re, o_im, c, s, N)
    out_re, out_im = np.empty_like(re), np.empty_like(im)
    out_re[..., 0::2], out_im[..., 0::2] = even
    out_re[..., 1::2], out_im[..., 1::2] = odd
    return out_re, out_im


def spectrum(captures, n_captures, log2_n, n_frames, window=None):
    """captures int8 [W, 2 N n_frames] -> ((re, im) int64 [W, n_frames, N] in natural order, power as Python ints [W][N])"""
    N = 1 << log2_n
    w = np.array(hann(N) if window is None else [int(v) for v in window], dtype=np.int64)
    x = np.asarray(captures, dtype=np.int8).astype(np.int64).reshape(n_captures, n_frames, N, 2)
    re = np.floor_divide(x[..., 0] * w + 128, 256)
    im = np.floor_divide(x[..., 1] * w + 128, 256)
    c, s = _tables(N)
    X_re, X_im = _dif(re, im, c, s, N)
    power = [[sum(int(X_re[cap, f, k]) ** 2 + int(X_im[cap, f, k]) ** 2 for f in range(n_frames)) for k in range(N)]
             for cap in range(n_captures)]
    return (X_re, X_im), power


def bands(power, N, band_list, n_frames):
    """[(band_power, present)] from a cumulative sum over the doubled row"""
    out = []
    for capture, first, n_bins, thr in band_list:
        cum = [0]
        for v in power[capture] + power[capture]:
            cum.append(cum[-1] + v)
        bp = cum[first + n_bins] - cum[first]
        out.append((bp, 1 if bp >= thr * n_frames else 0))
    return out


def float_spectrum(captures, n_captures, log2_n, n_frames, window=None):
    """float64: np.fft.fft(x * w / 256) / N per frame, complex [W, n_frames, N]"""
    N = 1 << log2_n
    w = np.array(hann(N) if window is None else window, dtype=np.float64)
    x = np.asarray(captures, dtype=np.int8).astype(np.float64).reshape(n_captures, n_frames, N, 2)
    u = (x[..., 0] + 1j * x[..., 1]) * w / 256.0
    return np.fft.fft(u, axis=-1) / N
