"""The conditioner bank's contract (include/hrfd.h, hrfd_cal_*) line by line in int64 numpy, the solver in float64.

record -> apply (Q8 offset, 2 x 2 Q14 matrix, rounding shift by 22, sat8) -> moments of the raw input and the clip count.
Every call asserts what the contract states: every intermediate of the apply step inside int32.  `recipe_*` build the
capture of the effect tests (two stations, noise, a DC offset and an IQ imbalance) and the float spectrum they are judged
on; the device tests run the same capture through the bank."""
import numpy as np

MAX_BYTES = 1 << 30
MAX_DC = 32512
MAX_ROW = 32768
IDENTITY = (16384, 0, 0, 16384)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def record_ok(dc, m):
    dc, m = [int(v) for v in dc], [int(v) for v in m]
    return (all(abs(v) <= MAX_DC for v in dc) and all(-32768 <= v <= 32767 for v in m) and
            abs(m[0]) + abs(m[1]) <= MAX_ROW and abs(m[2]) + abs(m[3]) <= MAX_ROW)


def _in_int32(*arrays):
    for a in arrays:
        assert INT32_MIN <= int(a.min()) and int(a.max()) <= INT32_MAX, "an intermediate left int32"


def apply(x, dc=(0, 0), m=IDENTITY):
    """x int8 [..., n_bytes] (I, Q interleaved) -> (out int8 of the same shape, clips)"""
    assert record_ok(dc, m)
    x = np.asarray(x, dtype=np.int8)
    assert x.shape[-1] % 2 == 0 and 2 <= x.shape[-1] <= MAX_BYTES
    I, Q = x[..., 0::2].astype(np.int64), x[..., 1::2].astype(np.int64)
    xi, xq = (I << 8) - int(dc[0]), (Q << 8) - int(dc[1])
    m_ii, m_iq, m_qi, m_qq = [int(v) for v in m]
    a, b, c, d = m_ii * xi, m_iq * xq, m_qi * xi, m_qq * xq
    si, sq = a + b + (1 << 21), c + d + (1 << 21)
    _in_int32(xi, xq, a, b, c, d, a + b, c + d, si, sq)
    yi, yq = si >> 22, sq >> 22
    clips = int(((yi < -128) | (yi > 127)).sum() + ((yq < -128) | (yq > 127)).sum())
    out = np.empty(x.shape, dtype=np.int8)
    out[..., 0::2] = np.clip(yi, -128, 127)
    out[..., 1::2] = np.clip(yq, -128, 127)
    return out, clips


def moments(x, clips=0):
    """x int8 [n_bytes] -> int64 [8]: {n, S_I, S_Q, S_II, S_QQ, S_IQ, clips, 0} of the raw input"""
    x = np.asarray(x, dtype=np.int8)
    I, Q = x[0::2].astype(np.int64), x[1::2].astype(np.int64)
    return np.array([I.size, I.sum(), Q.sum(), (I * I).sum(), (Q * Q).sum(), (I * Q).sum(), clips, 0], dtype=np.int64)


def solve(mom):
    """hrfd_cal_solve in float64, operation by operation: (dc [2], m [4], solved)"""
    n_, s_i, s_q, s_ii, s_qq, s_iq = [int(v) for v in np.asarray(mom, dtype=np.int64)[:6]]
    dc, m = [0, 0], list(IDENTITY)
    if n_ <= 0:
        return dc, m, False
    f = np.float64
    n = f(n_)
    mi, mq = f(s_i) / n, f(s_q) / n
    vii = f(s_ii) / n - mi * mi
    vqq = f(s_qq) / n - mq * mq
    viq = f(s_iq) / n - mi * mq
    D = vii * vqq - viq * viq
    for k, mean in enumerate((mi, mq)):
        v = np.floor(mean * f(256.0) + f(0.5))
        dc[k] = int(min(max(v, -MAX_DC), MAX_DC))
    if not vii > 0.0 or not D > 0.0:
        return dc, m, False
    r = np.sqrt(D)
    qi = np.floor(((-viq) / r) * f(16384.0) + f(0.5))
    qq = np.floor((vii / r) * f(16384.0) + f(0.5))
    if not abs(qi) + abs(qq) <= MAX_ROW or qi > 32767.0 or qq > 32767.0:
        return dc, m, False
    m[2], m[3] = int(qi), int(qq)
    return dc, m, True


class CalModel:
    def __init__(self, n_captures):
        assert 1 <= n_captures <= 65536
        self.W = n_captures
        self.dc = [(0, 0)] * n_captures
        self.m = [IDENTITY] * n_captures

    def set_correction(self, dc=None, m=None, capture=None):
        dc = (0, 0) if dc is None else tuple(int(v) for v in dc)
        m = IDENTITY if m is None else tuple(int(v) for v in m)
        assert record_ok(dc, m)
        for w in range(self.W):
            if capture is None or w == capture:
                self.dc[w], self.m[w] = dc, m

    def process(self, captures, want_out=True, want_moments=True):
        """captures int8 [W, n_bytes] -> (out int8 [W, n_bytes] or None, moments int64 [W, 8] or None)"""
        assert want_out or want_moments
        cap = np.asarray(captures, dtype=np.int8).reshape(self.W, -1)
        out = np.zeros_like(cap) if want_out else None
        mom = np.zeros((self.W, 8), dtype=np.int64) if want_moments else None
        for w in range(self.W):
            clips = 0
            if want_out:
                out[w], clips = apply(cap[w], self.dc[w], self.m[w])
            if want_moments:
                mom[w] = moments(cap[w], clips)
        return out, mom


# ------------------------------------------------------------------ the effect recipe
RECIPE_N = 1 << 18
RECIPE_STATIONS = ((60.0, 0.21, 3.0, 1.0), (12.0, -0.09, 2.0, 2.0))      # (A, f, d, s)
RECIPE_NOISE = 1.5
RECIPE_DC = (2.3, -1.7)
RECIPE_GAIN, RECIPE_SKEW = 1.06, np.deg2rad(4.0)
RECIPE_R, RECIPE_L, RECIPE_FRAMES = 8, 11, 128
RECIPE_OFFSETS_HZ = (-1_474_560.0, 3_440_640.0)                          # f x 16.384 MHz, sorted


def recipe_float():
    """the clean capture before rounding: two stations and noise"""
    t = np.arange(RECIPE_N, dtype=np.float64)
    x = np.zeros(RECIPE_N, dtype=np.complex128)
    for A, f, d, s in RECIPE_STATIONS:
        x += A * np.exp(1j * (2 * np.pi * f * t + d * np.sin(2 * np.pi * t / 5000 + s)))
    rng = np.random.default_rng(1)
    re = rng.standard_normal(RECIPE_N)
    im = rng.standard_normal(RECIPE_N)
    return x + RECIPE_NOISE * (re + 1j * im)


def to_int8(I, Q):
    out = np.empty(2 * I.size, dtype=np.int8)
    out[0::2] = np.clip(np.round(I), -128, 127)
    out[1::2] = np.clip(np.round(Q), -128, 127)
    return out


def recipe_clean():
    x = recipe_float()
    return to_int8(x.real, x.imag)


def recipe_impaired():
    """I = Re x + 2.3, Q = 1.06 (Im x cos 4 deg + Re x sin 4 deg) - 1.7, rounded and clipped to int8"""
    x = recipe_float()
    return to_int8(x.real + RECIPE_DC[0],
                   RECIPE_GAIN * (x.imag * np.cos(RECIPE_SKEW) + x.real * np.sin(RECIPE_SKEW)) + RECIPE_DC[1])


def recipe_injection():
    """the record with which the bank itself impairs the clean int8 capture: y = M (x - dc) with M the recipe's matrix
    and dc = -M^-1 (2.3, -1.7), so that the offsets come out behind the matrix as in the recipe"""
    g, a = RECIPE_GAIN, RECIPE_SKEW
    m = (16384, 0, int(round(g * np.sin(a) * 16384)), int(round(g * np.cos(a) * 16384)))
    dc_i = -RECIPE_DC[0]
    dc_q = -(RECIPE_DC[1] - g * np.sin(a) * RECIPE_DC[0]) / (g * np.cos(a))
    return (int(round(dc_i * 256)), int(round(dc_q * 256))), m


def float_spectrum(cap, n_fft=8192):
    """float64 power per bin of int8 IQ, Hann-windowed frames of n_fft samples, summed over the frames; natural FFT order"""
    z = cap[0::2].astype(np.float64) + 1j * cap[1::2].astype(np.float64)
    frames = z[:z.size // n_fft * n_fft].reshape(-1, n_fft) * np.hanning(n_fft)
    return (np.abs(np.fft.fft(frames, axis=1)) ** 2).sum(axis=0)


def band_power(spectrum, centre, half_width):
    """the power of the bins within half_width of centre (both as fractions of the rate, circular)"""
    f = np.fft.fftfreq(spectrum.size)
    d = np.abs((f - centre + 0.5) % 1.0 - 0.5)
    return float(spectrum[d <= half_width].sum())


def db(a, b):
    return 10 * np.log10(a / b)
