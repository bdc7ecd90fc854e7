"""The spectrum bank's contract (include/hrfd.h, hrfd_spec_*) line by line in int64 numpy.

window -> L in-place radix-2 decimation-in-frequency stages with a halving each -> power per bin, summed over the call's
frames, in natural bin order -> band sums and verdicts.  Every call asserts the invariants the contract states: components
inside int16, product sums inside int32, power terms below 2^30, sums inside uint64.  `stage_max` keeps the largest complex
magnitude squared seen after the window and after every stage, so a test can prove which edge its input reached."""
import numpy as np

FS_CH = 2_048_000
MIN_L, MAX_L = 8, 13
MAX_FRAMES = 65536
MAX_BANDS = 65536
MAX_THRESHOLD = 1 << 44
MAG2_LIMIT = 23171 ** 2            # the window leaves |u| <= 16384 per rail: |z|^2 <= 2 * 16384^2 < 23171^2


def hann(L):
    N = 1 << L
    return np.round(32767 * 0.5 * (1 - np.cos(2 * np.pi * np.arange(N) / N))).astype(np.int16)


def cos_sin(L):
    N = 1 << L
    a = 2 * np.pi * np.arange(N // 2) / N
    return np.round(32767 * np.cos(a)).astype(np.int64), np.round(32767 * np.sin(a)).astype(np.int64)


def bitrev(L):
    i = np.arange(1 << L)
    r = np.zeros_like(i)
    for b in range(L):
        r |= ((i >> b) & 1) << (L - 1 - b)
    return r


class SpecModel:
    def __init__(self, n_captures, decimation, log2_n):
        assert n_captures >= 1 and decimation in (1, 2, 4, 8) and MIN_L <= log2_n <= MAX_L
        self.W, self.R, self.L, self.N = n_captures, decimation, log2_n, 1 << log2_n
        self.window = hann(log2_n).astype(np.int64)
        self.c, self.s = cos_sin(log2_n)
        self.rev = bitrev(log2_n)
        self.bands = []
        self.stage_max = []          # max |z|^2 after the window and after each stage, of the last call
        self.max_term = 0            # the largest per-frame power term of the last call

    def set_window(self, w):
        w = np.asarray(w)
        assert w.shape == (self.N,) and w.min() >= -32768 and w.max() <= 32767
        self.window = w.astype(np.int64)

    def set_band(self, band, capture, first_bin, n_bins, threshold):
        assert 0 <= capture < self.W and 0 <= first_bin < self.N and 1 <= n_bins <= self.N
        assert 0 <= threshold <= MAX_THRESHOLD and band <= len(self.bands) and band < MAX_BANDS
        b = (capture, first_bin, n_bins, int(threshold))
        if band == len(self.bands):
            self.bands.append(b)
        else:
            self.bands[band] = b

    def clear_bands(self):
        self.bands = []

    def _note(self, re, im):
        m = int((re * re + im * im).max())
        assert m <= MAG2_LIMIT, f"the complex magnitude grew: {m} > {MAG2_LIMIT}"
        assert max(abs(int(re.min())), int(re.max()), abs(int(im.min())), int(im.max())) <= 32767
        self.stage_max.append(m)

    def transform(self, x):
        """x int8 [..., N, 2] -> (re, im) int64 [..., N] in bit-reversed order (position i holds X[rev[i]])"""
        N, L = self.N, self.L
        x = np.asarray(x, dtype=np.int64)
        re = (x[..., 0] * self.window + 128) >> 8
        im = (x[..., 1] * self.window + 128) >> 8
        assert np.abs(re).max() <= 16384 and np.abs(im).max() <= 16384
        self.stage_max = []
        self._note(re, im)
        i = np.arange(N)
        for t in range(L):
            span = N >> t
            h = span // 2
            ia = i[(i % span) < h]
            ib = ia + h
            k = (ia % span) * (N // span)
            c, s = self.c[k], self.s[k]
            ar, ai, br, bi = re[..., ia], im[..., ia], re[..., ib], im[..., ib]
            r = 1 - (t & 1)                                          # the even stages round up, the odd ones down
            dr, di = (ar - br + r) >> 1, (ai - bi + r) >> 1
            p_re, p_im = dr * c + di * s + (1 << 14), di * c - dr * s + (1 << 14)
            assert max(np.abs(p_re).max(), np.abs(p_im).max()) < 2 ** 31
            re, im = re.copy(), im.copy()
            re[..., ia], im[..., ia] = (ar + br + r) >> 1, (ai + bi + r) >> 1
            re[..., ib], im[..., ib] = p_re >> 15, p_im >> 15
            self._note(re, im)
        return re, im

    def process(self, captures, n_frames):
        """captures int8 [W, 2 N n_frames] -> (power uint64 [W, N], band_power uint64 [K], present uint8 [K])"""
        assert 1 <= n_frames <= MAX_FRAMES
        x = np.asarray(captures, dtype=np.int8).reshape(self.W, n_frames, self.N, 2)
        re, im = self.transform(x)
        p = re * re + im * im
        self.max_term = int(p.max())
        assert self.max_term < 2 ** 30
        total = np.zeros((self.W, self.N), dtype=np.uint64)
        acc = p.sum(axis=1)                                          # int64: n_frames 2^30 <= 2^46
        total[:, self.rev] = acc.astype(np.uint64)
        K = len(self.bands)
        band_power, present = np.zeros(K, dtype=np.uint64), np.zeros(K, dtype=np.uint8)
        for b, (w, first, n_bins, thr) in enumerate(self.bands):
            bp = sum(int(v) for v in total[w, (first + np.arange(n_bins)) % self.N])
            assert bp < 2 ** 64 and thr * n_frames < 2 ** 64
            band_power[b] = bp
            present[b] = 1 if bp >= thr * n_frames else 0
        return total, band_power, present


def lcg_captures(W, n_bytes, seed):
    """LCG bytes with runs of -128 and of +127 / -128 alternation, so that the window and the butterflies reach their edges"""
    a = np.arange(W * n_bytes, dtype=np.uint64)
    s = np.uint64(seed * 2654435761 + 12345)
    x = ((a * np.uint64(1103515245) + s) * np.uint64(2862933555777941757) >> np.uint64(40)).astype(np.uint32)
    cap = (x & 0xFF).astype(np.uint8).view(np.int8).reshape(W, n_bytes).copy()
    for w in range(W):
        o = (seed * 977 + w * 4001) % max(1, n_bytes - 3000)
        cap[w, o:o + 1200] = -128
        cap[w, o + 1500:o + 2700:2] = 127
        cap[w, o + 1501:o + 2700:2] = -128
    return cap
