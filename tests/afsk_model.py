"""The AFSK bank's contract (include/hrfd.h at "AFSK bank") restated in numpy, and the signals its tests decode.

AfskModel is written from the contract's text: taps from the DDC_COS table, four sliding dot products, powers in 64 bits, a
hard decision per sample, and the bit clock as the four numbered steps, one sample at a time over all channels at once.  It
keeps per channel what the contract calls the state: the last W - 1 samples, phi, h[n-1] and last.

The signal source is floating point and seeded: hdlc_bits (flags, bit stuffing, LSB first, CRC-16/X.25), nrzi_levels, and
afsk_signal, a continuous-phase two-tone generator with a sub-sample start, silence in front and Gaussian noise."""
import numpy as np

from hackrfdiags_amd import api

FS = 8000
BLOCK = 512
M32 = (1 << 32) - 1
BELL202 = dict(mark_hz=1200, space_hz=2200, baud=1200, window=8, loop_shift=2)
BELL103 = dict(mark_hz=1270, space_hz=1070, baud=300, window=27, loop_shift=2)

_COS = None


def cos_table():
    global _COS
    if _COS is None:
        _COS = api.q15_table("DDC_COS").astype(np.int64)
        assert _COS.size == 4096
    return _COS


def step(hz):
    return int(round(float(hz) / FS * 2.0 ** 32))


def taps(mark_step, space_step, W):
    """[4, W] int64: C_mark, S_mark, C_space, S_space"""
    cos = cos_table()
    k = np.arange(W, dtype=np.int64)
    out = []
    for s in (mark_step, space_step):
        i = ((((s * k) & M32) + (1 << 19)) >> 20) & 4095
        out.append(np.clip((cos[i] + 8) >> 4, -2047, 2047))
        out.append(np.clip((cos[(i - 1024) & 4095] + 8) >> 4, -2047, 2047))
    return np.stack(out)


def max_bits(baud_step, A, n_blocks):
    return ((BLOCK * n_blocks * (baud_step + ((1 << 31) >> A))) >> 32) + 1


def masked(pcm, n_pcm):
    """x of the contract: [C, n_blocks, 512] int64, 0 behind min(n_pcm, 512) of every block"""
    x = np.asarray(pcm).astype(np.int64).reshape(pcm.shape[0], -1, BLOCK).copy()
    if n_pcm is not None:
        lim = np.minimum(np.asarray(n_pcm).astype(np.int64).reshape(x.shape[0], x.shape[1]), BLOCK)
        x[np.arange(BLOCK)[None, None, :] >= lim[:, :, None]] = 0
    return x


def pack_hard(h):
    """[C, n] of 0 / 1 -> uint8 [C, n / 8]: bit n & 7 of byte n >> 3"""
    return np.packbits(h.astype(np.uint8), axis=1, bitorder="little")


def unpack_hard(hard):
    """uint8 [C, n_blocks, 64] -> [C, 512 n_blocks] of 0 / 1"""
    return np.unpackbits(np.asarray(hard, dtype=np.uint8).reshape(hard.shape[0], -1), axis=1, bitorder="little")


class AfskModel:
    def __init__(self, n_channels, mark_hz=1200, space_hz=2200, baud=1200, window=8, loop_shift=2, nrzi=True, steps=None):
        self.C = int(n_channels)
        self.min_power = 0
        self.max_abs_i = 0                      # the largest |I| or |Q| seen: the int32 bound
        self.max_power = 0                      # the largest P seen: the 64-bit bound
        self.set_modem(mark_hz, space_hz, baud, window, loop_shift, nrzi, steps)

    def set_modem(self, mark_hz=1200, space_hz=2200, baud=1200, window=8, loop_shift=2, nrzi=True, steps=None):
        m, s, b = steps if steps is not None else (step(mark_hz), step(space_hz), step(baud))
        assert 1 <= m <= 1 << 31 and 1 <= s <= 1 << 31 and 1 <= b <= 1 << 31 and 2 <= window <= 32 and 1 <= loop_shift <= 8
        self.mark_step, self.space_step, self.baud_step, self.W, self.A, self.nrzi = m, s, b, int(window), int(loop_shift), bool(nrzi)
        self.taps = taps(m, s, self.W)
        self.hist = np.zeros((self.C, self.W - 1), dtype=np.int64)
        self.phi = np.zeros(self.C, dtype=np.int64)
        self.h_prev = np.zeros(self.C, dtype=np.int64)
        self.last = np.zeros(self.C, dtype=np.int64)

    def set_carrier(self, min_power):
        self.min_power = int(min_power)

    def reset(self, channel=None):
        sel = slice(None) if channel is None else channel
        self.hist[sel] = 0
        self.phi[sel] = 0
        self.h_prev[sel] = 0
        self.last[sel] = 0

    def max_bits(self, n_blocks):
        return max_bits(self.baud_step, self.A, n_blocks)

    def discriminate(self, pcm, n_pcm=None):
        """the dense half: (h, carrier) [C, n] of 0 / 1; moves the sample history on"""
        x = masked(pcm, n_pcm).reshape(self.C, -1)
        n, W = x.shape[1], self.W
        xx = np.concatenate([self.hist, x], axis=1)
        acc = np.zeros((4, self.C, n), dtype=np.int64)
        for k in range(W):
            acc += self.taps[:, k][:, None, None] * xx[None, :, W - 1 - k:W - 1 - k + n]
        self.max_abs_i = max(self.max_abs_i, int(np.abs(acc).max()))
        assert self.max_abs_i < 1 << 31
        p_mark = acc[0] * acc[0] + acc[1] * acc[1]             # each square < 2^62, the sum < 2^63: exact in int64
        p_space = acc[2] * acc[2] + acc[3] * acc[3]
        self.max_power = max(self.max_power, int(p_mark.max()), int(p_space.max()))
        h = (p_mark - p_space > 0).astype(np.int64)
        self.total_power = p_mark.astype(np.uint64) + p_space.astype(np.uint64)      # of the last call, [C, n]
        carrier = (self.total_power > np.uint64(self.min_power)).astype(np.int64)
        self.hist = xx[:, n:].copy()
        return h, carrier

    def process(self, pcm, n_pcm=None, want_bits=True):
        """pcm [C, n_blocks, 512] -> (bits: a list of C uint8 arrays, or None; hard uint8 [C, n_blocks, 64])"""
        pcm = np.asarray(pcm).reshape(self.C, -1, BLOCK)
        n_blocks = pcm.shape[1]
        h, carrier = self.discriminate(pcm, n_pcm)
        hard = pack_hard(h).reshape(self.C, n_blocks, BLOCK // 8)
        if not want_bits:                                      # the clock does not run: phi and last stay
            self.h_prev = h[:, -1].copy()
            return None, hard
        cap = self.max_bits(n_blocks)
        rows = np.zeros((self.C, cap + 1), dtype=np.uint8)
        count = np.zeros(self.C, dtype=np.int64)
        phi, h_prev, last = self.phi, self.h_prev, self.last
        every = np.arange(self.C)
        for n in range(h.shape[1]):
            hn = h[:, n]
            new = (phi + self.baud_step) & M32                 # 1.
            wrap = new < phi                                   # 2.
            if wrap.any():
                value = 1 - (hn ^ last) if self.nrzi else hn
                w = every[wrap]
                assert (count[w] < cap).all(), "more bits than hrfd_afsk_max_bits"
                rows[w, count[w]] = (value | (carrier[:, n] << 1))[w]
                count[w] += 1
                if self.nrzi:
                    last = np.where(wrap, hn, last)
            new = np.where(hn != h_prev, new - ((new - (1 << 31)) >> self.A), new)      # 3.
            phi, h_prev = new, hn                              # 4.
        assert (phi >= 0).all() and (phi <= M32).all()
        self.phi, self.h_prev, self.last = phi, h_prev.copy(), last
        return [rows[c, :count[c]].copy() for c in range(self.C)], hard


# ---- the signal source
def hdlc_bits(payloads, n_lead_flags=12, n_between=2, n_tail_flags=3):
    """the bit stream of HDLC frames: flags, then per frame payload + CRC-16/X.25 (low byte first), LSB first, a zero stuffed
    behind five ones, flags between and behind"""
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    out = flag * n_lead_flags
    for i, p in enumerate(payloads):
        crc = api.crc16_x25(p)
        body = np.unpackbits(np.frombuffer(bytes(p) + bytes([crc & 255, crc >> 8]), dtype=np.uint8), bitorder="little").tolist()
        ones = 0
        for b in body:
            out.append(b)
            ones = ones + 1 if b else 0
            if ones == 5:
                out.append(0)
                ones = 0
        out += flag * (n_between if i + 1 < len(payloads) else n_tail_flags)
    return np.array(out, dtype=np.uint8)


def nrzi_levels(bits, start=1):
    """NRZI: a 0 toggles the level, a 1 keeps it"""
    toggles = np.cumsum(1 - np.asarray(bits, dtype=np.int64))
    return ((start + toggles) & 1).astype(np.uint8)


def afsk_signal(levels, rng, mark_hz=1200, space_hz=2200, baud=1200, amplitude=8000, sigma=0.0, max_silence=300, tail=64):
    """levels (1 = mark) as continuous-phase AFSK at 8 kS/s: int16 [n_blocks, 512].  A random sub-sample start, up to
    max_silence samples of silence in front, Gaussian noise of sigma over everything, zeros up to whole blocks"""
    spb = FS / float(baud)
    silence = int(rng.integers(0, max_silence + 1))
    frac = float(rng.random())
    n_sig = int(np.ceil(len(levels) * spb)) + tail
    t = np.arange(n_sig) + frac
    idx = np.minimum((t / spb).astype(np.int64), len(levels) - 1)
    f = np.where(np.asarray(levels)[idx] != 0, float(mark_hz), float(space_hz))
    phase = 2.0 * np.pi * np.cumsum(f) / FS + 2.0 * np.pi * float(rng.random())
    n_blocks = -(-(silence + n_sig) // BLOCK)
    x = np.zeros(n_blocks * BLOCK)
    x[silence:silence + n_sig] = amplitude * np.cos(phase)
    if sigma:
        x += rng.normal(0.0, sigma, size=x.size)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16).reshape(n_blocks, BLOCK)


def noisy_afsk(rng, modem, n_blocks):
    """random data on the modem's tones at a random level, with noise and a stretch of silence: [n_blocks, 512]"""
    levels = rng.integers(0, 2, size=int(n_blocks * 512 * modem["baud"] / 8000) + 2)
    x = afsk_signal(levels, rng, modem["mark_hz"], modem["space_hz"], modem["baud"], amplitude=int(rng.choice([300, 8000, 32000])),
                       sigma=float(rng.choice([0.0, 500.0])), max_silence=200).reshape(-1)[:n_blocks * 512].copy()
    at = int(rng.integers(0, x.size - 100))
    x[at:at + 100] = 0                                       # d = 0: h must be 0 there, not "as before"
    return x.reshape(n_blocks, 512)


def random_payloads(rng, n_frames=1, n_bytes=40):
    return [rng.integers(0, 256, size=n_bytes, dtype=np.uint8).tobytes() for _ in range(n_frames)]


# the end-to-end cases of the issue: (name, modem, amplitude, sigma); every one with frames of 40 random bytes
E2E_CASES = [("bell202-clean", BELL202, 8000, 0.0), ("bell202-noise", BELL202, 8000, 500.0), ("bell202-weak", BELL202, 300, 0.0),
             ("bell103-clean", BELL103, 8000, 0.0), ("bell103-noise", BELL103, 8000, 500.0), ("bell103-weak", BELL103, 300, 0.0)]
E2E_SEEDS = (1, 2, 3)


def e2e_signal(modem, amplitude, sigma, seed, n_frames=1):
    """(payloads, pcm int16 [n_blocks, 512]) of one end-to-end case"""
    rng = np.random.default_rng(seed)
    payloads = random_payloads(rng, n_frames)
    levels = nrzi_levels(hdlc_bits(payloads))
    pcm = afsk_signal(levels, rng, modem["mark_hz"], modem["space_hz"], modem["baud"], amplitude, sigma)
    return payloads, pcm
