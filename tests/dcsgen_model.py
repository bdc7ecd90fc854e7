"""The DCS generator bank's contract (include/hrfd.h, "DCS generator bank") restated in numpy and Python integers: the bit grid
and the turn-off grid over u = n mod 28750, the raw level of a segment, the shaping filter with its rounding, the saturating
sum, the active bytes, and the rules of a channel's queue (queue, cut with and without the tail, what has ended).  Integers
throughout, shifts arithmetic; nothing here is taken from the library."""
import numpy as np

BLOCK = 512
PERIOD = 28750                     # 23 * 1250 samples = 483 bit times
REACH = 511                        # a segment has ended when E + 511 <= N
MAX_SEGMENTS = 8
MAX_TAPS = 512
FOREVER = 0xFFFFFFFF
APPEND = 0xFFFFFFFFFFFFFFFF
NO_END = 0xFFFFFFFFFFFFFFFF
MAX_TIME = 1 << 63
DEFAULT_TAIL = 1440


class Refused(Exception):
    pass


def bit_index(u):
    return (21 * u // 1250) % 23


def sq_sign(u):
    """+1 in the first half of a bit time, -1 in the second"""
    return 1 - 2 * ((42 * u // 1250) & 1)


def raw_levels(segs, t0, n):
    """r at the stream times t0 .. t0 + n - 1 (t0 may be negative: 0 in front of the stream's start) as int64; segs: rows
    [start, mid, end, word, amp, tail]"""
    r = np.zeros(n, dtype=np.int64)
    u = (int(t0) % PERIOD + np.arange(n, dtype=np.int64)) % PERIOD
    for start, mid, end, word, amp, _ in segs:
        lo, m, hi = (min(max(v - t0, 0), n) for v in (start, mid, end))
        if lo < m:
            r[lo:m] = amp * (2 * ((word >> bit_index(u[lo:m])) & 1) - 1)
        if max(m, lo) < hi:
            k = max(m, lo)
            r[k:hi] = amp * sq_sign(u[k:hi])
    return r


def ended(seg, N):
    return seg[2] != NO_END and seg[2] + REACH <= N


class Queue:
    """one channel's queue: rows [start, mid, end, word, amp, tail] in order of their starts"""

    def __init__(self):
        self.segs = []

    def drop_ended(self, N):
        self.segs = [s for s in self.segs if not ended(s, N)]

    def lay_out(self, N, segs, start):
        """the queue as hrfd_dcsgen_queue would leave it, or Refused"""
        if not 1 <= len(segs) <= MAX_SEGMENTS:
            raise Refused("segments")
        for i, (gap, length, tail, word, amp) in enumerate(segs):
            if amp > 32767 or word > 0x7FFFFF or length == 0 or tail == 0xFFFFFFFF or (length == FOREVER and i + 1 < len(segs)):
                raise Refused("segment")
        if start != APPEND and start >= MAX_TIME:
            raise Refused("time")
        merged = [s for s in self.segs if not ended(s, N)]
        if start == APPEND:
            end = merged[-1][2] if merged else 0
            if end == NO_END:
                raise Refused("behind FOREVER")
            at = max(end, N)
        else:
            if start < N:
                raise Refused("before N")
            at = start
        for gap, length, tail, word, amp in segs:
            forever = length == FOREVER
            s = at + gap
            mid = NO_END if forever else s + length
            end = NO_END if forever else mid + tail
            if at >= MAX_TIME or s >= MAX_TIME or (not forever and end >= MAX_TIME):
                raise Refused("2^63")
            merged.append([s, mid, end, word, amp, tail])
            at = end
        merged.sort(key=lambda s: s[0])            # stable
        for a, b in zip(merged, merged[1:]):
            if a[2] == NO_END or a[2] > b[0]:
                raise Refused("overlap")
        if len(merged) > MAX_SEGMENTS:
            raise Refused("ninth")
        return merged

    def cut(self, N, with_tail):
        self.drop_ended(N)
        out = []
        for s in self.segs:
            start, mid, end, word, amp, tail = s
            if start >= N:
                continue                           # not yet begun, or beginning now
            if N < mid:
                mid, end = N, min(N + (tail if with_tail else 0), MAX_TIME - 1)
            elif N < end and not with_tail:
                end = N
            out.append([start, mid, end, word, amp, tail])
        self.segs = out


class DcsGenModel:
    """hrfd_dcsgen_* for C channels"""

    def __init__(self, n_channels):
        self.C = int(n_channels)
        self.taps = np.array([16384], dtype=np.int64)
        self.reset()

    def reset(self):
        self.N = 0
        self.q = [Queue() for _ in range(self.C)]
        self.clips = np.zeros(self.C, dtype=np.int64)

    def set_taps(self, taps):
        h = np.asarray(taps, dtype=np.int64).ravel()
        if not 1 <= h.size <= MAX_TAPS or np.abs(h).sum() > 65535:
            raise Refused("taps")
        self.taps = h

    def set_time(self, N):
        if N >= MAX_TIME:
            raise Refused("time")
        self.N = int(N)

    def _channels(self, channel):
        return range(self.C) if channel == 0xFFFFFFFF else [channel]

    def queue(self, channel, segs, start=APPEND):
        segs = [tuple(int(v) for v in s) for s in segs]
        merged = [self.q[c].lay_out(self.N, segs, start) for c in self._channels(channel)]      # refused whole
        for c, m in zip(self._channels(channel), merged):
            self.q[c].segs = m

    def cut(self, channel=0xFFFFFFFF, with_tail=True):
        for c in self._channels(channel):
            self.q[c].cut(self.N, with_tail)

    def pending(self, channel):
        live = [s for s in self.q[channel].segs if not ended(s, self.N)]
        return len(live), (live[-1][2] if live else self.N)

    def process(self, pcm, n_blocks=None, want_active=False):
        """pcm [C, n_blocks, 512] or None with n_blocks -> out int16 [C, n_blocks, 512] (and active uint8 [C, n_blocks])"""
        if pcm is not None:
            x = np.asarray(pcm, dtype=np.int64).reshape(self.C, -1)
            n_blocks = x.shape[1] // BLOCK
        n = BLOCK * n_blocks
        if self.N + n - 1 >= MAX_TIME:
            raise Refused("time")
        T = self.taps.size
        out = np.zeros((self.C, n), dtype=np.int64)
        active = np.zeros((self.C, n_blocks), dtype=np.uint8)
        for c in range(self.C):
            self.q[c].drop_ended(self.N)
            segs = self.q[c].segs
            if segs:
                r = raw_levels(segs, self.N - REACH, REACH + n)
                acc = np.convolve(r, self.taps)[REACH:REACH + n]
                assert np.abs(acc).max(initial=0) + (1 << 13) < (1 << 31)
                g = (acc + (1 << 13)) >> 14
            else:
                g = np.zeros(n, dtype=np.int64)
            s = g + (x[c] if pcm is not None else 0)
            y = np.clip(s, -32768, 32767)
            self.clips[c] += int((y != s).sum())
            out[c] = y
            for b in range(n_blocks):
                b0 = self.N + BLOCK * b
                active[c, b] = any(st < b0 + BLOCK and (e == NO_END or e + T - 1 > b0) for st, _, e, _, _, _ in segs)
        self.N += n
        out = out.astype(np.int16).reshape(self.C, n_blocks, BLOCK)
        return (out, active) if want_active else out
