"""numpy model of the tone generator bank (hrfd_tonegen_*, include/hrfd.h): int64 arithmetic over the samples, Python integers
for every stream time, the contract line by line.  It takes the calls of api.ToneGen (a refusal raises ValueError).  The GPU
tests compare the library with it bit for bit; tests/test_tonegen_model.py compares it with a sample-by-sample restatement in
Python integers."""
from __future__ import annotations

import numpy as np

from hackrfdiags_amd import api
from tests.ddc_model import COS

BLOCK = 512
TRACKS = 2
MAX_SEGMENTS = 32
MAX_BLOCKS = 1024
MAX_AMP = 32767
RAMP = 64
FOREVER = 0xFFFFFFFF
APPEND = (1 << 64) - 1
NO_END = (1 << 64) - 1
MAX_TIME = 1 << 63
MASK32 = (1 << 32) - 1
ALL = 0xFFFFFFFF
FAR = 1 << 40                               # a ramp term this large is as good as infinite


class Slot:
    """one queued segment: it sounds at stream times start <= n < end (NO_END: no end)"""
    __slots__ = ("start", "end", "step_a", "step_b", "amp_a", "amp_b")

    def __init__(self, start, end, step_a, step_b, amp_a, amp_b):
        self.start, self.end, self.step_a, self.step_b, self.amp_a, self.amp_b = start, end, step_a, step_b, amp_a, amp_b

    def copy(self):
        return Slot(self.start, self.end, self.step_a, self.step_b, self.amp_a, self.amp_b)


def segment_span(slot: Slot, lo: int, hi: int):
    """g int64 of the stream times max(lo, start) .. min(hi, end) - 1, and the first of them; None where there is none"""
    a, b = max(lo, slot.start), min(hi, slot.end)
    if a >= b:
        return None, a
    i = np.arange(b - a, dtype=np.int64)
    k0 = a - slot.start                                      # a Python integer of any size
    S = []
    for step in (slot.step_a, slot.step_b):
        theta = (((step * k0) & MASK32) + step * i) & MASK32  # step i < 2^32 x 2^19
        idx = ((theta + (1 << 19)) >> 20) & 4095
        S.append(COS[(idx - 1024) & 4095])
    v = (slot.amp_a * S[0] + slot.amp_b * S[1] + (1 << 14)) >> 15
    up = min(k0 + 1, FAR) + i
    down = (FAR if slot.end == NO_END else min(slot.end - a, FAR)) - i
    e = np.minimum(np.minimum(up, down), RAMP)
    return (v * e + 32) >> 6, a


class ToneGenModel:
    def __init__(self, n_channels: int):
        self.C = int(n_channels)
        self.reset()

    n = property(lambda self: self.C)

    # ---- the queue rules
    def _selected(self, channel):
        if channel == ALL:
            return range(self.C)
        if not 0 <= channel < self.C:
            raise ValueError(f"channel {channel}")
        return [channel]

    def _lay_out(self, q, segs, start):
        merged = [s.copy() for s in q if s.end > self.N]
        if start == APPEND:
            end = merged[-1].end if merged else 0
            if end == NO_END:
                raise ValueError("nothing can be appended behind a FOREVER segment")
            at = max(end, self.N)
        else:
            if start < self.N:
                raise ValueError(f"start {start} lies before the stream time {self.N}")
            at = start
        for gap, length, step_a, step_b, amp_a, amp_b in segs:
            s = at + gap
            e = NO_END if length == FOREVER else s + length
            if at >= MAX_TIME or s >= MAX_TIME or (e != NO_END and e >= MAX_TIME):
                raise ValueError("a segment would lie at or above stream time 2^63")
            merged.append(Slot(s, e, step_a, step_b, amp_a, amp_b))
            at = e
        merged.sort(key=lambda s: s.start)                   # stable
        for a, b in zip(merged, merged[1:]):
            if a.end == NO_END:
                raise ValueError(f"a segment at {b.start} would lie behind the FOREVER segment at {a.start}")
            if a.end > b.start:
                raise ValueError(f"the segments at {a.start} and {b.start} would overlap on the track")
        if len(merged) > MAX_SEGMENTS:
            raise ValueError(f"{len(merged)} segments that have not ended on one track (at most {MAX_SEGMENTS})")
        return merged

    def queue(self, channel: int, track: int, segs, start: int = APPEND):
        segs = [tuple(int(v) for v in s) for s in segs]
        if not 0 <= track < TRACKS:
            raise ValueError(f"track {track}")
        if not 1 <= len(segs) <= MAX_SEGMENTS:
            raise ValueError(f"need 1..{MAX_SEGMENTS} segments")
        for i, (gap, length, step_a, step_b, amp_a, amp_b) in enumerate(segs):
            if amp_a > MAX_AMP or amp_b > MAX_AMP:
                raise ValueError(f"segment {i} has an amp above {MAX_AMP}")
            if length == 0:
                raise ValueError(f"segment {i} has length 0")
            if length == FOREVER and i + 1 < len(segs):
                raise ValueError(f"segment {i + 1} lies behind a FOREVER segment")
        if start != APPEND and start >= MAX_TIME:
            raise ValueError(f"stream time {start} (below 2^63)")
        chans = self._selected(channel)
        merged = [self._lay_out(self.track[c][track], segs, start) for c in chans]      # refused whole
        for c, m in zip(chans, merged):
            self.track[c][track] = m

    def cut(self, channel: int = ALL, track: int = 0):
        if not 0 <= track < TRACKS:
            raise ValueError(f"track {track}")
        for c in self._selected(channel):
            q = [s for s in self.track[c][track] if s.start <= self.N < s.end]
            for s in q:
                s.end = min(s.end, self.N + RAMP)
            self.track[c][track] = q

    def reset(self):
        self.N = 0
        self.track = [[[] for _ in range(TRACKS)] for _ in range(self.C)]
        self._clips = [0] * self.C

    def set_time(self, N: int):
        if not 0 <= N < MAX_TIME:
            raise ValueError(f"stream time {N} (below 2^63)")
        self.N = int(N)

    def time(self) -> int:
        return self.N

    def pending(self, channel: int, track: int = 0):
        left = [s for s in self.track[channel][track] if s.end > self.N]
        return len(left), (left[-1].end if left else self.N)

    def clips(self, channel: int) -> int:
        return self._clips[channel]

    # ---- a call
    def process(self, pcm, n_blocks: int = None, want_active: bool = False):
        """pcm int16 [C, n_blocks x 512] (any shape with C rows) or None with n_blocks -> out int16 [C, n_blocks, 512], or
        (out, active uint8 [C, n_blocks]) with want_active"""
        C = self.C
        if pcm is None:
            x = np.zeros((C, BLOCK * int(n_blocks)), dtype=np.int64)
        else:
            x = np.asarray(pcm).reshape(C, -1).astype(np.int64)
        n = x.shape[1]
        n_blocks = n // BLOCK
        assert n == n_blocks * BLOCK and 1 <= n_blocks <= MAX_BLOCKS and self.N + n <= MAX_TIME
        lo, hi = self.N, self.N + n
        active = np.zeros((C, n_blocks), dtype=np.uint8)
        y = x.copy()
        for c in range(C):
            for t in range(TRACKS):
                q = self.track[c][t] = [s for s in self.track[c][t] if s.end > lo]      # what has ended leaves the queue
                for s in q:
                    g, a = segment_span(s, lo, hi)
                    if g is None:
                        continue
                    y[c, a - lo:a - lo + g.size] += g
                    active[c, (a - lo) // BLOCK:(a - lo + g.size - 1) // BLOCK + 1] |= 1 << t
        out = np.clip(y, -32768, 32767)
        for c in range(C):
            self._clips[c] += int((out[c] != y[c]).sum())
        self.N = hi
        out = out.astype(np.int16).reshape(C, n_blocks, BLOCK)
        return (out, active) if want_active else out

    # the helpers are api.ToneGen's own: they only call queue
    dial = api.ToneGen.dial
    ctcss = api.ToneGen.ctcss
    burst = api.ToneGen.burst
    tones = api.ToneGen.tones


def slow(model: ToneGenModel, x, n_blocks: int):
    """the contract sample by sample in Python integers, from the model's queues and clock as they stand (nothing is
    changed): x int [C][n_blocks x 512] or None -> (out lists [C][n], active lists [C][n_blocks], clips [C])"""
    cos = [int(v) for v in COS]
    outs, actives, clips = [], [], []
    for c in range(model.C):
        row, act, clipped = [], [0] * n_blocks, 0
        for j in range(BLOCK * n_blocks):
            n = model.N + j
            total = int(x[c][j]) if x is not None else 0
            for t in range(TRACKS):
                for s in model.track[c][t]:
                    if not s.start <= n < s.end:
                        continue
                    k = n - s.start
                    S = []
                    for step in (s.step_a, s.step_b):
                        theta = (step * k) % (1 << 32)
                        i = ((theta + (1 << 19)) >> 20) & 4095
                        S.append(cos[(i - 1024) & 4095])
                    v = (s.amp_a * S[0] + s.amp_b * S[1] + (1 << 14)) >> 15
                    e = min(k + 1, 64) if s.end == NO_END else min(k + 1, s.end - s.start - k, 64)
                    total += (v * e + 32) >> 6
                    act[j // BLOCK] |= 1 << t
            y = max(-32768, min(32767, total))
            clipped += y != total
            row.append(y)
        outs.append(row)
        actives.append(act)
        clips.append(clipped)
    return outs, actives, clips


# ---- the closed loop of tests/tone_model.py with this bank's audio in place of loop_audio()
def loop_queue(bank):
    """per station 16 segments of 512 samples, gap 0, row and column at 5000, following LOOP_KEYS; under station 0 a
    1000 Hz tone without an end at 2500 on track 1 (ToneGenModel and api.ToneGen take the same calls)"""
    from tests import tone_model as tm
    for c, keys in enumerate(tm.LOOP_KEYS):
        segs = []
        for key in keys[:16]:
            r, col = divmod(tm.DTMF_KEYS.index(key), 4)
            segs.append(api.tonegen_segment(BLOCK, tm.DTMF_LOW_HZ[r], 5000, tm.DTMF_HIGH_HZ[col], 5000))
        bank.queue(c, 0, segs, 0)
    bank.queue(0, 1, [api.tonegen_segment(FOREVER, tm.LOOP_PILOT_HZ, 2500)], 0)


_loop = {}


def loop_reference(oracle):
    """the loop on the models and the CPU oracle, computed once: (audio int16 [2, 8192], amplitudes, DUC clips, received PCM
    int16 [2, n], the generator's clips)"""
    if "ref" not in _loop:
        from tests import ddc_model as dm
        from tests import duc_model as um
        from tests import tone_model as tm
        gen = ToneGenModel(2)
        loop_queue(gen)
        audio = gen.process(None, 16).reshape(2, -1)
        streams, amps = tm.loop_streams(oracle, [audio[0], audio[1]])
        cap, duc = um.loop_duc(streams, amps)
        d = dm.DdcModel(1, 2, dm.SEL_R)
        for c, f in enumerate(dm.SEL_OFFSETS):
            d.set_tuning(c, 0, dm.ddc_step(f + 64_000, dm.SEL_R))
            d.set_gain_shift(c, dm.SEL_GAIN_SHIFT[c])
        rx_in = d.process(cap, dm.SEL_BLOCKS * 262144)
        pcm = np.stack([dm.oracle_rx_wbfm(oracle, rx_in[c]) for c in range(2)])
        for a in (audio, pcm):
            a.setflags(write=False)
        _loop["ref"] = (audio, amps, int(duc.clips[0]), pcm, gen.clips(0) + gen.clips(1))
    return _loop["ref"]
