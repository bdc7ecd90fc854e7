"""The squelch detector stated a second time, in plain numpy integer code, from the reference's formulas
(SignalDetector.cc:205-274, DbfsCalculator.cc:111-147, SignalTracker.cc:104-146, Squelch.cc:227-273):

    mean    = sum(max(|i|,|q|) + (min(|i|,|q|) >> 1)) / n      (unsigned, floor; n = 256 kS/s samples of the call)
    dbfs    = table[min(mean, 127)] - 42
    dbfs    = (int32)((uint32)dbfs - gain_db)
    present = dbfs >= threshold;  allowed = present || tracking;  tracking = present

It works on a call's 256 kS/s dump (what the oracle and the device return) and calls nobody's detector: the tests use
it to say what an input REACHED (which table index, which side of the threshold, which remainder of sum mod n), and
the oracle's detector is held to it as a second implementation.  Test infrastructure only."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

FULL_SCALE = 127
FULL_SCALE_DB = 42          # (uint32)(20 * log10(127.0))


@dataclass(frozen=True)
class Block:
    sum: int                # of the per-sample magnitudes
    n: int                  # 256 kS/s samples in the call
    mean: int               # sum // n (0 where n == 0)
    index: int              # the table entry read: min(mean, 127)
    dbfs: int               # after the gain term, as int32
    present: bool

    @property
    def rem(self) -> int:
        return self.sum % self.n if self.n else 0


def magnitudes(iq256) -> np.ndarray:
    """per-sample magnitude of an interleaved int8 I/Q stream: max + (min >> 1) of the absolute values (|-128| = 128)"""
    d = np.abs(np.asarray(iq256, dtype=np.int8).astype(np.int64))
    i, q = d[0::2], d[1::2]
    return np.maximum(i, q) + (np.minimum(i, q) >> 1)


def level(table, mean: int, gain_db: int = 0) -> int:
    """the detector's level for a block mean: table lookup with the clamp, minus full scale, minus the gain (mod 2^32)"""
    v = int(table[min(int(mean), FULL_SCALE)]) - FULL_SCALE_DB
    v = (v - int(gain_db)) & 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def detect(table, iq256, threshold: int, gain_db: int = 0) -> Block:
    m = magnitudes(iq256)
    n = int(m.size)
    s = int(m.sum())
    mean = s // n if n else 0
    db = level(table, mean, gain_db)
    return Block(s, n, mean, min(mean, FULL_SCALE), db, db >= int(threshold))


class Tracker:
    """SignalTracker + Squelch: one tail block after the signal drops"""

    def __init__(self):
        self.tracking = False

    def run(self, present: bool):
        """-> (allowed, the (tracking, present) pair this block was decided on)"""
        seen = (self.tracking, bool(present))
        allowed = bool(present) or self.tracking
        self.tracking = bool(present)
        return allowed, seen


def run(table, dumps, threshold: int, gain_db: int = 0, tracker: Tracker | None = None):
    """a sequence of calls' dumps -> ([Block], [allowed], [(tracking, present)])"""
    t = tracker if tracker is not None else Tracker()
    blocks, allowed, seen = [], [], []
    for d in dumps:
        b = detect(table, d, threshold, gain_db)
        a, s = t.run(b.present)
        blocks.append(b); allowed.append(a); seen.append(s)
    return blocks, allowed, seen
