"""Shared by the edge tests of the host transports (tests/test_gpu_ingest_edges.py, tests/test_gpu_fanout_edges.py): small
banks of FM tones, the sequential CPU oracle over them -- the reference of every comparison, computed once per scenario --
and the unit-by-unit comparison.  Test infrastructure only.

A UNIT is one block of one channel.  The oracle runs every channel block after block with the gain_db of the batch the block
belongs to: what a sequential caller of IqDataProcessor::acceptIqData gets, whatever the transport had in flight."""
from __future__ import annotations

import numpy as np

from hackrfdiags_amd import api, synth
from tests import squelch_model

SPEC = 21504          # (kMaxHal + 64) * 16: the shortest block that runs as a speculative multi-block batch
FLOW = 32768          # 2048 samples at 256 kS/s: the shortest block hrfd_rx_plan.h gives to the flow kernel (2 blocks or more)
G = 20                # the second gain of the gate-flipping inputs, dB
FLIP_THRESHOLD = -20  # between the tone's level at gain 0 (-4 dBFS) and at gain G (-24 dBFS)


def tones(C: int, T: int, bb: int, seed: int) -> np.ndarray:
    """int8 [C, T, bb]: channel c is the FM test tone of seed + c, amplitude 100, T blocks of bb bytes"""
    return np.stack([synth.fm_tone_iq(seed + c, T * bb // 2).reshape(T, bb) for c in range(C)])


class Want:
    """the oracle's answer for every unit: pcm[c][t], mag[c, t], allowed[c, t], and the 256 kS/s dumps"""

    def __init__(self, C, T):
        self.pcm = [[None] * T for _ in range(C)]
        self.mag = np.zeros((C, T), dtype=np.int64)
        self.allowed = np.zeros((C, T), dtype=bool)
        self.dump = [[None] * T for _ in range(C)]


class Bank:
    """C oracle receivers that go on from call to call (the transport under test is recreated, the streams continue)"""

    def __init__(self, oracle, modes, thresholds=None, gains=None):
        self.rx = []
        for c, m in enumerate(modes):
            o = oracle.rx()
            o.set_mode(m)
            if thresholds is not None and thresholds[c] is not None:
                o.set_threshold(thresholds[c])
            if gains is not None and gains[c] is not None:
                o.set_gain(m, gains[c])
            self.rx.append(o)

    def run(self, xs, gain_db_of_block) -> Want:
        C, T = xs.shape[0], xs.shape[1]
        w = Want(C, T)
        for c, o in enumerate(self.rx):
            for t in range(T):
                o.gain_db = int(gain_db_of_block[t])
                w.pcm[c][t], w.mag[c, t], w.allowed[c, t], w.dump[c][t] = o.process(xs[c, t])
        return w


def assert_flips(oracle, want: Want, c: int, gain_db_of_block):
    """a condition on the INPUTS: channel c's gate is open in a block at one gain and closed in a block at the other, and
    the detector's level (stated a second time by tests/squelch_model.py) is on either side of the threshold"""
    table = oracle.dbfs_table()
    g = np.asarray(gain_db_of_block)
    assert want.allowed[c][g == 0].any() and not want.allowed[c][g != 0].all(), (want.allowed[c], g)
    present = [squelch_model.detect(table, want.dump[c][t], FLIP_THRESHOLD, int(g[t])).present for t in range(len(g))]
    assert all(p == (int(g[t]) == 0) for t, p in enumerate(present)), present


def assert_batch(got, want: Want, k: int, B: int, t0: int = 0, channels=None, what=("pcm", "n_pcm", "mag", "allowed")):
    """got = (pcm [C, B, cap], n_pcm [C, B], mag [C, B] | None, allowed [C, B] | None) of batch k against the oracle's
    units t0 + k B .. : the samples, their count, the zeros behind them, the block magnitude and the gate"""
    pcm, n_pcm = got[0], got[1]
    mag = got[2] if len(got) > 2 else None
    allowed = got[3] if len(got) > 3 else None
    C = pcm.shape[0]
    for c in (range(C) if channels is None else channels):
        for b in range(B):
            t = t0 + k * B + b
            p = want.pcm[c][t]
            if "n_pcm" in what and n_pcm is not None:
                assert int(n_pcm[c, b]) == len(p), ("n_pcm", k, c, b, int(n_pcm[c, b]), len(p))
            if "pcm" in what:
                assert (pcm[c, b, :len(p)] == p).all(), ("pcm", k, c, b)
                assert (pcm[c, b, len(p):] == 0).all(), ("zeros behind n_pcm", k, c, b)
            if "mag" in what and mag is not None:
                assert int(mag[c, b]) == int(want.mag[c, t]), ("magnitude", k, c, b)
            if "allowed" in what and allowed is not None:
                assert bool(allowed[c, b]) == bool(want.allowed[c, t]), ("allowed", k, c, b)


def own_failures(want: Want, modes, B: int):
    """per batch, the channels whose "every gate open" speculation fails by itself: a closed gate in a multi-block batch of
    a channel that has a demodulator (k_rx_finish: gate_viol)"""
    C, T = want.allowed.shape
    return [{c for c in range(C) if modes[c] != api.NONE and not want.allowed[c, k * B:(k + 1) * B].all()}
            for k in range(T // B)]
