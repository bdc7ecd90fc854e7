"""Inputs for the squelch sweeps (tests/test_squelch_model.py, tests/test_gpu_squelch_sweep.py): DC levels that put a
block's mean magnitude on every value the detector can see, found by asking the oracle's front end (the half-band
decimators' DC gain and the int8 narrowing decide which raw level gives which 256 kS/s value: SURVEY A3), and blocks
perturbed until their magnitude sum sits just below a multiple of the sample count.  Nothing here decides what is
right: the tests check what these inputs reached through tests/squelch_model.py."""
from __future__ import annotations

import functools

import numpy as np

from tests import squelch_model as sm
from tests.reflib import NONE

MAX_MEAN = 192                      # |-128| + (|-128| >> 1)


@functools.lru_cache(maxsize=None)
def _dc_response(oracle):
    """raw DC level v on both rails -> the absolute 256 kS/s value in the steady state, read from the oracle's dump"""
    out = {}
    for v in range(-128, 128):
        r = oracle.rx()
        r.set_mode(NONE)
        x = np.full(2048, v, dtype=np.int8)
        r.process(x)
        d = np.abs(r.process(x)[3].astype(np.int64))
        if d.min() == d.max():                          # (a level whose steady state is not one value is not used)
            out[v] = int(d[0])
    return out


@functools.lru_cache(maxsize=None)
def dc_pairs(oracle):
    """{mean: (i, q)} for every block mean 0..MAX_MEAN a DC input can give; raw -128 and the 256 kS/s value -128
    (absolute 128) on either rail where a mean can be had that way"""
    resp = _dc_response(oracle)
    by_abs = {}
    for v in sorted(resp, key=lambda v: (v != -128, v >= 0, abs(v))):      # raw -128 first, then negative levels
        by_abs.setdefault(resp[v], v)
    pairs = {}
    for a, va in by_abs.items():
        for b, vb in by_abs.items():
            if b > a:
                continue
            mean = a + (b >> 1)
            cand = (va, vb) if (mean % 2) else (vb, va)                    # the larger rail is I for odd means, Q for even
            score = (a == 128) + (b == 128) + (va == -128) + (vb == -128)
            if mean not in pairs or score > pairs[mean][0]:
                pairs[mean] = (score, cand)
    return {m: p for m, (_, p) in sorted(pairs.items())}


def dc_block(pair, block_bytes):
    x = np.empty(block_bytes, dtype=np.int8)
    x[0::2], x[1::2] = pair
    return x


def dumps_of(oracle, blocks):
    """the 256 kS/s dump of every call of a sequence (front end only)"""
    r = oracle.rx()
    r.set_mode(NONE)
    return [r.process(b)[3] for b in blocks]


def perturb_below_multiple(oracle, table, before, block, seed, lo=8, tries=400):
    """change a few raw samples of `block` (which follows the blocks `before`) until its magnitude sum is 1..lo below a
    multiple of the sample count; returns the new block, or None"""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        y = block.copy()
        for _ in range(int(rng.integers(1, 4))):
            at = 2 * int(rng.integers(64, y.size // 2 - 64)) + int(rng.integers(0, 2))
            span = int(rng.integers(4, 17))
            v = y[at:at + 2 * span:2].astype(np.int64)
            y[at:at + 2 * span:2] = np.clip(v - np.sign(v) * int(rng.integers(1, 9)), -128, 127).astype(np.int8)
        b = sm.detect(table, dumps_of(oracle, list(before) + [y])[-1], 0)
        if b.n and b.n - lo <= b.rem <= b.n - 1:
            return y
    return None
