"""The squelch detector over its whole domain on the CPU: the oracle's detector (oracle/hrfd_oracle.c), the plain numpy
statement of it (tests/squelch_model.py) and the reference's own compiled sources (oracle/_ref) must agree on every
table index and the clamp, on both sides of every threshold with receive gains that take the level across zero and far
below -42, where the unsigned gain subtraction wraps, and on every step of the signal tracker, in every mode.

The reference's `allowed` is seen through its PCM (a demodulator runs or it does not); in mode NONE only its magnitude
is observable.  Every test first asserts, from the model, that its inputs reached what it claims to cover."""
import numpy as np
import pytest

from tests import squelch_inputs as si
from tests import squelch_model as sm
from tests.reflib import AM, FM, WBFM, LSB, USB, NONE

BB = 8192                                  # 512 samples at 256 kS/s and 16 PCM samples per call
GAINS = [0, 1, 6, 20, 40, 62]


def _sequence(pair):
    """loud, loud, silent, silent, loud, loud: every (tracking, present) pair when the threshold is at the loud level"""
    loud, quiet = si.dc_block(pair, BB), np.zeros(BB, dtype=np.int8)
    return [loud, loud, quiet, quiet, loud, loud]


def _three_way(oracle, ref, table, blocks, mode, threshold, gain_db):
    """one sequence through oracle, model and reference -> (model blocks, allowed, (tracking, present) pairs)"""
    a, b = oracle.rx(), ref.rx()
    for h in (a, b):
        h.set_mode(mode); h.set_threshold(threshold); h.gain_db = gain_db
    t = sm.Tracker()
    out = []
    for k, x in enumerate(blocks):
        pa, ma, allowed, dump = a.process(x)
        pb, mb, _, _ = b.process(x)
        m = sm.detect(table, dump, threshold, gain_db)
        want, seen = t.run(m.present)
        where = (mode, threshold, gain_db, k)
        assert ma == mb == m.mean, where
        assert allowed == want, where
        if mode != NONE:
            assert (len(pa) > 0) == (len(pb) > 0) == want and len(pa) == len(pb) and (pa == pb).all(), where
        else:
            assert len(pa) == len(pb) == 0, where
        out.append((m, want, seen))
    return out


def test_model_against_hand_values(oracle):
    table = oracle.dbfs_table()
    assert sm.magnitudes(np.array([-128, -128, 3, -4, 0, 0, 127, -128], dtype=np.int8)).tolist() == [192, 5, 0, 191]
    assert sm.level(table, 0) == sm.level(table, 1) == -42 and sm.level(table, 2) == -36
    assert sm.level(table, 127) == sm.level(table, 128) == sm.level(table, 192) == 0
    assert sm.level(table, 127, 62) == -62 and sm.level(table, 0, 1 << 31) == (1 << 31) - 42
    assert sm.level(table, 127, (1 << 32) - 1) == 1 and sm.level(table, 0, (1 << 32) - 1) == -41
    b = sm.detect(table, np.array([10, 0, 0, -11, 3, 3], dtype=np.int8), -23)        # 10 + 11 + 4 = 25 over 3
    assert (b.sum, b.n, b.mean, b.rem, b.index, b.dbfs, b.present) == (25, 3, 8, 1, 8, -24, False)
    assert sm.detect(table, np.zeros(0, dtype=np.int8), -42).mean == 0
    t = sm.Tracker()
    assert [t.run(p)[0] for p in (1, 0, 0, 1, 1, 0, 1, 0, 0)] == [True, True, False, True, True, True, True, True, False]


def test_every_mean_is_reachable_from_dc(oracle):
    """the mapping the device sweep relies on: one DC pair per block mean 0..192, found with the oracle's front end"""
    table = oracle.dbfs_table()
    pairs = si.dc_pairs(oracle)
    assert sorted(pairs) == list(range(si.MAX_MEAN + 1))
    raw_i = raw_q = dec_i = dec_q = False
    for mean, pair in pairs.items():
        d = si.dumps_of(oracle, [si.dc_block(pair, 2048)] * 2)[1]
        b = sm.detect(table, d, 0)
        assert (b.mean, b.rem) == (mean, 0), (mean, pair)
        raw_i |= pair[0] == -128; raw_q |= pair[1] == -128
        dec_i |= bool((d[0::2] == -128).any()); dec_q |= bool((d[1::2] == -128).any())
    assert raw_i and raw_q and dec_i and dec_q, "-128 on either rail, raw and at 256 kS/s"


def test_every_table_index_and_the_clamp(oracle, ref):
    table = oracle.dbfs_table()
    pairs = si.dc_pairs(oracle)
    indices, clamped = set(), set()
    for mean, pair in pairs.items():
        thr = sm.level(table, mean)
        for m, _, _ in _three_way(oracle, ref, table, _sequence(pair), AM, thr, 0):
            indices.add(m.index)
            if m.mean > 127:
                clamped.add(m.mean)
    assert indices == set(range(128))
    assert clamped == set(range(128, si.MAX_MEAN + 1))


@pytest.mark.parametrize("gain_db", GAINS)
def test_thresholds_around_every_level(oracle, ref, gain_db):
    """thresholds L-1, L, L+1 for every level L the table holds, at the first and the last mean that has it: `allowed`
    of the steady loud block flips exactly between L and L+1"""
    table = oracle.dbfs_table()
    pairs = si.dc_pairs(oracle)
    levels = {}
    for mean in pairs:
        levels.setdefault(sm.level(table, mean, gain_db), []).append(mean)
    assert sorted(levels) == [int(v) - 42 - gain_db for v in sorted(set(table[:128].tolist()))]
    deltas, transitions = set(), set()
    for L, means in levels.items():
        for mean in {means[0], means[-1]}:
            steady = {}
            for thr in (L - 1, L, L + 1):
                out = _three_way(oracle, ref, table, _sequence(pairs[mean]), [AM, FM, WBFM, LSB, USB][mean % 5], thr, gain_db)
                assert out[1][0].mean == mean and out[1][0].dbfs == L
                steady[thr] = out[1][0].present
                deltas.add(out[1][0].dbfs - thr)
                transitions |= {seen for _, _, seen in out}
            assert steady == {L - 1: True, L: True, L + 1: False}, (mean, L)
    assert deltas == {-1, 0, 1}
    assert transitions == {(False, False), (False, True), (True, False), (True, True)}
    assert (min(levels) < -42 or gain_db == 0) and (max(levels) == -gain_db)


@pytest.mark.parametrize("gain_db", [(1 << 31) - 43, (1 << 31) - 42, (1 << 31) - 41, 1 << 31, (1 << 31) + 42, (1 << 32) - 43,
                                     (1 << 32) - 42, (1 << 32) - 1])
def test_gain_that_wraps_the_unsigned_subtraction(oracle, ref, gain_db):
    """whatever the reference does is the answer: the level is (int32)((uint32)dbfs - gain_db), so a gain near 2^31
    turns the lowest levels into the highest, and one near 2^32 lifts every level"""
    table = oracle.dbfs_table()
    pairs = si.dc_pairs(oracle)
    seen_levels = set()
    for mean in (0, 2, 3, 40, 127, 192):
        L = sm.level(table, mean, gain_db)
        seen_levels.add(L)
        for thr in sorted({max(L - 1, -(1 << 31)), L, min(L + 1, (1 << 31) - 1), -200, 0, -(1 << 31), (1 << 31) - 1}):
            _three_way(oracle, ref, table, _sequence(pairs[mean]), FM if mean % 2 else WBFM, thr, gain_db)
    if gain_db >= (1 << 31) - 41:
        assert [L for L in seen_levels if L > 0], "no level above 0 dBFS: the subtraction did not wrap"
    else:
        assert max(seen_levels) < -(1 << 30), "the last gains before the wrap: every level far below any threshold in use"
    if gain_db in ((1 << 31) - 42, (1 << 31) - 41):
        assert -(1 << 31) in seen_levels or (1 << 31) - 1 in seen_levels, "the ends of int32 were to be reached"


@pytest.mark.parametrize("mode", [NONE, AM, FM, WBFM, LSB, USB])
def test_tracker_in_every_mode(oracle, ref, mode):
    """all four (tracking, present) pairs, the one tail block after a closing gate, two closings in a row"""
    table = oracle.dbfs_table()
    pair = si.dc_pairs(oracle)[37]
    loud, quiet = si.dc_block(pair, BB), np.zeros(BB, dtype=np.int8)
    pattern = "0110010010011"
    out = _three_way(oracle, ref, table, [loud if ch == "1" else quiet for ch in pattern], mode, sm.level(table, 37, 6), 6)
    allowed = "".join("1" if a else "0" for _, a, _ in out)
    assert allowed == "0111011011011"
    assert {seen for _, _, seen in out} == {(False, False), (False, True), (True, False), (True, True)}
    assert "0110110" in allowed                                  # open, tail, closed / open, tail, closed: twice in a row
