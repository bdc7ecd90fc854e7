"""The DUC model (tests/duc_model.py) held to two statements written apart from it (tests/duc_reference.py): an integer
restatement over whole streams, bit for bit across call sequences with every setter, and a float64 computation within
the error budget of the rounding steps."""
import numpy as np
import pytest

from tests import duc_model as um
from tests import duc_reference as ur


def branch_taps(rng, n, R, limit=65535):
    h = rng.integers(-32768, 32768, size=n).astype(np.int64)
    for p in range(R):
        s = np.abs(h[p::R]).sum()
        if s > limit:
            h[p::R] = np.sign(h[p::R]) * ((np.abs(h[p::R]) * limit) // s)
    return h


def rand_channels(rng, C, n_bytes):
    return rng.integers(-128, 128, size=(C, n_bytes)).astype(np.int8)


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_model_equals_whole_stream_restatement(R):
    rng = np.random.default_rng(10 + R)
    W, C = 3, 7
    m = um.DucModel(W, C, R)
    ref = ur.DucWhole(W, C, R, m.hA, m.hB)
    for c in range(C):
        s = int(rng.integers(0, 2 ** 32))
        w = 0 if c < 5 else 2                                      # many channels on capture 0, none on capture 1
        m.set_tuning(c, w, s)
        ref.set_tuning(c, w, s)
    # calls shorter than the history, around it and longer; a setter of every kind between them
    sizes = [2, 6, 100, 640, 30, 1500, 2, 900, 400]
    for i, ib in enumerate(sizes):
        if i == 1:
            c, w, s = 3, 1, int(rng.integers(0, 2 ** 32))
            m.set_tuning(c, w, s)
            ref.set_tuning(c, w, s)
        if i == 2:
            t = branch_taps(rng, int(rng.integers(1, 65)), R)     # asymmetric, random
            m.set_filter(0, t)
            ref.hA = t
        if i == 3:
            t = branch_taps(rng, int(rng.integers(1, 257)), 1)
            m.set_filter(1, t)
            ref.hB = t
        if i == 4:
            for c, a in ((0, 0), (1, 1), (2, 32767), (4, 20000)):
                m.set_amplitude(c, a)
                ref.amp[c] = a
        if i == 5:
            for w, s in ((0, 0), (1, 13), (2, 24)):
                m.set_output_shift(w, s)
                ref.shift[w] = s
        if i == 6:
            m.set_filter(0, [])
            ref.hA = np.zeros(0, dtype=np.int64)
            m.set_filter(1, [])
            ref.hB = np.zeros(0, dtype=np.int64)
        if i == 7:
            m.reset()
            ref.reset()
            t = branch_taps(rng, 64, R)
            m.set_filter(0, t)
            ref.hA = t
        ch = rand_channels(rng, C, ib)
        got, st = m.process(ch, ib, stages=True)
        want, S = ref.process(ch, ib)
        assert (st["S"] == S).all(), f"R={R} call {i}"
        assert (got == want).all(), f"R={R} call {i}"
        assert (m.clips == ref.clips).all()
    assert m.clips.sum() > 0


@pytest.mark.parametrize("R", [1, 2, 8])
def test_model_within_the_float_budget(R):
    rng = np.random.default_rng(30 + R)
    m = um.DucModel(1, 1, R)
    if R > 1:
        m.set_filter(0, branch_taps(rng, 37, R, limit=40000))
    m.set_amplitude(0, 23456)
    m.set_tuning(0, 0, int(rng.integers(0, 2 ** 32)))
    # a band-limited tone well inside full scale, so that no sat16 acts
    n = 3000
    t = np.arange(n)
    x = np.stack([np.round(60 * np.cos(0.05 * t)), np.round(60 * np.sin(0.05 * t))], axis=1).astype(np.int8)
    _, st = m.process(x.reshape(1, -1), 2 * n, stages=True)
    assert np.abs(st["a"]).max() < 32767
    theta = (m.phase(0, 0) + np.arange(R * n, dtype=np.int64) * int(m.step[0])) & um.MASK32
    fI, fQ = ur.float_sums(x, R, m.hA, m.hB, 23456, theta)
    err = max(np.abs(st["S"][0, 0] - fI).max(), np.abs(st["S"][0, 1] - fQ).max())
    budget = ur.error_budget(R, m.hA, m.hB, 23456)
    assert err <= budget, (err, budget)
    assert err > 0.05 * budget, "the comparison is not vacuous"
