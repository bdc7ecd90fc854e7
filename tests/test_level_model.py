"""tests/level_model.py against slow_channel, its own sample-by-sample restatement in Python integers, and against the
properties the contract of the level bank states: |y| <= target, |x gs| <= target << 12 < 2^27 (an int32, and a 24-bit
multiply), gs < 2^23, and the same bytes for every cut of a stream into calls.  No GPU."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import level_model as lm


def random_settings(rng):
    """W 1..64 with w[0] = 32768, target 0..32767, floor 16..32768, the edges among them"""
    W = int(rng.choice([1, 2, 3, 63, 64, int(rng.integers(1, 65))]))
    w = rng.integers(0, lm.UNITY + 1, size=W)
    w[0] = lm.UNITY
    target = int(rng.choice([0, 1, 32767, int(rng.integers(0, 32768))]))
    floor = int(rng.choice([16, 17, 32768, int(rng.integers(16, 32769))]))
    return w, target, floor


def random_pcm(rng, C, n_blocks):
    """amplitudes from 1 to full scale, a new one every few frames, -32768 among the samples"""
    n = 512 * n_blocks
    x = np.zeros((C, n), dtype=np.int64)
    for c in range(C):
        at = 0
        while at < n:
            run = int(rng.integers(1, 12)) * 64 - int(rng.integers(0, 2)) * 17
            amp = int(rng.choice([0, 1, 15, 16, 17, 300, 32767, 32768, int(rng.integers(1, 32769))]))
            x[c, at:at + run] = rng.integers(-amp, amp + 1, size=min(run, n - at))
            at += run
    x = np.clip(x, -32768, 32767)
    x[0, n // 2] = -32768
    return x.astype(np.int16)


@pytest.mark.parametrize("seed", range(12))
def test_model_equals_the_slow_restatement(seed):
    rng = np.random.default_rng(seed)
    C, B = 2, 3
    w, target, floor = random_settings(rng)
    m = lm.LevelModel(C)
    m.set_weights(w)
    m.set(target, floor)
    hist = [np.zeros(lm.HIST, dtype=np.int64) for _ in range(C)]
    for call in range(2):                                   # the second call starts from the first one's peaks
        pcm = random_pcm(rng, C, B)
        n_pcm = rng.choice(np.array([0, 1, 63, 64, 65, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32), size=(C, B))
        x = lm.masked(pcm, n_pcm)
        out, gain, peak = m.process(pcm, n_pcm)
        for c in range(C):
            y, g, p, hist[c] = lm.slow_channel(x[c].ravel(), hist[c], w, target, floor)
            assert out[c].ravel().tolist() == y and gain[c].tolist() == g and peak[c].tolist() == p, (seed, call, c)
            assert m.hist[c].tolist() == hist[c]
        assert np.abs(out.astype(np.int64)).max() <= target
        assert m.max_product <= target << 12 < 1 << 27 and gain.max() < 1 << 23


@pytest.mark.parametrize("seed", range(6))
def test_every_cut_into_calls_gives_the_same_bytes(seed):
    rng = np.random.default_rng(100 + seed)
    C, B = 2, 5
    w, target, floor = random_settings(rng)
    pcm = random_pcm(rng, C, B).reshape(C, B, 512)
    n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C, B))

    def run(cuts):
        m = lm.LevelModel(C)
        m.set_weights(w)
        m.set(target, floor)
        m.set_bypass(True, 1)
        parts, at = [], 0
        for k in cuts:
            parts.append(m.process(pcm[:, at:at + k], n_pcm[:, at:at + k]))
            at += k
        return [np.concatenate([p[i] for p in parts], axis=1) for i in range(3)], m.hist

    whole, hist = run([B])
    for mask in range(1 << (B - 1)):                        # every composition of 5 blocks
        cuts, k = [], 1
        for bit in range(B - 1):
            if mask >> bit & 1:
                cuts.append(k)
                k = 1
            else:
                k += 1
        cuts.append(k)
        got, h = run(cuts)
        assert all((a == b).all() for a, b in zip(got, whole)) and (h == hist).all(), cuts
    assert (whole[0][1] == lm.masked(pcm, n_pcm)[1]).all()  # the bypassed channel


def test_defaults_and_the_weights_helper():
    w = lm.default_weights()
    assert w.size == 64 and (w[:8] == 32768).all() and w[8] == 32768 and w[9] == (32768 * 55) // 56 and w[63] == 32768 // 56
    assert (np.diff(w[8:]) < 0).all()
    h = api.level_weights(64.0, 200.0)
    assert h.dtype == np.uint16 and h.size == 64 and (h[:9] == 32768).all() and h[9] == round(32768 * np.exp(-8 / 200.0))
    assert (np.diff(h[8:].astype(np.int64)) < 0).all()
    assert api.level_weights(0.0, 1e-3, 3).tolist() == [32768, 0, 0] and api.level_weights(1e9, 1.0, 1).tolist() == [32768]
    m = lm.LevelModel(1)
    m.set_weights(h)                                        # the helper's tables pass the model's own check
    for bad in ((0.0, 1.0, 0), (0.0, 1.0, 65), (-1.0, 1.0, 64), (0.0, 0.0, 64)):
        with pytest.raises(ValueError):
            api.level_weights(*bad)


def test_largest_gain_and_both_extremes():
    m = lm.LevelModel(1)
    m.set(32767, 16)
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, 64:128] = 16
    x[0, 130] = -16
    out, gain, peak = m.process(x)
    assert gain[0, 0] == lm.MAX_GAIN == 8388352 and peak[0, 1] == 16
    assert out[0, 0, 64] == 32767 and out[0, 0, 130] == -32767
    m = lm.LevelModel(1)
    m.set(32767, 32768)
    x[:] = -32768
    x[0, 1::2] = 32767
    out, gain, peak = m.process(x)
    assert (peak == 32768).all() and (gain == 4095).all()
    assert out[0, 0, 0] == (-32768 * 4095 + 2048) >> 12 == -32760 and out[0, 0, 1] == (32767 * 4095 + 2048) >> 12
