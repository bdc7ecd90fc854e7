"""The walks of tests/ragged_walks.py on the CPU: what they cover, asserted from the builders' own bookkeeping (the count
formulas of DESIGN.md 3.2b, nothing measured), and the CPU oracle against the compiled reference on every one of them,
call for call and live (the reference's answers are not recorded: they would be megabytes; where oracle/_ref is absent
the `ref` fixture skips).  tests/test_gpu_ragged_sweep.py runs the same walks on the device against the oracle."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import ragged_walks as W
from tests.ragged_walks import MODES


def _seed(mode):
    return W.GATED_SEED + mode


# ---------------------------------------------------------------- coverage, from the bookkeeping alone
def test_the_walks_capacities_are_the_librarys():
    for n in list(range(2, 4200, 2)) + [261632, 262142, 262144]:
        assert W.pcm_capacity(n) == api.pcm_capacity(n) and W.iq256_capacity(n) == api.iq256_capacity(n)


@pytest.mark.parametrize("mode", MODES)
def test_phase_sweep_starts_every_class_from_every_position(mode):
    w = W.phase_sweep(mode)
    pairs = {(b.position, b.cls) for b in w.blocks if b.cls >= 0}
    assert len(pairs) == 256 * len(W.SWEEP_CLASSES) == 2560
    # the plain stream: the position alone says where the front end and the three commutators stand, and what comes out
    for b in w.blocks:
        assert b.held == b.position % 8 and b.dpos == b.position // 8
        assert b.n256 == (b.position % 8 + b.samples) // 8 and b.n_pcm == (b.position + b.samples) // 256 and b.allowed
    # multi-block calls and single-block calls both
    assert {nb for _, nb, _ in w} >= {1, 100, 153}
    # the full block that fills every array: 16384 samples at 256 kS/s from 7 pending, 512 PCM samples
    full = [b for b in w.blocks if b.samples == W.FULL_BYTES // 2]
    assert [(b.position, b.n256, b.n_pcm) for b in full] == [(255, 16384, 512), (1, 16384, 512)]
    # even classes that keep a non-zero position
    assert {(b.samples, b.held) for b in w.blocks if b.samples in (256, 1000)} == {(256, 1), (1000, 1)}
    assert len({b.dpos for b in w.blocks if b.samples == 1000}) == 32
    # one call that completes nothing
    assert sum(b.n256 == 0 for b in w.blocks) == 1


def test_phase_sweep_fills_the_rows_and_never_exceeds_them():
    w = W.phase_sweep(W.WBFM)
    swept = [b for b in w.blocks if b.cls >= 0]
    at_capacity = sum(b.n_pcm == api.pcm_capacity(2 * b.samples) for b in swept)
    assert at_capacity == 946 and 3 * at_capacity >= len(swept) == 2560
    for b in w.blocks:
        assert b.n_pcm <= api.pcm_capacity(2 * b.samples) and 2 * b.n256 <= api.iq256_capacity(2 * b.samples)
    assert any(2 * b.n256 == api.iq256_capacity(2 * b.samples) and b.held == 7 for b in w.blocks)


@pytest.mark.parametrize("mode", MODES)
def test_inner_sweep_starts_every_class_from_every_position(mode):
    w = W.inner_sweep(mode)
    pairs = {(b.position, b.cls) for b in w.blocks if b.cls >= 0}
    assert len(pairs) == 32 * len(W.INNER_CLASSES) == 352
    resets = [b for (_, _, ev), b in zip(w, w.blocks) if ev]
    assert len(resets) == 2 and all(b.position == 0 for b in resets)
    before = [w.blocks[b.call - 1] for b in resets]
    assert all((p.position + p.samples) % 32 != 0 for p in before)          # the commutators were not at rest
    last = w.blocks[-1]
    assert (last.position, last.samples, last.n_pcm) == (15, 16384, 512) == (15, 16384, W.demod_pcm_capacity(32768))
    for b in w.blocks:
        assert b.n_pcm == (b.position + b.samples) // 32 <= W.demod_pcm_capacity(2 * b.samples)
        assert 2 * b.samples <= 32768


@pytest.mark.parametrize("mode", MODES)
def test_gated_walk_pulls_the_demodulators_away_from_the_front_end(mode):
    w = W.gated_walk(mode, _seed(mode))
    assert w.n_channels == 8
    ran = [b for b in w.blocks if b.allowed and b.mode != W.NONE]
    pairs = {(b.held, b.dpos) for b in ran}
    assert len(pairs) >= 250, len(pairs)
    # at one and the same block the channels' demodulators stand at different positions
    spread = max(len({b.dpos for b in w.blocks if b.call == k and b.block == 0}) for k in range(len(w)))
    assert spread >= 6
    kinds = [e[0] for _, _, ev in w for e in ev]
    assert kinds.count("mode") >= 5 and kinds.count("reset") >= 3 and kinds.count("gain") >= 2 and kinds.count("reduce") >= 15
    assert {bb // 2 for bb, _, ev in w if not any(e[0] == "reduce" for e in ev)} >= set(W.GATED_LENGTHS)
    assert sum(b.n256 == 0 for b in w.blocks) == w.n_channels              # one call that completes nothing
    for b in w.blocks:
        assert b.n_pcm <= api.pcm_capacity(2 * b.samples) and 2 * b.n256 <= api.iq256_capacity(2 * b.samples)


# ---------------------------------------------------------------- the oracle against the compiled reference
def _same(a, b, where):
    pa, ma, _, da = a
    pb, mb, _, db = b
    if pa is not None:
        assert len(pa) == len(pb) and (pa == pb).all(), where
        assert ma == mb, where
    assert len(da) == len(db) and (da == db).all(), where


@pytest.mark.parametrize("mode", MODES)
def test_oracle_equals_reference_on_the_phase_sweep(oracle, ref, mode):
    w = W.phase_sweep(mode)
    xs = W.sweep_inputs(w, 900 + mode)
    for c in range(xs.shape[0]):
        got = W.replay_outer(oracle.rx(), w, xs[c], 0)
        want = W.replay_outer(ref.rx(), w, xs[c], 0, mixes=False)
        for b, g, r in zip(w.blocks, got, want):
            _same(g, r, (c, b))
            assert len(g[0]) == b.n_pcm and len(g[3]) == 2 * b.n256 and g[2] == b.allowed, (c, b)
            if b.n256 == 0:
                assert g[1] == 0 and r[1] == 0, b


@pytest.mark.parametrize("mode", MODES)
def test_oracle_equals_reference_on_the_gated_walk(oracle, ref, mode):
    """Twice, because the compiled reference has no entry that resets a demodulator behind its IqDataProcessor (and
    oracle/_ref may be a prebuilt one: the harness stays as it is).  (a) the walk WITHOUT its resets through the
    reference's own acceptIqData: its gates, mode switches, gains and reduceSampleRate calls, call for call.  (b) the
    whole walk, resets included, against the reference's parts (tests/ragged_walks.py ChainOfParts): its front end and
    its demodulator objects with their own resetDemodulator, gated by the oracle's `allowed`."""
    w = W.gated_walk(mode, _seed(mode))
    xs = W.gated_inputs(w, 300 + mode)
    per_channel = len(w.blocks) // w.n_channels
    for c in range(w.n_channels):
        plain = W.replay_outer(oracle.rx(), w, xs[c], c, resets=False)
        want = W.replay_outer(ref.rx(), w, xs[c], c, mixes=False, resets=False)
        got = W.replay_outer(oracle.rx(), w, xs[c], c)
        parts = W.replay_outer(W.ChainOfParts(ref, [g[2] for g in got if g[0] is not None]), w, xs[c], c, mixes=False)
        books = [b for b in w.blocks if b.channel == c]
        assert len(books) == per_channel == len(got) == len(plain)
        for b, p, r, g, q in zip(books, plain, want, got, parts):
            _same(p, r, b)
            _same(g, q, b)
            assert len(g[3]) == 2 * b.n256, b
            if g[0] is not None:
                # `allowed` cannot be read from the reference: the oracle's, the bookkeeping's and the PCM count agree
                assert g[2] == b.allowed == p[2] and len(g[0]) == b.n_pcm == len(q[0]), b
        assert any(len(p[0]) != len(g[0]) for p, g in zip(plain, got) if g[0] is not None)   # the resets moved the commutators


@pytest.mark.parametrize("mode", MODES)
def test_oracle_equals_reference_on_the_inner_sweep(oracle, ref, mode):
    w = W.inner_sweep(mode)
    xs = W.inner_inputs(w, 500 + mode)
    for c in range(xs.shape[0]):
        got = W.replay_inner(oracle.demod(mode), w, xs[c])
        want = W.replay_inner(ref.demod(mode), w, xs[c])
        for b, g, r in zip(w.blocks, got, want):
            assert len(g) == len(r) == b.n_pcm and (g == r).all(), (c, b)
