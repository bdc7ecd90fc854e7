"""The squelch detector on the device, swept over every block mean, both sides of every threshold and several receive
gains, on every kernel that holds a copy of it -- each output bit for bit against the CPU oracle.

The bank: one channel per block mean 0..192 (a DC pair found with the oracle's front end: tests/squelch_inputs.py), a
few more with raw -128 on one rail, six blocks of 32 KiB each -- loud, loud, silent, silent, loud, loud -- so that with
the threshold on the channel's own level the tracker meets all four (tracking, present) pairs inside one call.  Sixteen
channels have their last block perturbed until its magnitude sum is 1..8 below a multiple of the sample count (a sample
counted twice changes that block's mean); their second block is pure DC (sum an exact multiple: a sample lost changes
it).  Channel c's threshold is its steady level L plus (c // 9 + c + g) % 3 - 1, where g numbers the receive gain: over the
three gains every channel sees L-1, L and L+1.

What was REACHED is asserted from the oracle's 256 kS/s dumps through tests/squelch_model.py (never from device
output): table indices 0..127 complete and clamped means, level - threshold in {-1, 0, +1}, both remainders, the four
tracker transitions -- per configuration, so on every path that takes it.  Mutants of the detector (>= to >, the gain
term dropped, the clamp at 126, a table entry off by one, half the lanes of the reduction lost, n + 1 in the division,
the host's may_close shortcut off by one or without its gain term, the tail block dropped) each fail tests of this file."""
import functools

import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import squelch_inputs as si
from tests import squelch_model as sm
from tests.hooks import HOOKS_ON
from tests.reflib import AM, FM, WBFM, LSB, USB, NONE

pytestmark = pytest.mark.gpu

BB, B = 32768, 6
PATTERN = "110011"
GAINS = [0, 6, 40]
REM_MEANS = [12 * k for k in range(1, 17)]                  # 12 .. 192: the channels whose last block is perturbed
EXTRA_PAIRS = [(-128, 3), (3, -128), (-128, -128), (127, -128)]
ALL_PAIRS = {(False, False), (False, True), (True, False), (True, True)}
KINDS = {"wbfm": [WBFM], "fm": [FM], "am_ssb": [AM, LSB, USB],
         "mixed": [WBFM, FM, AM, WBFM, FM, LSB, WBFM, FM, USB]}


# ------------------------------------------------------------------------------------------------ the bank and what it reaches
@functools.lru_cache(maxsize=None)
def _bank(oracle, bb=BB, lead=0):
    """-> (x int8 [C, B, bb], lead-in int8 [C, lead], model blocks [C][B] (threshold-free: sum, n, mean), dumps)"""
    table = oracle.dbfs_table()
    pairs = si.dc_pairs(oracle)
    assert sorted(pairs) == list(range(si.MAX_MEAN + 1)), "a block mean no DC input reaches"
    chans = [pairs[m] for m in range(si.MAX_MEAN + 1)] + EXTRA_PAIRS
    C = len(chans)
    x = np.zeros((C, B, bb), dtype=np.int8)
    head = np.zeros((C, lead), dtype=np.int8)
    for c, pair in enumerate(chans):
        head[c] = si.dc_block(pair, lead)
        for b, ch in enumerate(PATTERN):
            if ch == "1":
                x[c, b] = si.dc_block(pair, bb)
    for m in REM_MEANS:
        y = si.perturb_below_multiple(oracle, table, [head[m]] * (lead > 0) + list(x[m, :B - 1]), x[m, B - 1], seed=m)
        assert y is not None, f"no perturbation of mean {m} leaves its sum just below a multiple of n"
        x[m, B - 1] = y
    blocks = []
    for c in range(C):
        dumps = si.dumps_of(oracle, [head[c]] * (lead > 0) + list(x[c]))[(lead > 0):]
        blocks.append([sm.detect(table, d, 0) for d in dumps])
    return x, head, blocks


def _modes(kind, g, C):
    cyc = KINDS[kind]
    modes = [cyc[(c + g) % len(cyc)] for c in range(C)]
    if kind == "mixed":
        modes = [NONE if c % 16 == 15 else m for c, m in enumerate(modes)]   # channels without a demodulator detect too
    return modes


def _thresholds(oracle, blocks, g):
    table = oracle.dbfs_table()
    return [sm.level(table, blk[1].mean, GAINS[g]) + (c // 9 + c + g) % 3 - 1 for c, blk in enumerate(blocks)]


@functools.lru_cache(maxsize=None)
def _expect(oracle, kind, g, bb=BB, lead=0):
    """the oracle's outputs for a configuration, held to the model, and the proof of what the configuration reaches"""
    table = oracle.dbfs_table()
    x, head, blocks = _bank(oracle, bb, lead)
    C = x.shape[0]
    modes, thr, gain = _modes(kind, g, C), _thresholds(oracle, blocks, g), GAINS[g]
    want, indices, clamped, deltas, pairs_seen, per_mode_pairs = [], set(), set(), set(), set(), {}
    for c in range(C):
        o = oracle.rx()
        o.set_mode(modes[c]); o.set_threshold(thr[c]); o.gain_db = gain
        if lead:
            o.process(head[c])
        t = sm.Tracker()
        if lead:
            t.run(sm.level(table, sm.detect(table, si.dumps_of(oracle, [head[c]])[0], 0).mean, gain) >= thr[c])
        rows = []
        for b in range(B):
            p, m, a, _ = o.process(x[c, b])
            blk = blocks[c][b]
            db = sm.level(table, blk.mean, gain)
            allowed, seen = t.run(db >= thr[c])
            assert (m, a) == (blk.mean, allowed), ("oracle != model", kind, g, c, b)
            assert (len(p) > 0) == (modes[c] != NONE and a) and (lead or len(p) in (0, bb // 512)), (kind, g, c, b)
            rows.append((p, m, a))
            indices.add(blk.index)
            if blk.mean > 127:
                clamped.add(blk.mean)
            deltas.add(db - thr[c])
            pairs_seen.add(seen)
            per_mode_pairs.setdefault(modes[c], set()).add(seen)
        want.append(rows)
    # proof of reach, from the model alone
    assert indices == set(range(128)), sorted(set(range(128)) - indices)
    assert clamped >= set(range(128, si.MAX_MEAN + 1))
    assert deltas >= {-1, 0, 1}
    assert pairs_seen == ALL_PAIRS and all(v == ALL_PAIRS for v in per_mode_pairs.values()), per_mode_pairs
    assert gain == GAINS[g] and (g == 0 or gain != 0)
    for m in REM_MEANS:
        hi, lo = blocks[m][B - 1], blocks[m][1]
        assert m > 8 and hi.n - 8 <= hi.rem <= hi.n - 1 and 0 <= lo.rem <= 7 and lo.mean == m, (m, hi, lo)
        assert (hi.n & (hi.n - 1) != 0) == bool(lead), "n is a power of two exactly on the grid"
    return x, head, modes, thr, want


def _rx(oracle, kind, g, bb=BB, lead=0):
    x, head, modes, thr, want = _expect(oracle, kind, g, bb, lead)
    rx = api.Rx(x.shape[0])
    for c in range(x.shape[0]):
        rx.set_mode(modes[c], channel=c)
        rx.set_threshold(thr[c], channel=c)
    rx.gain_db = GAINS[g]
    return rx, x, head, want


def _check(got, want, b0=0, what=""):
    """got = (pcm [C, nb, cap], n_pcm, magnitude, allowed) of blocks b0.. against the oracle's rows; names the first
    channel (= block mean) and block that differ"""
    pcm, n_pcm, mag, allowed = got[:4]
    bad = []
    for c in range(len(want)):
        for k in range(pcm.shape[1]):
            p, m, a = want[c][b0 + k]
            if int(mag[c, k]) != m or bool(allowed[c, k]) != a or int(n_pcm[c, k]) != len(p):
                bad.append((c, b0 + k, "magnitude/allowed/n_pcm", (int(mag[c, k]), bool(allowed[c, k]), int(n_pcm[c, k])), (m, a, len(p))))
            elif not (pcm[c, k, :len(p)] == p).all():
                bad.append((c, b0 + k, "pcm"))
    assert not bad, (what, len(bad), bad[:6])


# ------------------------------------------------------------------------------------------------ every kernel with a detector
@pytest.mark.parametrize("g", range(3), ids=[f"gain{v}" for v in GAINS])
def test_per_block_kernels(oracle, g):
    """n_blocks = 1: k_rx_wbfm / k_rx_fir, the reference's cadence"""
    rx, x, _, want = _rx(oracle, "mixed", g)
    for b in range(B):
        _check(rx.process_block(x[:, b], 1), want, b, "per-block")


@pytest.mark.parametrize("g", range(3), ids=[f"gain{v}" for v in GAINS])
def test_batch_block_kernels(oracle, g):
    """the block kernels over a batch (runs of two blocks per WBFM workgroup), closed gates replayed by the host; in the
    shipped state the same batch on the dispatch a user gets"""
    rx, x, _, want = _rx(oracle, "mixed", g)
    if HOOKS_ON:
        rx.debug_set_fir_flow(0)
        rx.debug_set_stream(0)
        rx.debug_set_run_len(2)
    _check(rx.process_block(x, B), want, 0, "batch, block kernels")


@pytest.mark.parametrize("g", range(3), ids=[f"gain{v}" for v in GAINS])
@pytest.mark.parametrize("kind", ["wbfm", "fm", "am_ssb"])
def test_flow_kernel_one_kind(oracle, kind, g):
    """k_rx_wbfm_flow in its three modes: a bank of one kind, large enough to go there by itself; the gates that close
    inside the batch are redone by the gated pass"""
    rx, x, _, want = _rx(oracle, kind, g)
    _check(rx.process_block(x, B), want, 0, kind)


@pytest.mark.parametrize("g", range(3), ids=[f"gain{v}" for v in GAINS])
@pytest.mark.parametrize("gated", [True, False], ids=["gated_pass", "host_replay"])
def test_flow_bank_and_its_host_replay_twin(oracle, gated, g):
    """k_rx_flow_bank: every kind in one launch, with the gated pass behind it, and the same with the gated pass off
    (the host replays the channels whose gates closed)"""
    rx, x, _, want = _rx(oracle, "mixed", g)
    if not gated:
        rx.debug_set_gated(False)
    _check(rx.process_block(x, B), want, 0, "bank")
    c = rx.debug_counters()
    print(f"\ncounters {'gated' if gated else 'host replay'} gain {GAINS[g]}: {c}")
    # c[5]: channels a launch of this handle left uncommitted (the host then replays them block by block)
    if gated:
        assert c[5] == 0, ("the gated pass left a channel to the host", c)
    else:
        assert c[5] > 0, ("closed gates and no gated pass: the host must have replayed channels", c)


@pytest.mark.parametrize("g", range(3), ids=[f"gain{v}" for v in GAINS])
def test_ragged_kernel(oracle, g):
    """k_rx_ragged: the bank after one 1000-byte call, blocks of 30000 bytes (1875 samples at 256 kS/s a block: not a
    power of two, and four raw samples pending throughout)"""
    rx, x, head, want = _rx(oracle, "mixed", g, 30000, 1000)
    rx.process_block(head, 1)
    assert rx.debug_ragged()[0] is True and rx.pending_samples() == 4
    n0 = rx.debug_ragged()[1]
    _check(rx.process_block(x[:, :2], 2), want, 0, "ragged")
    for b in range(2, B):
        _check(rx.process_block(x[:, b], 1), want, b, "ragged")
    assert rx.debug_ragged()[1] > n0


def test_more_than_64_blocks_in_one_call(oracle):
    """host chunking: 72 blocks of 32 KiB in one call (chunks of 64 and 8), the bank's six blocks twelve times over, so
    gates close and reopen in both chunks and across the boundary; every 8th channel of the bank, receive gain 6"""
    g = 1
    x, _, blocks = _bank(oracle)
    table = oracle.dbfs_table()
    sel = list(range(4, x.shape[0], 8))
    modes = _modes("mixed", g, x.shape[0])
    thr = _thresholds(oracle, blocks, g)
    reps = 12
    xs = np.concatenate([x[sel]] * reps, axis=1)
    rx = api.Rx(len(sel))
    want, closed, deltas = [], [0, 0], set()
    for i, c in enumerate(sel):
        rx.set_mode(modes[c], channel=i); rx.set_threshold(thr[c], channel=i)
        o = oracle.rx(); o.set_mode(modes[c]); o.set_threshold(thr[c]); o.gain_db = GAINS[g]
        rows = [o.process(xs[i, b])[:3] for b in range(reps * B)]
        dumps = si.dumps_of(oracle, list(xs[i]))
        _, allowed, _ = sm.run(table, dumps, thr[c], GAINS[g])
        assert allowed == [r[2] for r in rows], ("oracle != model", c)
        deltas |= {sm.detect(table, d, thr[c], GAINS[g]).dbfs - thr[c] for d in dumps}
        if modes[c] != NONE:
            closed[0] += sum(not a for a in allowed[:64]); closed[1] += sum(not a for a in allowed[64:])
        want.append(rows)
    assert closed[0] > 0 and closed[1] > 0 and deltas >= {-1, 0, 1}
    rx.gain_db = GAINS[g]
    if HOOKS_ON:
        rx.debug_set_run_len(64)
        rx.debug_set_fir_flow(1)
    _check(rx.process_block(xs, reps * B), want, 0, "72 blocks")


# ------------------------------------------------------------------------------------------------ the host's shortcut
@pytest.mark.parametrize("gain", GAINS, ids=[f"gain{v}" for v in GAINS])
@pytest.mark.parametrize("kind", ["wbfm", "fm", "am_ssb", "mixed"])
def test_threshold_on_the_lowest_level(oracle, kind, gain):
    """may_close: with every threshold at -42 - gain_db (the level of silence) no gate can close and the gated pass may
    be skipped; with ONE channel at -41 - gain_db it must run.  Six batches on one handle: (1) all at -42 - gain;
    (2) channel 17 at -41 - gain: its silent blocks close after one tail block, nobody else's; (3) back; (4) channel 5
    without a demodulator and at -41 - gain: its `allowed` follows the detector, the others stay open; (5) channel 5 gets
    its demodulator back, the threshold still in place: it closes; (6) channel 5 without a demodulator again."""
    table = oracle.dbfs_table()
    C, nb = 50, 5
    cyc = KINDS[kind]
    modes = [cyc[c % len(cyc)] for c in range(C)]
    rng = np.random.default_rng(7)
    loud = rng.integers(-60, 61, size=(C, 6 * nb, BB)).astype(np.int8)
    for k in range(6):
        loud[:, k * nb + 1:k * nb + 3] = 0                   # silent, silent inside every batch
        loud[:, k * nb + 4] = 0                              # and a silent last block: the tail crosses into the next batch
    rx = api.Rx(C)
    orc = []
    for c in range(C):
        rx.set_mode(modes[c], channel=c)
        o = oracle.rx(); o.set_mode(modes[c]); o.gain_db = gain; orc.append(o)
    rx.gain_db = gain
    lo, hi = -42 - gain, -41 - gain
    # A shortcut that wrongly skips the gated pass does not change the outputs of this entry (the channel fails its
    # "all gates open" speculation and the host replays it): it shows as a channel left uncommitted.  One run per channel
    # (nothing else is speculated) where the bank's shape is the test's to choose; the FIR kinds have one anyway.
    strict = HOOKS_ON or kind in ("fm", "am_ssb")
    if HOOKS_ON:
        rx.debug_set_run_len(64)

    def both(fn, *a, channel=None):
        getattr(rx, fn)(*a, **({} if channel is None else {"channel": channel}))
        for c in (range(C) if channel is None else [channel]):
            getattr(orc[c], fn)(*a)

    steps = [lambda: both("set_threshold", lo),
             lambda: both("set_threshold", hi, channel=17),
             lambda: both("set_threshold", lo, channel=17),
             lambda: (both("set_mode", NONE, channel=5), both("set_threshold", hi, channel=5)),
             lambda: both("set_mode", modes[5], channel=5),
             lambda: both("set_mode", NONE, channel=5)]
    closing = {0: [], 1: [17], 2: [], 3: [5], 4: [5], 5: [5]}
    for k, step in enumerate(steps):
        step()
        xs = loud[:, k * nb:(k + 1) * nb]
        want = []
        for c in range(C):
            rows = []
            for b in range(nb):
                p, m, a, d = orc[c].process(xs[c, b])
                blk = sm.detect(table, d, hi if c in closing[k] else lo, gain)
                assert blk.mean == m
                if not xs[c, b].any():
                    assert blk.dbfs == -42 - gain and blk.present == (c not in closing[k]), (k, c, b)
                else:
                    assert blk.present, "the loud blocks are above both thresholds"
                rows.append((p, m, a))
            al = [r[2] for r in rows]
            # silent blocks 1, 2, 4: with the threshold one above silence, block 1 is the tail and block 2 closes
            assert al == ([True, True, False, True, True] if c in closing[k] else [True] * 5), (k, c, al)
            want.append(rows)
        _check(rx.process_block(xs, nb), want, 0, f"batch {k + 1}")
        if strict:
            assert rx.debug_counters()[5] == 0, (f"batch {k + 1}: a closed gate was left to the host", rx.debug_counters())


# ------------------------------------------------------------------------------------------------ gain_db through every entry
def test_process_device_with_gain(oracle):
    import torch
    g = 2
    rx, x, _, want = _rx(oracle, "mixed", g)
    dev = torch.device("cuda:0")
    C = x.shape[0]
    d_x = torch.from_numpy(x).to(dev)
    pcm = torch.zeros((C, B, BB // 512), dtype=torch.int16, device=dev)
    n = torch.zeros((C, B), dtype=torch.int32, device=dev)
    mag = torch.zeros((C, B), dtype=torch.int32, device=dev)
    al = torch.zeros((C, B), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rx.process_device(d_x.data_ptr(), B * BB, BB, B, pcm.data_ptr(), n.data_ptr(), mag.data_ptr(), al.data_ptr())
    failed = rx.sync()
    if failed == 0:                                          # (channels that did not commit are the caller's to replay)
        _check([t.cpu().numpy() for t in (pcm, n, mag, al)], want, 0, "process_device")
    else:
        ok = rx.failed_channels() == 0
        got = [t.cpu().numpy()[ok] for t in (pcm, n, mag, al)]
        _check(got, [w for w, k in zip(want, ok) if k], 0, "process_device, committed channels")
        assert ok.sum() > len(want) // 2


@pytest.mark.parametrize("g", [1, 2], ids=["gain6", "gain40"])
def test_ingest_with_gain(oracle, g):
    rx, x, _, want = _rx(oracle, "mixed", g)
    rx.gain_db = 0                                           # the transport carries its own gain argument
    ing = api.Ingest(rx, BB, B, 2)
    ing.acquire()[...] = x
    ing.submit(GAINS[g])
    got = [np.array(a) for a in ing.collect()]
    ing.close()
    _check(got, want, 0, "ingest")


@pytest.mark.parametrize("g", [1, 2], ids=["gain6", "gain40"])
def test_fanout_with_gain(oracle, g):
    """hrfd_fanout_process(gain_db): the fan-out hands back PCM and its counts only, so `allowed` shows as n_pcm"""
    import torch
    x, _, modes, thr, want = _expect(oracle, "mixed", g)
    C = x.shape[0]
    dev = torch.device("cuda:0")
    fo = api.Fanout(C, [0, 0, 0])
    for c in range(C):
        fo.set_mode(modes[c], channel=c)
        fo.set_threshold(thr[c], channel=c)
    d_x = torch.from_numpy(x).to(dev)
    out = torch.zeros((C, B, BB // 512), dtype=torch.int16, device=dev)
    npcm = torch.zeros((C, B), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    fo.scatter(0, d_x.data_ptr(), BB, B)
    fo.process(GAINS[g])
    fo.collect(0, out.data_ptr(), npcm.data_ptr())
    got, gn = out.cpu().numpy(), npcm.cpu().numpy()
    bad = [(c, b) for c in range(C) for b in range(B)
           if gn[c, b] != len(want[c][b][0]) or not (got[c, b, :gn[c, b]] == want[c][b][0]).all()]
    assert not bad, bad[:8]
    assert any(len(want[c][b][0]) == 0 for c in range(C) for b in range(B) if modes[c] != NONE)


@pytest.mark.parametrize("gain", [6, 40])
@pytest.mark.parametrize("mode", [WBFM, FM])
def test_ddc_receive_with_gain(oracle, mode, gain):
    """hrfd_ddc_receive takes the receive gain from the Rx it feeds: the scenario of the DDC suite whose level drops
    inside the batch, threshold and gain moved together (the decision is the same, the level is gain_db lower)"""
    import torch
    from tests.test_gpu_ddc import BATCH_BLOCK, _receive_case
    al, _, _ = _receive_case(torch, torch.device("cuda:0"), oracle, mode, 2, BATCH_BLOCK, 12, threshold=-30 - gain,
                             level_drop=True, gain_db=gain, seed=9 + mode)
    assert al[:, 0].all() and not al[:, -1].any(), "the scenario must open and then close the gates"
    al0, _, _ = _receive_case(torch, torch.device("cuda:0"), oracle, mode, 2, BATCH_BLOCK, 12, threshold=-30 - gain,
                              level_drop=True, gain_db=0, seed=9 + mode)
    assert al0.sum() > al.sum(), "without the gain the same threshold lets more blocks through: the gain decided"
