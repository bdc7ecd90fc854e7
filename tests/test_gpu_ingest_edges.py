"""hrfd_ingest_* at its edges: the slot ring, the gain_db a slot was submitted with, the host replay of failed channels in
every arrangement of batches in flight, the modes, off-grid blocks, the state errors and what hrfd_ingest_destroy leaves
behind.  Every unit -- PCM, n_pcm, the zeros behind it, magnitude, gate -- against the sequential CPU oracle, bit-exact.

Shapes (tests/transport_support.py): 21504-byte blocks are the shortest that run as a speculative batch; they run on the
block kernels, which have no gated pass on the device, so a channel whose gate closes inside a batch is replayed by the
HOST in the shipped configuration too (the hook that switches the gated pass off is then only an extra).  32768 x 2 is the
smallest call hrfd_rx_plan.h gives to the WBFM flow kernel, where the gated pass exists."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import api, synth
from tests import transport_support as S
from tests.hooks import HOOKS_ON
from tests.reflib import NONE, AM, FM, WBFM, LSB, USB

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -4
BLK = synth.BLOCK_BYTES


def _views(ing):
    """hrfd_ingest_collect through the C ABI: the arrays IN PLACE (pinned memory of the slot), not copied"""
    ps = [C.c_void_p() for _ in range(4)]
    api.check(ing.L.hrfd_ingest_collect(ing.h, *[C.byref(p) for p in ps]), "hrfd_ingest_collect")
    units, cap = ing.C * ing.n_blocks, api.pcm_capacity(ing.block_bytes)

    def view(p, ctype, dtype, count, shape):
        return np.frombuffer((ctype * count).from_address(p.value), dtype=dtype).reshape(shape)

    cb = (ing.C, ing.n_blocks)
    return (view(ps[0], C.c_int16, np.int16, units * cap, cb + (cap,)), view(ps[1], C.c_uint32, np.uint32, units, cb),
            view(ps[2], C.c_uint32, np.uint32, units, cb), view(ps[3], C.c_uint8, np.uint8, units, cb))


def _submit(ing, xs, k, B, gain_db=0):
    ing.acquire()[...] = xs[:, k * B:(k + 1) * B]
    ing.submit(gain_db)


def _pipeline(ing, xs, B, n_slots, gains=None, first=0, last=None):
    """batches first .. last - 1 with the ring as full as it gets: -> their results in order (copies)"""
    last = xs.shape[1] // B if last is None else last
    out, submitted = [], first
    while first + len(out) < last:
        while submitted < last and submitted - first - len(out) < n_slots:
            _submit(ing, xs, submitted, B, 0 if gains is None else gains[submitted])
            submitted += 1
        out.append(ing.collect())
    return out


def _silence(xs, B, fails):
    """fails: {batch: channels}: both blocks of the batch silent -- the first is still let through (SignalTracker's one
    block of tail), the second is squelched: the batch, and no other, has a closed gate of that channel"""
    for k, chans in fails.items():
        for c in chans:
            xs[c, k * B:k * B + 2] = 0
    return xs


def _expected_replays(own, n_slots):
    """the slots hrfd_ingest_collect replays with the ring as full as it gets: a batch fails a channel of its own, or one
    that failed in a batch launched before it and has not been repaired since (the device's sticky flag) -- collect then
    redoes every batch in flight that has a failed channel.  -> (slots replayed, the largest number in flight at a replay)"""
    NB, poison, fail, out, submitted, replays, deepest = len(own), set(), {}, 0, 0, 0, 0
    while out < NB:
        while submitted < NB and submitted - out < n_slots:
            fail[submitted] = set(own[submitted]) | poison
            poison = set(fail[submitted]) | poison
            submitted += 1
        if fail[out]:
            deepest = max(deepest, submitted - out)
            for k in range(out, submitted):
                replays += 1 if fail[k] else 0
                fail[k] = set()
            poison = set()
        out += 1
    return replays, deepest


# ---------------------------------------------------------------- gain_db per slot
@pytest.mark.parametrize("shape", ["flow_gated_pass", "flow_host_replay", "block_kernels"])
def test_every_slot_is_replayed_with_its_own_gain_db(oracle, shape):
    """batches with gain_db 0 / G / 0 / G ..., three in flight: the tone of channels 0 and 2 is above their threshold at
    gain 0 and below it at gain G, so their gates close inside every second batch and those batches are redone -- by the
    device's gated pass, or by the host (gated pass off; block kernels) with the gain THAT slot was submitted with"""
    bb = S.SPEC if shape == "block_kernels" else S.FLOW
    Cn, B, NB, n_slots = 3, 2, 6, 3
    gains = [0, S.G] * (NB // 2)
    xs = S.tones(Cn, NB * B, bb, 200)
    thresholds = [S.FLIP_THRESHOLD, None, S.FLIP_THRESHOLD]
    want = S.Bank(oracle, [WBFM] * Cn, thresholds).run(xs, np.repeat(gains, B))
    for c in (0, 2):
        S.assert_flips(oracle, want, c, np.repeat(gains, B))
    assert want.allowed[1].all()
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    for c in (0, 2):
        rx.set_threshold(S.FLIP_THRESHOLD, c)
    if shape == "flow_host_replay":
        rx.debug_set_gated(False)
    ing = api.Ingest(rx, bb, B, n_slots)
    got = _pipeline(ing, xs, B, n_slots, gains)
    for k in range(NB):
        S.assert_batch(got[k], want, k, B)
    if shape != "flow_gated_pass":
        assert ing.replayed() >= NB // 2, ing.replayed()
    ing.close()
    rx.close()


# ---------------------------------------------------------------- the replay in every arrangement
def _case(name, n_slots):
    NB = max(7, n_slots + 2)
    return NB, {"ring_full_at_the_failure": {0: [0]},
                "two_channels_failing_in_successive_batches": {1: [0], 2: [1]},
                "failure_behind_a_clean_tail": {2: [2]},
                "failure_in_the_final_batch": {NB - 1: [1]},
                "every_channel_failing": {1: [0, 1, 2, 3], NB - 2: [3]}}[name]


_REPLAY_WANT = {}


@pytest.mark.parametrize("n_slots", [2, 3, 16])
@pytest.mark.parametrize("case", ["ring_full_at_the_failure", "two_channels_failing_in_successive_batches",
                                  "failure_behind_a_clean_tail", "failure_in_the_final_batch", "every_channel_failing"])
def test_host_replay_matrix(oracle, case, n_slots):
    """the host replay of hrfd_ingest_collect (the only repair of a channel the device did not redo), every batch of every
    channel against the sequential oracle.  The arrangement each case is named after is asserted on the schedule first"""
    Cn, B = 4, 2
    NB, fails = _case(case, n_slots)
    xs = _silence(S.tones(Cn, NB * B, S.SPEC, 300), B, fails)
    key = (case, NB)
    if key not in _REPLAY_WANT:
        _REPLAY_WANT[key] = S.Bank(oracle, [WBFM] * Cn, [-30] * Cn).run(xs, [0] * (NB * B))
    want = _REPLAY_WANT[key]
    own = S.own_failures(want, [WBFM] * Cn, B)
    assert own == [set(fails.get(k, ())) for k in range(NB)], own           # the inputs do what the case says
    replays, deepest = _expected_replays(own, n_slots)
    if case == "ring_full_at_the_failure":
        assert deepest == n_slots
    if case == "two_channels_failing_in_successive_batches":
        assert deepest >= 2 and replays >= 2                                 # batch 2 was in flight when batch 1 was repaired
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    rx.set_threshold(-30)
    if HOOKS_ON:
        rx.debug_set_gated(False)                                            # (no gated pass at this block length anyway)
    ing = api.Ingest(rx, S.SPEC, B, n_slots)
    got = _pipeline(ing, xs, B, n_slots)
    for k in range(NB):
        S.assert_batch(got[k], want, k, B)
    assert replays <= ing.replayed() <= NB, (ing.replayed(), replays)
    ing.close()
    rx.close()


def test_expired_wait_through_the_transport(oracle):
    """the shipped configuration (gated pass on): a workgroup of the flow kernel whose bounded wait expires fails its
    channel with kFailExpired, which the gated pass does not redo -- three batches in flight, the hook armed before the
    first: the host replays channel 0 in all three, and the stream continues exactly for two more batches"""
    Cn, B, NB = 3, 4, 5
    xs = np.stack([synth.make_input("fmtone", 60 + c, B * NB).reshape(B * NB, BLK) for c in range(Cn)])
    want = S.Bank(oracle, [WBFM] * Cn).run(xs, [0] * (NB * B))
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    rx.debug_expire(3)                                       # wait 3 is polled by every workgroup at its start
    ing = api.Ingest(rx, BLK, B, 3)
    got = _pipeline(ing, xs, B, 3)
    for k in range(NB):
        S.assert_batch(got[k], want, k, B)
    assert ing.replayed() == 3, ing.replayed()
    ing.close()
    rx.close()


# ---------------------------------------------------------------- modes
BANKS = {"fm": [FM, FM, FM], "am": [AM, AM, AM], "ssb": [LSB, USB, LSB], "mixed_with_none": [WBFM, NONE, AM, FM, USB]}


@pytest.mark.parametrize("gated", [True, False], ids=["shipped", "gated_pass_off"])
@pytest.mark.parametrize("bank", list(BANKS))
def test_modes_through_the_transport(oracle, bank, gated):
    """FM, AM, LSB / USB and a mixed bank with a mode-NONE channel; channel 0 (and the NONE channel) go silent inside
    batches 1 and 4.  Mode NONE has no demodulator: no PCM, n_pcm 0, but its magnitude and its gate are the detector's"""
    modes = BANKS[bank]
    Cn, B, NB, n_slots = len(modes), 2, 6, 3
    fails = {1: [0, 1] if bank == "mixed_with_none" else [0], 4: [0]}
    xs = _silence(S.tones(Cn, NB * B, S.SPEC, 400), B, fails)
    gain = [None] * Cn
    gain[-1] = 2.5                                           # one demodulator gain off its default
    want = S.Bank(oracle, modes, [-30] * Cn, gain).run(xs, [0] * (NB * B))
    assert not want.allowed[0].all()
    rx = api.Rx(Cn)
    for c, m in enumerate(modes):
        rx.set_mode(m, c)
    rx.set_gain(modes[-1], 2.5, Cn - 1)
    rx.set_threshold(-30)
    if not gated:
        rx.debug_set_gated(False)
    ing = api.Ingest(rx, S.SPEC, B, n_slots)
    got = _pipeline(ing, xs, B, n_slots)
    for k in range(NB):
        S.assert_batch(got[k], want, k, B)
    if bank == "mixed_with_none":
        assert not want.allowed[1].all() and want.mag[1].any()
        for k in range(NB):
            assert (got[k][0][1] == 0).all() and (got[k][1][1] == 0).all()
    assert ing.replayed() >= 2                               # block kernels: the host repairs, shipped or not
    if WBFM not in modes:
        # every block of every replay was exact at its first attempt: the failed batch left no channel marked, so no
        # launch of the replay was refused and redone (the FIR kinds have no speculation of their own that could fail)
        assert rx.debug_counters()[7] == 0, rx.debug_counters()
    ing.close()
    rx.close()


# ---------------------------------------------------------------- occupancy
def _walk(n_slots, NB):
    """a fixed seeded order of "submit" and "collect" over NB batches: long runs in one direction, so that the ring both
    fills up and drains"""
    rng = np.random.default_rng(1234 + n_slots)
    ops, submitted, collected = [], 0, 0
    while collected < NB:
        flight = submitted - collected
        want_submit = rng.random() < (0.8 if (submitted // (2 * n_slots)) % 2 == 0 else 0.35)
        if submitted < NB and flight < n_slots and (want_submit or flight == 0):
            ops.append("submit")
            submitted += 1
        else:
            ops.append("collect")
            collected += 1
    return ops


@pytest.mark.parametrize("n_slots", [2, 16])
def test_irregular_occupancy_and_results_held_in_place(oracle, n_slots):
    """a fixed seeded walk of submit and collect with 0 .. n_slots batches in flight, the ring wrapped more than three
    times.  The arrays collect returned for batch k are NOT copied: they are compared just before their slot is acquired
    again, after later collects and after replays of later batches (a channel goes silent in every fourth batch)"""
    Cn, B = 3, 2
    NB = max(3 * n_slots + 4, 24)
    fails = {k: [k % Cn] for k in range(2, NB, 4)}
    xs = _silence(S.tones(Cn, NB * B, S.SPEC, 500), B, fails)
    want = S.Bank(oracle, [WBFM] * Cn, [-30] * Cn).run(xs, [0] * (NB * B))
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    rx.set_threshold(-30)
    ing = api.Ingest(rx, S.SPEC, B, n_slots)
    held, submitted, collected, seen, checked = {}, 0, 0, set(), 0
    replays_while_held = 0
    for op in _walk(n_slots, NB):
        seen.add(submitted - collected)
        if op == "submit":
            old = submitted - n_slots
            if old in held:                                  # its slot is acquired next: the last moment the views are valid
                views, replayed_then = held.pop(old)
                S.assert_batch(views, want, old, B)
                replays_while_held += ing.replayed() - replayed_then
                checked += 1
            _submit(ing, xs, submitted, B)
            submitted += 1
        else:
            held[collected] = (_views(ing), ing.replayed())
            collected += 1
    for k, (views, _) in held.items():
        S.assert_batch(views, want, k, B)
    assert {0, n_slots} <= seen and checked >= 2 * n_slots and NB > 3 * n_slots, (seen, checked)
    assert replays_while_held > 0 and ing.replayed() >= len(fails)
    ing.close()
    rx.close()


# ---------------------------------------------------------------- off-grid blocks
def test_blocks_off_the_512_byte_grid(oracle):
    """21762-byte blocks (42.5 PCM samples and an odd number of IQ samples), two per batch: the handle leaves the grid and every batch runs on k_rx_ragged; the rows have
    hrfd_rx_pcm_capacity(block_bytes) samples and n_pcm varies from block to block"""
    bb, B, NB = 21762, 2, 4
    modes = [WBFM, AM, FM]
    xs = _silence(S.tones(3, NB * B, bb, 600), B, {1: [0]})
    want = S.Bank(oracle, modes, [-30] * 3).run(xs, [0] * (NB * B))
    assert len({len(p) for p in want.pcm[1]}) > 1 and not want.allowed[0].all()
    rx = api.Rx(3)
    for c, m in enumerate(modes):
        rx.set_mode(m, c)
    rx.set_threshold(-30)
    ing = api.Ingest(rx, bb, B, 2)
    got = _pipeline(ing, xs, B, 2)
    assert got[0][0].shape == (3, B, api.pcm_capacity(bb)) and api.pcm_capacity(bb) == 43
    for k in range(NB):
        S.assert_batch(got[k], want, k, B)
    offgrid, launches = rx.debug_ragged()
    assert offgrid and launches >= NB
    ing.close()
    rx.close()


# ---------------------------------------------------------------- the handle between batches
def test_setters_on_the_drained_handle(oracle):
    """collect everything, change mode, demodulator gain and threshold on the rx handle, submit more: the oracle does the
    same between the same blocks"""
    Cn, B, NB = 3, 2, 6
    xs = _silence(S.tones(Cn, NB * B, S.SPEC, 700), B, {4: [1]})
    bank = S.Bank(oracle, [WBFM, FM, AM])
    w1 = bank.run(xs[:, :3 * B], [0] * (3 * B))
    bank.rx[0].set_mode(FM)
    bank.rx[1].set_threshold(-30)
    bank.rx[2].set_gain(AM, 3.0)
    w2 = bank.run(xs[:, 3 * B:], [0] * (3 * B))
    assert not w2.allowed[1].all()
    rx = api.Rx(Cn)
    for c, m in enumerate([WBFM, FM, AM]):
        rx.set_mode(m, c)
    ing = api.Ingest(rx, S.SPEC, B, 2)
    got = _pipeline(ing, xs, B, 2, last=3)
    rx.set_mode(FM, 0)
    rx.set_threshold(-30, 1)
    rx.set_gain(AM, 3.0, 2)
    got += _pipeline(ing, xs, B, 2, first=3)
    for k in range(3):
        S.assert_batch(got[k], w1, k, B)
        S.assert_batch(got[3 + k], w2, k, B)
    ing.close()
    rx.close()


def test_collect_with_each_out_pointer_null(oracle):
    Cn, B, NB = 3, 2, 5
    xs = S.tones(Cn, NB * B, S.SPEC, 800)
    want = S.Bank(oracle, [WBFM] * Cn).run(xs, [0] * (NB * B))
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    ing = api.Ingest(rx, S.SPEC, B, 2)
    units, cap = Cn * B, api.pcm_capacity(S.SPEC)
    shapes = [(C.c_int16, np.int16, (Cn, B, cap)), (C.c_uint32, np.uint32, (Cn, B)), (C.c_uint32, np.uint32, (Cn, B)),
              (C.c_uint8, np.uint8, (Cn, B))]
    for k in range(NB):
        _submit(ing, xs, k, B)
        ps = [C.c_void_p() for _ in range(4)]
        args = [None if (i == k or k == 4) else C.byref(p) for i, p in enumerate(ps)]     # batch 4: all four NULL
        assert ing.L.hrfd_ingest_collect(ing.h, *args) == 0
        got = []
        for i, (ctype, dtype, shape) in enumerate(shapes):
            if args[i] is None:
                assert ps[i].value is None
                got.append(None)
            else:
                got.append(np.frombuffer((ctype * int(np.prod(shape))).from_address(ps[i].value), dtype=dtype).reshape(shape))
        if got[0] is not None:
            S.assert_batch(got, want, k, B, what=("pcm", "mag", "allowed") + (("n_pcm",) if got[1] is not None else ()))
        else:
            assert k in (0, 4)
            if k == 0:
                assert (got[1] == [[len(want.pcm[c][b]) for b in range(B)] for c in range(Cn)]).all()
                assert (got[2] == want.mag[:, :B]).all() and (got[3].astype(bool) == want.allowed[:, :B]).all()
    ing.close()
    rx.close()


def test_state_errors_leave_the_pipeline_intact(oracle):
    Cn, B, NB = 3, 2, 5
    xs = S.tones(Cn, NB * B, S.SPEC, 900)
    want = S.Bank(oracle, [WBFM] * Cn).run(xs, [0] * (NB * B))
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    ing = api.Ingest(rx, S.SPEC, B, 2)
    L, p = ing.L, C.c_void_p()
    four = [C.byref(C.c_void_p()) for _ in range(4)]
    assert L.hrfd_ingest_collect(ing.h, *four) == ESTATE                     # nothing submitted
    assert L.hrfd_ingest_submit(ing.h, 0) == ESTATE                          # nothing acquired
    _submit(ing, xs, 0, B)
    assert L.hrfd_ingest_submit(ing.h, 0) == ESTATE
    slot = ing.acquire()
    assert L.hrfd_ingest_acquire(ing.h, C.byref(p)) == ESTATE and p.value is None   # the acquired slot is not handed out twice
    slot[...] = xs[:, B:2 * B]
    ing.submit(0)
    assert L.hrfd_ingest_acquire(ing.h, C.byref(p)) == ESTATE and p.value is None   # both slots in flight
    assert L.hrfd_ingest_acquire(ing.h, None) == EINVAL
    got = [ing.collect()]
    _submit(ing, xs, 2, B)
    assert L.hrfd_ingest_acquire(ing.h, C.byref(p)) == ESTATE
    got += [ing.collect(), ing.collect()]
    assert L.hrfd_ingest_collect(ing.h, *four) == ESTATE
    got += _pipeline(ing, xs, B, 2, first=3)
    for k in range(NB):
        S.assert_batch(got[k], want, k, B)
    assert ing.replayed() == 0
    ing.close()
    rx.close()


def test_create_refusals():
    rx = api.Rx(2)
    L = rx.L
    h = C.c_void_p(0x1234)
    for bb, nb, ns in [(S.SPEC, 2, 1), (S.SPEC, 2, 17), (S.SPEC, 2, 0), (S.SPEC + 1, 2, 2), (0, 2, 2), (BLK + 2, 2, 2),
                       (BLK + 1, 1, 2), (S.SPEC, 0, 2)]:
        assert L.hrfd_ingest_create(rx.h, bb, nb, ns, C.byref(h)) == EINVAL, (bb, nb, ns)
        assert L.hrfd_last_error().decode().startswith("hrfd_ingest_create")
        assert h.value == 0x1234
    assert L.hrfd_ingest_create(None, S.SPEC, 2, 2, C.byref(h)) == EINVAL
    assert L.hrfd_ingest_create(rx.h, S.SPEC, 2, 2, None) == EINVAL
    for ns in (2, 16):                                                       # the limits themselves are taken
        ing = api.Ingest(rx, BLK if ns == 2 else 2, 1, ns)
        ing.close()
    rx.close()


# ---------------------------------------------------------------- destroy
@pytest.mark.parametrize("behind", ["clean_batches", "a_failed_batch"])
def test_destroy_with_batches_in_flight_leaves_the_sequential_state(oracle, behind):
    """hrfd_ingest_destroy with uncollected batches: the rx handle is where a sequential caller stands after every
    SUBMITTED batch -- behind a failed batch too (channel 0's gate closes in batch 1; batch 2 is in flight behind it):
    failed channels are replayed, nothing stays poisoned, and the stream goes on through hrfd_rx_process_block"""
    Cn, B, NB = 3, 2, 5
    fails = {1: [0]} if behind == "a_failed_batch" else {}
    xs = _silence(S.tones(Cn, NB * B, S.SPEC, 1000), B, fails)
    want = S.Bank(oracle, [WBFM] * Cn, [-30] * Cn).run(xs, [0] * (NB * B))
    assert want.allowed[0].all() == (not fails)
    rx = api.Rx(Cn)
    rx.set_mode(WBFM)
    rx.set_threshold(-30)
    if fails and HOOKS_ON:
        rx.debug_set_gated(False)                            # (no gated pass at this block length anyway)
    ing = api.Ingest(rx, S.SPEC, B, 3)
    got = [None] * NB
    _submit(ing, xs, 0, B)
    got[0] = ing.collect()
    _submit(ing, xs, 1, B)
    _submit(ing, xs, 2, B)
    ing.acquire()                                            # a slot that was handed out and never submitted: not a batch
    ing.close()
    for k in (3, 4):
        got[k] = rx.process_block(xs[:, k * B:(k + 1) * B], B)[:4]
    for k in (0, 3, 4):
        S.assert_batch(got[k], want, k, B)
    rx.close()
