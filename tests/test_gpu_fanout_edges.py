"""hrfd_fanout_* at its edges, several shards on one device: the "host feeds every shard itself" path (hrfd_fanout_input),
scatter and input mixed with changing block sizes, the gain_db and the count of the replay in collect, the setters across
shard boundaries, and the one-batch-at-a-time state machine.  Against the sequential CPU oracle (and one hrfd_rx over the
whole bank where that is the same device code in another partition), bit-exact."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import transport_support as S
from tests.reflib import NONE, AM, FM, WBFM, LSB, USB

pytestmark = pytest.mark.gpu
EINVAL, ESTATE = -1, -4
H2D = 1


def _fill_through_input(fo, xs_batch, bb, B, n_shards):
    """every shard's input buffer filled by the host itself, no scatter: checks what hrfd_fanout_input says it owns"""
    rt = _lib._load_hip_runtime()
    Cn = xs_batch.shape[0]
    bufs = [fo.input(g, bb, B) for g in range(n_shards)]      # (the first call sizes every shard's buffer)
    for g, (ptr, first, count) in enumerate(bufs):
        assert (first, count) == api.fanout_channel_range(Cn, n_shards, g), g
        assert ptr != 0 and fo.input(g, bb, B)[0] == ptr
        rows = np.ascontiguousarray(xs_batch[first:first + count])
        assert rows.nbytes == count * B * bb
        assert rt.hipMemcpy(C.c_void_p(ptr), C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), H2D) == 0


def _collect(fo, torch, Cn, B, bb, with_n_pcm=True):
    cap = api.pcm_capacity(bb)
    out = torch.full((Cn, B, cap), 0x5A5A, dtype=torch.int16, device="cuda:0")
    npcm = torch.full((Cn, B), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0") if with_n_pcm else None
    torch.cuda.synchronize()
    replayed = fo.collect(0, out.data_ptr(), npcm.data_ptr() if with_n_pcm else None)
    return (out.cpu().numpy(), npcm.cpu().numpy().view(np.uint32) if with_n_pcm else None), replayed


def _scatter(fo, torch, xs_batch, bb, B, stream=None):
    if stream is None:
        x = torch.from_numpy(np.ascontiguousarray(xs_batch)).to("cuda:0")
        torch.cuda.synchronize()
        fo.scatter(0, x.data_ptr(), bb, B)
    else:
        with torch.cuda.stream(stream):
            x = torch.from_numpy(np.ascontiguousarray(xs_batch)).to("cuda:0")
        fo.scatter(0, x.data_ptr(), bb, B, src_stream=stream.cuda_stream)
    return x


def _modes(Cn):
    return [[WBFM, AM, FM, LSB, NONE, USB][c % 6] for c in range(Cn)]


@pytest.mark.parametrize("n_shards,Cn", [(5, 5), (3, 7), (4, 9)], ids=["a_channel_per_shard", "3_2_2", "3_2_2_2"])
def test_input_path_equals_one_handle_and_the_oracle(oracle, n_shards, Cn):
    import torch
    bb, B, NB = S.SPEC, 2, 2
    modes = _modes(Cn)
    xs = S.tones(Cn, NB * B, bb, 1100)
    xs[1, 1:3] = 0                                           # a gate that closes inside the second batch
    want = S.Bank(oracle, modes, [-30] * Cn).run(xs, [0] * (NB * B))
    fo, one = api.Fanout(Cn, [0] * n_shards), api.Rx(Cn)
    assert fo.shards() == n_shards
    for c, m in enumerate(modes):
        fo.set_mode(m, c)
        one.set_mode(m, c)
    fo.set_threshold(-30)
    one.set_threshold(-30)
    for k in range(NB):
        _fill_through_input(fo, xs[:, k * B:(k + 1) * B], bb, B, n_shards)
        fo.process(0)
        got, replayed = _collect(fo, torch, Cn, B, bb)
        S.assert_batch(got, want, k, B)
        ref = one.process_block(xs[:, k * B:(k + 1) * B], B)
        assert (got[0] == ref[0]).all() and (got[1] == ref[1]).all()
        assert replayed == len(S.own_failures(want, modes, B)[k])
    assert not want.allowed[1].all()
    fo.close()
    one.close()


def test_scatter_and_input_mixed_with_changing_sizes(oracle):
    """four batches, scatter / input / scatter / input: the second larger in both block length and count (the shards'
    buffers grow), the third smaller (one block: the exact path; the buffers keep their size), the fourth off the 512-byte
    grid (k_rx_ragged from there on).  One stream per channel through all of it"""
    import torch
    Cn, n_shards = 7, 3
    modes = _modes(Cn)
    sizes = [(S.SPEC, 2), (S.FLOW, 3), (S.SPEC, 1), (21506, 2)]
    total = sum(bb * B for bb, B in sizes)
    stream = S.tones(Cn, 1, total, 1200)[:, 0]
    bank = S.Bank(oracle, modes, [-30] * Cn)
    fo = api.Fanout(Cn, [0] * n_shards)
    for c, m in enumerate(modes):
        fo.set_mode(m, c)
    fo.set_threshold(-30)
    s, off = torch.cuda.Stream(), 0
    for k, (bb, B) in enumerate(sizes):
        xs = stream[:, off:off + bb * B].reshape(Cn, B, bb).copy()
        if k == 1:
            xs[0, 1:3] = 0                                   # a closed gate in the batch that runs as the largest launch
        off += bb * B
        want = bank.run(xs, [0] * B)
        if k % 2 == 0:
            keep = _scatter(fo, torch, xs, bb, B, s)
        else:
            _fill_through_input(fo, xs, bb, B, n_shards)
        fo.process(0)
        got, _ = _collect(fo, torch, Cn, B, bb)
        S.assert_batch(got, want, 0, B)
    fo.close()


def test_collect_replays_with_the_gain_db_of_its_batch(oracle):
    """the gate-flipping inputs of tests/test_gpu_ingest_edges.py: gain_db 0 / G / 0 / G from batch to batch; the replay
    count of collect is the number of channels whose oracle gate closes inside the batch"""
    import torch
    Cn, n_shards, bb, B, NB = 7, 3, S.SPEC, 2, 4
    flip = [0, 2, 3, 6]                                      # 2 | 3: the last channel of shard 0, the first of shard 1
    assert api.fanout_channel_range(Cn, n_shards, 0) == (0, 3) and api.fanout_channel_range(Cn, n_shards, 1) == (3, 2)
    gains = [0, S.G] * (NB // 2)
    xs = S.tones(Cn, NB * B, bb, 1300)
    thresholds = [S.FLIP_THRESHOLD if c in flip else None for c in range(Cn)]
    want = S.Bank(oracle, [WBFM] * Cn, thresholds).run(xs, np.repeat(gains, B))
    for c in flip:
        S.assert_flips(oracle, want, c, np.repeat(gains, B))
    own = S.own_failures(want, [WBFM] * Cn, B)
    assert [len(o) for o in own] == [0, len(flip), 0, len(flip)]
    fo = api.Fanout(Cn, [0] * n_shards)
    fo.set_mode(WBFM)
    for c in flip:
        fo.set_threshold(S.FLIP_THRESHOLD, c)
    s = torch.cuda.Stream()
    for k in range(NB):
        keep = _scatter(fo, torch, xs[:, k * B:(k + 1) * B], bb, B, s)
        fo.process(gains[k])
        got, replayed = _collect(fo, torch, Cn, B, bb)
        S.assert_batch(got, want, k, B)
        assert replayed == len(own[k]), (k, replayed)
    fo.close()


def test_setters_across_shard_boundaries(oracle):
    """per-channel demodulator gains, thresholds and modes addressed by GLOBAL channel number on either side of both shard
    boundaries (shards of 3, 2, 2), a mode-NONE channel, no n_pcm destination, no source stream"""
    import torch
    Cn, n_shards, bb, B, NB = 7, 3, S.SPEC, 2, 2
    modes = [AM, AM, AM, AM, NONE, AM, AM]
    gain = [None, 0.25, 2.0, 0.5, None, 4.0, 8.0]            # 2 | 3 and 4 | 5 are the boundaries
    thresholds = [None, None, -30, None, -30, None, None]
    xs = S.tones(Cn, NB * B, bb, 1400)
    xs[2, 0:2] = 0
    xs[3, 2:4] = 0                                           # silent, but channel 3's threshold is the default: open
    xs[4, 0:2] = 0
    bank = S.Bank(oracle, modes, thresholds, gain)
    want = bank.run(xs, [0] * (NB * B))
    assert not want.allowed[2].all() and want.allowed[3].all() and not want.allowed[4].all()
    plain = S.Bank(oracle, modes, thresholds).run(xs[:, 0:2], [0] * 2)         # the gains are audible: a setter that reaches
    for c in (1, 3, 5, 6):                                                    # the neighbour's channel changes the PCM
        assert not np.array_equal(plain.pcm[c][1], want.pcm[c][1]), c
    fo = api.Fanout(Cn, [0] * n_shards)
    fo.set_mode(AM)
    fo.set_mode(NONE, 4)
    for c in range(Cn):
        if gain[c] is not None:
            fo.set_gain(AM, gain[c], c)
        if thresholds[c] is not None:
            fo.set_threshold(thresholds[c], c)
    for k in range(NB):
        keep = _scatter(fo, torch, xs[:, k * B:(k + 1) * B], bb, B, None)
        fo.process(0)
        got, _ = _collect(fo, torch, Cn, B, bb, with_n_pcm=False)
        S.assert_batch(got, want, k, B, what=("pcm",))
        assert (got[0][4] == 0).all()
    # n_pcm of the same stream, now asked for: zero for the NONE channel and the squelched units, per shard offset
    xs2 = S.tones(Cn, B, bb, 1450)
    xs2[5, 0:2] = 0
    fo.set_threshold(-30, 5)
    bank.rx[5].set_threshold(-30)
    want2 = bank.run(xs2, [0] * B)
    keep = _scatter(fo, torch, xs2, bb, B, None)
    fo.process(0)
    got, replayed = _collect(fo, torch, Cn, B, bb)
    S.assert_batch(got, want2, 0, B)
    assert replayed == 1 and got[1][4].sum() == 0 and got[1][5, 1] == 0 and got[1][6, 1] != 0
    fo.close()


def test_state_machine_and_refusals(oracle):
    """collect before process and process before any scatter are HRFD_ESTATE; so are scatter, input and process while a
    batch is in flight, and they leave that batch alone: it still collects to the oracle's PCM (its failed channels are
    replayed from the shards' input buffers with ITS gain_db, which a second scatter or process would have replaced)"""
    import torch
    Cn, n_shards, bb, B = 5, 2, S.SPEC, 2
    flip = [1, 3]
    xs = S.tones(Cn, 2 * B, bb, 1500)
    other = S.tones(Cn, 3, S.FLOW, 1550)
    thresholds = [S.FLIP_THRESHOLD if c in flip else None for c in range(Cn)]
    gains = [S.G, 0]
    want = S.Bank(oracle, [WBFM] * Cn, thresholds).run(xs, np.repeat(gains, B))
    assert [len(o) for o in S.own_failures(want, [WBFM] * Cn, B)] == [2, 0]
    fo = api.Fanout(Cn, [0] * n_shards)
    L, h = fo.L, fo.h
    fo.set_mode(WBFM)
    for c in flip:
        fo.set_threshold(S.FLIP_THRESHOLD, c)
    out = torch.zeros((Cn, B, api.pcm_capacity(bb)), dtype=torch.int16, device="cuda:0")
    p, u = C.c_void_p(), C.c_uint32(77)
    d_other = torch.from_numpy(other).to("cuda:0")
    torch.cuda.synchronize()
    assert L.hrfd_fanout_process(h, 0) == ESTATE                             # nothing scattered yet
    assert L.hrfd_fanout_collect(h, 0, out.data_ptr(), None, C.byref(u)) == ESTATE
    # refused arguments (no batch in flight)
    for bad_bb, bad_B in [(bb + 1, B), (0, B), (bb, 0), (api.BLOCK_BYTES + 2, B)]:
        assert L.hrfd_fanout_scatter(h, 0, d_other.data_ptr(), bad_bb, bad_B, None) == EINVAL
        assert L.hrfd_fanout_input(h, 0, bad_bb, bad_B, C.byref(p), None, None) == EINVAL
    assert L.hrfd_fanout_input(h, n_shards, bb, B, C.byref(p), None, None) == EINVAL
    assert L.hrfd_fanout_input(h, 0, bb, B, None, None, None) == EINVAL
    assert L.hrfd_fanout_scatter(h, 0, None, bb, B, None) == EINVAL
    for ch in (Cn, Cn + 1, 0xFFFFFFFE):
        assert L.hrfd_fanout_set_mode(h, ch, WBFM) == EINVAL
        assert L.hrfd_fanout_set_gain(h, ch, WBFM, C.c_float(1.0)) == EINVAL
        assert L.hrfd_fanout_set_threshold(h, ch, -30) == EINVAL
    assert L.hrfd_fanout_process(h, 0) == ESTATE and p.value is None and u.value == 77
    for k in range(2):
        keep = _scatter(fo, torch, xs[:, k * B:(k + 1) * B], bb, B, None)
        fo.process(gains[k])
        # in flight: nothing else is taken, and nothing is touched
        assert L.hrfd_fanout_scatter(h, 0, d_other.data_ptr(), S.FLOW, 3, None) == ESTATE
        assert L.hrfd_fanout_scatter(h, 0, d_other.data_ptr(), bb, B, None) == ESTATE
        assert L.hrfd_fanout_input(h, 0, S.FLOW, 3, C.byref(p), None, None) == ESTATE and p.value is None
        assert L.hrfd_fanout_process(h, 0 if k == 0 else S.G) == ESTATE
        assert L.hrfd_last_error().decode().startswith("hrfd_fanout_process")
        got, replayed = _collect(fo, torch, Cn, B, bb)
        S.assert_batch(got, want, k, B)
        assert replayed == (2 if k == 0 else 0)
        assert L.hrfd_fanout_collect(h, 0, out.data_ptr(), None, None) == ESTATE           # collected already
    assert L.hrfd_fanout_collect(h, 0, None, None, None) == EINVAL
    fo.close()
