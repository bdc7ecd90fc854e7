"""The packet banks (Afsk, AfskGen, Hdlc) in the launch shapes and streams their own suites do not reach, tolerance 0 everywhere.

H. k_hdlc: more than 256 flags in one tile (the frame close's second round, with the offset it carries), the most flags a tile
   can hold, rows of 70 000 and 2^20 bits (end_bit above 16 bits, 512 tiles), a carried partial frame of exactly cap bits with
   its closing bit in the next call, 1300 channels, rows more than 4 GiB apart.
A. k_afsk: every window 2..32, a call of 1024 blocks, 1300 channels, rows more than 4 GiB apart.
G. k_afskgen and afskgen_stage: 1300 channels whose dirty slots go up in several uploads, in runs broken where neighbours need
   different things; a call of 1024 blocks; rows more than 4 GiB apart.

Everything but the far rows compares with the banks' numpy models through the guarded run_device of the banks' own suites; the
far rows make the same call on twin handles with far and with dense rows and assert equal outputs and untouched sentinels
(tests/test_gpu_bank_launch_shapes.py's section D, whose helpers are used as they are), and compare the far call with the model
as well.  What decides whether a shape reaches its path is restated in tests/test_packet_launch_shapes_model.py, checked there
without a device, and asserted here next to every call."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import afsk_model as am
from tests import afskgen_model as gm
from tests import hdlc_model as hm
from tests import test_gpu_afsk as ta
from tests import test_gpu_afskgen as tg
from tests import test_gpu_hdlc as th
from tests import test_packet_launch_shapes_model as ps
from tests.test_gpu_bank_launch_shapes import TwoRows, big, equal, far_equals_dense, far_rows, host, release, torch_dev, zeros      # noqa: F401

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
MANY = ps.MANY
TILE = ps.HDLC_TILE
payloads = ps.payloads


# ================================================================ H. the HDLC bank
def test_hdlc_more_than_256_flags_in_one_tile(torch_dev):
    """H1: 265 flags in tile 0, the second frame closed by flag 264, in the frame close's second round.  Channel 1 is the same
    row with the first frame's check sequence broken: nothing of round one goes into round two's offset there.  A row of
    records that holds both, one that holds exactly one (round two's record is the one dropped on channel 0, and fits at
    offset 0 on channel 1), and the row behind a call that leaves a frame open: round one's first segment starts in the
    carried bits."""
    row, broken = ps.h1_row(), ps.h1_row(broken=True)
    assert ps.hdlc_flags_per_tile(row) == ps.hdlc_flags_per_tile(broken) == [265] and 265 > ps.HDLC_ROUND
    uncut = ps.model_frames(row)[0][0]
    assert payloads(uncut) == [ps.H1_A, ps.H1_B] and uncut[1][0] == len(row) - 1
    one = len(hm.record(0, ps.H1_A, 0))
    assert one == len(hm.record(0, ps.H1_B, 0)) == 16

    d, m = th.both(2)
    frames = th.run_device(torch_dev, d, m, [row, broken], "H1, a row that holds both", out_bytes=2 * one)
    assert frames[0] == uncut and payloads(frames[1]) == [ps.H1_B]

    d, m = th.both(2)
    _, n_frames, n_bad, dropped, _ = hm.HdlcModel(2).process([row, broken], one)
    assert n_frames.tolist() == [1, 1] and n_bad.tolist() == [0, 1] and dropped.tolist() == [1, 0]
    frames = th.run_device(torch_dev, d, m, [row, broken], "H1, one record short", out_bytes=one, out_pad=0)
    assert payloads(frames[0]) == [ps.H1_A] and payloads(frames[1]) == [ps.H1_B]

    d, m = th.both(2)
    th.run_device(torch_dev, d, m, [ps.h1_open(), ps.h1_open()[:20]], "H1, the call that leaves a frame open")
    assert m.ch[0].in_frame and len(m.ch[0].bits) == 8 * (len(ps.H1_OPEN) + 2) and len(m.ch[1].bits) == 12
    frames = th.run_device(torch_dev, d, m, [row, broken], "H1, behind the open frame")
    assert payloads(frames[0]) == [ps.H1_OPEN, ps.H1_A, ps.H1_B] and frames[0][0][0] == 7 and payloads(frames[1]) == [ps.H1_B]


def test_hdlc_the_most_flags_a_tile_can_hold(torch_dev):
    """H2: flags that share their zeros, seven bits apart, at every phase against the tile: 293 flags in a tile at four of the
    seven shifts, fl[] and dead[] one below their bound; a good frame behind them on every channel"""
    rows = [ps.h2_row(s) for s in range(7)]
    per_tile = [ps.hdlc_flags_per_tile(r) for r in rows]
    assert [s for s in range(7) if max(per_tile[s]) == 293] == [0, 4, 5, 6] and max(max(p) for p in per_tile) == ps.HDLC_MAX_FLAGS - 1
    assert all(len(r) > 2 * TILE for r in rows) and all(min(p[:2]) > ps.HDLC_ROUND for p in per_tile)
    d, m = th.both(7)
    frames = th.run_device(torch_dev, d, m, rows, "H2")
    assert [payloads(f) for f in frames] == [[ps.H2_FRAME]] * 7
    frames = th.run_device(torch_dev, d, m, rows[::-1], "H2, a second call at the other shifts")
    assert [payloads(f) for f in frames] == [[ps.H2_FRAME]] * 7


def test_hdlc_rows_of_70000_bits(torch_dev):
    """H3: 35 tiles a row, end_bit above 16 bits; the same stream cut as 69 999 + 1 on a second pair of handles"""
    x, want = ps.h3_rows(2, 70000), ps.h3_frames(2, 70000)
    assert all(f[-1][0] > 65535 for f in want) and all(sum(1 for e, _, _ in f if e > 65535) > 5 for f in want)
    d, m = th.both(2, 1, ps.H3_P)
    whole = th.run_device(torch_dev, d, m, list(x), "H3, 70 000 bits")
    assert whole == want
    d, m = th.both(2, 1, ps.H3_P)
    first = th.run_device(torch_dev, d, m, list(x[:, :69999]), "H3, 69 999 bits")
    last = th.run_device(torch_dev, d, m, list(x[:, 69999:]), "H3, the last bit")
    for c in range(2):
        assert first[c] + [(69999 + e, p, fcs) for e, p, fcs in last[c]] == whole[c]


def test_hdlc_a_row_of_max_bits(torch_dev):
    """H3: one channel x 2^20 bits, 512 tiles in one call: max_bits at its limit"""
    n = ps.HDLC_MAX_BITS
    assert n == hm.MAX_BITS == api.HDLC_MAX_BITS and n // TILE == 512
    x, want = ps.h3_rows(1, n), ps.h3_frames(1, n)
    assert want[0][-1][0] > 65535 and want[0][-1][0] > n - 4096 and len(want[0]) > 1000
    d, m = th.both(1, 1, ps.H3_P)
    assert th.run_device(torch_dev, d, m, list(x), "H3, 2^20 bits", bits_pad=0) == want


def test_hdlc_the_carried_frame_at_its_bound(torch_dev):
    """H4: P = 1021.  A frame of 1021 bytes and one of 1022, each cut in two launches at every bit from 20 in front of the
    long frame's closing zero to 4 behind it, one channel per cut.  At the cut one bit in front of the closing zero the
    carried frame is cap = 8191 bits and its closing bit arrives in the next call.  The joined frames are the uncut
    stream's for every cut: the frame of 1022 bytes never appears, b"next" always does"""
    P = ps.H4_P
    rows, cuts, uncut = [], [], []
    for n_bytes in (P, P + 1):
        row, z, long = ps.h4_row(n_bytes)
        frames = ps.model_frames(row, P)[0][0]
        assert payloads(frames) == ([long] if n_bytes == P else []) + [b"next"]
        for k in ps.H4_CUTS:
            rows.append(row)
            cuts.append(z + k)
            uncut.append(frames)
    C = len(rows)
    longest = max(len(r) for r in rows)
    d, m = th.both(C, 1, P)
    first = th.run_device(torch_dev, d, m, [r[:c] for r, c in zip(rows, cuts)], "H4, up to the cut", max_bits=longest)
    at_bound = list(ps.H4_CUTS).index(0)
    assert m.ch[at_bound].in_frame and len(m.ch[at_bound].bits) == ps.H4_CAP == api.HDLC_MAX_PAYLOAD * 8 + 23
    assert len(m.ch[at_bound - 1].bits) == ps.H4_CAP - 1 and len(m.ch[at_bound + 1].bits) == 0       # a bit either side
    over = C // 2 + at_bound                                   # the same cut of the frame of 1022 bytes: dead since its last bit
    assert len(m.ch[over - 8].bits) == ps.H4_CAP and not any(m.ch[c].in_frame for c in range(over - 7, over + 1))
    second = th.run_device(torch_dev, d, m, [r[c:] for r, c in zip(rows, cuts)], "H4, from the cut on", max_bits=longest)
    for c in range(C):
        assert first[c] + [(cuts[c] + e, p, fcs) for e, p, fcs in second[c]] == uncut[c], f"row {c // len(ps.H4_CUTS)} cut at {cuts[c]}"


def test_hdlc_1300_channels(torch_dev):
    """H5: rows of 2049 bits (a tile and a bit) at an odd stride; between two calls the reset of channels on both sides of
    1024; the second call's counts are 0, 1, 2048, 2049 and above max_bits.  Each reset channel carries a good frame
    across the cut and takes its whole row in the second call: a reset the kernel did not see would close that frame as
    the call's first record, which the model behind the reset does not have"""
    rows, counts, n = ps.h5_rows(), ps.h5_counts(), ps.H5_BITS
    carried, fresh = ps.h5_second_call(reset=False), ps.h5_second_call(reset=True)
    for i, c in enumerate(ps.H5_RESET):
        assert payloads(carried[i])[0] == ps.h5_payload(c) and carried[i][1:] == fresh[i] and counts[c] == n
    assert set(counts.tolist()) == {0, 1, 2048, 2049, 2050, 0xFFFFFFFF}
    d, m = th.both(MANY, 1, ps.H3_P)
    first = th.run_device(torch_dev, d, m, [r[:n] for r in rows], "H5, the first call", bits_pad=2)
    assert all(m.ch[c].in_frame and len(m.ch[c].bits) > 80 for c in ps.H5_RESET) and sum(len(f) for f in first) > MANY
    for c in ps.H5_RESET:
        d.reset(c)
        m.reset(c)
    second = th.run_device(torch_dev, d, m, [r[n:] for r in rows], "H5, behind the resets", max_bits=n, counts=counts, bits_pad=2)
    assert [second[c] for c in ps.H5_RESET] == fresh and sum(len(f) for f in second) > MANY // 2
    assert len(first[MANY - 1]) + len(second[MANY - 1]) > 0


def test_far_rows_hdlc(torch_dev, big):
    """H6: the rows of bits and the rows of records each more than 4 GiB apart (two allocations); three tiles a row"""
    n = 5000
    x = th.streams(2, 10000)[:, :n]
    want, n_frames, n_bad, _, _ = hm.HdlcModel(2, 1, 24).process(list(x))

    def call(far):
        torch = torch_dev[0]
        d = api.Hdlc(2, 1, 24, device=0)
        ob = d.max_out(n)
        src, out = far_rows(torch_dev, n, 61, x, far), far_rows(torch_dev, ob, 62, None, far)
        assert out.stride % 4 == 0 and (not far or min(src.stride, out.stride) > 1 << 32)
        d_n, cnt = zeros(torch_dev, (2,), "int32") + n, zeros(torch_dev, (3, 2), "int32")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, d_n.data_ptr(), n, out.ptr, out.stride, ob, cnt[0].data_ptr(), cnt[1].data_ptr(), cnt[2].data_ptr())
        torch.cuda.synchronize()
        src.check("the bits", unchanged=True)
        return {"records": out.check("the records"), "counts": host(cnt)[0]}

    got = far_equals_dense(torch_dev, call, "Hdlc")
    assert got["counts"].tolist() == [n_frames.tolist(), n_bad.tolist(), [0, 0]] and n_frames[1] > 0
    assert [api.Hdlc.parse(got["records"][c], n_frames[c]) for c in range(2)] == want


# ================================================================ A. the AFSK bank
@pytest.mark.parametrize("W", range(2, 33))
def test_afsk_every_window(torch_dev, W):
    """A1: every window has a (parity, lead, pair count) of its own in k_afsk; a call of 5 blocks (two steps, the second one
    partial) and one of 1 block that continues the state.  run_device compares `hard` first, then the counts and the bits"""
    A, nrzi = ps.afsk_window_setting(W)
    par, lead, J = ps.afsk_window(W)
    assert par == (W - 1) % 2 and 2 * lead - par == W - 1 and 2 * (J - 1) in (W - 1, W)
    d, m, modem = ta.both(2, nrzi=nrzi, window=W, loop_shift=A)
    assert am.taps(m.mark_step, m.space_step, W).shape == (4, W)
    x = ta.signal(2, 6, modem)
    bits, _ = ta.run_device(torch_dev, d, m, x[:, :5], None, f"A1, W={W} A={A} nrzi={nrzi}: 5 blocks")
    assert 0 < min(len(b) for b in bits) and max(len(b) for b in bits) <= d.max_bits(5)
    ta.run_device(torch_dev, d, m, x[:, 5:], None, f"A1, W={W} A={A} nrzi={nrzi}: the block behind them")


def test_afsk_the_longest_call(torch_dev):
    """A2: n_blocks = 1024, 256 steps of one workgroup a channel.  Channel 1 with n_pcm of 0, 100, 512 and 600; the rows of
    bits exactly max_bits apart, so a count one too high lands in the neighbour's row or in the guard"""
    B = 1024
    assert B == gm.MAX_BLOCKS and B // 4 == 256
    d, m, modem = ta.both(2)
    x = ta.signal(2, B, modem, seed=5)
    n_pcm = np.full((2, B), 512, dtype=np.uint32)
    n_pcm[1] = np.random.default_rng(6).choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=B)
    want, _ = am.AfskModel(2, **modem).process(x, n_pcm)       # the reach first, by a model of its own: twice the model's time
    assert min(len(b) for b in want) > 70000 and max(len(b) for b in want) <= d.max_bits(B)
    bits, _ = ta.run_device(torch_dev, d, m, x, n_pcm, "A2, 1024 blocks", bits_pad=0)
    ta.same_bits(bits, want, "A2, the two runs of the model")


def test_afsk_1300_channels(torch_dev):
    """A3: 1300 channels x 2 blocks, three calls: the reset of channels 0, 1024 and 1299 behind the first, set_modem to
    Bell 103 (which resets every channel) behind the second.  A few noisy AFSK rows tiled, small noise of its own on every
    channel"""
    C = MANY
    d, m, modem = ta.both(C)
    base = ta.signal(8, 6, modem).reshape(8, -1).astype(np.int32)
    noise = np.random.default_rng(7).integers(-40, 41, size=(C, base.shape[1]))
    x = np.clip(base[np.arange(C) % 8] + noise, -32768, 32767).astype(np.int16).reshape(C, 6, 512)
    first, _ = ta.run_device(torch_dev, d, m, x[:, :2], None, "A3, the first call", residue=2, pad=6, bits_pad=3)
    assert min(len(b) for b in first) > 120 and len({b.tobytes() for b in first}) > 8
    for c in (0, 1024, 1299):
        d.reset(c)
        m.reset(c)
    n_pcm = np.random.default_rng(8).choice(np.array([512, 512, 600, 100, 0], dtype=np.uint32), size=(C, 2))
    ta.run_device(torch_dev, d, m, x[:, 2:4], n_pcm, "A3, behind the resets", residue=4, pad=2, bits_pad=1)
    d.set_modem(**am.BELL103)
    m.set_modem(**am.BELL103)
    third, _ = ta.run_device(torch_dev, d, m, x[:, 4:], None, "A3, behind set_modem", residue=6)
    assert 0 < min(len(b) for b in third) and max(len(b) for b in third) <= d.max_bits(2) == am.max_bits(am.step(300), 2, 2)


def test_far_rows_afsk(torch_dev, big):
    """A4: the PCM rows and the rows of bits each more than 4 GiB apart; hard and n_bits are dense"""
    B = 5
    modem = dict(am.BELL202)
    x = ta.signal(2, B, modem)
    want_bits, want_hard = am.AfskModel(2, **modem).process(x)

    def call(far):
        torch = torch_dev[0]
        d = api.Afsk(2, device=0, **modem)
        cap = d.max_bits(B)
        src, bits = far_rows(torch_dev, 1024 * B, 63, x, far), far_rows(torch_dev, cap, 64, None, far)
        assert not far or min(src.stride, bits.stride) > 1 << 32
        count, hard = zeros(torch_dev, (2,), "int32"), zeros(torch_dev, (2, B, 64), "uint8")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, None, B, bits.ptr, bits.stride, count.data_ptr(), hard.data_ptr())
        torch.cuda.synchronize()
        src.check("the PCM", unchanged=True)
        return dict(zip(("bits", "n_bits", "hard"), [bits.check("the bits")] + host(count, hard)))

    got = far_equals_dense(torch_dev, call, "Afsk")
    equal(got["hard"], want_hard, "hard of the far rows against the model")
    assert got["n_bits"].tolist() == [len(b) for b in want_bits] and got["n_bits"][1] > 300
    ta.same_bits([got["bits"][c, :got["n_bits"][c]] for c in range(2)], want_bits, "the far rows against the model")


# ================================================================ G. the AFSK generator bank
def test_afskgen_staging_in_several_uploads(torch_dev):
    """G1: 1300 channels, four calls without a host synchronisation, alternating between two streams, each into its own
    output.  (0) two messages on every channel: the dirty ids 0..2599 go up as ten runs of 256 and one of 40 through the one
    pinned buffer, one run across the boundary between slot 0 and slot 1; (1) cut on every odd channel and a third message on
    every third: 867 runs in slot 0 alone, neighbours that need the slot next to neighbours that need its levels as well,
    while call 0 may still run; (2) a message on 255, 256, 257 and 1299; (3) cut(ALL).  What is dirty at each call is
    AfskgenDirty's restatement, checked against pending() of the library and of the model; the output is the model's"""
    torch, dev = torch_dev
    C, B = MANY, ps.G1_BLOCKS
    n = 512 * B
    d, m = tg.both(C)
    shadow = ps.AfskgenDirty(C)
    pcm = tg.reference(C, n, 13)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 4
    d_out = torch.zeros((calls, C, B, 512), dtype=torch.int16, device=dev)
    d_act = torch.zeros((calls, C, B), dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        ps.g1_apply((d, m), shadow, i)
        for c in range(C):
            assert d.pending(c) == m.pending(c) == shadow.pending(c), f"in front of call {i}: pending({c})"
        dirty = shadow.launch(B)
        runs = ps.afskgen_runs(dirty)
        assert dirty == ps.g1_dirty()[i]
        if i == 0:
            assert sorted(dirty) == list(range(2 * C)) and set(dirty.values()) == {2}
            assert runs == [(256 * k, 256, 2) for k in range(10)] + [(2560, 40, 2)] and (1280, 256, 2) in runs
        if i == 1:
            assert len(ps.touching_kinds(runs)) > 800 and {dirty[c] for c in range(256, 512)} == {1, 2} and dirty[511] == 1
        d.process_device(d_pcm.data_ptr(), 1024 * B, B, d_out[i].data_ptr(), 0, d_act[i].data_ptr(), streams[i % 2].cuda_stream)
        want.append(m.process(pcm, B, want_active=True))
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        equal(d_out[i].cpu().numpy(), want[i][0], f"G1, call {i}: out")
        equal(d_act[i].cpu().numpy(), want[i][1], f"G1, call {i}: active")
    act = [w[1] for w in want]
    assert act[0].tolist() == [[1, 1]] * C                     # `first`, then `second`
    assert act[1][3].tolist() == [1, 1] and act[1][1].tolist() == [1, 0] and act[1][0].tolist() == [1, 1]      # `third` behind the cut; the cut alone
    assert act[2][0].tolist() == [1, 1] and act[2][256].tolist() == [1, 1] and act[2][257].tolist() == [1, 1] and act[2][1].tolist() == [0, 0]
    assert act[3][:, 1].max() == 0 and act[3][0, 0] == 1 and act[3][255, 0] == 1 and act[3][1, 0] == 0       # cut(ALL): silent behind 64 samples
    tg.same_state(d, m, "G1, behind the four calls")


def test_afskgen_the_longest_call(torch_dev):
    """G2: n_blocks = 1024, 256 tiles of one workgroup a channel, in place over full-range PCM.  Channel 0: 8192 bits at
    300 baud on Bell 103's tones, 218 454 samples, begun 100 000 samples in front of the call's end, so that the call of 5
    blocks behind it continues the message; channel 1: four short messages spread over the call"""
    B = 1024
    n = 512 * B
    d, m = tg.both(2)
    starts = (1000, 150001, 300007, 523000)
    for h in (d, m):
        h.queue(0, tg.rbits(8192, 71), steps=tg.MODEMS[1], amplitude=20000, start=n - 100000)
        for i, s in enumerate(starts):
            h.queue(1, tg.rbits(200 + i, 72 + i), steps=tg.MODEMS[(0, 2, 1, 0)[i]], amplitude=32767, nrzi=bool(i & 1), start=s)
    L = gm.length(8192, tg.MODEMS[1][2])
    assert B == gm.MAX_BLOCKS and L // 2048 >= 106 and d.pending(0) == (1, n - 100000 + L) and d.pending(1)[0] == 4
    _, act = tg.run_device(torch_dev, d, m, tg.reference(2, n), B, "G2, 1024 blocks", mode="in_place")
    assert np.flatnonzero(act[0]).tolist() == list(range((n - 100000) // 512, B))
    assert [act[1, s // 512] for s in starts] == [1] * 4 and 0 < int(act[1].sum()) < 40 and act[1, B - 1] == 1
    assert d.pending(0)[0] == 1 and d.pending(1)[0] == 1 and d.clips(1) > 0
    _, act = tg.run_device(torch_dev, d, m, tg.reference(2, 2560, 8), 5, "G2, the 5 blocks behind", mode="in_place")
    assert act[0].tolist() == [1] * 5 and d.pending(0)[0] == 1


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_far_rows_afskgen(torch_dev, big, in_place):
    """G3: one tile (4 blocks) per row; out of place the input and the output are each more than 4 GiB apart, in place the
    one pair is.  Channel 1 has messages of its own"""
    pcm = tg.reference(2, 2048, 35)
    m = gm.AfskGenModel(2)

    def queues(h):
        h.queue(0, tg.rbits(200, 91), amplitude=20000, start=100)
        h.queue(1, tg.rbits(120, 92), steps=tg.MODEMS[2], amplitude=32767, nrzi=False, start=300)
        h.queue(1, tg.rbits(40, 93), steps=tg.MODEMS[1], amplitude=32767, gap=70)

    queues(m)
    want, want_act = m.process(pcm, 4, want_active=True)

    def call(far):
        torch = torch_dev[0]
        d = api.AfskGen(2, device=0)
        queues(d)
        src = far_rows(torch_dev, 4096, 65, pcm, far)
        out = src if in_place else far_rows(torch_dev, 4096, 66, None, far)
        assert not far or min(src.stride, out.stride) > 1 << 32
        act = zeros(torch_dev, (2, 4), "uint8")
        torch.cuda.synchronize()
        d.process_device(src.ptr, src.stride, 4, out.ptr, out.stride, act.data_ptr())
        torch.cuda.synchronize()
        if not in_place:
            src.check("the input", unchanged=True)
        return {"out": out.check("out"), "active": host(act)[0], "clips": np.array([d.clips(0), d.clips(1)])}

    got = far_equals_dense(torch_dev, call, "AfskGen")
    equal(got["out"], want.reshape(2, -1).view(np.uint8), "out of the far rows against the model")
    equal(got["active"], want_act, "active of the far rows against the model")
    assert got["clips"].tolist() == [m.clips(0), m.clips(1)] and got["clips"][1] > 0 and (got["out"][1] != pcm[1].view(np.uint8)).any()
