"""The DDC bank on the device (hrfd_ddc_*) against the numpy model (tests/ddc_model.py), bit for bit, and
hrfd_ddc_receive against the model followed by the CPU oracle's receive chain."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import ddc_model as dm
from tests.reflib import AM, FM, LSB, USB, WBFM

pytestmark = pytest.mark.gpu

FULL = 262144


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def lcg_captures(W, n_bytes, seed):
    """LCG bytes with runs of -128 and of full scale, so that the outputs saturate"""
    x = np.empty(W * n_bytes, dtype=np.uint32)
    s = np.uint64(seed * 2654435761 + 12345)
    a = np.arange(x.size, dtype=np.uint64)
    x = ((a * np.uint64(1103515245) + s) * np.uint64(2862933555777941757) >> np.uint64(40)).astype(np.uint32)
    cap = (x & 0xFF).astype(np.uint8).view(np.int8).reshape(W, n_bytes).copy()
    for w in range(W):
        o = (seed * 977 + w * 4001) % max(1, n_bytes - 3000)
        cap[w, o:o + 1200] = -128
        cap[w, o + 1500:o + 2700:2] = 127
        cap[w, o + 1501:o + 2700:2] = -128
    return cap


def both(W, C, R):
    return api.Ddc(W, C, R, device=0), dm.DdcModel(W, C, R)


def tune_both(d, m, c, w, step):
    d.set_step(c, w, step)
    m.set_tuning(c, w, step)


# 1. bit-exact against the model
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_default_filters_bit_exact(R):
    W, C = 3, 7
    d, m = both(W, C, R)
    fs = R * dm.FS_OUT
    offsets = [0, fs / 4, -fs / 4, fs / 2 - 1000, -fs / 2 + 1000, -123_456.7, 250_000]
    caps = [2, 0, 2, 1, 0, 2, 1]                                   # non-contiguous channel -> capture map
    for c in range(C):
        tune_both(d, m, c, caps[c], dm.ddc_step(offsets[c], R))
        d.set_gain_shift(c % 8, c)
        m.set_gain_shift(c, c % 8)
    for call, ob in enumerate((4096, 3000)):
        cap = lcg_captures(W, R * ob, 11 * R + call)
        got = d.process(cap, ob)
        want = m.process(cap, ob)
        assert (got == want).all(), f"R={R} call {call}: {np.argwhere(got != want)[:5]}"
        assert ((got == 127) | (got == -128)).any()


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_random_taps_and_every_gain_bit_exact(R):
    rng = np.random.default_rng(R)
    W, C = 2, 8
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, int(rng.integers(0, 2 ** 32)))
        d.set_gain_shift(c, c)
        m.set_gain_shift(c, c)

    def taps(n, limit=65535):
        if n == 0:
            return np.zeros(0, dtype=np.int16)
        h = rng.integers(-32768, 32768, size=n).astype(np.int64)
        s = np.abs(h).sum()
        if s > limit:
            h = np.sign(h) * ((np.abs(h) * limit) // s)
        return h.astype(np.int16)

    for ta, tb in ((1, 1), (2, 146), (64, 256), (0, 37), (33, 0), (0, 0), (7, 255)):
        for stage, t in ((0, taps(ta)), (1, taps(tb))):
            d.set_filter(stage, t)
            m.set_filter(stage, t)
        cap = lcg_captures(W, R * 2500, ta * 7 + tb)
        got, want = d.process(cap, 2500), m.process(cap, 2500)
        assert (got == want).all(), f"R={R} taps {ta}/{tb}"


# 2. streaming
# tile remainders: M in {1 .. 5, 255 .. 257, 511 .. 513, 1023 .. 1025, 2047, 2049, 4095, 4097} outputs, one stream of
# calls per R (history and phase cross every shape; the sizes cover tiles of 256, 512, 1024 or 2048 outputs)
TILE_SEQ = [2 * M for M in (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 4095, 4097)]
STREAM_CASES = [(4, [2, 510, 1000, 1026, 262144, 3074, 2])] + [(R, TILE_SEQ) for R in (1, 2, 4, 8)]


@pytest.mark.parametrize("R,seq", STREAM_CASES, ids=["r4_mixed", "r1_tiles", "r2_tiles", "r4_tiles", "r8_tiles"])
def test_streaming_calls_retune_filter_change_capture_switch_reset(R, seq):
    W, C = 2, 3
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, dm.ddc_step(100_000 * (c + 1) - 150_000, R))
    for i, ob in enumerate(seq):
        if i == 2:
            tune_both(d, m, 1, 1, dm.ddc_step(-777_000, R))       # retune
        if i == 3:
            t = dm.default_taps(R)[1][::2].astype(np.int16)
            d.set_filter(1, t)
            m.set_filter(1, t)                                    # filter change
        if i == 4:
            tune_both(d, m, 0, 1, dm.ddc_step(55_000, R))         # capture switch
        if i == 5:
            d.reset()
            m.reset()
        cap = lcg_captures(W, R * ob, 100 + i)
        got, want = d.process(cap, ob), m.process(cap, ob)
        assert (got == want).all(), f"call {i} ({ob} bytes)"
        for c in range(C):
            assert d.phase(c) == m.phase(c), f"phase ch{c} after call {i}"


# 3. strides, and calls on different streams
def _legacy_layout(R, ob, k):
    """capture offset, capture stride, output offset, output stride of call k"""
    return 0, R * ob + 1234, 3, ob + 77 * 2 + 6


def _sweep_layout(R, ob, k):
    """over the 8 calls: capture base offsets 0, 2, .. 14 bytes, capture strides at every even residue mod 16, output
    base offsets 0 .. 7, odd and even output strides (ob is a multiple of 16)"""
    return 2 * k, R * ob + 16 + 2 * ((5 * k) % 8), (3 * k) % 8, ob + 8 + (k % 2)


STRIDE_CASES = [(2, 5000, 3, _legacy_layout)] + [(R, 3008, 8, _sweep_layout) for R in (1, 2, 4, 8)]


@pytest.mark.parametrize("R,ob,n_calls,layout", STRIDE_CASES,
                         ids=["r2_odd_output", "r1_alignment", "r2_alignment", "r4_alignment", "r8_alignment"])
def test_padded_strides_leave_guard_bytes(torch_dev, R, ob, n_calls, layout):
    """padded capture / output strides, unaligned capture and output addresses; the calls alternate between a stream
    of the caller and the handle's own without waiting in between (the handle orders them on the device).  Guard bytes
    before, between and after the output rows stay; the captures stay unchanged"""
    torch, dev = torch_dev
    W, C = 2, 5
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, (c + 1) % W, dm.ddc_step(-300_000 + 90_000 * c, R))
    caps = [lcg_captures(W, R * ob, 5 + k) for k in range(n_calls)]
    lay = [layout(R, ob, k) for k in range(n_calls)]
    dcaps, douts, ref_caps = [], [], []
    for k in range(n_calls):
        co, cs, oo, os_ = lay[k]
        host = np.full(co + W * cs + 16, 0x33, dtype=np.int8)
        for w in range(W):
            host[co + w * cs:co + w * cs + R * ob] = caps[k][w]
        ref_caps.append(host)
        dcaps.append(torch.from_numpy(host).to(dev))
        douts.append(torch.full((oo + C * os_ + 16,), 0x5A, dtype=torch.int8, device=dev))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k in range(n_calls):
        co, cs, oo, os_ = lay[k]
        stream = side.cuda_stream if k % 2 == 0 else None
        d.process_device(dcaps[k].data_ptr() + co, cs, ob, douts[k].data_ptr() + oo, os_, stream)
    torch.cuda.synchronize()
    for k in range(n_calls):
        co, cs, oo, os_ = lay[k]
        want = m.process(caps[k], ob)
        host = douts[k].cpu().numpy()
        for c in range(C):
            row = host[oo + c * os_:oo + c * os_ + ob]
            assert (row == want[c]).all(), f"call {k} ch{c}"
            guard = host[oo + c * os_ + ob:oo + (c + 1) * os_]
            assert (guard == 0x5A).all(), f"call {k}: guard bytes behind ch{c} touched"
        assert (host[:oo] == 0x5A).all() and (host[oo + C * os_:] == 0x5A).all(), f"call {k}: guard bytes touched"
        assert (dcaps[k].cpu().numpy() == ref_caps[k]).all(), f"call {k}: the captures changed"


# 4. receive against model + oracle
def _receive_case(torch, dev, oracle, mode, R, block_bytes, n_blocks, threshold=None, level_drop=False, seed=0,
                  calls=None, gain_db=0, mode_gain=None, squelch_outputs=True):
    """hrfd_ddc_receive over `calls` ([(block_bytes, n_blocks)], default one call) on one (Ddc, Rx) pair against the
    model followed by the CPU oracle's rx chain, block by block, state carried across the calls on both sides.
    squelch_outputs=False passes d_magnitude / d_allowed as NULL (the PCM and its counts are still checked)."""
    W, C = 2, 4
    calls = calls or [(block_bytes, n_blocks)]
    d, m = both(W, C, R)
    rx = api.Rx(C, device=0)
    rx.set_mode(mode)
    if threshold is not None:
        rx.set_threshold(threshold)
    if mode_gain is not None:
        rx.set_gain(mode, mode_gain)
    rx.gain_db = gain_db
    offs = [-400_000, 150_000, 0, 320_000]
    for c in range(C):
        tune_both(d, m, c, c % W, dm.ddc_step(offs[c] + 64_000, R))
        d.set_gain_shift(2, c)
        m.set_gain_shift(c, 2)
    orcs = []
    for c in range(C):
        o = oracle.rx()
        o.set_mode(mode)
        if threshold is not None:
            o.set_threshold(threshold)
        if mode_gain is not None:
            o.set_gain(mode, mode_gain)
        o.gain_db = gain_db
        orcs.append(o)
    total = sum(bb * nb for bb, nb in calls)
    cap_all = lcg_captures(W, R * total, seed).astype(np.int16)
    cap_all = (cap_all // 6).astype(np.int8)                     # a noise floor the rx chain can demodulate
    if level_drop:
        cap_all[:, R * total // 3:] = (cap_all[:, R * total // 3:] // 16).astype(np.int8)   # gates close mid-batch
    als, replayed = [], 0
    pos = 0
    for call, (bb, nb) in enumerate(calls):
        ob = bb * nb
        cap = np.ascontiguousarray(cap_all[:, R * pos:R * (pos + ob)])
        pos += ob
        dcap = torch.from_numpy(cap).to(dev)
        npcm_cap = api.pcm_capacity(bb)
        d_pcm = torch.zeros((C, nb, npcm_cap), dtype=torch.int16, device=dev)
        d_n = torch.zeros((C, nb), dtype=torch.int32, device=dev)
        d_mag = torch.zeros((C, nb), dtype=torch.int32, device=dev)
        d_al = torch.zeros((C, nb), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        replayed += d.receive(rx, dcap.data_ptr(), R * ob, bb, nb, d_pcm.data_ptr(), d_n.data_ptr(),
                              d_mag.data_ptr() if squelch_outputs else None, d_al.data_ptr() if squelch_outputs else None)
        streams = m.process(cap, ob)
        pcm, n, mag, al = (t.cpu().numpy() for t in (d_pcm, d_n, d_mag, d_al))
        oal = np.zeros((C, nb), dtype=bool)
        for c in range(C):
            for b in range(nb):
                p, mg, allowed, _ = orcs[c].process(streams[c, b * bb:(b + 1) * bb])
                oal[c, b] = allowed
                assert int(n[c, b]) == p.size, f"{mode} call {call} ch{c} blk{b} n_pcm"
                assert (pcm[c, b, :p.size] == p).all(), f"{mode} call {call} ch{c} blk{b} pcm"
                if squelch_outputs:
                    assert int(mag[c, b]) == mg and bool(al[c, b]) == allowed, f"{mode} call {call} ch{c} blk{b} squelch"
        if not squelch_outputs:
            assert not mag.any() and not al.any(), "NULL squelch outputs: the caller's rows must stay untouched"
        als.append(al if squelch_outputs else oal)
    return np.concatenate(als, axis=1), replayed, rx.debug_counters()


# 32768-byte blocks: long enough for the rx bank's speculative batch launch (hrfd_rx_process_block takes blocks of at
# least (kMaxHal + 64) * 16 = 21504 bytes that way; shorter ones go block by block on the exact path)
BATCH_BLOCK = 32768


@pytest.mark.parametrize("mode", [WBFM, FM, AM, LSB, USB])
def test_receive_equals_model_plus_oracle(torch_dev, oracle, mode):
    torch, dev = torch_dev
    _receive_case(torch, dev, oracle, mode, 4, BATCH_BLOCK, 3, seed=mode)


@pytest.mark.parametrize("mode,n_blocks", [(WBFM, 70), (FM, 12), (USB, 12)])
def test_receive_with_closing_gates(torch_dev, oracle, mode, n_blocks):
    """gates that close inside a batch of speculative launches: the rx bank repairs them (on the device, or by replaying
    the channels on the exact path), over 70 blocks in chunks of at most 64 as well; the outputs stay exact"""
    torch, dev = torch_dev
    al, replayed, counters = _receive_case(torch, dev, oracle, mode, 2, BATCH_BLOCK, n_blocks, threshold=-30,
                                           level_drop=True, seed=9 + mode)
    assert al[:, 0].all() and not al[:, -1].any(), "the scenario must open and then close the gates"
    repairs = counters[4]                       # device repairs over the handle's life (hrfd_rx_debug_counters)
    assert replayed + repairs > 0, f"no repair ran (n_replayed {replayed}, counters {counters})"


# hrfd_ddc_receive beyond one call: consecutive calls on one pair, block lengths off the 1024-byte grid (k_rx_ragged),
# off the 512-byte grid (the handle stays off it), below the batch threshold (the exact per-block path), the smallest
# batched length, gains, and the squelch outputs passed as NULL
RECEIVE_CASES = {
    "three_calls": dict(mode=WBFM, R=4, calls=[(BATCH_BLOCK, 2)] * 3),
    "ragged_261632": dict(mode=FM, R=2, calls=[(261632, 2)]),
    "ragged_16896": dict(mode=AM, R=8, calls=[(16896, 3), (16896, 2)]),
    "offgrid_1000": dict(mode=LSB, R=2, calls=[(FULL, 1), (1000, 3), (FULL, 1)]),
    "exact_20480": dict(mode=USB, R=4, calls=[(20480, 3), (20480, 2)]),
    "batched_21504_gains": dict(mode=WBFM, R=2, calls=[(21504, 3), (21504, 4)], gain_db=20, mode_gain=4000.0),
    "fm_mode_gain": dict(mode=FM, R=1, calls=[(21504, 3)], gain_db=6, mode_gain=4321.0),
    "null_squelch_outputs": dict(mode=FM, R=4, calls=[(BATCH_BLOCK, 3), (BATCH_BLOCK, 2)], threshold=-30,
                                 level_drop=True, squelch_outputs=False),
}


@pytest.mark.parametrize("case", list(RECEIVE_CASES), ids=list(RECEIVE_CASES))
def test_receive_beyond_one_call(torch_dev, oracle, case):
    torch, dev = torch_dev
    kw = dict(RECEIVE_CASES[case])
    mode, R = kw.pop("mode"), kw.pop("R")
    al, _, _ = _receive_case(torch, dev, oracle, mode, R, 0, 0, seed=31 + len(case), **kw)
    if case == "null_squelch_outputs":
        assert al[:, 0].all() and not al[:, -1].any(), "the squelch must open and close in this scenario"


# 5. size
def test_sixteen_captures_by_64_channels_at_r8(torch_dev):
    torch, dev = torch_dev
    R, W, C = 8, 16, 64
    d = api.Ddc(W, C, R, device=0)
    rng = np.random.default_rng(5)
    steps = rng.integers(0, 2 ** 32, size=C)
    for c in range(C):
        d.set_step(c, c % W, int(steps[c]))
        d.set_gain_shift(c % 8, c)
    cap = lcg_captures(W, R * FULL, 77)
    dcap = torch.from_numpy(cap).to(dev)
    dout = torch.zeros((C, FULL), dtype=torch.int8, device=dev)
    # a stream of the caller's.  (torch's default stream has the handle 0, which this entry reads as "the handle's own":
    # a non-blocking stream that synchronising the default stream does not wait for, so the copy back raced the kernel)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    d.process_device(dcap.data_ptr(), R * FULL, FULL, dout.data_ptr(), FULL, stream.cuda_stream)
    stream.synchronize()
    out = dout.cpu().numpy()
    check = list(range(0, C, 2))                                 # 32 channels over all 16 captures
    m = dm.DdcModel(W, len(check), R)
    for i, c in enumerate(check):
        m.set_tuning(i, c % W, int(steps[c]))
        m.set_gain_shift(i, c % 8)
    want = m.process(cap, FULL)
    for i, c in enumerate(check):
        assert (out[c] == want[i]).all(), f"ch{c}"


# 6. end to end: the selectivity scenario through Ddc.receive
def test_selectivity_scenario_through_receive(torch_dev, oracle):
    torch, dev = torch_dev
    cap, audio = dm.selectivity_capture(oracle)
    d = api.Ddc(1, 2, dm.SEL_R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.WBFM)
    for c, f in enumerate(dm.SEL_OFFSETS):
        d.tune(c, 0, f)
        d.set_gain_shift(dm.SEL_GAIN_SHIFT[c], c)
    B = dm.SEL_BLOCKS
    dcap = torch.from_numpy(cap).to(dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    d.receive(rx, dcap.data_ptr(), cap.shape[1], FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    pcm = d_pcm.cpu().numpy()
    assert (d_n.cpu().numpy() == 512).all()
    m = dm.DdcModel(1, 2, dm.SEL_R)
    for c, f in enumerate(dm.SEL_OFFSETS):
        m.set_tuning(c, 0, dm.ddc_step(f + 64_000, dm.SEL_R))
        m.set_gain_shift(c, dm.SEL_GAIN_SHIFT[c])
    streams = m.process(cap, B * FULL)
    for c in range(2):
        want = dm.oracle_rx_wbfm(oracle, streams[c])
        assert (pcm[c].reshape(-1) == want).all(), f"station {c}"
    assert min(dm.best_corr(audio[c], pcm[c].reshape(-1)) for c in range(2)) >= 0.85
