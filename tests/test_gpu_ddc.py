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
def test_streaming_calls_retune_filter_change_capture_switch_reset():
    R, W, C = 4, 2, 3
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, dm.ddc_step(100_000 * (c + 1) - 150_000, R))
    seq = [2, 510, 1000, 1026, 262144, 3074, 2]
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
def test_padded_strides_leave_guard_bytes(torch_dev):
    """padded capture / output strides, an odd output address; the calls alternate between a stream of the caller and
    the handle's own without waiting in between (the handle orders them on the device)"""
    torch, dev = torch_dev
    R, W, C, ob = 2, 2, 5, 5000
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, (c + 1) % W, dm.ddc_step(-300_000 + 90_000 * c, R))
    cs, os_ = R * ob + 1234, ob + 77 * 2 + 6
    n_calls = 3
    caps = [lcg_captures(W, R * ob, 5 + k) for k in range(n_calls)]
    dcap = torch.zeros((n_calls, W, cs), dtype=torch.int8, device=dev)
    for k in range(n_calls):
        dcap[k, :, :R * ob] = torch.from_numpy(caps[k]).to(dev)
    douts = [torch.full((C + 1, os_), 0x5A, dtype=torch.int8, device=dev) for _ in range(n_calls)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k in range(n_calls):
        stream = side.cuda_stream if k % 2 == 0 else None
        d.process_device(dcap[k].data_ptr(), cs, ob, douts[k].data_ptr() + 3, os_, stream)
    torch.cuda.synchronize()
    for k in range(n_calls):
        want = m.process(caps[k], ob)
        host = douts[k].cpu().numpy().reshape(-1)
        for c in range(C):
            row = host[3 + c * os_:3 + c * os_ + ob]
            assert (row == want[c]).all(), f"call {k} ch{c}"
            guard = host[3 + c * os_ + ob:3 + (c + 1) * os_]
            assert (guard == 0x5A).all(), f"guard bytes of ch{c} touched"
        assert (host[:3] == 0x5A).all() and (host[3 + C * os_:] == 0x5A).all()


# 4. receive against model + oracle
def _receive_case(torch, dev, oracle, mode, R, block_bytes, n_blocks, threshold=None, level_drop=False, seed=0):
    W, C = 2, 4
    d, m = both(W, C, R)
    rx = api.Rx(C, device=0)
    rx.set_mode(mode)
    if threshold is not None:
        rx.set_threshold(threshold)
    offs = [-400_000, 150_000, 0, 320_000]
    for c in range(C):
        tune_both(d, m, c, c % W, dm.ddc_step(offs[c] + 64_000, R))
        d.set_gain_shift(2, c)
        m.set_gain_shift(c, 2)
    ob = block_bytes * n_blocks
    cap = lcg_captures(W, R * ob, seed).astype(np.int16)
    cap = (cap // 6).astype(np.int8)                             # a noise floor the rx chain can demodulate
    if level_drop:
        cap[:, R * ob // 3:] = (cap[:, R * ob // 3:] // 16).astype(np.int8)   # gates close mid-batch
    dcap = torch.from_numpy(cap).to(dev)
    npcm_cap = api.pcm_capacity(block_bytes)
    d_pcm = torch.zeros((C, n_blocks, npcm_cap), dtype=torch.int16, device=dev)
    d_n = torch.zeros((C, n_blocks), dtype=torch.int32, device=dev)
    d_mag = torch.zeros((C, n_blocks), dtype=torch.int32, device=dev)
    d_al = torch.zeros((C, n_blocks), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    replayed = d.receive(rx, dcap.data_ptr(), R * ob, block_bytes, n_blocks, d_pcm.data_ptr(), d_n.data_ptr(),
                         d_mag.data_ptr(), d_al.data_ptr())
    streams = m.process(cap, ob)
    pcm, n, mag, al = (t.cpu().numpy() for t in (d_pcm, d_n, d_mag, d_al))
    for c in range(C):
        o = oracle.rx()
        o.set_mode(mode)
        if threshold is not None:
            o.set_threshold(threshold)
        for b in range(n_blocks):
            p, mg, allowed, _ = o.process(streams[c, b * block_bytes:(b + 1) * block_bytes])
            assert int(n[c, b]) == p.size, f"{mode} ch{c} blk{b} n_pcm"
            assert (pcm[c, b, :p.size] == p).all(), f"{mode} ch{c} blk{b} pcm"
            assert int(mag[c, b]) == mg and bool(al[c, b]) == allowed, f"{mode} ch{c} blk{b} squelch"
    return al, replayed, rx.debug_counters()


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
    stream = torch.cuda.current_stream()
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
