"""The DUC bank on the device (hrfd_duc_*) against the numpy model (tests/duc_model.py), bit for bit, and
hrfd_duc_transmit against the modulator bank followed by the DUC, on the device and on the CPU oracle plus the model."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import duc_model as um

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def lcg_channels(C, n_bytes, seed):
    """LCG bytes with runs of -128 and of full scale, so that the filters and the sums reach their edges"""
    a = np.arange(C * n_bytes, dtype=np.uint64)
    s = np.uint64(seed * 2654435761 + 12345)
    x = ((a * np.uint64(1103515245) + s) * np.uint64(2862933555777941757) >> np.uint64(40)).astype(np.uint32)
    ch = (x & 0xFF).astype(np.uint8).view(np.int8).reshape(C, n_bytes).copy()
    for c in range(C):
        o = (seed * 977 + c * 4001) % max(1, n_bytes - 3000)
        ch[c, o:o + 1200] = -128
        ch[c, o + 1500:o + 2700:2] = 127
        ch[c, o + 1501:o + 2700:2] = -128
    return ch


def both(W, C, R):
    return api.Duc(W, C, R, device=0), um.DucModel(W, C, R)


def tune_both(d, m, c, w, step):
    d.set_step(c, w, step)
    m.set_tuning(c, w, step)


def amp_both(d, m, c, a):
    d.set_amplitude(a, c)
    m.set_amplitude(c, a)


def shift_both(d, m, w, s):
    d.set_output_shift(s, w)
    m.set_output_shift(w, s)


def filter_both(d, m, stage, t):
    d.set_filter(stage, t)
    m.set_filter(stage, t)


def check_call(d, m, ch, ib, what):
    got, want = d.process(ch, ib), m.process(ch, ib)
    assert (got == want).all(), f"{what}: {np.argwhere(got != want)[:5]}"
    for w in range(m.W):
        assert d.clips(w) == int(m.clips[w]), (what, w)
    return got


def branch_taps(rng, n, R, limit=65535):
    """random asymmetric taps whose every polyphase branch has sum |h| <= limit"""
    h = rng.integers(-32768, 32768, size=n).astype(np.int64)
    for p in range(R):
        s = np.abs(h[p::R]).sum()
        if s > limit:
            h[p::R] = np.sign(h[p::R]) * ((np.abs(h[p::R]) * limit) // s)
    return h.astype(np.int16)


# 1. bit-exact against the model
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_default_filters_bit_exact(R):
    W, C = 4, 8
    d, m = both(W, C, R)
    fs = R * um.FS_CH
    offsets = [0, fs / 4, -fs / 4, fs / 2 - 1000, -fs / 2 + 1000, -123_456.7, 250_000, 0]
    caps = [2, 0, 2, 1, 0, 2, 1, 0]                                # non-contiguous; capture 3 has no channel
    for c in range(C):
        tune_both(d, m, c, caps[c], um.duc_step(offsets[c], R))
    shift_both(d, m, 1, 9)
    for call, ib in enumerate((4096, 3000)):
        got = check_call(d, m, lcg_channels(C, ib, 11 * R + call), ib, f"R={R} call {call}")
        assert not got[3].any(), "a capture without channels is silence"
        assert ((got == 127) | (got == -128)).any()


@pytest.mark.parametrize("R", [1, 8])
def test_every_channel_on_one_capture(R):
    W, C = 2, 40
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, 1, um.duc_step((c - 20) * 37_000.0 * R, R))
    shift_both(d, m, 1, 12)
    got = check_call(d, m, lcg_channels(C, 2050, R), 2050, f"R={R}")
    assert not got[0].any()


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_random_taps_every_shift_and_amplitude(R):
    rng = np.random.default_rng(R)
    W, C = 3, 8
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, int(rng.integers(0, 2 ** 32)))
        amp_both(d, m, c, (0, 1, 32767, 32768, 20000, 32768, 1, 32767)[c])
    shifts = iter(range(25))
    for ta, tb in ((1, 1), (2, 146), (64, 256), (0, 37), (33, 0), (0, 0), (7, 255), (R * 3 + 1, 5), (64, 2)):
        filter_both(d, m, 0, branch_taps(rng, ta, R))
        filter_both(d, m, 1, branch_taps(rng, tb, 1))
        for w in range(W):
            s = next(shifts, int(rng.integers(0, 25)))
            shift_both(d, m, w, s)
        check_call(d, m, lcg_channels(C, 2500, ta * 7 + tb), 2500, f"R={R} taps {ta}/{tb}")


# 2. streaming: tile remainders around 1024 channel samples, and 2 .. 262144 bytes with every setter between calls
TILE_SEQ = [2 * M for M in (1, 2, 3, 255, 256, 511, 512, 513, 1023, 1024, 1025, 2047, 2049, 3071, 4097)]
STREAM_CASES = [(4, [2, 510, 1000, 1026, 262144, 3074, 2])] + [(R, TILE_SEQ) for R in (1, 2, 4, 8)]


@pytest.mark.parametrize("R,seq", STREAM_CASES, ids=["r4_mixed", "r1_tiles", "r2_tiles", "r4_tiles", "r8_tiles"])
def test_streaming_calls_with_setters_and_reset(R, seq):
    W, C = 2, 3
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, um.duc_step(100_000 * (c + 1) - 150_000, R))
    for i, ib in enumerate(seq):
        if i == 2:
            tune_both(d, m, 1, 1, um.duc_step(-777_000, R))       # retune
        if i == 3:
            filter_both(d, m, 1, um.default_taps(R)[1][::2].astype(np.int16))   # filter change
        if i == 4:
            amp_both(d, m, 2, 12345)                              # amplitude change
        if i == 5:
            tune_both(d, m, 0, 1, um.duc_step(55_000, R))         # capture switch
        if i == 6:
            d.reset()
            m.reset()
        if i == 8:
            shift_both(d, m, 0, 5)
        check_call(d, m, lcg_channels(C, ib, 100 + i), ib, f"call {i} ({ib} bytes)")
        assert d.phase(1) == m.phase(1)


# 3. device buffers: padded strides with guard bytes, two streams
def test_padded_strides_and_guard_bytes(torch_dev):
    torch, dev = torch_dev
    R, W, C, ib = 4, 3, 5, 6146
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, (c * 2) % W, um.duc_step(-300_000 + 140_000 * c, R))
    cs, ws = ib + 38, R * ib + 70                                  # odd multiples of 2: rows start unaligned
    for call in range(3):
        ch = lcg_channels(C, ib, 50 + call)
        hin = np.full((C, cs), 77, dtype=np.int8)
        hin[:, :ib] = ch
        din = torch.from_numpy(hin).to(dev)
        dout = torch.full((W + 1, ws), -99, dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        d.process_device(din.data_ptr() + 2 * (call % 2), cs, ib - 4 * (call % 2), dout.data_ptr() + 1, ws)
        torch.cuda.synchronize()
        want = m.process(hin[:, 2 * (call % 2):2 * (call % 2) + ib - 4 * (call % 2)], ib - 4 * (call % 2))
        got = dout.cpu().numpy()
        n = R * (ib - 4 * (call % 2))
        assert (got[:W, 1:1 + n] == want).all(), call
        assert (got[:W, 0] == -99).all() and (got[:W, 1 + n:] == -99).all() and (got[W] == -99).all(), call


def test_calls_alternating_between_two_streams(torch_dev):
    torch, dev = torch_dev
    R, W, C = 8, 2, 6
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, um.duc_step(50_000.0 * c - 120_000, R))
    side = torch.cuda.Stream()
    sizes = [4096, 2, 6000, 2048, 1026, 8192]
    chs = [lcg_channels(C, ib, 200 + i) for i, ib in enumerate(sizes)]
    dins = [torch.from_numpy(x).to(dev) for x in chs]
    douts = [torch.zeros((W, R * ib), dtype=torch.int8, device=dev) for ib in sizes]
    torch.cuda.synchronize()
    for i, ib in enumerate(sizes):
        s = side.cuda_stream if i % 2 else None
        d.process_device(dins[i].data_ptr(), ib, ib, douts[i].data_ptr(), R * ib, s)
    torch.cuda.synchronize()
    for i, ib in enumerate(sizes):
        assert (douts[i].cpu().numpy() == m.process(chs[i], ib)).all(), i


# 4. transmit: the modulator bank followed by the DUC
KINDS = [api.MOD_SSB, api.MOD_INTERP, api.MOD_AM, api.MOD_FM, api.MOD_WBFM, api.MOD_SIG_AM, api.MOD_SIG_DSB,
         api.MOD_SIG_PM, api.MOD_SIG_FM]


def pcm_for(kind, C, n, seed):
    rng = np.random.default_rng(seed)
    k = 2 if kind == api.MOD_INTERP else 1
    t = np.arange(k * n)
    return np.stack([(8000 * np.sin(2 * np.pi * (0.01 + 0.003 * c) * t) + rng.integers(-2000, 2000, k * n))
                     .astype(np.int16) for c in range(C)])


@pytest.mark.parametrize("kind", KINDS)
def test_transmit_equals_mod_then_duc(torch_dev, kind):
    torch, dev = torch_dev
    R, W, C, n = 4, 2, 3, 3
    ma, mb = api.Mod(kind, C, device=0), api.Mod(kind, C, device=0)
    da, db = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0)
    for d in (da, db):
        for c in range(C):
            d.tune(c, c % W, -400_000 + 350_000 * c)
    ib = 512 * n
    mid = torch.zeros((C, ib), dtype=torch.int8, device=dev)
    s = torch.cuda.Stream()
    for call in range(2):
        pcm = torch.from_numpy(pcm_for(kind, C, n, call)).to(dev)
        got = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        want = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        # one stream for both chains: the modulator's output is read by the DUC behind it in stream order
        da.transmit(ma, pcm.data_ptr(), n, got.data_ptr(), R * ib, s.cuda_stream)
        mb.process_device(pcm.data_ptr(), n, mid.data_ptr(), s.cuda_stream)
        db.process_device(mid.data_ptr(), ib, ib, want.data_ptr(), R * ib, s.cuda_stream)
        torch.cuda.synchronize()
        assert (got.cpu().numpy() == want.cpu().numpy()).all(), (kind, call)


@pytest.mark.parametrize("name,kind,param", [("ssbmod", api.MOD_SSB, None), ("ammod", api.MOD_AM, 0.5),
                                             ("fmmod", api.MOD_FM, 2500.0), ("wbfmmod", api.MOD_WBFM, 70000.0)])
def test_transmit_against_oracle_modulator_and_model(torch_dev, oracle, name, kind, param):
    torch, dev = torch_dev
    R, W, C, n = 8, 1, 2, 4
    mod = api.Mod(kind, C, device=0)
    d, m = both(W, C, R)
    orc = [getattr(oracle, name)() for _ in range(C)]
    if param is not None:
        mod.set_param(param)
        for o in orc:
            o.set_param(param)
    for c in range(C):
        tune_both(d, m, c, 0, um.duc_step(-200_000 + 400_000 * c, R))
    ib = 512 * n
    for call in range(2):
        pcm = pcm_for(kind, C, n, 7 + call)
        got = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        dpcm = torch.from_numpy(pcm).to(dev)
        torch.cuda.synchronize()
        d.transmit(mod, dpcm.data_ptr(), n, got.data_ptr(), R * ib)
        torch.cuda.synchronize()
        ch = np.stack([orc[c].process(pcm[c]) for c in range(C)])
        assert (got.cpu().numpy() == m.process(ch, ib)).all(), (name, call)


# 5. the closed loop on the device: Mod (WBFM) -> hrfd_duc_transmit -> hrfd_ddc_receive
def test_closed_loop_transmit_then_receive(torch_dev, oracle):
    """the stations of tests/test_duc_model.py's closed loop: the capture equals the model chain's bit for bit (the
    oracle's modulator, then the DUC model), the PCM equals the DDC model plus the oracle's receive chain, and each
    station's audio comes back (own >= 0.85, the other's <= 0.05)"""
    from tests import ddc_model as dm
    torch, dev = torch_dev
    streams, audio, amps = um.loop_stations(oracle)
    R, B, FULL = dm.SEL_R, dm.SEL_BLOCKS, 262144
    mod = api.Mod(api.MOD_WBFM, 2, device=0)
    duc = api.Duc(1, 2, R, device=0)
    for c, f in enumerate(dm.SEL_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(amps[c], c)
    d_pcm_in = torch.from_numpy(np.stack(audio).astype(np.int16)).to(dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_pcm_in.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    cap_model, m = um.loop_duc(streams, amps)
    assert (dcap.cpu().numpy() == cap_model).all(), "transmit equals the oracle's modulator and the DUC model"
    assert duc.clips(0) == int(m.clips[0]) == 0
    ddc = api.Ddc(1, 2, R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.WBFM)
    for c, f in enumerate(dm.SEL_OFFSETS):
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(dm.SEL_GAIN_SHIFT[c], c)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    assert (d_n.cpu().numpy() == 512).all()
    dd = dm.DdcModel(1, 2, R)
    for c, f in enumerate(dm.SEL_OFFSETS):
        dd.set_tuning(c, 0, dm.ddc_step(f + 64_000, R))
        dd.set_gain_shift(c, dm.SEL_GAIN_SHIFT[c])
    rx_in = dd.process(cap_model, B * FULL)
    for c in range(2):
        assert (pcm[c] == dm.oracle_rx_wbfm(oracle, rx_in[c])).all(), f"station {c}"
        assert dm.best_corr(audio[c], pcm[c]) >= 0.85 and dm.best_corr(audio[1 - c], pcm[c]) <= 0.05, c
