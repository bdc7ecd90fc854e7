"""The spectrum bank on the device (hrfd_spec_*) against the numpy model (tests/spec_model.py), tolerance 0, and the closed
loop it exists for: hrfd_duc_transmit -> Spectrum.process -> find_stations -> tune_from_scan -> hrfd_ddc_receive."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import spec_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(W, R, L):
    return api.Spectrum(W, R, L, device=0), sm.SpecModel(W, R, L)


def window_both(d, m, w):
    d.set_window(w)
    m.set_window(w)


def band_both(d, m, band, capture, first, n_bins, thr):
    d.set_band(band, capture, first, n_bins, thr)
    m.set_band(band, capture, first, n_bins, thr)


def check_call(d, m, cap, n_frames, what):
    got, want = d.process(cap, n_frames), m.process(cap, n_frames)
    for g, w, name in zip(got, want, ("power", "band_power", "present")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert (g == w).all(), f"{what}: {name} differs at {np.argwhere(g != w)[:5]}"
    return got


# 1. bit-exact against the model: every L x a spread of W and R
@pytest.mark.parametrize("L", range(sm.MIN_L, sm.MAX_L + 1))
@pytest.mark.parametrize("W,R", [(1, 1), (3, 4), (16, 8)])
def test_default_window_bit_exact(L, W, R):
    d, m = both(W, R, L)
    N = 1 << L
    for b in range(4):
        band_both(d, m, b, b % W, (b * 977) % N, 1 + (b * 131) % N, 1000 * (b + 1))
    for call, nf in enumerate((1, 5)):
        cap = sm.lcg_captures(W, 2 * N * nf, 7 * L + call)
        power, _, _ = check_call(d, m, cap, nf, f"L={L} W={W} R={R} call {call}")
        assert power.any()


@pytest.mark.parametrize("L", range(sm.MIN_L, sm.MAX_L + 1))
def test_random_and_extreme_windows(L):
    rng = np.random.default_rng(L)
    W, N = 2, 1 << L
    d, m = both(W, 8, L)
    windows = [rng.integers(-32768, 32768, size=N).astype(np.int16), np.full(N, -32768, dtype=np.int16),
               np.full(N, 32767, dtype=np.int16), np.zeros(N, dtype=np.int16)]
    windows[0][::5] = -32768
    windows[0][1::5] = 0
    for i, w in enumerate(windows):
        window_both(d, m, w)
        power, _, _ = check_call(d, m, sm.lcg_captures(W, 2 * N * 3, 31 * L + i), 3, f"L={L} window {i}")
        if i == 3:
            assert not power.any(), "a window of zeros gives an empty spectrum"
    d.set_window(None)
    m.set_window(sm.hann(L))
    check_call(d, m, sm.lcg_captures(W, 2 * N * 2, L), 2, f"L={L} default window restored")


# 2. frame counts: 1, odd, large, and counts that do not divide among the workgroups of a capture
@pytest.mark.parametrize("L,W,frames", [(8, 1, (1, 2, 3, 511, 512, 513, 1000, 4099)), (11, 2, (1, 7, 255, 257, 300)),
                                        (13, 1, (1, 3, 129, 200)), (10, 40, (1, 13, 14, 27))])
def test_frame_counts(L, W, frames):
    d, m = both(W, 2, L)
    N = 1 << L
    band_both(d, m, 0, W - 1, N - 3, 9, 5000)
    for nf in frames:
        check_call(d, m, sm.lcg_captures(W, 2 * N * nf, nf), nf, f"L={L} W={W} n_frames={nf}")


# 3. the default tables are the contract's
@pytest.mark.parametrize("L", range(sm.MIN_L, sm.MAX_L + 1))
def test_tables(L):
    assert (api.q15_table(f"SPEC_HANN_{L}") == sm.hann(L)).all()
    c, s = sm.cos_sin(L)
    assert (api.q15_table(f"SPEC_COS_{L}") == c).all() and (api.q15_table(f"SPEC_SIN_{L}") == s).all()


# 4. the closed loop: three WBFM stations on the air, found, tuned and received
LOOP_R, LOOP_L, LOOP_BLOCKS = 8, 13, 16
LOOP_OFFSETS = (-3_000_000.0, 600_000.0, 5_200_000.0)       # on the 200 kHz raster
LOOP_LEVELS = (64.0, 16.0, 32.0)                            # int8 amplitudes: 12 dB between the strongest and the weakest
LOOP_GAIN_SHIFT = (0, 2, 1)
LOOP_AUDIO = (9000, 25000, 0)                               # where each station's audio starts in count.raw
LOOP_AUDIO_DIV = (1, 1, 2)                                  # the file's first excerpt is its loudest: at half level


def test_closed_loop_scan_tune_receive(torch_dev, oracle):
    """Mod (WBFM, three count.raw excerpts at unequal amplitudes) -> hrfd_duc_transmit at R = 8 -> Spectrum.process ->
    find_stations -> tune_from_scan -> hrfd_ddc_receive.

    Exactly the three offsets come back within one raster step.  The 20 dB rule: the weakest station (amplitude 16,
    power 256 in its band) stands 10 log10(256 / (200 kHz / 16.384 MHz / 12 * 2)) = 51 dB above the int8 rounding
    noise of a 200 kHz band, the strongest station's images behind the DUC's stage A (>= 60 dB down: 4096e-6) at most
    5 dB above it.  The PCM equals the CPU chain's (tests/ddc_model.py and the oracle's receive chain over the same capture,
    the same tunings) bit for bit.  Each station's audio correlates with its own source as in tests/test_gpu_duc.py's loop
    (own >= 0.85) and not with the others': that test's 0.05 stands 0.003 above its two excerpts' own mutual correlation
    (0.047); the third excerpt correlates with the others at up to 0.063 at the source, so the bound here is
    max(0.05, the sources' own figure + 0.003) per pair."""
    from tests import ddc_model as dm
    torch, dev = torch_dev
    R, L, B, FULL = LOOP_R, LOOP_L, LOOP_BLOCKS, 262144
    pcm = dm.count_raw()
    audio = [pcm[o:o + B * 512] // LOOP_AUDIO_DIV[c] for c, o in enumerate(LOOP_AUDIO)]
    streams = np.stack([oracle.wbfmmod().process(a) for a in audio])
    rms = np.sqrt(np.mean(streams.astype(np.float64) ** 2) * 2)
    mod = api.Mod(api.MOD_WBFM, 3, device=0)
    duc = api.Duc(1, 3, R, device=0)
    for c, f in enumerate(LOOP_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(int(round(32768 * LOOP_LEVELS[c] / rms)), c)
    d_audio = torch.from_numpy(np.stack(audio).astype(np.int16)).to(dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_audio.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    assert duc.clips(0) == 0
    cap = dcap.cpu().numpy()

    spec, m = both(1, R, L)
    n_frames = cap.shape[1] // (2 << L)
    power, _, _ = spec.process(cap, n_frames)
    assert (power == m.process(cap, n_frames)[0]).all()
    raster = 200_000.0
    stations = api.find_stations(power, n_frames, R, L, 200_000.0, raster, 20.0)
    print("found", stations)
    assert len(stations) == 3, stations
    for (w, off, _), want in zip(stations, sorted(LOOP_OFFSETS)):
        assert w == 0 and abs(off - want) <= raster, (off, want)
    order = [sorted(LOOP_OFFSETS).index(f) for f in LOOP_OFFSETS]      # station c is the order[c]-th found

    ddc = api.Ddc(1, 3, R, device=0)
    chan_map = api.tune_from_scan(ddc, stations)
    assert sorted(chan_map) == [0, 1, 2]
    rx = api.Rx(3, device=0)
    rx.set_mode(api.WBFM)
    dd = dm.DdcModel(1, 3, R)
    for c in range(3):
        ch = order[c]
        ddc.set_gain_shift(LOOP_GAIN_SHIFT[c], ch)
        dd.set_tuning(ch, 0, dm.ddc_step(chan_map[ch][1] + 64_000, R))
        dd.set_gain_shift(ch, LOOP_GAIN_SHIFT[c])
    d_pcm = torch.zeros((3, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((3, B), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    got = d_pcm.cpu().numpy().reshape(3, -1)
    assert (d_n.cpu().numpy() == 512).all()
    rx_in = dd.process(cap, B * FULL)
    for c in range(3):
        ch = order[c]
        assert (got[ch] == dm.oracle_rx_wbfm(oracle, rx_in[ch])).all(), f"station {c}"
        own = dm.best_corr(audio[c], got[ch])
        print("station", c, "own", own)
        assert own >= 0.85, (c, own)
        for o in range(3):
            if o != c:
                src = max(dm.best_corr(audio[o], audio[c]), dm.best_corr(audio[c], audio[o]))
                cross = dm.best_corr(audio[o], got[ch])
                print("station", c, "other", o, "cross", cross, "sources", src)
                assert cross <= max(0.05, src + 0.003), (c, o, cross, src)
