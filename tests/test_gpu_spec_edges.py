"""The spectrum bank at its edges.  Each test proves from the model's stage values (SpecModel.stage_max, max_term) or
from the expected sums that the edge was reached, then compares the device with the model, tolerance 0."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import spec_model as sm
from tests.test_gpu_spec import band_both, both, check_call, torch_dev, window_both  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", [8, 10, 11, 13])
def test_largest_magnitude_and_power_term(L):
    """all -128 under a window of -32768: u = (16384, 16384), |u|^2 = 2^29 = 23170.5^2, and DC keeps it through every
    stage; +127 / -128 alternation puts the same energy at +-Fs/2; an Fs/4 tone lands on bin N / 4"""
    N = 1 << L
    d, m = both(1, 8, L)
    window_both(d, m, np.full(N, -32768, dtype=np.int16))
    x = np.full((1, 2 * N * 2), -128, dtype=np.int8)
    power, _, _ = check_call(d, m, x, 2, "all -128")
    assert m.stage_max == [1 << 29] * (L + 1) and m.max_term == 1 << 29
    assert int(power[0, 0]) == 2 << 29 and not power[0, 1:].any()
    alt = np.empty((N, 2), dtype=np.int8)
    alt[0::2], alt[1::2] = 127, -128
    power, _, _ = check_call(d, m, alt.reshape(1, -1), 1, "alternation")
    assert power[0].argmax() == N // 2 and m.stage_max[0] >= 16256 ** 2 * 2
    t = np.arange(N)
    tone = np.stack([np.round(127 * np.cos(np.pi * t / 2)), np.round(127 * np.sin(np.pi * t / 2))], axis=1).astype(np.int8)
    power, _, _ = check_call(d, m, tone.reshape(1, -1), 1, "Fs/4 tone")
    assert power[0].argmax() == N // 4


def test_sums_past_32_bits():
    """4096 frames of a full-scale DC input: P[0] = 4096 * 2^29 = 2^41, far past a 32-bit sum; the band over it too"""
    L, nf = 8, 4096
    N = 1 << L
    d, m = both(2, 1, L)
    window_both(d, m, np.full(N, -32768, dtype=np.int16))
    band_both(d, m, 0, 1, N - 2, 5, (1 << 29))
    band_both(d, m, 1, 1, N - 2, 5, (1 << 29) + 1)
    x = sm.lcg_captures(2, 2 * N * nf, 3)
    x[1] = -128
    power, bp, pr = check_call(d, m, x, nf, "4096 frames")
    assert int(power[1, 0]) == 1 << 41 and int(bp[0]) == 1 << 41
    assert list(pr) == [1, 0], "thresholds on both sides of equality"


@pytest.mark.parametrize("L", [8, 12])
def test_bands_wrap_both_ways_one_bin_and_all(L):
    N = 1 << L
    W = 3
    d, m = both(W, 4, L)
    cap = sm.lcg_captures(W, 2 * N * 3, L)
    power = m.process(cap, 3)[0]

    def s(w, first, n):
        return sum(int(v) for v in power[w, (first + np.arange(n)) % N])

    bands = [(0, N - 4, 9), (1, N // 2 - 3, 7), (2, 5, 1), (0, 0, N), (1, N - 1, N), (2, N // 2, N // 2 + 1), (0, N - 1, 1)]
    k = 0
    for w, first, n in bands:
        for thr3 in (s(w, first, n), s(w, first, n) + 3):             # reached exactly, missed by one unit per frame
            band_both(d, m, k, w, first, n, (thr3 + 2) // 3 if thr3 == s(w, first, n) else thr3 // 3 + 1)
            k += 1
    _, bp, pr = check_call(d, m, cap, 3, f"L={L} bands")
    assert bp.size == 2 * len(bands) and (pr[1::2] == 0).all()
    exact = [i for i, (w, first, n) in enumerate(bands) if s(w, first, n) % 3 == 0]
    assert all(pr[2 * i] == 1 for i in exact)
    d.clear_bands()
    m.clear_bands()
    got = check_call(d, m, cap, 3, "K = 0")
    assert got[1].size == 0 and got[2].size == 0


def test_offsets_strides_guard_bytes_and_unchanged_inputs(torch_dev):
    """capture base addresses and strides of every residue modulo 16, guard bytes around the outputs, inputs unchanged"""
    torch, dev = torch_dev
    L, W, nf = 9, 3, 3
    N = 1 << L
    row = 2 * N * nf
    d, m = both(W, 2, L)
    band_both(d, m, 0, 2, N - 1, 3, 100)
    for res in range(16):
        stride = row + 16 + res
        host = np.full(W * stride + 32, 77, dtype=np.int8)
        cap = sm.lcg_captures(W, row, 40 + res)
        for w in range(W):
            host[res + w * stride:res + w * stride + row] = cap[w]
        din = torch.from_numpy(host).to(dev)
        dpow = torch.full((W * N + 2,), -1, dtype=torch.int64, device=dev)
        dbp = torch.full((3,), -1, dtype=torch.int64, device=dev)
        dpr = torch.full((3,), 99, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        d.process_device(din.data_ptr() + res, stride, nf, dpow.data_ptr() + 8, dbp.data_ptr() + 8, dpr.data_ptr() + 1)
        torch.cuda.synchronize()
        want = m.process(cap, nf)
        got = dpow.cpu().numpy().view(np.uint64)
        assert (got[1:1 + W * N].reshape(W, N) == want[0]).all(), res
        assert got[0] == 2 ** 64 - 1 and got[-1] == 2 ** 64 - 1, res
        assert list(dbp.cpu().numpy().view(np.uint64)) == [2 ** 64 - 1, int(want[1][0]), 2 ** 64 - 1], res
        assert list(dpr.cpu().numpy()) == [99, int(want[2][0]), 99], res
        assert (din.cpu().numpy() == host).all(), res


def test_two_streams_and_queued_calls_with_setters(torch_dev):
    """20 asynchronous calls alternating between two streams, a window or a band changed before each: every call sees the
    settings current when it was made"""
    torch, dev = torch_dev
    L, W, nf = 10, 2, 4
    N = 1 << L
    rng = np.random.default_rng(5)
    d, m = both(W, 8, L)
    side = torch.cuda.Stream()
    caps = [sm.lcg_captures(W, 2 * N * nf, 300 + i) for i in range(20)]
    dins = [torch.from_numpy(c).to(dev) for c in caps]
    dpow = [torch.zeros((W, N), dtype=torch.int64, device=dev) for _ in caps]
    dbp = [torch.zeros((8,), dtype=torch.int64, device=dev) for _ in caps]
    dpr = [torch.zeros((8,), dtype=torch.uint8, device=dev) for _ in caps]
    want, ks = [], []
    torch.cuda.synchronize()
    for i in range(20):
        if i % 2 == 0:
            window_both(d, m, rng.integers(-32768, 32768, size=N).astype(np.int16))
        else:
            band = min(i // 4, len(m.bands))
            band_both(d, m, band, i % W, int(rng.integers(0, N)), int(rng.integers(1, N + 1)), int(rng.integers(0, 1 << 20)))
        s = side.cuda_stream if i % 2 else None
        d.process_device(dins[i].data_ptr(), 2 * N * nf, nf, dpow[i].data_ptr(), dbp[i].data_ptr(), dpr[i].data_ptr(), s)
        want.append(m.process(caps[i], nf))
        ks.append(len(m.bands))
    torch.cuda.synchronize()
    for i in range(20):
        k = ks[i]
        assert (dpow[i].cpu().numpy().view(np.uint64) == want[i][0]).all(), i
        assert (dbp[i].cpu().numpy().view(np.uint64)[:k] == want[i][1]).all(), i
        assert (dpr[i].cpu().numpy()[:k] == want[i][2]).all(), i


def test_largest_call_the_header_allows():
    """65536 frames (HRFD_SPEC_MAX_FRAMES) at N = 256 with the largest threshold: 2^44 * 2^16 stays inside uint64"""
    L, nf = 8, sm.MAX_FRAMES
    N = 1 << L
    d, m = both(1, 1, L)
    window_both(d, m, np.full(N, -32768, dtype=np.int16))
    band_both(d, m, 0, 0, 0, N, sm.MAX_THRESHOLD)
    band_both(d, m, 1, 0, 0, N, 1 << 29)
    x = np.full((1, 2 * N * nf), -128, dtype=np.int8)
    power, bp, pr = check_call(d, m, x, nf, "65536 frames")
    assert int(power[0, 0]) == 1 << 45 and int(bp[0]) == 1 << 45 and list(pr) == [0, 1]


def test_arguments_are_refused():
    d = api.Spectrum(1, 8, 8, device=0)
    x = np.zeros((1, 512), dtype=np.int8)
    with pytest.raises(api.HrfdError):
        d.process(np.zeros((1, 0), dtype=np.int8), 0)
    with pytest.raises(api.HrfdError):
        d.process(np.zeros((1, 512 * 65537), dtype=np.int8), 65537)
    for bad in [(0, 1, 0, 1, 0), (0, 0, 256, 1, 0), (0, 0, 0, 0, 0), (0, 0, 0, 257, 0), (1, 0, 0, 1, 0),
                (0, 0, 0, 1, sm.MAX_THRESHOLD + 1)]:
        with pytest.raises(api.HrfdError):
            d.set_band(*bad)
    for args in [(0, 8, 8), (1, 3, 8), (1, 8, 7), (1, 8, 14)]:
        with pytest.raises(api.HrfdError):
            api.Spectrum(*args, device=0)
    assert d.process(x, 1)[0].shape == (1, 256)
