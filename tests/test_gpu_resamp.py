"""The resampler bank on the device (hrfd_resamp_*) against the numpy model (tests/resamp_model.py), tolerance 0: the ratios
(interpolating, decimating, both, the most branches, the widest input span of a tile), the tap counts where the packing of a
branch changes, the rounding and saturation boundaries, a stream cut into calls with calls that give no output, reset and
set_taps, n_pcm at its edges with other bytes behind it, channel counts and the longest call, every even residue of both rows
with padded strides and guard bytes around every buffer, a call on a second stream, what needs a handle to be refused, and
the closed loop: Audio.process_device's out and mix through Resampler.process_device on the same stream."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import audio_model as am
from tests import resamp_model as rm
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def random_taps(T, L, seed):
    """T int16 taps with sum |h| <= 65535 over every one of the L branches, most of the bound used"""
    K = -(-T // L)
    top = min(32767, 65535 // K)
    return np.random.default_rng(seed).integers(-top, top + 1, size=T).astype(np.int16)


def both(C, L, M, taps=None):
    d, m = api.Resampler(C, L, M, device=0), rm.ResampModel(C, L, M)
    if taps is not None:
        d.set_taps(taps)
        m.set_taps(taps)
    return d, m


_reference = {}


def reference(C, n, seed=7):
    """random int16 over the full range, one array per shape, computed once and left unchanged"""
    key = (C, n, seed)
    if key not in _reference:
        x = np.random.default_rng(seed).integers(-32768, 32768, size=(C, n), dtype=np.int16)
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def run_device(torch_dev, d, m, pcm, n_pcm, what, residue=0, out_residue=0, pad=0, out_pad=0, spare=0, stream=None):
    """process_device over rows at `residue` modulo 16, 2 n_in + pad bytes apart, out rows of out_count + spare samples at
    out_residue, 2 capacity + out_pad bytes apart, every buffer between guards; the model takes the same call.  The count
    must be out_count's and the model's, the input unchanged, and nothing but the first n_out samples of each row written."""
    torch, dev = torch_dev
    C, n = pcm.shape
    want = m.process(pcm, n_pcm)
    cap = want.shape[1] + spare
    assert d.out_count(n) == want.shape[1], what
    stride, out_stride = 2 * n + pad, 2 * cap + out_pad
    src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
    for c in range(C):
        src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
    src.put(0, pcm[0])
    d_n = None if n_pcm is None else torch.from_numpy(np.ascontiguousarray(n_pcm, dtype=np.uint32).view(np.int32)).to(dev)
    out = Guarded(torch_dev, out_stride * (C - 1) + 2 * cap + 2, out_residue, 16, 22)      # (2 bytes so that no buffer is empty)
    torch.cuda.synchronize()
    n_out = d.process_device(src.ptr, stride, None if d_n is None else d_n.data_ptr(), n, out.ptr, out_stride, cap, stream)
    torch.cuda.synchronize()
    assert n_out == want.shape[1], f"{what}: {n_out} outputs, the model has {want.shape[1]}"
    src.check(None, what + ": the input")
    rows = out.host[out.off:out.off + out.n].copy()
    for c in range(C):
        rows[c * out_stride:c * out_stride + 2 * n_out] = want[c].view(np.uint8)
    out.check(rows, what + ": out")
    return want


# 1. the ratios: identity, interpolation, decimation, both, the most branches, 44.1 kS/s in both directions
@pytest.mark.parametrize("L,M,n_in", [(1, 1, 1536), (2, 1, 1536), (6, 1, 1536), (1, 6, 1536), (3, 2, 1536), (2, 3, 1536), (7, 8, 1536),
                                      (1, 8, 1536), (512, 1, 64), (441, 80, 1536), (80, 441, 1536)])
def test_ratios(torch_dev, L, M, n_in):
    pcm = reference(3, n_in)
    if L == 1 and M == 1:
        d, m = both(3, 1, 1)
        got = d.process(pcm)
        assert (got == pcm).all() and (m.process(pcm) == pcm).all()      # the default: the identity
    taps = random_taps(min(9 * L - 1, 16384) if L > 1 else 9, L, L + M)
    d, m = both(3, L, M, taps)
    got, want = d.process(pcm), m.process(pcm)
    assert got.shape == want.shape and (got == want).all(), f"{L}/{M}, host path: differs at {np.argwhere(got != want)[:4].tolist()}"
    assert got.shape[1] == -(-n_in * L // M)
    run_device(torch_dev, d, m, pcm, None, f"{L}/{M} behind a call")
    run_device(torch_dev, d, m, pcm[:, :777], None, f"{L}/{M} behind two calls", spare=5)


# the widest tile: 1024 outputs 8 samples apart with 512 taps in front of them, two whole tiles and a partial one
def test_widest_input_span(torch_dev):
    d, m = both(2, 1, 8, random_taps(512, 1, 3))
    pcm = reference(2, 8 * 2048 + 8 * 100 + 3)
    run_device(torch_dev, d, m, pcm, None, "1/8 with 512 taps")
    run_device(torch_dev, d, m, pcm, None, "1/8 with 512 taps, behind a call")


# 2. the tap counts: a branch without a tap, one tap per branch, both parities of K, the longest branch, the most taps
@pytest.mark.parametrize("L,T", [(6, 1), (6, 5), (6, 6), (6, 7), (6, 11), (6, 12), (6, 13), (6, 17), (6, 18), (6, 19), (6, 383), (6, 384),
                                 (6, 385), (1, 512), (32, 16384)])
def test_tap_counts(torch_dev, L, T):
    d, m = both(3, L, 1, random_taps(T, L, T))
    pcm = reference(3, 1536 if L < 32 else 192)
    run_device(torch_dev, d, m, pcm, None, f"L={L} T={T}")
    run_device(torch_dev, d, m, pcm[:, :100], None, f"L={L} T={T}, behind a call", out_residue=2)


# 3. the rounding and saturation boundaries, and the largest accumulators the tap check allows, in both signs
def test_rounding_and_saturation_boundaries():
    d, m = both(1, 1, 1, [16384, 1])
    # acc = 16384 x[n] + x[n-1]: (acc + 2^13) >> 14 = x[n] + ((x[n-1] + 2^13) >> 14)
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, 110:112] = (8191, 32767)                          # 32767
    x[0, 120:122] = (8192, 32767)                          # 32768 -> 32767
    x[0, 130:132] = (-8192, -32768)                        # -32768
    x[0, 140:142] = (-8193, -32768)                        # -32769 -> -32768
    x[0, 150:152] = (-8193, 5)                             # 4: the shift is arithmetic
    got, want = d.process(x), m.process(x)
    assert (got == want).all()
    assert [int(got[0, i]) for i in (111, 121, 131, 141, 151)] == [32767, 32767, -32768, -32768, 4]
    # sum |h| |x| = 65535 x 32768 on every branch: L = 1, and L = 2 with the two lists interleaved
    for L, taps, y in ((1, [-32768, -32767], 32767), (1, [32767, 32767, 1], -32768), (1, [-128] * 511 + [-127], 32767),
                       (1, [128] * 511 + [127], -32768), (2, [-32768, 32767, -32767, 32767, 0, 1], None)):
        d, m = both(1, L, 1, taps)
        x = np.full((1, 1024), -32768, dtype=np.int16)
        got, want = d.process(x), m.process(x)
        assert (got == want).all(), f"taps {taps[:4]}.."
        if y is not None:
            assert (got[0, 512:] == y).all()
        else:
            assert (got[0, 1024::2] == 32767).all() and (got[0, 1025::2] == -32768).all()


# 4. a stream cut into calls, calls without output among them; every call's n_out is out_count's
@pytest.mark.parametrize("L,M", [(1, 3), (2, 3), (1, 6), (3, 2), (1, 1), (5, 8), (6, 1)])
def test_call_cutting(torch_dev, L, M):
    C = 3
    cuts = [1, 2, 3, 511, 512, 513, 1, 1, 2, 1]
    pcm = reference(C, sum(cuts))
    taps = random_taps(37 * L - 1 if L > 1 else 37, L, 40 + L)
    whole, mw = both(C, L, M, taps)
    out = whole.process(pcm)
    assert (out == mw.process(pcm)).all() and out.shape[1] == -(-sum(cuts) * L // M)
    parts, mp = both(C, L, M, taps)
    at, got, zero = 0, [], 0
    for k, n in enumerate(cuts):
        x = pcm[:, at:at + n]
        if k % 2:
            count = parts.out_count(n)
            y = parts.process(x)
            assert y.shape[1] == count
            assert (y == mp.process(x)).all(), f"{L}/{M}: call {k} of {n}"
        else:
            y = run_device(torch_dev, parts, mp, x, None, f"{L}/{M}: call {k} of {n}", residue=2 * (k % 8), out_residue=(6 * k + 2) % 16)
        zero += y.shape[1] == 0
        got.append(y)
        at += n
    assert (np.concatenate(got, axis=1) == out).all()
    assert zero > 0 or L > 1 or M == 1                     # (1, 3) and (1, 6): the calls of one or two samples behind the first


# 5. reset of one channel and of all; set_taps between calls
def test_reset_and_set_taps(torch_dev):
    C, L, M = 3, 3, 2
    taps = random_taps(3 * 200, L, 51)
    pcm = reference(C, 1001)
    d, m = both(C, L, M, taps)
    first = run_device(torch_dev, d, m, pcm, None, "first call")          # 1001 x 3 is odd: d = 1 behind it
    assert m.d == 1
    d.reset(1)
    m.reset(1)
    nxt = run_device(torch_dev, d, m, pcm, None, "behind reset(1)")
    fresh, mf = both(C, L, M, taps)
    assert (fresh.process(pcm) == first).all()
    assert (nxt[0] != first[0][1:]).any() and (nxt[2] != first[2][1:]).any()     # the others go on, one output later in phase
    # channel 1 as from zeros, at the handle's phase
    y, _ = rm.slow_channel(pcm[1], [], taps, L, M, 1)
    assert nxt[1].tolist() == y
    d.reset()
    m.reset()
    assert (run_device(torch_dev, d, m, pcm, None, "behind reset()") == first).all()
    # set_taps, even with the same taps: as from a new handle
    run_device(torch_dev, d, m, pcm, None, "a call in between")
    d.set_taps(taps)
    m.set_taps(taps)
    assert (run_device(torch_dev, d, m, pcm, None, "behind set_taps") == first).all()
    other = random_taps(3 * 7 + 1, L, 52)
    d.set_taps(other)
    m.set_taps(other)
    run_device(torch_dev, d, m, pcm, None, "behind other taps")
    run_device(torch_dev, d, m, pcm, None, "behind other taps, second call")


# 6. n_pcm at its edges: the bytes behind it are random and must not matter, in their own call and through the history
@pytest.mark.parametrize("L,M", [(6, 1), (1, 6), (2, 3)])
def test_n_pcm_edges(torch_dev, L, M):
    edges = np.array([0, 1, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32)
    n_pcm = np.stack([edges, edges[::-1], np.roll(edges, 2)])
    taps = random_taps(500 * L, L, 61)
    d, m = both(3, L, M, taps)
    pcm = reference(3, 512 * 6)
    want = run_device(torch_dev, d, m, pcm, n_pcm, "n_pcm edges")
    tail = run_device(torch_dev, d, m, pcm[:, :700], None, "the call behind a short last block")
    taken = np.minimum(n_pcm.astype(np.int64), 512)
    other = pcm.copy()
    for c in range(3):
        for b in range(6):
            other[c, 512 * b + int(taken[c, b]):512 * (b + 1)] ^= 0x5A5A
    d2, _ = both(3, L, M, taps)
    assert (d2.process(other, n_pcm) == want).all(), "other bytes behind n_pcm"
    assert (d2.process(pcm[:, :700]) == tail).all(), "other bytes behind n_pcm, the next call"


# 7. sizes: partial last workgroups over the channels, and the longest call
@pytest.mark.parametrize("C", [1, 2, 255, 257])
def test_channel_counts(C):
    d, m = both(C, 3, 2, random_taps(33, 3, C))
    pcm = reference(C, 1536)
    rng = np.random.default_rng(C)
    n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C, 3))
    assert (d.process(pcm, n_pcm) == m.process(pcm, n_pcm)).all(), f"C={C}"
    assert (d.process(pcm[:, :99]) == m.process(pcm[:, :99])).all(), f"C={C}, second call"


def test_longest_call():
    d, m = both(1, 1, 6, random_taps(12, 1, 71))
    pcm = reference(1, 524288, seed=8)
    for what in ("524288 samples", "behind them"):
        got, want = d.process(pcm), m.process(pcm)
        assert got.shape == want.shape and (got == want).all(), what


# 8. every even residue of both rows modulo 16, padded strides on both sides, guard bytes around both buffers
@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_addresses_and_strides(torch_dev, residue):
    d, m = both(3, 3, 2, random_taps(3 * (6 + residue) - 1, 3, 13))
    pcm = reference(3, 701)
    for out_residue in range(0, 16, 2):
        pad, out_pad = ((2, 6), (6, 16), (16, 2), (0, 0))[(residue + out_residue) // 2 % 4]
        run_device(torch_dev, d, m, pcm, None, f"residues {residue} {out_residue} pads {pad} {out_pad}", residue, out_residue, pad, out_pad,
                   spare=out_residue // 2)


# 9. a call on a second stream behind one on the first, settings changed while calls run
def test_streams_and_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    C, L, M, n_in = 16, 6, 1, 2048
    taps = api.resample_taps(L, M, 40)
    d, m = both(C, L, M, taps)
    pcm = reference(C, n_in)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 6
    d_out = torch.zeros((calls, C, n_in * L), dtype=torch.int16, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        if i == 2:
            d.reset(5)
            m.reset(5)
        if i == 3:
            other = random_taps(6 * 12, L, 91)
            d.set_taps(other)
            m.set_taps(other)
        st = streams[1 if i in (1, 4) else 0]
        n = d.process_device(d_pcm.data_ptr(), 2 * n_in, None, n_in, d_out[i].data_ptr(), 0, n_in * L, st.cuda_stream)
        want.append(m.process(pcm))
        assert n == want[-1].shape[1]
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        got = d_out[i].cpu().numpy()
        assert (got == want[i]).all(), f"call {i}: differs at {np.argwhere(got != want[i])[:4].tolist()}"


# what needs a handle to be refused
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=dev)
    p = buf.data_ptr()
    d = api.Resampler(4, 6, 1, device=0)
    x = np.zeros((4, 8), dtype=np.int16)
    with pytest.raises(api.HrfdError, match=r"hrfd_resamp_process failed \(-4\).*set_taps"):
        d.process(x)
    with pytest.raises(api.HrfdError, match=r"hrfd_resamp_process_device failed \(-4\).*set_taps"):
        d.process_device(p, 16, None, 8, p + 8192, 96, 48)
    assert d.out_count(8) == 48                            # the count needs no taps
    with pytest.raises(api.HrfdError, match="hrfd_resamp_set_taps.*513 taps per branch"):
        d.set_taps([1] * (6 * 512 + 1))
    with pytest.raises(api.HrfdError, match="hrfd_resamp_set_taps.*branch 5 of 6 has sum .h. = 65536"):
        d.set_taps([0, 0, 0, 0, 0, 32767, 0, 0, 0, 0, 0, -32767, 0, 0, 0, 0, 0, 2])
    d.set_taps([0, 0, 0, 0, 0, 32767, 0, 0, 0, 0, 0, -32767, 0, 0, 0, 0, 0, 1])
    with pytest.raises(api.HrfdError, match="hrfd_resamp_reset.*channel 4"):
        d.reset(4)
    with pytest.raises(api.HrfdError, match="hrfd_resamp_process_device.*out_capacity 47 is below the 48"):
        d.process_device(p, 16, None, 8, p + 8192, 96, 47)
    assert d.out_count(8) == 48                            # nothing moved
    # out behind the first input row but inside the fourth
    with pytest.raises(api.HrfdError, match="hrfd_resamp_process_device.*overlaps"):
        d.process_device(p, 1024, None, 8, p + 3 * 1024 + 14, 96, 48)
    # the longest call at the most branches: n_in x up = 2^28, far below the 2^31 the kernel's 32-bit q needs
    big = api.Resampler(1, 512, 1, device=0)
    assert big.out_count(524288) == 512 * 524288
    with pytest.raises(api.HrfdError, match="hrfd_resamp_out_count.*n_in must be 1..524288"):
        big.out_count(524289)
    # a decimator's phase: the second call of one sample gives nothing, and a capacity of 0 is enough for it
    dec = api.Resampler(1, 1, 6, device=0)
    dec.set_taps([16384])
    one = np.array([[1234]], dtype=np.int16)
    assert dec.process(one).tolist() == [[1234]] and dec.out_count(1) == 0
    assert dec.process_device(p, 2, None, 1, p + 8192, 2, 0) == 0
    assert dec.out_count(4) == 0 and dec.out_count(5) == 1
    assert d.process(x).shape == (4, 48)                   # the handle still works


# 10. the closed loop on the device: the audio bank's out and mix rows to 48 kS/s, no host copy between
def test_closed_loop_audio_to_sound_card_rate(torch_dev):
    torch, dev = torch_dev
    C, B, n_blocks = 3, 2, 2
    n = 512 * n_blocks
    voice = api.audio_highpass_taps(63)
    abank, amodel = api.Audio(C, B, device=0), am.AudioModel(C, B)
    for a in (abank, amodel):
        a.set_taps(voice)
        a.set_bus(0, [0, 1, 2], [api.AUDIO_UNITY_GAIN // 2] * 3)
        a.set_bus(1, [2], [api.AUDIO_UNITY_GAIN])
    taps = api.resample_taps(6, 1, 40)
    r_out, m_out = both(C, 6, 1, taps)
    r_mix, m_mix = both(B, 6, 1, taps)
    pcm = reference(C, n)
    n_pcm = np.array([[512, 300], [512, 512], [0, 512]], dtype=np.uint32)
    open_ = np.array([[1, 1], [1, 0], [1, 1]], dtype=np.uint8)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    d_n = torch.from_numpy(n_pcm.view(np.int32)).to(dev)
    d_open = torch.from_numpy(open_).to(dev)
    d_z = torch.zeros((C, n), dtype=torch.int16, device=dev)
    d_mix = torch.zeros((B, n), dtype=torch.int16, device=dev)
    d_clips = torch.zeros(B, dtype=torch.int32, device=dev)
    d_out48 = torch.zeros((C, 6 * n), dtype=torch.int16, device=dev)
    d_mix48 = torch.zeros((B, 6 * n), dtype=torch.int16, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    for call in range(2):                                  # the second call runs on both banks' histories
        abank.process_device(d_pcm.data_ptr(), 2 * n, d_n.data_ptr(), d_open.data_ptr(), n_blocks, d_z.data_ptr(), 0, d_mix.data_ptr(),
                             d_clips.data_ptr(), st.cuda_stream)
        assert r_out.process_device(d_z.data_ptr(), 2 * n, None, n, d_out48.data_ptr(), 0, 6 * n, st.cuda_stream) == 6 * n
        assert r_mix.process_device(d_mix.data_ptr(), 2 * n, None, n, d_mix48.data_ptr(), 0, 6 * n, st.cuda_stream) == 6 * n
        st.synchronize()
        torch.cuda.synchronize()
        z, mix, clips = amodel.process(pcm, n_pcm, open_)
        assert (d_z.cpu().numpy() == z.reshape(C, n)).all() and (d_mix.cpu().numpy() == mix.reshape(B, n)).all()
        assert (d_out48.cpu().numpy() == m_out.process(z.reshape(C, n))).all(), f"call {call}: out at 48 kS/s"
        assert (d_mix48.cpu().numpy() == m_mix.process(mix.reshape(B, n))).all(), f"call {call}: mix at 48 kS/s"
