"""The tone bank on the device (hrfd_tone_*) against the numpy model (tests/tone_model.py), tolerance 0: every frame length,
the tone counts where the tiling over the waves changes, channel and frame counts with a partial last workgroup, n_pcm at its
edges, every even residue of the input with padded strides and guard bytes around every buffer, each output alone, the
largest sums the law allows and the thresholds on their boundaries, ties, setter changes behind running calls, and the closed
loop the bank exists for: Mod -> Duc.transmit -> Ddc.receive -> Tones.process_device on the buffers receive filled."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import tone_model as tm

pytestmark = pytest.mark.gpu

GUARD = 64
OUTPUTS = ("power", "energy", "valid", "best", "present")
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C, L, steps, groups=None):
    d, m = api.Tones(C, L, device=0), tm.ToneModel(C, L)
    d.set_tones(steps=steps, groups=groups)
    m.set_tones(steps, groups)
    return d, m


def random_steps(K, seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 1 << 32, size=K, dtype=np.uint64)]


_reference = {}


def reference(C, n, seed=7):
    """random int16 over the full range, one array per shape, computed once and left unchanged"""
    key = (C, n, seed)
    if key not in _reference:
        x = np.random.default_rng(seed).integers(-32768, 32768, size=(C, n), dtype=np.int16)
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def same(got, want, what):
    for name, g, w in zip(OUTPUTS, got, want):
        assert g.shape == w.shape and (g == w).all(), f"{what}: {name} differs at {np.argwhere(g != w)[:4].tolist()}"


class Guarded:
    """n bytes of device memory at an address of the given residue modulo `align`, random bytes in it, before and behind"""

    def __init__(self, torch_dev, n, residue, align, seed):
        torch, dev = torch_dev
        self.torch, self.n = torch, n
        self.host = np.random.default_rng(seed).integers(0, 256, size=GUARD + align + n + GUARD, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host).to(dev)
        self.off = GUARD + (residue - (self.dev.data_ptr() + GUARD)) % align
        self.ptr = self.dev.data_ptr() + self.off

    def put(self, offset, data):
        b = np.ascontiguousarray(data).view(np.uint8).ravel()
        self.host[self.off + offset:self.off + offset + b.size] = b
        self.dev.copy_(self.torch.from_numpy(self.host))

    def check(self, want, what):
        """the buffer as it must look when only `want` (an array laid over the n bytes, or None) has changed"""
        expect = self.host.copy()
        if want is not None:
            b = np.ascontiguousarray(want).view(np.uint8).ravel()
            assert b.size == self.n
            expect[self.off:self.off + self.n] = b
        got = self.dev.cpu().numpy()
        assert (got == expect).all(), f"{what}: differs at bytes {np.argwhere(got != expect)[:5].ravel()} (the region starts at {self.off})"


def run_device(torch_dev, d, m, pcm, n_pcm, what, residue=0, pad=0, outputs=OUTPUTS, stream=None):
    """process_device over rows at `residue` modulo 16, 1024 n_blocks + pad bytes apart, every buffer between guards"""
    torch, dev = torch_dev
    C, n = pcm.shape
    n_blocks = n // 512
    stride = 2 * n + pad
    src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
    for c in range(C):
        src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
    src.put(0, pcm[0])
    d_n = None if n_pcm is None else torch.from_numpy(np.ascontiguousarray(n_pcm, dtype=np.uint32).view(np.int32)).to(dev)
    want = dict(zip(OUTPUTS, m.process(pcm, n_pcm)))
    bufs = {name: Guarded(torch_dev, want[name].nbytes, 0, 8, 22 + i) for i, name in enumerate(OUTPUTS)}
    torch.cuda.synchronize()
    d.process_device(src.ptr, stride, None if d_n is None else d_n.data_ptr(), n_blocks,
                     *[bufs[name].ptr if name in outputs else None for name in OUTPUTS], stream)
    torch.cuda.synchronize()
    src.check(None, what + ": the input")
    for name in OUTPUTS:
        bufs[name].check(want[name] if name in outputs else None, f"{what}: {name}")
    return want


# 1. every frame length, two frames per channel, through the host path and the device path
@pytest.mark.parametrize("L", [128, 256, 512, 1024, 2048, 4096, 8192])
def test_every_frame_length(torch_dev, L):
    steps = [tm.tone_step(f) for f in (67.0, 697.0, 1000.0, 1633.0, 3999.0)]
    d, m = both(3, L, steps, [0, 1, 1, 0, 1])
    pcm = reference(3, max(2 * L, 512))
    same(d.process(pcm), m.process(pcm), f"L={L}, host path")
    run_device(torch_dev, d, m, pcm, None, f"L={L}")


# 2. the tone counts where the tiling changes: four waves take a tone each at a time
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128])
def test_tone_counts(K):
    d, m = both(2, 256, random_steps(K, K), [k % 3 for k in range(K)])
    pcm = reference(2, 512)
    same(d.process(pcm), m.process(pcm), f"K={K}")
    assert d.n_tones == K


# 3. channel and frame counts where the last workgroup is partial (16 frames of 128 per workgroup), and a frame count per
#    channel that is no power of two
@pytest.mark.parametrize("C", [1, 2, 255, 257])
def test_partial_last_workgroup(C):
    d, m = both(C, 128, random_steps(3, 5), [0, 1, 0])
    pcm = reference(C, 512)
    same(d.process(pcm), m.process(pcm), f"C={C}")


@pytest.mark.parametrize("L,n_blocks,C", [(512, 3, 5), (1024, 6, 3), (128, 3, 7), (4096, 24, 2)])
def test_odd_frame_counts(L, n_blocks, C):
    d, m = both(C, L, random_steps(6, 9), [0, 1, 2, 3, 0, 1])
    pcm = reference(C, 512 * n_blocks)
    rng = np.random.default_rng(L)
    n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C, n_blocks))
    same(d.process(pcm), m.process(pcm), f"L={L} x {n_blocks} blocks")
    same(d.process(pcm, n_pcm), m.process(pcm, n_pcm), f"L={L} x {n_blocks} blocks with n_pcm")


# 4. n_pcm at its edges: the bytes behind it are random and must not matter, valid is exact
@pytest.mark.parametrize("L", [128, 1024])
def test_n_pcm_edges(torch_dev, L):
    edges = np.array([0, 1, 2, 255, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32)
    n_pcm = np.stack([edges, edges[::-1], np.roll(edges, 3)])
    d, m = both(3, L, random_steps(4, 11), [0, 1, 2, 3])
    d.set_threshold(ALL, ratio_q8=0, min_energy=0)
    m.set_threshold(ALL, 0, 0)
    pcm = reference(3, 512 * 8)
    want = run_device(torch_dev, d, m, pcm, n_pcm, f"L={L}")
    taken = np.minimum(n_pcm.astype(np.int64), 512)
    assert want["valid"].sum() == taken.sum()
    if L == 128:
        assert list(want["valid"][0, 12:16]) == [128, 127, 0, 0] and list(want["valid"][0, 16:20]) == [128, 128, 128, 127]
        assert (want["present"][0, :4] == 0).all() and (want["present"][0, 20:32] == 1).all()
    else:
        assert list(want["valid"][0]) == [1, 257, 1023, 1024]
    # other bytes behind n_pcm, the same answers
    other = pcm.copy()
    for c in range(3):
        for b in range(8):
            other[c, 512 * b + int(taken[c, b]):512 * (b + 1)] ^= 0x5A5A
    same(d.process(other, n_pcm), [want[k] for k in OUTPUTS], f"L={L}: other bytes behind n_pcm")


# 5. every even residue of the input, padded strides, guard bytes around every buffer, each output alone
@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_addresses_strides_and_single_outputs(torch_dev, residue):
    d, m = both(3, 256, random_steps(5, 13), [0, 1, 1, 2, 0])
    pcm = reference(3, 1024)
    n_pcm = np.array([[512, 300], [0, 512], [512, 512]], dtype=np.uint32)
    for i, pad in enumerate((2, 6, 16)):
        run_device(torch_dev, d, m, pcm, n_pcm if i == 1 else None, f"residue {residue} pad {pad}", residue, pad)
        one = OUTPUTS[(3 * (residue // 2) + i) % len(OUTPUTS)]
        run_device(torch_dev, d, m, pcm, n_pcm, f"residue {residue} pad {pad} {one} alone", residue, pad, outputs=(one,))


def test_each_output_alone(torch_dev):
    d, m = both(2, 128, random_steps(3, 14), [0, 1, 1])
    pcm = reference(2, 512)
    for one in OUTPUTS:
        run_device(torch_dev, d, m, pcm, None, f"{one} alone", 2, 6, outputs=(one,))


# 6. the largest |I|, P and E the law allows (the 64-bit widening), and the thresholds on their boundaries
def test_extremes_and_threshold_boundaries(torch_dev):
    L = 8192
    steps = [0, 1, 1 << 31, (1 << 32) - 1]
    d, m = both(1, L, steps, [0, 1, 2, 3])
    flat = np.full(L, 32767, dtype=np.int16)
    d.set_window(flat)
    m.set_window(flat)
    for v in (-32768, 32767):
        pcm = np.full((1, 2 * L), v, dtype=np.int16)
        u = (v * 32767 + (1 << 14)) >> 15
        E = L * u * u
        for e_min, ratio, expect in ((E, 0, 1), (E + 1, 0, 0), (0, 1 << 20, None), (1 << 43, 0, 0)):
            d.set_threshold(ALL, ratio_q8=ratio, min_energy=e_min)
            m.set_threshold(ALL, ratio, e_min)
            want = run_device(torch_dev, d, m, pcm, None, f"all {v}, E_min {e_min}, T {ratio}")
            assert int(want["energy"][0, 0]) == E
            assert int(want["power"][0, 0, 0]) == ((L * u * 32767 + (1 << 14)) >> 15) ** 2      # step 0: I = L u 32767, Q = 0
            if expect is not None:
                assert (want["present"] == expect).all(), (v, e_min, want["present"])
    # P_best == (E T) >> 8 exactly: one sample of 16 under the flat window gives E = 256, so (E T) >> 8 = T
    pcm = np.zeros((1, 2 * L), dtype=np.int16)
    pcm[0, 5] = pcm[0, L + 77] = 16
    P = m.process(pcm)[0]
    assert int(m.process(pcm)[1][0, 0]) == 256
    for g in range(4):
        p = int(P[0, 0, g])
        for ratio, expect in ((p, 1), (p + 1, 0), (p - 1, 1)):
            d.set_threshold(g, ratio_q8=ratio, min_energy=0)
            m.set_threshold(g, ratio, 0)
            want = run_device(torch_dev, d, m, pcm, None, f"group {g}, T = P {ratio - p:+d}", outputs=("present", "best"))
            assert want["present"][0, 0, g] == expect, (g, ratio, p)


# 7. ties: equal steps in one group, the lower index wins; a group without tones answers 255 and 0
def test_ties_and_empty_groups():
    s = tm.tone_step(941.0)
    d, m = both(2, 256, [s, 123456789, s, s, 123456789], [1, 3, 1, 1, 3])
    d.set_threshold(ALL, ratio_q8=0, min_energy=0)
    m.set_threshold(ALL, 0, 0)
    pcm = reference(2, 1024)
    got = d.process(pcm)
    same(got, m.process(pcm), "ties")
    power, energy, valid, best, present = got
    assert (power[:, :, 0] == power[:, :, 2]).all() and (power[:, :, 1] == power[:, :, 4]).all()
    assert set(best[:, :, 1].ravel()) <= {0} and set(best[:, :, 3].ravel()) <= {1}
    assert (best[:, :, 0] == 255).all() and (best[:, :, 2] == 255).all()
    assert (present[:, :, 0] == 0).all() and (present[:, :, 2] == 0).all() and (present[:, :, 1] == 1).all()


# 8. the settings of a call are those set before it, whatever still runs
def test_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    C, L, n_blocks = 64, 256, 16
    F = 512 * n_blocks // L
    d, m = both(C, L, random_steps(8, 15), [0] * 4 + [1] * 4)
    pcm = reference(C, 512 * n_blocks)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 6
    K = [8, 8, 5, 5, 128, 3]
    d_power = [torch.zeros((C, F, k), dtype=torch.int64, device=dev) for k in K]
    d_present = torch.zeros((calls, C, F, 4), dtype=torch.uint8, device=dev)
    d_best = torch.zeros((calls, C, F, 4), dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rng = np.random.default_rng(16)
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        if i == 1:
            w = rng.integers(-32767, 32768, size=L).astype(np.int16)
            d.set_window(w)
            m.set_window(w)
        if i in (2, 4, 5):
            steps, groups = random_steps(K[i], 17 + i), [int(g) for g in rng.integers(0, 4, size=K[i])]
            d.set_tones(steps=steps, groups=groups)
            m.set_tones(steps, groups)
        if i == 3:
            d.set_window(None)
            m.set_window(None)
        d.set_threshold(i % 4, ratio_q8=100 * i, min_energy=1000 * i)
        m.set_threshold(i % 4, 100 * i, 1000 * i)
        # four calls on one stream, then one on a second stream directly behind them, then the first stream again
        st = streams[1 if i == 4 else 0]
        d.process_device(d_pcm.data_ptr(), 1024 * n_blocks, None, n_blocks, d_power[i].data_ptr(), None, None,
                         d_best[i].data_ptr(), d_present[i].data_ptr(), st.cuda_stream)
        want.append(m.process(pcm))
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        assert (d_power[i].cpu().numpy().view(np.uint64) == want[i][0]).all(), f"call {i}: power"
        assert (d_best[i].cpu().numpy() == want[i][3]).all() and (d_present[i].cpu().numpy() == want[i][4]).all(), f"call {i}"


# what needs a handle to be refused
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    d = api.Tones(2, 1024, device=0)
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=dev)
    p = buf.data_ptr()
    with pytest.raises(api.HrfdError, match="hrfd_tone_process_device.*no tones"):
        d.process_device(p, 2048, None, 2, p + 32768)
    with pytest.raises(api.HrfdError, match="hrfd_tone_process.*no tones"):
        d.process(np.zeros((2, 1024), dtype=np.int16))
    assert d.n_tones == 0
    d.set_tones([1000.0])
    with pytest.raises(api.HrfdError, match="hrfd_tone_process_device.*frames"):
        d.process_device(p, 4096, None, 3, p + 32768)
    with pytest.raises(api.HrfdError, match="hrfd_tone_set_window.*-32768"):
        d.set_window(np.full(1024, -32768, dtype=np.int16))
    with pytest.raises(api.HrfdError, match="hrfd_tone_set_tones"):
        d.set_tones(steps=list(range(129)))
    with pytest.raises(api.HrfdError, match="hrfd_tone_set_threshold"):
        d.set_threshold(4, ratio_q8=1, min_energy=1)
    assert d.n_tones == 1
    power, energy, valid, best, present = d.process(np.zeros((2, 1024), dtype=np.int16))      # the handle still works
    assert (power == 0).all() and (valid == 1024).all() and (best[:, :, 0] == 0).all() and (present == 0).all()


# 9. the closed loop on the device
def test_closed_loop_transmit_receive_decode(torch_dev, oracle):
    """tests/test_tone_model.py's closed loop on the device: two WBFM stations whose audio is a DTMF digit per 64 ms block,
    a 1000 Hz pilot under the first, through Mod, Duc.transmit and Ddc.receive; Tones.process_device reads the d_pcm and
    d_n_pcm receive filled, no host copy between.  (a) the outputs equal the model's on that PCM bit for bit, (b) every
    frame that lies wholly inside a digit decodes the row, the column and the pilot's presence."""
    from tests import ddc_model as dm
    torch, dev = torch_dev
    audio = tm.loop_audio()
    streams, amps = tm.loop_streams(oracle, audio)
    R, B, FULL = dm.SEL_R, dm.SEL_BLOCKS, 262144
    mod = api.Mod(api.MOD_WBFM, 2, device=0)
    duc = api.Duc(1, 2, R, device=0)
    ddc = api.Ddc(1, 2, R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.WBFM)
    for c, f in enumerate(dm.SEL_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(amps[c], c)
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(dm.SEL_GAIN_SHIFT[c], c)
    tones = api.Tones(2, tm.LOOP_L, device=0)
    steps, groups, thresholds = tm.loop_settings(tones)
    tones.set_tones(steps=steps, groups=groups)
    for g, r in thresholds:
        tones.set_threshold(g, ratio_q8=r, min_energy=256 * tm.LOOP_L)
    F = 512 * B // tm.LOOP_L
    d_pcm_in = torch.from_numpy(np.stack(audio).astype(np.int16)).to(dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_power = torch.zeros((2, F, len(steps)), dtype=torch.int64, device=dev)
    d_energy = torch.zeros((2, F), dtype=torch.int64, device=dev)
    d_valid = torch.zeros((2, F), dtype=torch.int32, device=dev)
    d_best = torch.zeros((2, F, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((2, F, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_pcm_in.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    tones.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_power.data_ptr(), d_energy.data_ptr(),
                         d_valid.data_ptr(), d_best.data_ptr(), d_present.data_ptr())
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    n_pcm = d_n.cpu().numpy().view(np.uint32)
    assert (n_pcm == 512).all()
    got = (d_power.cpu().numpy().view(np.uint64), d_energy.cpu().numpy().view(np.uint64), d_valid.cpu().numpy().view(np.uint32),
           d_best.cpu().numpy(), d_present.cpu().numpy())
    same(got, tm.loop_model().process(pcm, n_pcm), "the bank on the PCM receive wrote")
    tm.loop_check(got[3], got[4])
