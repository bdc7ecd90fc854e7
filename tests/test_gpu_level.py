"""The level bank on the device (hrfd_level_*) against the numpy model (tests/level_model.py), tolerance 0: the weight counts
at their edges, the boundaries of every rule, attack, release and hang, a stream cut into calls with setters and resets
between, n_pcm at its edges with other bytes behind it, channel and block counts on both sides of the kernel's step, every
even residue of the input with padded strides and guard bytes around every buffer, each output alone, in place, setter
changes behind running calls, and the closed loop the bank exists for: Mod -> Duc.transmit -> Ddc.receive ->
Leveler.process_device on the buffers receive filled.  Every comparison also checks the contract's own property:
max |y| <= target on every channel that is not bypassed."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import level_model as lm
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

OUTPUTS = ("out", "gain", "peak")
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C, w=None, target=None, floor=None):
    d, m = api.Leveler(C, device=0), lm.LevelModel(C)
    if w is not None:
        d.set_weights(w)
        m.set_weights(w)
    if target is not None:
        d.set(target, floor)
        m.set(target, floor)
    return d, m


def random_weights(W, seed):
    w = np.random.default_rng(seed).integers(0, 32769, size=W)
    w[0] = 32768
    return w


_reference = {}


def reference(C, n, seed=7):
    """random int16 over the full range, one array per shape, computed once and left unchanged"""
    key = (C, n, seed)
    if key not in _reference:
        x = np.random.default_rng(seed).integers(-32768, 32768, size=(C, n), dtype=np.int16)
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def bursts(C, n, seed):
    """int16 whose amplitude changes every few frames, from silence to full scale: the gain moves both ways"""
    rng = np.random.default_rng(seed)
    frames = n // 64
    amp = rng.choice(np.array([0, 3, 40, 63, 64, 65, 700, 9000, 32768]), size=(C, frames // 3 + 1)).repeat(3, axis=1)[:, :frames]
    x = (rng.uniform(-1.0, 1.0, size=(C, frames, 64)) * amp[:, :, None]).round()
    return np.clip(x, -32768, 32767).astype(np.int16).reshape(C, n)


def bounded(m, out, what):
    """9. the property: |y| <= target wherever the channel is not bypassed"""
    peak = np.abs(np.asarray(out).astype(np.int64)).reshape(m.C, -1).max(axis=1)
    assert (peak[~m.bypass] <= m.target[~m.bypass]).all(), f"{what}: |y| above the target: {peak.tolist()} against {m.target.tolist()}"


def same(m, got, want, what):
    for name, g, w in zip(OUTPUTS, got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), f"{what}: {name} differs at {np.argwhere(g != w)[:4].tolist()}"
    if got[0] is not None:
        bounded(m, got[0], what)


def run_device(torch_dev, d, m, pcm, n_pcm, what, residue=0, pad=0, out_pad=0, outputs=OUTPUTS, stream=None, in_place=False):
    """process_device over rows at `residue` modulo 16, 1024 n_blocks + pad bytes apart; out rows at 14 - residue modulo 16,
    1024 n_blocks + out_pad apart, or the input rows themselves (in_place); gain at 4 modulo 8, peak at residue + 2; every
    buffer between guards.  The model takes the same call"""
    torch, dev = torch_dev
    pcm = np.asarray(pcm).reshape(m.C, -1)
    C, n = pcm.shape
    n_blocks = n // 512
    stride = 2 * n + pad
    out_stride = stride if in_place else 2 * n + out_pad
    src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
    for c in range(C):
        src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
    src.put(0, pcm[0])
    d_n = None if n_pcm is None else torch.from_numpy(np.ascontiguousarray(n_pcm, dtype=np.uint32).view(np.int32)).to(dev)
    want = dict(zip(OUTPUTS, m.process(pcm, n_pcm)))
    bufs = {"out": src if in_place else Guarded(torch_dev, out_stride * (C - 1) + 2 * n, 14 - residue, 16, 22),
            "gain": Guarded(torch_dev, want["gain"].nbytes, 4, 8, 23),
            "peak": Guarded(torch_dev, want["peak"].nbytes, (residue + 2) % 16, 16, 24)}
    torch.cuda.synchronize()
    d.process_device(src.ptr, stride, None if d_n is None else d_n.data_ptr(), n_blocks,
                     bufs["out"].ptr if "out" in outputs else None, out_stride, bufs["gain"].ptr if "gain" in outputs else None,
                     bufs["peak"].ptr if "peak" in outputs else None, stream)
    torch.cuda.synchronize()
    rows = None
    if "out" in outputs:
        # the rows of out as they must lie between what was there before
        rows = bufs["out"].host[bufs["out"].off:bufs["out"].off + bufs["out"].n].copy()
        for c in range(C):
            rows[c * out_stride:c * out_stride + 2 * n] = want["out"][c].reshape(-1).view(np.uint8)
        bounded(m, want["out"], what)
    if not in_place:
        src.check(None, what + ": the input")
    bufs["out"].check(rows, f"{what}: out")
    for name in ("gain", "peak"):
        bufs[name].check(want[name] if name in outputs else None, f"{what}: {name}")
    return want


# 1. the weight counts: one weight, the smallest tables, the largest
@pytest.mark.parametrize("W", [1, 2, 3, 63, 64])
def test_weight_counts(torch_dev, W):
    d, m = both(3, random_weights(W, W), 20000, 40)
    pcm = reference(3, 512 * 3)
    same(m, d.process(pcm), m.process(pcm), f"W={W}, host path")
    run_device(torch_dev, d, m, pcm, None, f"W={W}")
    run_device(torch_dev, d, m, bursts(3, 512 * 3, W), None, f"W={W}, behind a call")


# 2. the boundaries of every rule, on one channel
def test_full_scale_at_both_floors():
    x = np.zeros((1, 1024), dtype=np.int16)
    x[0, 0::2], x[0, 1::2] = -32768, 32767
    for floor, g in ((16, 4095), (32768, 4095)):
        d, m = both(1, None, 32767, floor)
        got = d.process(x)
        same(m, got, m.process(x), f"full scale, floor {floor}")
        assert (got[2] == 32768).all() and (got[1] == g).all()
        assert got[0][0, 0, 0] == -32760 and got[0][0, 0, 1] == 32759 and got[0][0, 1, 510] == -32760


def test_target_zero_and_the_largest_gain():
    d, m = both(1, None, 0, 16)
    x = reference(1, 1024)
    got = d.process(x)
    same(m, got, m.process(x), "target 0")
    assert (got[0] == 0).all() and (got[1] == 0).all() and got[2].max() > 30000
    d, m = both(1, None, 32767, 16)
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, 64:128] = 16
    x[0, 130], x[0, 200], x[0, 201] = -16, 15, -1
    got = d.process(x)
    same(m, got, m.process(x), "the largest gain")
    assert (got[1] == 8388352).all() and got[2][0].tolist() == [0, 16, 16, 15, 0, 0, 0, 0]
    assert got[0][0, 0, 64] == 32767 and got[0][0, 0, 130] == -32767 and got[0][0, 0, 200] == 30719 and got[0][0, 0, 201] == -2048


@pytest.mark.parametrize("floor", [16, 64, 32768])
def test_peaks_around_the_floor(floor):
    d, m = both(1, [32768], 32767, floor)                   # W = 1: E[f] = max(floor, p[f])
    peaks = [floor - 1, floor, min(floor + 1, 32768), floor - 1]
    x = np.zeros((1, 512), dtype=np.int16)
    for f, p in enumerate(peaks):
        x[0, 64 * f + 7] = -p                               # (-32768 where floor + 1 does not fit: |-32768| counts)
    got = d.process(x)
    same(m, got, m.process(x), f"floor {floor}")
    assert got[2][0, :4].tolist() == peaks
    assert got[1][0, :4].tolist() == [(32767 << 12) // max(floor, p) for p in peaks]


def test_both_sides_of_the_envelope_tie():
    """33 x 16384 = 16.5 x 2^15 rounds up to 17; 33 x 16383 stays below the tie and gives 16, the floor"""
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, 5] = 33
    for w1, E in ((16384, 17), (16383, 16)):
        d, m = both(1, [32768, w1], 20000, 16)
        got = d.process(x)
        same(m, got, m.process(x), f"w[1] = {w1}")
        assert got[1][0, :3].tolist() == [(20000 << 12) // 33, (20000 << 12) // E, (20000 << 12) // 16]


def test_both_sides_of_the_output_tie_for_negative_products():
    """g = 2048: -1 x 2048 + 2^11 = 0 -> 0, -3 x 2048 + 2^11 = -4096 -> -1; g = 2049: -1 -> -1, -3 -> -2 (the shift is arithmetic)"""
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, 100:104] = (-1, -3, 1, 3)
    for target, floor, g, y in ((100, 200, 2048, [0, -1, 1, 2]), (2049, 4096, 2049, [-1, -2, 1, 2])):
        d, m = both(1, None, target, floor)
        got = d.process(x)
        same(m, got, m.process(x), f"g = {g}")
        assert (got[1] == g).all() and got[0][0, 0, 100:104].tolist() == y


# 3. attack, release, a constant tone, the hang
def test_attack_release_constant_tone_and_hang():
    sign = np.where(np.arange(64) % 2 == 0, 1, -1)
    # quiet -> loud -> quiet under W = 1: the new gain at once where it falls, over the frame's ramp where it rises
    d, m = both(1, [32768], 8192, 64)
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, :128], x[0, 128:256], x[0, 256:] = np.tile(100 * sign, 2), np.tile(10000 * sign, 2), np.tile(100 * sign, 4)
    out, gain, peak = got = d.process(x)
    same(m, got, m.process(x), "steps")
    lo, hi = (8192 << 12) // 100, (8192 << 12) // 10000
    assert gain[0].tolist() == [lo, lo, hi, hi, lo, lo, lo, lo]
    assert out[0, 0, 128] == (10000 * hi + 2048) >> 12 and (np.abs(out[0, 0, 128:256]) == out[0, 0, 128]).all()       # attack: at the boundary
    ramp = np.abs(out[0, 0, 256:320].astype(np.int64))
    assert ramp[0] == (100 * (hi + ((lo - hi) >> 6)) + 2048) >> 12 and ramp[63] == (100 * lo + 2048) >> 12
    assert (np.diff(ramp) >= 0).all() and ramp[0] < ramp[31] < ramp[63]                                              # release: a ramp
    assert (np.abs(out[0, 0, 320:]) == ramp[63]).all()
    # a constant tone under the default table: one gain, and the tone itself times that gain
    d, m = both(1)
    tone = np.round(3000 * np.sin(2 * np.pi * 1000 * np.arange(1536) / 8000 + 0.3)).astype(np.int16)[None, :]
    out, gain, peak = got = d.process(tone)
    same(m, got, m.process(tone), "a constant tone")
    assert (gain == gain[0, 0]).all() and (peak == peak[0, 0]).all()
    assert (out.reshape(-1) == (tone[0].astype(np.int64) * int(gain[0, 0]) + 2048) >> 12).all()
    # the hang: five unity weights hold the gain of the last loud frame for four frames more, exactly
    d, m = both(1, [32768] * 5, 8192, 64)
    x = np.zeros((1, 1024), dtype=np.int16)
    x[0, :256] = np.tile(10000 * sign, 4)
    out, gain, peak = got = d.process(x)
    same(m, got, m.process(x), "the hang")
    assert gain[0, :8].tolist() == [hi] * 8 and (gain[0, 8:] == (8192 << 12) // 64).all()


# 4. a stream cut into calls; set_weights and set keep the peaks; reset of one channel and of all clears them
def test_call_cutting_setters_and_reset():
    C = 3
    pcm = bursts(C, 512 * 7, 41).reshape(C, 7, 512)
    n_pcm = np.random.default_rng(42).choice(np.array([0, 7, 511, 512, 600], dtype=np.uint32), size=(C, 7))
    whole, mw = both(C)
    out = whole.process(pcm, n_pcm)
    same(mw, out, mw.process(pcm, n_pcm), "seven blocks")
    for cuts in ((1, 6), (3, 4), (1,) * 7):
        parts, mp = both(C)
        got, at = [], 0
        for k in cuts:
            got.append(parts.process(pcm[:, at:at + k], n_pcm[:, at:at + k]))
            at += k
        for i, name in enumerate(OUTPUTS):
            assert (np.concatenate([g[i] for g in got], axis=1) == out[i]).all(), f"cut {cuts}: {name}"
    # the peaks outlive set_weights and set: the next call differs from a new handle's, and equals the model's
    w = random_weights(64, 43)
    for h in (whole, mw, parts):
        h.set_weights(w)
        h.set(20000, 16, 1)
    nxt = whole.process(pcm[:, :2])
    same(mw, nxt, mw.process(pcm[:, :2]), "behind set_weights and set")
    same(mw, parts.process(pcm[:, :2]), nxt, "behind set_weights and set, the cut handle")
    fresh, mf = both(C, w)
    fresh.set(20000, 16, 1)
    mf.set(20000, 16, 1)
    first = fresh.process(pcm[:, :2])
    same(mf, first, mf.process(pcm[:, :2]), "a new handle")
    assert all((nxt[1][c, :8] != first[1][c, :8]).any() for c in range(C))
    # reset of channel 1: that channel as from a new handle, the others go on
    for h in (whole, mw):
        h.reset(1)
    nxt = whole.process(pcm[:, 2:4])
    same(mw, nxt, mw.process(pcm[:, 2:4]), "behind reset(1)")
    fresh, mf = both(C, w)
    fresh.set(20000, 16, 1)
    alone = fresh.process(pcm[:, 2:4])
    assert all((nxt[i][1] == alone[i][1]).all() for i in range(3))
    assert (nxt[1][0, :8] != alone[1][0, :8]).any() and (nxt[1][2, :8] != alone[1][2, :8]).any()
    for h in (whole, mw):
        h.reset()
    nxt = whole.process(pcm[:, 2:4])
    same(mw, nxt, mw.process(pcm[:, 2:4]), "behind reset()")
    assert all((a == b).all() for a, b in zip(nxt, alone))


# 5. n_pcm at its edges: the bytes behind it are random and must not matter; the bypassed channel obeys it too
def test_n_pcm_edges(torch_dev):
    edges = np.array([0, 1, 63, 64, 65, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32)
    n_pcm = np.stack([edges, edges[::-1], np.roll(edges, 4)])
    pcm = reference(3, 512 * 9)
    d, m = both(3, None, 12000, 16)
    for h in (d, m):
        h.set_bypass(True, 1)
    want = run_device(torch_dev, d, m, pcm, n_pcm, "n_pcm edges")
    tail = run_device(torch_dev, d, m, pcm[:, :512], None, "the call behind a short last block")
    taken = np.minimum(n_pcm.astype(np.int64), 512)
    other = pcm.copy()
    for c in range(3):
        for b in range(9):
            other[c, 512 * b + int(taken[c, b]):512 * (b + 1)] ^= 0x5A5A
    d2, m2 = both(3, None, 12000, 16)
    d2.set_bypass(True, 1)
    m2.set_bypass(True, 1)
    same(m2, d2.process(other, n_pcm), [want[k] for k in OUTPUTS], "other bytes behind n_pcm")
    same(m2, d2.process(pcm[:, :512]), [tail[k] for k in OUTPUTS], "other bytes behind n_pcm, the next call")
    x = lm.masked(pcm, n_pcm)
    assert (want["out"][1] == x[1]).all() and (want["out"][0, 0] == 0).all() and want["peak"][0, 0] == 0
    assert want["peak"][0, 8] == abs(int(pcm[0, 512])) and (want["out"][0, 1, 1:] == 0).all()


# 6. sizes: k_level takes one workgroup per channel and walks its row in steps of 4 blocks: 1 block (a quarter step), 3, 4
#    and 5 (both sides of one step), 8 and 9 (both sides of two), and the most, 1024
@pytest.mark.parametrize("C", [1, 2, 5, 65])
@pytest.mark.parametrize("n_blocks", [1, 3, 4, 5, 8, 9])
def test_channel_and_block_counts(C, n_blocks):
    d, m = both(C, random_weights(64, 60 + C), 9000, 20)
    pcm = bursts(C, 512 * n_blocks, 61 + n_blocks)
    n_pcm = np.random.default_rng(C).choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C, n_blocks))
    for h in (d, m):
        h.set_bypass(True, C - 1)
    same(m, d.process(pcm, n_pcm), m.process(pcm, n_pcm), f"C={C}, {n_blocks} blocks")
    same(m, d.process(pcm), m.process(pcm), f"C={C}, {n_blocks} blocks, the second call")


def test_the_most_blocks():
    d, m = both(2)
    pcm = bursts(2, 512 * 1024, 62)
    same(m, d.process(pcm), m.process(pcm), "1024 blocks")
    same(m, d.process(pcm[:, :512]), m.process(pcm[:, :512]), "1024 blocks, the call behind")


# 7. every even residue of the input, padded strides on both sides, guard bytes around every buffer, each output alone, the
#    meter call (out == NULL), in place (residues 4 and 12 put the rows on an odd dword)
@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_addresses_strides_single_outputs_and_in_place(torch_dev, residue):
    d, m = both(3, random_weights(6 + residue, 13), 15000, 30)
    pcm = bursts(3, 512 * 5, 70)
    n_pcm = np.array([[512, 300, 512, 0, 512], [0, 512, 512, 64, 512], [512, 512, 511, 512, 1]], dtype=np.uint32)
    singles = (("out",), ("gain",), ("peak",), ("gain", "peak"))
    for i, (pad, out_pad) in enumerate(((2, 6), (6, 16), (16, 2))):
        what = f"residue {residue} pads {pad} {out_pad}"
        run_device(torch_dev, d, m, pcm, n_pcm if i == 1 else None, what, residue, pad, out_pad)
        one = singles[(residue // 2 + i) % 4]
        run_device(torch_dev, d, m, pcm, n_pcm, f"{what} {one} alone", residue, pad, out_pad, outputs=one)
        run_device(torch_dev, d, m, pcm, n_pcm if i != 1 else None, f"{what} in place", residue, pad, in_place=True)
    run_device(torch_dev, d, m, pcm, None, f"residue {residue} in place, out alone", residue, 0, in_place=True, outputs=("out",))


# 8. the settings of a call are those set before it, whatever still runs
def test_per_channel_settings():
    d, m = both(5)
    pcm = bursts(5, 2048, 80)
    for h in (d, m):
        h.set(32767, 16, 0)
        h.set(0, 32768, 1)
        h.set_bypass(True, 2)
        h.set(100, 200, 3)
    got = d.process(pcm)
    same(m, got, m.process(pcm), "five settings")
    assert (got[0][1] == 0).all() and (got[0][2] == pcm[2].reshape(4, 512)).all() and np.abs(got[0][3]).max() <= 100
    for h in (d, m):
        h.set_bypass(False)
        h.set_bypass(True, 4)
        h.set(5000, 100)
        h.set(6000, 16, 2)
    same(m, d.process(pcm), m.process(pcm), "the settings of all, then of one")
    assert m.bypass.tolist() == [False] * 4 + [True] and m.target.tolist() == [5000, 5000, 6000, 5000, 5000]


def test_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    C, n_blocks = 64, 16
    d, m = both(C)
    pcm = bursts(C, 512 * n_blocks, 81)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 7
    d_out = torch.zeros((calls, C, n_blocks, 512), dtype=torch.int16, device=dev)
    d_gain = torch.zeros((calls, C, 8 * n_blocks), dtype=torch.int32, device=dev)
    d_peak = torch.zeros((calls, C, 8 * n_blocks), dtype=torch.int16, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    rng = np.random.default_rng(82)
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        if i in (1, 4):
            w = random_weights(64 if i == 1 else 4, 83 + i)
            d.set_weights(w)
            m.set_weights(w)
        if i in (2, 5):
            d.reset(i)
            m.reset(i)
        if i == 6:
            d.reset()
            m.reset()
        c, target, floor = int(rng.integers(0, C)), int(rng.integers(0, 32768)), int(rng.integers(16, 32769))
        for h in (d, m):
            h.set(target, floor, c)
            h.set_bypass(i % 2 == 1, (c + 1) % C)
        # four calls on one stream, then one on a second stream directly behind them, then the first stream again
        st = streams[1 if i == 4 else 0]
        d.process_device(d_pcm.data_ptr(), 1024 * n_blocks, None, n_blocks, d_out[i].data_ptr(), 0, d_gain[i].data_ptr(),
                         d_peak[i].data_ptr(), st.cuda_stream)
        want.append(m.process(pcm))
        bounded(m, want[-1][0], f"call {i}")
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        got = (d_out[i].cpu().numpy(), d_gain[i].cpu().numpy().view(np.uint32), d_peak[i].cpu().numpy().view(np.uint16))
        for name, g, w in zip(OUTPUTS, got, want[i]):
            assert (g == w).all(), f"call {i}: {name} differs at {np.argwhere(g != w)[:4].tolist()}"


# what needs a handle to be refused
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    d = api.Leveler(4, device=0)
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=dev)
    p = buf.data_ptr()
    with pytest.raises(api.HrfdError, match="hrfd_level_set.*channel 4"):
        d.set(100, 100, 4)
    with pytest.raises(api.HrfdError, match="hrfd_level_set_bypass.*channel 4"):
        d.set_bypass(True, 4)
    with pytest.raises(api.HrfdError, match="hrfd_level_reset.*channel 4"):
        d.reset(4)
    with pytest.raises(api.HrfdError, match="hrfd_level_set_weights.*w\\[0\\] must be 32768"):
        d.set_weights([32767, 5])
    # out behind the first input row but inside the fourth
    with pytest.raises(api.HrfdError, match="hrfd_level_process_device.*overlaps"):
        d.process_device(p, 1024, None, 1, p + 3 * 1024 + 1022, 1024, None, None)
    with pytest.raises(api.HrfdError, match="hrfd_level_process_device.*overlaps"):
        d.process_device(p, 1024, None, 1, p, 1026, None, None)
    with pytest.raises(api.HrfdError, match="hrfd_level_process_device.*no output"):
        d.process_device(p, 1024, None, 1, None, 1024, None, None)
    x = np.arange(-1024, 1024, dtype=np.int16).reshape(4, 512)
    out, gain, peak = d.process(x)                          # the handle still works, with its defaults
    m = lm.LevelModel(4)
    same(m, (out, gain, peak), m.process(x), "defaults")
    assert gain[3, 7] == (8192 << 12) // 1023 and peak[0, 0] == 1024


# 10. the closed loop on the device
LOOP_BLOCKS = 4
LOOP_AMPS = (32768, 2048)                                  # the DUC's amplitudes: the second station 16 times (24 dB) weaker
LOOP_OFFSETS = (-200_000.0, 200_000.0)
LOOP_TARGET, LOOP_FLOOR = 8192, 16


def loop_audio():
    """[2][4 x 512] int16: two notes whose loudness swells and fades, so that the envelope rises onto new peaks"""
    t = np.arange(LOOP_BLOCKS * 512) / 8000.0
    swell = 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t)
    return [np.round(20000 * swell * np.sin(2 * np.pi * f * t)).astype(np.int16) for f in (440.0, 587.0)]


def test_closed_loop_transmit_receive_level(torch_dev):
    """Two AM stations on one capture, the second 16 times weaker in amplitude: Mod (AM), Duc.transmit, Ddc.receive (AM), then
    Leveler.process_device on the d_pcm and d_n_pcm receive filled, no host copy between.  (a) out, gain and peak equal the
    model's on the PCM receive wrote.  (b) On every frame where the model has E[f] == p[f] >= floor the frame's output peak is
    at least target - 9: there g > (target << 12) / p - 1, so the sample that carries the peak comes out above
    target - p / 4096 - 1/2 once it is under the frame's own gain (which it is wherever the gain does not rise into the
    frame: a frame that sets a new peak while the release still ramps is the one case the argument leaves open, and the
    assertion is made for it all the same).  (c) Each station has such a frame by the model alone, and
    the two stations, 24 dB apart going in, come out with the same loudest sample to within those 9."""
    torch, dev = torch_dev
    R, B, FULL = 4, LOOP_BLOCKS, 262144
    mod = api.Mod(api.MOD_AM, 2, device=0)
    duc = api.Duc(1, 2, R, device=0)
    ddc = api.Ddc(1, 2, R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.AM)
    for c, f in enumerate(LOOP_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(LOOP_AMPS[c], c)
        ddc.tune(c, 0, f)
    bank, model = both(2, None, LOOP_TARGET, LOOP_FLOOR)
    d_pcm_in = torch.from_numpy(np.stack(loop_audio())).to(dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_out = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_gain = torch.zeros((2, 8 * B), dtype=torch.int32, device=dev)
    d_peak = torch.zeros((2, 8 * B), dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_pcm_in.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    bank.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_out.data_ptr(), 0, d_gain.data_ptr(), d_peak.data_ptr())
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    n_pcm = d_n.cpu().numpy().view(np.uint32)
    p, E, g = model.envelope(pcm, n_pcm)
    got = (d_out.cpu().numpy(), d_gain.cpu().numpy().view(np.uint32), d_peak.cpu().numpy().view(np.uint16))
    same(model, got, model.process(pcm, n_pcm), "the bank on the PCM receive wrote")
    out_peak = np.abs(got[0].astype(np.int64)).reshape(2, 8 * B, 64).max(axis=2)
    on_peak = (E == p) & (p >= LOOP_FLOOR)
    print("peaks in", p.max(axis=1).tolist(), "frames on their own peak", on_peak.sum(axis=1).tolist(), "their output peaks",
          [out_peak[c][on_peak[c]].tolist() for c in range(2)])
    assert on_peak.any(axis=1).all(), f"no frame with E == p >= floor: input peaks {p.max(axis=1).tolist()}"
    assert p[0].max() >= 8 * p[1].max() > 0, f"the stations are not apart going in: {p.max(axis=1).tolist()}"
    assert (out_peak[on_peak] >= LOOP_TARGET - 9).all(), (out_peak[on_peak].tolist(), np.argwhere(on_peak).tolist())
    assert abs(int(out_peak[0].max()) - int(out_peak[1].max())) <= 9
