"""The DDC bank on the device at its edges, bit for bit against the numpy model (tests/ddc_model.py): saturation inside
both FIR stages (with proof from the model that it was reached), the mixer through a transparent path over every table
index, every tap count, setters between asynchronous calls, the largest call the ABI takes and a counter past 2^32.
Tile remainders, addresses and hrfd_ddc_receive beyond one call are cases of tests/test_gpu_ddc.py."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import ddc_model as dm
from tests import ddc_reference as dr
from tests.test_gpu_ddc import both, lcg_captures, tune_both

pytestmark = pytest.mark.gpu

MASK32 = dm.MASK32
LARGEST = 1 << 25                                   # the largest out_bytes of one call
TILE = 1024                                         # outputs per workgroup of k_ddc today (the checks do not rely on it)


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def set_filter_both(d, m, stage, taps):
    t = np.asarray(taps, dtype=np.int16)
    d.set_filter(stage, t)
    m.set_filter(stage, t)


def prime_phases(d, m, R, thetas, final_steps, capture=0):
    """one call of one output (R input samples) with steps that leave channel c at theta(N) = thetas[c], then the
    final steps; thetas[c] must be a multiple of R"""
    for c, th in enumerate(thetas):
        assert th % R == 0
        tune_both(d, m, c, capture, (th // R) & MASK32)
    z = np.zeros((m.W, 2 * R), dtype=np.int8)
    assert (d.process(z, 2) == m.process(z, 2)).all()
    for c, s in enumerate(final_steps):
        tune_both(d, m, c, capture, s)
        assert d.phase(c) == m.phase(c) == thetas[c]


# ---- 3. value ranges
RAILS = ((127, 127), (-128, -128), (127, -128), (-128, 127))


def rail_runs(R, M, run):
    """[1, R * 2M] int8: runs of `run` input samples at each of the four rail pairs in turn"""
    n = R * M
    x = np.empty((n, 2), dtype=np.int8)
    for j in range(0, n, run):
        x[j:j + run] = RAILS[(j // run) % 4]
    return x.reshape(1, -1)


@pytest.mark.parametrize("stage_b", ["default", "max_positive", "max_negative"])
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_saturation_inside_both_stages(R, sign, stage_b):
    """Stage A: sum |hA| = 65535, every tap of one sign; inputs on both rails, seen at theta = 45, 135, 225 and 315
    degrees, where |y| = 128 sqrt(2) 32767 / 256 ~ 23 170 lies on one axis: |a| reaches ~46 000, so sat16 clips both
    ways (the model's sums prove it), at R = 1 too.  A kernel that wrapped a to int16 would differ.

    Stage B ("max_*"): taps [-32768, -32767] and [32767, 32767, 1] under runs of saturated a16 make sum h a reach
    +65535 * 32768 and -65535 * 32768, the largest magnitude the contract allows (sum |h| <= 65535), in the int32
    accumulator with its rounding constant.  Any |b| >= 32767 gives 127 / -128 for every g, so stage B's sat16 cannot be
    told from no clamp at the output: what this catches is a wrap (to int16, or of the accumulator)."""
    W, C, M = 1, 4, 3 * TILE + 77
    d, m = both(W, C, R)
    set_filter_both(d, m, 0, sign * np.full(3, 21845))
    hb = {"default": dm.default_taps(R)[1], "max_positive": [-32768, -32767], "max_negative": [32767, 32767, 1]}[stage_b]
    set_filter_both(d, m, 1, hb)
    prime_phases(d, m, R, [(2 * c + 1) << 29 for c in range(C)], [0] * C)
    for c in range(C):
        d.set_gain_shift(c % 8, c)
        m.set_gain_shift(c, c % 8)
    cap = rail_runs(R, M, 300 * R)
    got = d.process(cap, 2 * M)
    want, st = m.process(cap, 2 * M, stages=True)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    acc_a = st["accA"]
    assert ((acc_a + (1 << 14)) >> 15).max() > 32767 and ((acc_a + (1 << 14)) >> 15).min() < -32768, \
        "stage A must clip both ways"
    assert (st["a"] == 32767).any() and (st["a"] == -32768).any()
    acc_b = st["accB"]
    if stage_b == "max_positive":
        assert acc_b.max() == 65535 * 32768 and acc_b.min() < -(1 << 31) + 65536 * 1024
    elif stage_b == "max_negative":
        assert acc_b.min() == -65535 * 32768 and acc_b.max() > (1 << 31) - 65536 * 1024
    assert (got == 127).any() and (got == -128).any()


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_mixer_through_a_transparent_path(R):
    """T_A = 0, stage B = [-32768], g = 7: b = -y exactly and out = sat8(-y); with |I|, |Q| <= 1 the mixer's output is
    read at the output.  Channel 0 samples theta at k 2^20 - 2^19 - R, just below every rounding boundary, channel 1 at
    every boundary exactly (both at the decimated samples m R + R - 1, R step = 2^20 per output): together all 4096
    table indices on both sides of every boundary, the wrap from 4095 to 0 included.  Channel 2 runs at a random step.
    Besides the model, the outputs must equal sat8(-y) from the contract's mixer formula (tests/ddc_reference.py)."""
    rng = np.random.default_rng(40 + R)
    W, C, M = 1, 3, 4096 + 300
    d, m = both(W, C, R)
    set_filter_both(d, m, 0, [])
    set_filter_both(d, m, 1, [-32768])
    for c in range(C):
        d.set_gain_shift(7, c)
        m.set_gain_shift(c, 7)
    sigma = (1 << 20) // R                                   # R sigma = 2^20: one table step per output
    off = (R - 1) * sigma                                     # theta(m R + R - 1) = theta(N) + off + m 2^20
    b0 = (1 << 32) - (1 << 19)                                # the boundary between index 4095 and 0
    targets = [(b0 - R - off) & MASK32, (b0 - off) & MASK32, 0]
    rand_step = int(rng.integers(0, 2 ** 32)) | 1
    prime_phases(d, m, R, targets, [sigma, sigma, rand_step])
    N0 = m.N
    cap = rng.integers(-1, 2, size=(W, 2 * R * M)).astype(np.int8)
    got = d.process(cap, 2 * M)
    want = m.process(cap, 2 * M)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    x = cap.reshape(R * M, 2).astype(np.int64)
    j = np.arange(M) * R + R - 1                              # the decimated samples of the call
    seen_below, seen_at = set(), set()
    for c, step in enumerate([sigma, sigma, rand_step]):
        theta = (targets[c] + (j.astype(np.int64) * step)) & MASK32
        yi, yq = dr.mixer(x[j, 0], x[j, 1], theta)
        out = got[c].reshape(M, 2).astype(np.int64)
        assert (out[:, 0] == np.clip(-yi, -128, 127)).all() and (out[:, 1] == np.clip(-yq, -128, 127)).all(), c
        k = ((theta + (1 << 19)) >> 20) & 4095
        frac = (theta + (1 << 19)) & ((1 << 20) - 1)           # distance above the boundary below index k
        if c < 2:
            seen_below |= set(((k[frac >= (1 << 20) - R] + 1) & 4095).tolist())   # just below boundary k + 1
            seen_at |= set(k[frac == 0].tolist())
    assert seen_below == set(range(4096)) and seen_at == set(range(4096)), (len(seen_below), len(seen_at))
    assert N0 == R


# ---- 4. every tap count
def sweep_taps(rng, n, limit=60000):
    if n == 0:
        return np.zeros(0, dtype=np.int16)
    h = rng.integers(-32768, 32768, size=n).astype(np.int64)
    s = int(np.abs(h).sum())
    if s > limit:
        h = np.sign(h) * ((np.abs(h) * limit) // s)
    return h.astype(np.int16)


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_every_tap_count(R):
    """T_A = 0..64 with the default stage B, then T_B = 0..256 with the default stage A (random asymmetric taps), one
    stream of calls of ~1 500 outputs (a partial second tile) each"""
    rng = np.random.default_rng(60 + R)
    W, C = 1, 2
    d, m = both(W, C, R)
    tune_both(d, m, 0, 0, dm.ddc_step(170_000, R))
    tune_both(d, m, 1, 0, int(rng.integers(0, 2 ** 32)))
    a0 = dm.default_taps(R)[0]
    cases = [(0, ta) for ta in range(65)] + [(1, tb) for tb in range(257)]
    for i, (stage, n) in enumerate(cases):
        if i == 65:
            set_filter_both(d, m, 0, a0)
        set_filter_both(d, m, stage, sweep_taps(rng, n))
        ob = 2 * (1400 + (i * 37) % 300)
        cap = (lcg_captures(W, R * ob, 1000 * R + i).astype(np.int16) // 3).astype(np.int8)
        got, want = d.process(cap, ob), m.process(cap, ob)
        assert (got == want).all(), f"R={R} stage {'AB'[stage]} with {n} taps: {np.argwhere(got != want)[:5]}"


# ---- 5. the host side under asynchronous use
def test_setters_between_asynchronous_calls(torch_dev):
    """~20 process_device calls with no host synchronisation, alternating between a caller's stream and the handle's
    own, each into its own buffer, a different setter change before each; the first call is large, so that the host
    runs ahead of the device while the setters' uploads queue behind it.  get_phase after every call, the outputs
    after one synchronisation at the end, against the model run in the same order."""
    torch, dev = torch_dev
    rng = np.random.default_rng(77)
    R, W, C = 8, 2, 8
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, int(rng.integers(0, 2 ** 32)))
    big = LARGEST                                             # ~4.5 ms on the device: the host's calls queue behind it
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    dbig = torch.randint(-128, 128, (W, R * big), dtype=torch.int8, device=dev, generator=gen)
    dbig_out = torch.zeros((C, big), dtype=torch.int8, device=dev)
    changes = ["retune", "capture", "gain_one", "gain_all", "filter_a", "filter_b", "bypass", "reset"] * 3
    changes = changes[:19]
    sizes = [2 * int(rng.integers(200, 3000)) for _ in changes]
    caps = [lcg_captures(W, R * ob, 300 + k) for k, ob in enumerate(sizes)]
    dcaps = [torch.from_numpy(c).to(dev) for c in caps]
    douts = [torch.zeros((C, ob), dtype=torch.int8, device=dev) for ob in sizes]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    # the model's side of every call, in order; the host-side calls of the handle queue without a wait
    record = []
    d.process_device(dbig.data_ptr(), R * big, big, dbig_out.data_ptr(), big, side.cuda_stream)
    record.append(("big", None))
    phases = [[d.phase(c) for c in range(C)]]
    for k, ch in enumerate(changes):
        c = k % C
        if ch == "retune":
            st = int(rng.integers(0, 2 ** 32))
            d.set_step(c, int(m.capture[c]), st)
            record.append(("set_tuning", (c, int(m.capture[c]), st)))
        elif ch == "capture":
            d.set_step(c, (int(m.capture[c]) + 1) % W, int(m.step[c]))
            record.append(("set_tuning", (c, (int(m.capture[c]) + 1) % W, int(m.step[c]))))
        elif ch == "gain_one":
            g = int(rng.integers(0, 8))
            d.set_gain_shift(g, c)
            record.append(("gain", (c, g)))
        elif ch == "gain_all":
            g = int(rng.integers(0, 8))
            d.set_gain_shift(g, api.ALL)
            record.append(("gain_all", g))
        elif ch == "filter_a":
            t = sweep_taps(rng, int(rng.integers(1, 65)))
            d.set_filter(0, t)
            record.append(("filter", (0, t)))
        elif ch == "filter_b":
            t = sweep_taps(rng, int(rng.integers(1, 257)))
            d.set_filter(1, t)
            record.append(("filter", (1, t)))
        elif ch == "bypass":
            d.set_filter((k // 8) % 2, np.zeros(0, dtype=np.int16))              # stage A, then stage B
            record.append(("filter", ((k // 8) % 2, np.zeros(0, dtype=np.int16))))
        else:
            d.reset()
            record.append(("reset", None))
        stream = side.cuda_stream if k % 2 == 1 else None
        d.process_device(dcaps[k].data_ptr(), R * sizes[k], sizes[k], douts[k].data_ptr(), sizes[k], stream)
        record.append(("call", k))
        # mirror the model up to here to compare get_phase (the model's own state runs ahead of the device's, which
        # is the point: get_phase never waits)
        phases.append([d.phase(cc) for cc in range(C)])
    torch.cuda.synchronize()
    # replay on the model; the big call through seek windows (first and last tile) and the H samples in front of the
    # next call
    H = m.H
    n_phase = 0
    for kind, arg in record:
        if kind == "big":
            for o0 in (0, big // 2 - TILE):                     # in outputs
                if o0:
                    m.seek(R * o0, dbig[:, 2 * (R * o0 - H):2 * R * o0].cpu().numpy())
                want = m.process(dbig[:, 2 * R * o0:2 * R * (o0 + TILE)].cpu().numpy(), 2 * TILE)
                got = dbig_out[:, 2 * o0:2 * (o0 + TILE)].cpu().numpy()
                assert (got == want).all(), f"big call, outputs {o0}..{o0 + TILE}"
            m.seek(R * big // 2, dbig[:, R * big - 2 * H:].cpu().numpy())
            assert [m.phase(c) for c in range(C)] == phases[0]
            n_phase = 1
        elif kind == "set_tuning":
            m.set_tuning(*arg)
        elif kind == "gain":
            m.set_gain_shift(*arg)
        elif kind == "gain_all":
            for c in range(C):
                m.set_gain_shift(c, arg)
        elif kind == "filter":
            m.set_filter(*arg)
        elif kind == "reset":
            m.reset()
        else:
            want = m.process(caps[arg], sizes[arg])
            got = douts[arg].cpu().numpy()
            assert (got == want).all(), f"call {arg} after {changes[arg]}: {np.argwhere(got != want)[:5]}"
            assert [m.phase(c) for c in range(C)] == phases[n_phase], f"get_phase after call {arg}"
            n_phase += 1


# ---- 6. the largest call and a long run
@pytest.mark.parametrize("R", [1, 8])
def test_largest_call(torch_dev, R):
    """out_bytes = 2^25 (2^24 outputs per channel): the first tile, a window across a tile boundary in the middle and
    the last tile against the model moved there with seek (the H samples in front of the window as its history)"""
    torch, dev = torch_dev
    W, C = 2, 3
    d, m = both(W, C, R)
    rng = np.random.default_rng(90 + R)
    for c in range(C):
        tune_both(d, m, c, (c + 1) % W, int(rng.integers(0, 2 ** 32)))
        d.set_gain_shift(c, c)
        m.set_gain_shift(c, c)
    M = LARGEST // 2
    gen = torch.Generator(device=dev)
    gen.manual_seed(R)
    dcap = torch.randint(-128, 128, (W, R * LARGEST), dtype=torch.int8, device=dev, generator=gen)
    dout = torch.zeros((C, LARGEST), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    d.process_device(dcap.data_ptr(), R * LARGEST, LARGEST, dout.data_ptr(), LARGEST, None)
    torch.cuda.synchronize()
    H = m.H
    for o0, n in ((0, TILE), (M // 2 - 700, 1400), (M - TILE, TILE)):
        if o0 > 0:
            m.seek(R * o0, dcap[:, 2 * (R * o0 - H):2 * R * o0].cpu().numpy())
        win = dcap[:, 2 * R * o0:2 * R * (o0 + n)].cpu().numpy()
        want = m.process(win, 2 * n)
        got = dout[:, 2 * o0:2 * (o0 + n)].cpu().numpy()
        assert (got == want).all(), f"R={R} outputs {o0}..{o0 + n}: {np.argwhere(got != want)[:5]}"
    for c in range(C):
        assert d.phase(c) == m.phase(c)


def test_counter_past_2_pow_32(torch_dev):
    """R = 8: 33 calls of zero captures at the largest size take N past 2^32; then a retune and two LCG calls against the
    model moved there with seek (zero history).  theta uses (n - N_ref) mod 2^32 today: a guard against a rewrite"""
    torch, dev = torch_dev
    R, W, C = 8, 1, 2
    d, m = both(W, C, R)
    steps = [dm.ddc_step(123_456.7, R), 0x9E3779B9]
    for c in range(C):
        tune_both(d, m, c, 0, steps[c])
    dz = torch.zeros((W, R * LARGEST), dtype=torch.int8, device=dev)
    dout = torch.zeros((C, LARGEST), dtype=torch.int8, device=dev)
    n_calls = 33
    torch.cuda.synchronize()
    for _ in range(n_calls):
        d.process_device(dz.data_ptr(), R * LARGEST, LARGEST, dout.data_ptr(), LARGEST, None)
    torch.cuda.synchronize()
    assert not dout.any().item()
    N = n_calls * R * LARGEST // 2
    assert N > 1 << 32
    m.seek(N, np.zeros((W, m.H, 2), dtype=np.int64))
    for c in range(C):
        assert d.phase(c) == m.phase(c), f"phase ch{c} at N = {N}"
    tune_both(d, m, 1, 0, dm.ddc_step(-321_000, R))
    for k, ob in enumerate((6000, 2 * TILE + 6)):
        cap = lcg_captures(W, R * ob, 500 + k)
        got, want = d.process(cap, ob), m.process(cap, ob)
        assert (got == want).all(), f"call {k} past 2^32: {np.argwhere(got != want)[:5]}"
        for c in range(C):
            assert d.phase(c) == m.phase(c)
