"""The DUC bank at its edges, on the device against the model (tests/duc_model.py), with proof from the model's stage
values that every edge was reached: both saturations of both filters, every mixer table index, the output saturation
and its clip counter, S at its bound with the most channels on one capture, setters between queued asynchronous calls,
the largest call and a counter past 2^32."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import duc_model as um
from tests.test_gpu_duc import amp_both, both, check_call, filter_both, lcg_channels, shift_both, tune_both

pytestmark = pytest.mark.gpu
LARGEST = 1 << 25


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def runs(C, n_bytes):
    """runs of (127, 127) and (-128, -128) samples, 64 samples each"""
    x = np.empty((C, n_bytes // 2, 2), dtype=np.int8)
    sgn = (np.arange(n_bytes // 2) // 64) % 2 == 0
    x[:, sgn] = 127
    x[:, ~sgn] = -128
    return x.reshape(C, n_bytes)


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_stage_b_saturates_both_ways(R):
    d, m = both(1, 2, R)
    filter_both(d, m, 1, np.array([32767, 32767], dtype=np.int16))
    shift_both(d, m, 0, 9)
    tune_both(d, m, 1, 0, um.duc_step(300_000, R))
    ch = runs(2, 2048)
    got = d.process(ch, 2048)
    want, st = m.process(ch, 2048, stages=True)
    assert (got == want).all()
    q = (st["accB"] + (1 << 14)) >> 15
    assert q.max() > 32767 and q.min() < -32768, "both saturations of stage B reached"


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_stage_a_saturates_both_ways(R):
    d, m = both(1, 1, R)
    filter_both(d, m, 1, np.zeros(0, dtype=np.int16))
    filter_both(d, m, 0, np.full(2 * R, 32767, dtype=np.int16))
    tune_both(d, m, 0, 0, um.duc_step(-250_000, R))
    ch = runs(1, 2048)
    got = d.process(ch, 2048)
    want, st = m.process(ch, 2048, stages=True)
    assert (got == want).all()
    q = (st["accA"] + (1 << 14)) >> 15
    assert q.max() > 32767 and q.min() < -32768, "both saturations of stage A reached"


@pytest.mark.parametrize("R", [1, 8])
def test_every_mixer_index_through_a_transparent_path(R):
    """stage B and stage A bypassed, A = 128 (a = x), Q = 0, shift 0: the output is the mixer's y itself"""
    d, m = both(1, 1, R)
    filter_both(d, m, 0, np.zeros(0, dtype=np.int16))
    filter_both(d, m, 1, np.zeros(0, dtype=np.int16))
    amp_both(d, m, 0, 128)
    shift_both(d, m, 0, 0)
    step = (1 << 20) + 3
    tune_both(d, m, 0, 0, step)
    M = 4200 // R + 1
    x = np.empty((1, M, 2), dtype=np.int8)
    x[0, :, 0], x[0, :, 1] = 127, 0
    x[0, ::3, 0] = -77
    x = x.reshape(1, -1)
    theta0 = m.phase(0)
    got = d.process(x, 2 * M)
    want, st = m.process(x, 2 * M, stages=True)
    assert (got == want).all()
    assert not (np.abs(st["S"]) > 127).any() and d.clips(0) == 0, "transparent: nothing saturates"
    theta = (theta0 + np.arange(R * M, dtype=np.int64) * step) & um.MASK32
    assert np.unique(((theta + (1 << 19)) >> 20) & 4095).size == 4096, "every table index reached"


@pytest.mark.parametrize("R", [2, 8])
def test_output_saturates_both_ways_and_clips_are_counted(R):
    W, C = 2, 6
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, c % W, um.duc_step(-500_000 + 170_000 * c, R))
    shift_both(d, m, 0, 7)
    shift_both(d, m, 1, 10)
    for call in range(3):
        ch = lcg_channels(C, 3000, 400 + call)
        got, (want, st) = d.process(ch, 3000), m.process(ch, 3000, stages=True)
        assert (got == want).all()
        y = (st["S"][0] + (1 << 6)) >> 7
        assert y.max() > 127 and y.min() < -128, "both output saturations reached"
    for w in range(W):
        assert d.clips(w) == int(m.clips[w]) > 0, w
    d.reset()
    assert d.clips(0) == 0


def test_sum_at_its_bound_with_the_most_channels_on_one_capture():
    """32768 channels at full scale on one capture, all at 45 degrees: S near 32768 x 46341 (int32 holds it)"""
    R, C, M = 1, 32768, 6
    d, m = both(2, C, R)
    filter_both(d, m, 0, np.zeros(0, dtype=np.int16))
    filter_both(d, m, 1, np.zeros(0, dtype=np.int16))
    shift_both(d, m, 1, 24)
    for c in range(C):
        d.set_step(c, 1, 1 << 29)
    m.capture[:] = 1
    m.step[:] = 1 << 29
    x = np.empty((C, M, 2), dtype=np.int8)
    x[..., 0], x[..., 1] = -128, 127
    x = x.reshape(C, -1)
    got = d.process(x, 2 * M)
    # every channel is the same: the model runs one and scales the sum
    one = um.DucModel(2, 1, R)
    one.set_filter(0, []), one.set_filter(1, []), one.set_output_shift(1, 24), one.set_tuning(0, 1, 1 << 29)
    _, st = one.process(x[:1], 2 * M, stages=True)
    S = st["S"][1] * C
    assert np.abs(S).max() > 32768 * 46000 and np.abs(S).max() < 2 ** 31
    want = np.clip((S + (1 << 23)) >> 24, -128, 127).T.reshape(-1).astype(np.int8)
    assert (got[1] == want).all() and not got[0].any()


def test_stage_a_bound_is_per_branch():
    t = np.full(64, 8000, dtype=np.int16)                          # 512 000 in total, 64 000 per branch at R = 8
    api.Duc(1, 1, 8, device=0).set_filter(0, t)
    with pytest.raises(api.HrfdError):
        api.Duc(1, 1, 4, device=0).set_filter(0, t)


def test_setters_between_asynchronous_calls(torch_dev):
    torch, dev = torch_dev
    R, W, C = 4, 2, 5
    d, m = both(W, C, R)
    rng = np.random.default_rng(5)
    sizes = [int(2 * rng.integers(1, 3000)) for _ in range(20)]
    chs = [lcg_channels(C, ib, 600 + i) for i, ib in enumerate(sizes)]
    dins = [torch.from_numpy(x).to(dev) for x in chs]
    douts = [torch.zeros((W, R * ib), dtype=torch.int8, device=dev) for ib in sizes]
    torch.cuda.synchronize()
    ops = []
    for i, ib in enumerate(sizes):
        k = i % 5
        c = int(rng.integers(0, C))
        if k == 0:
            op = ("tune", c, int(rng.integers(0, W)), int(rng.integers(0, 2 ** 32)))
            d.set_step(*op[1:])
        elif k == 1:
            op = ("amp", c, int(rng.integers(0, 32769)))
            d.set_amplitude(op[2], c)
        elif k == 2:
            op = ("shift", int(rng.integers(0, W)), int(rng.integers(4, 14)))
            d.set_output_shift(op[2], op[1])
        elif k == 3:
            op = ("filt", 1, rng.integers(-300, 300, size=int(rng.integers(0, 200))).astype(np.int16))
            d.set_filter(1, op[2])
        else:
            op = ("filt", 0, rng.integers(-3000, 3000, size=int(rng.integers(0, 64))).astype(np.int16))
            d.set_filter(0, op[2])
        ops.append(op)
        d.process_device(dins[i].data_ptr(), ib, ib, douts[i].data_ptr(), R * ib)
    torch.cuda.synchronize()
    for i, ib in enumerate(sizes):
        op = ops[i]
        if op[0] == "tune":
            m.set_tuning(*op[1:])
        elif op[0] == "amp":
            m.set_amplitude(op[1], op[2])
        elif op[0] == "shift":
            m.set_output_shift(op[1], op[2])
        else:
            m.set_filter(op[1], op[2])
        assert (douts[i].cpu().numpy() == m.process(chs[i], ib)).all(), i


def test_largest_call(torch_dev):
    """2^25 bytes per channel at R = 8 (256 MiB per capture): the model checks the first and the last 3000 samples"""
    torch, dev = torch_dev
    R, W, C = 8, 1, 2
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, 0, um.duc_step(-300_000 + 600_000 * c, R))
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    din = torch.randint(-128, 128, (C, LARGEST), dtype=torch.int8, device=dev, generator=gen)
    dout = torch.zeros((W, R * LARGEST), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    d.process_device(din.data_ptr(), LARGEST, LARGEST, dout.data_ptr(), R * LARGEST)
    torch.cuda.synchronize()
    K = 6000
    head = din[:, :K].cpu().numpy()
    assert (dout[:, :R * K].cpu().numpy() == m.process(head, K)).all()
    tail_in = din[:, LARGEST - K:].cpu().numpy()
    hist = din[:, LARGEST - K - 2 * um.H:LARGEST - K].cpu().numpy()
    m.seek(R * (LARGEST - K) // 2, hist)
    assert (dout[:, R * (LARGEST - K):].cpu().numpy() == m.process(tail_in, K)).all()


def test_counter_past_2_pow_32(torch_dev):
    torch, dev = torch_dev
    R, W, C = 8, 1, 2
    d, m = both(W, C, R)
    for c in range(C):
        tune_both(d, m, c, 0, 0x9E3779B9 + 12345 * c)
    dz = torch.zeros((C, LARGEST), dtype=torch.int8, device=dev)
    dout = torch.zeros((W, R * LARGEST), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    calls = (1 << 32) // (R * LARGEST // 2) + 1                    # 33 calls of 2^27 wideband samples
    for _ in range(calls):
        d.process_device(dz.data_ptr(), LARGEST, LARGEST, dout.data_ptr(), R * LARGEST)
    torch.cuda.synchronize()
    N = calls * R * LARGEST // 2
    assert N > 1 << 32
    m.seek(N, np.zeros((C, 2 * um.H), dtype=np.int8))
    assert d.phase(1) == m.phase(1)
    ch = lcg_channels(C, 4000, 9)
    check_call(d, m, ch, 4000, "past 2^32")
