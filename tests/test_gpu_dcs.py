"""The DCS bank on the device (hrfd_dcs_*) against the numpy model (tests/dcs_model.py), bit for bit: channel and block counts on
both sides of the kernel's tile of 4 blocks and of the 3.6 blocks a word and the filter reach back, the tap and list counts at
their edges with full, sparse and empty groups, n_pcm at its edges with other bytes behind it, padded strides and every even
residue with guard bytes around every buffer, each output alone, a stream cut into calls with resets and setters between,
ties in best, the chain Dcs -> Audio.gate_device -> Audio.process_device without a host copy, and the closed loop the bank
exists for: Mod -> Duc.transmit -> Ddc.receive -> Dcs.process_device on the buffers receive filled."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import dcs_model as dm
from tests.test_dcs_model import distinct_codes, random_taps
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

OUTPUTS = ("hits", "best", "present")
ALL = 0xFFFFFFFF
SENT = [(0o754, False), (0o023, True), (0o411, False), (0o132, True)]       # what the channels of `signals` send, in turn


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C, taps=None, codes=None, inv=None, grp=None):
    d, m = api.Dcs(C, device=0), dm.DcsModel(C)
    for b in (d, m):
        if taps is not None:
            b.set_taps(taps)
        if codes is not None:
            b.set_codes(codes, inv, grp)
    return d, m


def listed(K, groups=4):
    """K entries with the codes of SENT in front; entry k in group k % groups"""
    codes, inv = distinct_codes(K, SENT)
    return codes, inv, [k % groups for k in range(K)]


_signals = {}


def signals(C, n, seed=3):
    """int16 [C, n], one array per shape, computed once and left unchanged: channel c sends SENT[c % 4] at an amplitude and
    under a noise of its own, from a start of its own; every fifth channel is full-scale noise, channel 7 silence"""
    key = (C, n, seed)
    if key not in _signals:
        rng = np.random.default_rng(seed)
        x = np.zeros((C, n), dtype=np.int64)
        for c in range(C):
            code, inv = SENT[c % 4]
            x[c] = dm.levels(code, n, int(rng.integers(300, 6000)), int(rng.integers(0, 5000)), inv) + dm.white(rng, n, float(rng.integers(0, 700)))
            if c % 5 == 4:
                x[c] = rng.integers(-32768, 32768, size=n)
            if c == 7:
                x[c] = 0
        x = dm.to_pcm(x)
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


def same(got, want, what):
    for name, g, w in zip(OUTPUTS, got, want):
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), f"{what}: {name} differs at {np.argwhere(g != w)[:4].tolist()}"


def run_device(torch_dev, d, m, pcm, n_pcm, what, residue=0, pad=0, outputs=OUTPUTS, stream=None):
    """process_device over rows at `residue` modulo 16, 1024 n_blocks + pad bytes apart; hits at residue + 2 modulo 16 (2 modulo
    4 for some: the halfword path), best and present at odd addresses; every buffer between guards.  The model takes the same
    call"""
    torch, dev = torch_dev
    pcm = np.asarray(pcm).reshape(m.C, -1)
    C, n = pcm.shape
    n_blocks = n // 512
    stride = 2 * n + pad
    src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
    for c in range(C):
        src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
    src.put(0, pcm[0])
    d_n = None if n_pcm is None else torch.from_numpy(np.ascontiguousarray(n_pcm, dtype=np.uint32).view(np.int32)).to(dev)
    want = dict(zip(OUTPUTS, m.process(pcm, n_pcm)))
    bufs = {"hits": Guarded(torch_dev, max(want["hits"].nbytes, 2), (residue + 2) % 16, 16, 22),
            "best": Guarded(torch_dev, want["best"].nbytes, 1, 4, 23), "present": Guarded(torch_dev, want["present"].nbytes, 3, 4, 24)}
    torch.cuda.synchronize()
    d.process_device(src.ptr, stride, None if d_n is None else d_n.data_ptr(), n_blocks,
                     *[bufs[name].ptr if name in outputs else None for name in OUTPUTS], stream)
    torch.cuda.synchronize()
    src.check(None, what + ": the input")
    for name in OUTPUTS:
        filled = name in outputs and want[name].size > 0
        bufs[name].check(want[name] if filled else None, f"{what}: {name}")
    return want


LOW = api.dcs_lowpass_taps()


# 1. channel and block counts: one workgroup and many, both sides of a tile (4 blocks) and of the history's reach (3.6 blocks)
@pytest.mark.parametrize("n_blocks", [1, 3, 4, 5, 16])
@pytest.mark.parametrize("C", [1, 3, 65])
def test_channels_and_blocks(torch_dev, C, n_blocks):
    d, m = both(C, LOW, *listed(6))
    pcm = signals(C, 512 * n_blocks)
    want = m.process(pcm)
    same(d.process(pcm), want, f"C={C}, {n_blocks} blocks, host path")
    if n_blocks >= 5:
        assert want[2][0, 4:, 0].all() and want[1][0, 4, 0] == 0          # the comparison is not one of zeros
    run_device(torch_dev, d, m, signals(C, 512 * n_blocks, 4), None, f"C={C}, {n_blocks} blocks, behind a call", residue=2 * (C % 8))


# 2. tap and list counts at their edges; entries in all four groups, and with one group empty
@pytest.mark.parametrize("K,groups", [(1, 4), (2, 4), (63, 4), (65, 3), (128, 4), (128, 3)])
@pytest.mark.parametrize("T", [1, 2, 255, 512])
def test_taps_and_list_sizes(torch_dev, T, K, groups):
    taps = {1: [16384], 2: [-20000, 30000], 255: LOW}.get(T, random_taps(np.random.default_rng(T), T))
    d, m = both(3, taps, *listed(K, groups))
    for b in (d, m):
        b.set_min_hits(ALL, 300)
        b.set_min_hits(1, 1)
    pcm = signals(3, 512 * 5)
    want = run_device(torch_dev, d, m, pcm, None, f"T={T}, K={K}, {groups} groups", pad=6)
    if groups == 3:
        assert (want["best"][:, :, 3] == dm.NO_BEST).all() and not want["present"][:, :, 3].any()
    if T in (1, 255):
        assert want["hits"][0, 4, 0] > 400
    same(d.process(pcm), m.process(pcm), f"T={T}, K={K}: a second call, host path")


def test_an_empty_list(torch_dev):
    d, m = both(2, LOW)
    assert d.n_codes() == 0
    pcm = signals(2, 512 * 2)
    hits, best, present = d.process(pcm)
    same((hits, best, present), m.process(pcm), "K=0, host path")
    assert hits.shape == (2, 2, 0) and (best == dm.NO_BEST).all() and not present.any()
    run_device(torch_dev, d, m, pcm, None, "K=0", outputs=("best", "present"))
    d.set_codes(*listed(3))
    m.set_codes(*listed(3))
    assert d.n_codes() == 3
    same(d.process(pcm), m.process(pcm), "a list behind none: the state of the calls before counts")


# 3. n_pcm at its edges, other bytes behind the limit
def test_n_pcm_limits(torch_dev):
    C, B = 5, 9
    d, m = both(C, LOW, *listed(4))
    rng = np.random.default_rng(11)
    n_pcm = rng.choice(np.array([0, 1, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32), size=(C, B))
    n_pcm[0] = 512
    n_pcm[1, ::2], n_pcm[1, 1::2] = 511, 1
    n_pcm[2] = 0
    want = run_device(torch_dev, d, m, signals(C, 512 * B), n_pcm, "n_pcm mixed", residue=6, pad=2)
    assert want["hits"][2].max() == 0 and want["present"][0, 4:, 0].all()
    same(d.process(signals(C, 512 * B, 5), n_pcm), m.process(signals(C, 512 * B, 5), n_pcm), "n_pcm mixed, host path")


# 4. every even residue of the input, padded strides that are odd multiples of 2
@pytest.mark.parametrize("residue,pad", [(0, 0), (2, 2), (4, 6), (6, 1026), (8, 14), (10, 2), (12, 30), (14, 18)])
def test_residues_and_strides(torch_dev, residue, pad):
    d, m = both(4, LOW, *listed(7 + residue // 2))          # odd and even list lengths: rows of hits at 0 and 2 modulo 4
    run_device(torch_dev, d, m, signals(4, 512 * 6), None, f"residue {residue}, pad {pad}", residue=residue, pad=pad)


# 5. each output alone, in pairs, all together
@pytest.mark.parametrize("outputs", [("hits",), ("best",), ("present",), ("hits", "present"), ("best", "present"), OUTPUTS])
def test_each_output_alone(torch_dev, outputs):
    d, m = both(3, LOW, *listed(5))
    run_device(torch_dev, d, m, signals(3, 512 * 5), None, f"outputs {outputs}", outputs=outputs)
    run_device(torch_dev, d, m, signals(3, 512 * 5, 4), None, f"outputs {outputs}, the state behind such a call", residue=4)


# 6. a stream cut into calls
def test_six_single_blocks_against_one_call_of_six(torch_dev):
    C, B = 3, 6
    pcm = signals(C, 512 * B).reshape(C, B, 512)
    d1, m = both(C, LOW, *listed(5))
    whole = d1.process(pcm)
    same(whole, m.process(pcm), "one call of six")
    d2, _ = both(C, LOW, *listed(5))
    parts = [d2.process(pcm[:, b:b + 1]) for b in range(B)]                # each reaches three calls back for its bits
    same([np.concatenate([p[i] for p in parts], axis=1) for i in range(3)], whole, "six calls of one")
    d3, _ = both(C, LOW, *listed(5))
    parts = [d3.process(pcm[:, :5]), d3.process(pcm[:, 5:])]               # a whole tile and a block, then one block
    same([np.concatenate([p[i] for p in parts], axis=1) for i in range(3)], whole, "5 + 1")
    assert whole[2][0, 4:, 0].all()


# 7. reset of one channel mid-stream; 8. set_codes keeps the state, set_taps clears it
def test_reset_and_setters_mid_stream(torch_dev):
    C = 3
    d, m = both(C, LOW, *listed(5))
    pcm = signals(C, 512 * 15).reshape(C, 15, 512)
    same(d.process(pcm[:, :5]), m.process(pcm[:, :5]), "the first call")
    for b in (d, m):
        b.reset(1)
    got = d.process(pcm[:, 5:8])
    same(got, m.process(pcm[:, 5:8]), "behind reset(1)")
    assert got[2][0, :, 0].all() and got[2][2, :, 2].all() and not got[2][1, :2].any()          # the others go on; channel 1 starts anew
    codes, inv, grp = listed(9, 2)
    for b in (d, m):
        b.set_codes(codes[::-1], inv[::-1], grp)
    got = d.process(pcm[:, 8:9])
    same(got, m.process(pcm[:, 8:9]), "behind set_codes")
    assert got[2][0, 0, 0] == 1 and got[1][0, 0, 0] == 8                    # found at once under its new index: the state was kept
    for b in (d, m):
        b.set_taps(LOW[:-2])
    got = d.process(pcm[:, 9:12])
    same(got, m.process(pcm[:, 9:12]), "behind set_taps")
    assert not got[2][:, :2].any()                                          # every channel starts anew
    for b in (d, m):
        b.reset()
        b.set_min_hits(0, 512)
    same(d.process(pcm[:, 12:]), m.process(pcm[:, 12:]), "behind reset(ALL) and min_hits 512")


# 9. ties in best: entries with 0 hits, and a row that switches codes inside a block so that two entries draw
def test_ties_in_best(torch_dev):
    codes, inv = distinct_codes(6, SENT)
    grp = [0, 0, 1, 1, 1, 2]
    d, m = both(2, [16384], codes, inv, grp)
    for b in (d, m):
        b.set_min_hits(ALL, 1)
    n = 512 * 12
    x = np.stack([dm.levels(0o754, n, 1000), np.zeros(n, dtype=np.int64)])
    got = d.process(dm.to_pcm(x))
    same(got, m.process(dm.to_pcm(x)), "0 hits in a group")
    assert (got[1][:, :, 1] == 2).all() and (got[1][:, :, 2] == 5).all() and (got[1][1, :, 0] == 0).all() and not got[2][:, :, 1:].any()
    # D754 up to sample s of block 6, D023I from there on: over a sweep of s both orders of the two counts occur, and the
    # model's argmax decides a draw; the channels cut at neighbouring samples
    C = 24
    d, m = both(C, [16384], codes, inv, grp)
    x = np.zeros((C, n), dtype=np.int64)
    for c in range(C):
        s = 512 * 6 + 20 * c
        x[c, :s], x[c, s:] = dm.levels(0o754, s, 1000), dm.levels(0o023, n - s, 1000, s, True)
    got = d.process(dm.to_pcm(x))
    same(got, m.process(dm.to_pcm(x)), "a switch of codes inside a block")
    h = got[0].astype(np.int64)
    assert (h[:, :, 0] > h[:, :, 1]).any() and (h[:, :, 1] > h[:, :, 0]).any() and ((h[:, :, 0] == h[:, :, 1]) & (got[1][:, :, 0] == 0)).any()


def test_refusals_that_need_a_handle():
    d = api.Dcs(2, device=0)
    for call, word in ((lambda: d.reset(2), "channel 2"), (lambda: d.set_min_hits(4, 100), "group 4"), (lambda: d.set_min_hits(0, 513), "min_hits 513"),
                       (lambda: d.set_codes([0o023, 0o766]), "aliases"), (lambda: d.set_taps([32767, 32767, 2]), "sum |h|")):
        with pytest.raises(api.HrfdError, match=word):
            call()
    d.set_codes([0o023])
    hits, best, present = d.process(dm.to_pcm(dm.levels(0o023, 512 * 5, 1000)).reshape(1, -1).repeat(2, axis=0))
    assert present[:, 4, 0].all()                           # the handle works on


# 10. Dcs.process_device -> Audio.gate_device -> Audio.process_device, no host copy in between
def test_dcs_opens_the_audio_gate_on_the_device(torch_dev):
    from tests.audio_model import AudioModel
    torch, dev = torch_dev
    C, B = 4, 10
    codes, inv, grp = listed(4, 1)
    pcm = signals(C, 512 * B)
    d, m = both(C, LOW, codes, inv, grp)
    a, am = api.Audio(C, 1, device=0), AudioModel(C, 1)
    voice = api.audio_highpass_taps(255)
    for b in (a, am):
        b.set_taps(voice)
        b.set_bus(0, list(range(C)), [1024] * C)
        for c in range(C):
            b.set_want(0 if c == 3 else c, c)               # channel 3 waits for a code it is not sent
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    d_best = torch.zeros((C, B, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((C, B, 4), dtype=torch.uint8, device=dev)
    d_open = torch.zeros((C, B), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    d_mix = torch.zeros((1, B, 512), dtype=torch.int16, device=dev)
    d_clips = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    d.process_device(d_pcm.data_ptr(), 1024 * B, None, B, None, d_best.data_ptr(), d_present.data_ptr(), s.cuda_stream)
    a.gate_device(d_best.data_ptr(), d_present.data_ptr(), 512, 0, B, d_open.data_ptr(), s.cuda_stream)
    a.process_device(d_pcm.data_ptr(), 1024 * B, None, d_open.data_ptr(), B, d_out.data_ptr(), 0, d_mix.data_ptr(), d_clips.data_ptr(),
                     s.cuda_stream)
    torch.cuda.synchronize()
    hits, best, present = m.process(pcm)
    opened = am.gate(best, present, 512, 0)
    out, mix, clips = am.process(pcm, None, opened)
    assert (d_best.cpu().numpy() == best).all() and (d_present.cpu().numpy() == present).all()
    assert (d_open.cpu().numpy() == opened).all() and (d_out.cpu().numpy() == out).all() and (d_mix.cpu().numpy() == mix).all()
    assert opened[:3, 4:].all() and not opened[3].any() and not opened[:, :2].any()


# 11. the closed loop
def test_closed_loop_transmit_receive_decode(torch_dev, oracle):
    """tests/test_dcs_model.py's closed loop on the device: two WBFM stations whose audio is a DCS code under a 1 kHz tone,
    through Mod, Duc.transmit and Ddc.receive; Dcs.process_device reads the d_pcm and d_n_pcm receive filled, no host copy
    between.  (a) the outputs equal the model's on that PCM bit for bit, (b) from block 4 on every block has its station's code
    present (the CPU oracle's chain showed it: the receive chain passes 134.4 bit/s NRZ)."""
    from tests import ddc_model as ddm
    from tests import tone_model as tm
    torch, dev = torch_dev
    audio = dm.loop_audio()
    streams, amps = tm.loop_streams(oracle, audio)
    R, B, FULL = ddm.SEL_R, ddm.SEL_BLOCKS, 262144
    assert B == dm.LOOP_BLOCKS
    mod = api.Mod(api.MOD_WBFM, 2, device=0)
    duc = api.Duc(1, 2, R, device=0)
    ddc = api.Ddc(1, 2, R, device=0)
    rx = api.Rx(2, device=0)
    rx.set_mode(api.WBFM)
    for c, f in enumerate(ddm.SEL_OFFSETS):
        duc.tune(c, 0, f)
        duc.set_amplitude(amps[c], c)
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(ddm.SEL_GAIN_SHIFT[c], c)
    model = dm.loop_model()
    dcs = api.Dcs(2, device=0)
    dcs.set_taps(model.taps)
    dcs.set_codes([c for c, _ in dm.LOOP_CODES], [i for _, i in dm.LOOP_CODES])
    d_pcm_in = torch.from_numpy(np.stack(audio).astype(np.int16)).to(dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_hits = torch.zeros((2, B, 2), dtype=torch.int16, device=dev)
    d_best = torch.zeros((2, B, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((2, B, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_pcm_in.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    dcs.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_hits.data_ptr(), d_best.data_ptr(), d_present.data_ptr())
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    n_pcm = d_n.cpu().numpy().view(np.uint32)
    assert (n_pcm == 512).all()
    got = (d_hits.cpu().numpy().view(np.uint16), d_best.cpu().numpy(), d_present.cpu().numpy())
    same(got, model.process(pcm, n_pcm), "the bank on the PCM receive wrote")
    print("hits of each station's own code per block:", got[0][0, :, 0].tolist(), got[0][1, :, 1].tolist())
    dm.loop_check(*got)
