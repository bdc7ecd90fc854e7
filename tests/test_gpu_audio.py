"""The audio bank on the device (hrfd_audio_*) against the numpy model (tests/audio_model.py), tolerance 0: the tap counts
where the packing and the steps of the filter change, the rounding and saturation boundaries of the filter and of the buses,
a batch cut into calls, reset and set_taps, n_pcm at its edges with other bytes behind it, every gate transition and the ramp,
the tone squelch, the bus lists at their limits, channel and block counts with partial workgroups, every even residue of the
input with padded strides and guard bytes around every buffer, each output alone, setter changes behind running calls, and the
closed loop the bank exists for: Mod -> Duc.transmit -> Ddc.receive -> Tones.process_device -> Audio.gate_device ->
Audio.process_device on the buffers receive filled."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import audio_model as am
from tests import tone_model as tm
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

OUTPUTS = ("out", "mix", "clips")
ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C, M=1, taps=None, buses=()):
    d, m = api.Audio(C, M, device=0), am.AudioModel(C, M)
    if taps is not None:
        d.set_taps(taps)
        m.set_taps(taps)
    for i, (ch, g) in enumerate(buses):
        d.set_bus(i, ch, g)
        m.set_bus(i, ch, g)
    return d, m


def random_taps(T, seed):
    """T int16 taps with sum |h| <= 65535, most of the bound used"""
    top = min(32767, 65535 // T)
    return np.random.default_rng(seed).integers(-top, top + 1, size=T).astype(np.int16)


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


def run_device(torch_dev, d, m, pcm, n_pcm, open_, what, residue=0, pad=0, out_pad=0, outputs=OUTPUTS, stream=None):
    """process_device over rows at `residue` modulo 16, 1024 n_blocks + pad bytes apart, out rows at the same residue
    1024 n_blocks + out_pad apart, mix at residue + 2, every buffer between guards; the model takes the same call"""
    torch, dev = torch_dev
    C, n = pcm.shape
    n_blocks = n // 512
    stride, out_stride = 2 * n + pad, 2 * n + out_pad
    src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
    for c in range(C):
        src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
    src.put(0, pcm[0])
    d_n = None if n_pcm is None else torch.from_numpy(np.ascontiguousarray(n_pcm, dtype=np.uint32).view(np.int32)).to(dev)
    d_o = None if open_ is None else torch.from_numpy(np.ascontiguousarray(open_, dtype=np.uint8)).to(dev)
    want = dict(zip(OUTPUTS, m.process(pcm, n_pcm, open_)))
    bufs = {"out": Guarded(torch_dev, out_stride * (C - 1) + 2 * n, residue, 16, 22),
            "mix": Guarded(torch_dev, want["mix"].nbytes, (residue + 2) % 16, 16, 23),
            "clips": Guarded(torch_dev, want["clips"].nbytes, 4, 8, 24)}
    torch.cuda.synchronize()
    d.process_device(src.ptr, stride, None if d_n is None else d_n.data_ptr(), None if d_o is None else d_o.data_ptr(), n_blocks,
                     bufs["out"].ptr if "out" in outputs else None, out_stride, bufs["mix"].ptr if "mix" in outputs else None,
                     bufs["clips"].ptr if "clips" in outputs else None, stream)
    torch.cuda.synchronize()
    src.check(None, what + ": the input")
    rows = None
    if "out" in outputs:
        # the rows of out as they must lie between what was there before
        rows = bufs["out"].host[bufs["out"].off:bufs["out"].off + bufs["out"].n].copy()
        for c in range(C):
            rows[c * out_stride:c * out_stride + 2 * n] = want["out"][c].reshape(-1).view(np.uint8)
    bufs["out"].check(rows, f"{what}: out")
    for name in ("mix", "clips"):
        bufs[name].check(want[name] if name in outputs else None, f"{what}: {name}")
    return want


# 1. the tap counts: one tap, both parities, whole and partial steps of 8 packed dwords, the most
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512])
def test_tap_counts(torch_dev, T):
    taps = random_taps(T, T)
    d, m = both(3, 1, taps, [([0, 1, 2], [4096, -2000, 1500])])
    pcm = reference(3, 512 * 3)
    same(d.process(pcm), m.process(pcm), f"T={T}, host path")
    d.reset()
    m.reset()
    run_device(torch_dev, d, m, pcm, None, None, f"T={T}")
    run_device(torch_dev, d, m, pcm, None, None, f"T={T}, behind a call")


# 2. the filter's rounding and saturation boundaries, and the largest accumulators the tap check allows
def test_rounding_and_saturation_boundaries():
    d, m = both(1, 1, [16384, 1])
    # acc = 16384 x[n] + x[n-1]: (acc + 2^13) >> 14 = x[n] + ((x[n-1] + 2^13) >> 14)
    # (behind sample 63: a new handle's first block ramps up from a shut gate)
    x = np.zeros((1, 512), dtype=np.int16)
    x[0, 110:112] = (8191, 32767)                          # 32767
    x[0, 120:122] = (8192, 32767)                          # 32768 -> 32767
    x[0, 130:132] = (-8192, -32768)                        # -32768
    x[0, 140:142] = (-8193, -32768)                        # -32769 -> -32768
    x[0, 150:152] = (-8193, 5)                             # 4: the shift is arithmetic
    got, want = d.process(x), m.process(x)
    same(got, want, "boundaries")
    assert [int(got[0][0, 0, i]) for i in (111, 121, 131, 141, 151)] == [32767, 32767, -32768, -32768, 4]
    for taps, level, y in (([-32768, -32767], -32768, 32767), ([32767, 32767, 1], -32768, -32768),
                           ([-128] * 511 + [-127], -32768, 32767), ([128] * 511 + [127], -32768, -32768),
                           ([128, -128] * 255 + [128, -127], None, None)):
        d.set_taps(taps)
        m.set_taps(taps)
        if level is None:                                  # the signs of the input follow the taps': every product positive at odd n
            x = np.where(np.arange(1024) % 2 == 1, 32767, -32768).astype(np.int16)[None, :]
        else:
            x = np.full((1, 1024), level, dtype=np.int16)
        got = d.process(x)
        same(got, m.process(x), f"taps {taps[:3]}..")
        if y is not None:
            assert (got[0][0, 1] == y).all()               # the second block: sum |h| |x| = 65535 * 32768 at every sample


# 3. a batch cut into calls; reset of one channel; set_taps clears history and gate
@pytest.mark.parametrize("T", [2, 512])
def test_call_cutting_reset_and_set_taps(T):
    C = 3
    taps = random_taps(T, 30 + T)
    buses = [([0, 1, 2, 1], [4096, 3000, -3000, 77])]
    pcm = reference(C, 512 * 6).reshape(C, 6, 512)
    rng = np.random.default_rng(31)
    n_pcm = rng.choice(np.array([0, 7, 511, 512, 600], dtype=np.uint32), size=(C, 6))
    open_ = rng.integers(0, 2, size=(C, 6), dtype=np.uint8)
    open_[:, 5] = 1                                        # prev = 1 behind the batch: reset and set_taps have something to clear
    whole, mw = both(C, 1, taps, buses)
    parts, mp = both(C, 1, taps, buses)
    out = whole.process(pcm, n_pcm, open_)
    same(out, mw.process(pcm, n_pcm, open_), f"T={T}: six blocks")
    cut = [parts.process(pcm[:, a:b], n_pcm[:, a:b], open_[:, a:b]) for a, b in ((0, 1), (1, 3), (3, 6))]
    assert (np.concatenate([c[0] for c in cut], axis=1) == out[0]).all()
    assert (np.concatenate([c[1] for c in cut], axis=1) == out[1]).all()
    assert (sum(c[2].astype(np.int64) for c in cut) == out[2]).all()
    # reset of channel 1: the others go on as if nothing had happened
    for d, m in ((whole, mw), (parts, mp)):
        d.reset(1)
        m.reset(1)
    nxt = whole.process(pcm[:, :2], None, open_[:, :2])
    same(nxt, mw.process(pcm[:, :2], None, open_[:, :2]), f"T={T}: behind reset(1)")
    same(parts.process(pcm[:, :2], None, open_[:, :2]), nxt, f"T={T}: behind reset(1), the cut handle")
    fresh, mf = both(C, 1, taps, buses)
    first = fresh.process(pcm[:, :2], None, open_[:, :2])
    assert (nxt[0][1] == first[0][1]).all()                # channel 1 as from a new handle
    if T > 2:
        assert (nxt[0][0, 0, :8] != first[0][0, 0, :8]).any() and (nxt[0][2, 0, :8] != first[0][2, 0, :8]).any()
    # set_taps, even with the same taps: every channel as from a new handle
    whole.set_taps(taps)
    mw.set_taps(taps)
    again = whole.process(pcm[:, :2], None, open_[:, :2])
    same(again, mw.process(pcm[:, :2], None, open_[:, :2]), f"T={T}: behind set_taps")
    same(again, first, f"T={T}: behind set_taps, against a new handle")


# 4. n_pcm at its edges: the bytes behind it are random and must not matter, in their own block and, through the history, in
#    the next (a short block in front of a full one) and in the next call
def test_n_pcm_edges(torch_dev):
    edges = np.array([0, 1, 2, 255, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32)
    n_pcm = np.stack([edges, edges[::-1], np.roll(edges, 3)])
    taps = random_taps(512, 41)
    buses = [([0, 1, 2], [4096, 4096, 4096])]
    d, m = both(3, 1, taps, buses)
    pcm = reference(3, 512 * 8)
    want = run_device(torch_dev, d, m, pcm, n_pcm, None, "n_pcm edges")
    tail = run_device(torch_dev, d, m, pcm[:, :512], None, None, "the call behind a short last block")
    taken = np.minimum(n_pcm.astype(np.int64), 512)
    other = pcm.copy()
    for c in range(3):
        for b in range(8):
            other[c, 512 * b + int(taken[c, b]):512 * (b + 1)] ^= 0x5A5A
    d2, _ = both(3, 1, taps, buses)
    same(d2.process(other, n_pcm), [want[k] for k in OUTPUTS], "other bytes behind n_pcm")
    same(d2.process(pcm[:, :512]), [tail[k] for k in OUTPUTS], "other bytes behind n_pcm, the next call")
    # a squelched block is silent once the filter has run out of the block before it
    d3, m3 = both(3, 1, [16384])
    got = d3.process(pcm, n_pcm)
    same(got, m3.process(pcm, n_pcm), "identity")
    z = got[0]
    assert (z[0, 0] == 0).all() and (z[0, 1, 0] == pcm[0, 512]) and (z[0, 1, 1:] == 0).all() and (z[0, 5] == pcm[0, 2560:3072]).all()


# 5. the four gate transitions inside a call and across a call boundary, the ramp, open values other than 0 and 1
def test_gate_transitions_and_ramp(torch_dev):
    d, m = both(2, 1, None, [([0], [4096])])
    level = np.stack([np.full(512 * 5, 32767, dtype=np.int16), np.full(512 * 5, -32768, dtype=np.int16)])
    calls = [np.array([[0, 1, 1, 0, 0], [0, 2, 255, 0, 0]], dtype=np.uint8),      # 00 (from create) 01 11 10 00
             np.array([[1, 1, 0, 0, 128], [7, 1, 0, 0, 1]], dtype=np.uint8),      # 01 across the boundary, .. ends open
             np.array([[1, 0, 1, 0, 0], [1, 0, 1, 0, 0]], dtype=np.uint8),        # 11 across the boundary, .. ends shut
             np.array([[0, 0, 0, 0, 1], [0, 0, 0, 0, 1]], dtype=np.uint8),        # 00 across the boundary, .. ends open
             np.array([[0, 1, 1, 1, 1], [0, 1, 1, 1, 1]], dtype=np.uint8)]        # 10 across the boundary
    outs = [run_device(torch_dev, d, m, level, None, op, f"gate call {i}")["out"] for i, op in enumerate(calls)]
    z = outs[0]
    assert (z[:, 0] == 0).all() and (z[:, 4] == 0).all()
    assert [int(z[0, 1, n]) for n in (0, 62, 63, 64, 511)] == [512, 32255, 32767, 32767, 32767]       # opens
    assert [int(z[1, 1, n]) for n in (0, 62, 63, 64, 511)] == [-512, -32256, -32768, -32768, -32768]
    assert (z[0, 2] == 32767).all() and (z[1, 2] == -32768).all()
    assert [int(z[0, 3, n]) for n in (0, 62, 63, 64, 511)] == [32255, 512, 0, 0, 0]                   # shuts
    assert [int(z[1, 3, n]) for n in (0, 62, 63, 64, 511)] == [-32256, -512, 0, 0, 0]
    assert int(outs[1][0, 0, 0]) == 512 and int(outs[1][1, 0, 63]) == -32768                          # 01 across calls
    assert (outs[2][0, 0] == 32767).all() and int(outs[2][0, 1, 0]) == 32255                          # 11 across calls
    assert (outs[3][:, 0] == 0).all()                                                                 # 00 across calls
    assert int(outs[4][0, 0, 0]) == 32255 and int(outs[4][1, 0, 62]) == -512 and (outs[4][:, 0, 63:] == 0).all()      # 10 across calls
    # NULL = all open: the first block ramps up from the handle's prev after a reset
    d.reset()
    m.reset()
    z = run_device(torch_dev, d, m, level[:, :1024], None, None, "no gate behind a reset")["out"]
    assert int(z[0, 0, 0]) == 512 and (z[0, 1] == 32767).all()


# 6. the tone squelch
@pytest.mark.parametrize("L", [128, 512, 4096])
def test_gate_device(torch_dev, L):
    torch, dev = torch_dev
    C, n_blocks = 5, 16
    F = 512 * n_blocks // L
    d, m = both(C)
    rng = np.random.default_rng(L)
    best = rng.choice(np.array([0, 9, 127, 255], dtype=np.uint8), size=(C, F, 4))
    present = rng.choice(np.array([0, 0, 1, 200], dtype=np.uint8), size=(C, F, 4))
    d_best, d_present = torch.from_numpy(best).to(dev), torch.from_numpy(present).to(dev)
    for wants in ([am.NO_TONE] * C, [9] * C, [am.ANY_TONE] * C, [0, 9, 127, am.ANY_TONE, am.NO_TONE]):
        for c, w in enumerate(wants):
            d.set_want(w, c)
            m.set_want(w, c)
        for group in range(4):
            want = m.gate(best, present, L, group)
            buf = Guarded(torch_dev, C * n_blocks, 1, 8, 61)
            d.gate_device(d_best.data_ptr(), d_present.data_ptr(), L, group, n_blocks, buf.ptr)
            torch.cuda.synchronize()
            buf.check(want, f"L={L} wants {wants} group {group}")
            assert (d.gate(best, present, L, group) == want).all()
        if wants[0] == am.NO_TONE:
            assert (want == 1).all()
    d.set_want(255 - 1, ALL)                               # ANY: a present verdict whose best is 255 cannot exist, but matches
    m.set_want(am.ANY_TONE)
    assert (d.gate(best, present, L, 0) == m.gate(best, present, L, 0)).all()


# 7. the buses
def bus_lists(C, M, seed):
    """lists of 0, 1, 2 (a duplicate), 3 and 4096 entries with gains of +-32767 and 0 among them; a channel on several buses"""
    rng = np.random.default_rng(seed)
    lists = [([], []), ([C - 1], [-32767]), ([0, 0], [32767, 32767]), ([1, 0, 1], [0, -4096, 4095]),
             (rng.integers(0, C, size=4096), rng.choice(np.array([-32767, -300, 0, 1, 200, 32767]), size=4096))]
    while len(lists) < M:
        n = int(rng.integers(1, 6))
        lists.append((rng.integers(0, C, size=n), rng.integers(-32767, 32768, size=n)))
    order = rng.permutation(len(lists)) if M >= 5 else np.arange(len(lists))
    return [lists[i] for i in order][:M]


@pytest.mark.parametrize("M", [1, 2, 64])
def test_buses(torch_dev, M):
    C = 5
    lists = bus_lists(C, max(M, 5), M)
    for first in range(0, 5 if M < 5 else 1, M):           # M = 1, 2: the five special lists in turn
        buses = (lists[first:first + M] + lists[:M])[:M]
        d, m = both(C, M, [9000, -3000, 500], buses)
        pcm = reference(C, 1024)
        want = run_device(torch_dev, d, m, pcm, None, None, f"M={M} lists from {first}", residue=2, pad=2, out_pad=6)
        for i, (ch, g) in enumerate(buses):
            if len(ch) == 0:
                assert (want["mix"][i] == 0).all() and want["clips"][i] == 0
        # clearing a bus and replacing another
        d.set_bus(M - 1)
        m.set_bus(M - 1)
        d.set_bus(0, [2, 3], [-32767, 32767])
        m.set_bus(0, [2, 3], [-32767, 32767])
        run_device(torch_dev, d, m, pcm, None, None, f"M={M} lists from {first}, lists replaced", outputs=("mix", "clips"))


def test_bus_rounding_and_clips():
    # the identity filter, all open: z = x; s = 4096 z0 + z1, (s + 2^11) >> 12 = z0 + ((z1 + 2^11) >> 12)
    d, m = both(2, 3, None, [([0, 1], [4096, 1]), ([1], [1]), ([0] * 4096, [32767] * 4096)])
    # (behind sample 63: a new handle's first block ramps up from a shut gate)
    x = np.zeros((2, 512), dtype=np.int16)
    x[:, 110] = (32767, 2047)                              # 32767
    x[:, 120] = (32767, 2048)                              # 32768: clips
    x[:, 130] = (-32768, -2048)                            # -32768
    x[:, 140] = (-32768, -2049)                            # -32769: clips
    x[:, 150] = (0, -2049)                                 # -1, and -1 on bus 1
    got = d.process(x)
    same(got, m.process(x), "bus boundaries")
    out, mix, clips = got
    assert [int(mix[0, 0, i]) for i in (110, 120, 130, 140, 150)] == [32767, 32767, -32768, -32768, -1]
    assert int(mix[1, 0, 150]) == -1 and int(mix[1, 0, 110]) == 0
    assert clips.tolist() == [2, 0, 4]                     # bus 2: 4096 x 32767 x z0 clips at the four full-scale samples
    # the largest sum: 4096 entries of 32767 over -32768
    x[:] = -32768
    got = d.process(x)
    same(got, m.process(x), "the largest sums")
    assert (got[1][2] == -32768).all() and got[2][2] == 512
    # clips are written, not accumulated
    x[:] = 0
    assert d.process(x)[2].tolist() == [0, 0, 0]


# 8. sizes: partial last workgroups over the channels and over the runs of four blocks
@pytest.mark.parametrize("C", [1, 2, 255, 257])
def test_channel_counts(C):
    d, m = both(C, 2, random_taps(33, C), [(list(range(C)), [100] * C), ([C - 1, 0], [4096, -4096])])
    pcm = reference(C, 512)
    rng = np.random.default_rng(C)
    n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C, 1))
    open_ = rng.integers(0, 2, size=(C, 1), dtype=np.uint8)
    same(d.process(pcm, n_pcm, open_), m.process(pcm, n_pcm, open_), f"C={C}")
    same(d.process(pcm), m.process(pcm), f"C={C}, second call")


@pytest.mark.parametrize("n_blocks", [1, 2, 1024])
def test_block_counts(n_blocks):
    d, m = both(1, 1, random_taps(512, 81), [([0], [5000])])
    pcm = reference(1, 512 * n_blocks, seed=8)
    rng = np.random.default_rng(n_blocks)
    n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(1, n_blocks))
    open_ = rng.integers(0, 2, size=(1, n_blocks), dtype=np.uint8)
    same(d.process(pcm, n_pcm, open_), m.process(pcm, n_pcm, open_), f"{n_blocks} blocks")
    same(d.process(pcm[:, :512]), m.process(pcm[:, :512]), f"{n_blocks} blocks, the call behind")


@pytest.mark.parametrize("n_blocks", [3, 4, 5, 8, 9])
def test_runs_of_four_blocks(n_blocks):
    d, m = both(2, 1, random_taps(511, 82), [([0, 1], [4096, 4096])])
    pcm = reference(2, 512 * n_blocks, seed=9)
    same(d.process(pcm), m.process(pcm), f"{n_blocks} blocks")


# 9. every even residue of the input, padded strides on both sides, guard bytes around every buffer, each output alone
@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_addresses_strides_and_single_outputs(torch_dev, residue):
    d, m = both(3, 2, random_taps(6 + residue, 13), [([0, 1, 2], [4096, 4096, -4096]), ([2], [32767])])
    pcm = reference(3, 1024)
    n_pcm = np.array([[512, 300], [0, 512], [512, 512]], dtype=np.uint32)
    open_ = np.array([[1, 0], [1, 1], [0, 1]], dtype=np.uint8)
    singles = (("out",), ("mix",), ("mix", "clips"))
    for i, (pad, out_pad) in enumerate(((2, 6), (6, 16), (16, 2))):
        run_device(torch_dev, d, m, pcm, n_pcm if i == 1 else None, open_ if i != 1 else None, f"residue {residue} pads {pad} {out_pad}",
                   residue, pad, out_pad)
        one = singles[(residue // 2 + i) % 3]
        run_device(torch_dev, d, m, pcm, n_pcm, open_, f"residue {residue} pads {pad} {out_pad} {one} alone", residue, pad, out_pad,
                   outputs=one)


# 10. the settings of a call are those set before it, whatever still runs
def test_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    C, M, n_blocks = 64, 3, 16
    d, m = both(C, M)
    pcm = reference(C, 512 * n_blocks)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 7
    rng = np.random.default_rng(16)
    opens = rng.integers(0, 2, size=(calls, C, n_blocks), dtype=np.uint8)
    d_open = torch.from_numpy(opens).to(dev)
    d_out = torch.zeros((calls, C, n_blocks, 512), dtype=torch.int16, device=dev)
    d_mix = torch.zeros((calls, M, n_blocks, 512), dtype=torch.int16, device=dev)
    d_clips = torch.zeros((calls, M), dtype=torch.int32, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        if i in (1, 4):
            taps = random_taps(511 if i == 1 else 4, 17 + i)
            d.set_taps(taps)
            m.set_taps(taps)
        if i in (2, 5):
            d.reset(i)
            m.reset(i)
        if i == 6:
            d.reset()
            m.reset()
        bus, n = i % M, int(rng.integers(0, 40))
        ch, g = rng.integers(0, C, size=n), rng.integers(-32767, 32768, size=n)
        d.set_bus(bus, ch, g)
        m.set_bus(bus, ch, g)
        # four calls on one stream, then one on a second stream directly behind them, then the first stream again
        st = streams[1 if i == 4 else 0]
        d.process_device(d_pcm.data_ptr(), 1024 * n_blocks, None, d_open[i].data_ptr(), n_blocks, d_out[i].data_ptr(), 0,
                         d_mix[i].data_ptr(), d_clips[i].data_ptr(), st.cuda_stream)
        want.append(m.process(pcm, None, opens[i]))
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        got = (d_out[i].cpu().numpy(), d_mix[i].cpu().numpy(), d_clips[i].cpu().numpy().view(np.uint32))
        same(got, want[i], f"call {i}")


# what needs a handle to be refused
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    d = api.Audio(4, 2, device=0)
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=dev)
    p = buf.data_ptr()
    with pytest.raises(api.HrfdError, match="hrfd_audio_set_bus.*names channel 4"):
        d.set_bus(0, [0, 4], [1, 1])
    with pytest.raises(api.HrfdError, match="hrfd_audio_set_bus.*bus 2"):
        d.set_bus(2, [0], [1])
    with pytest.raises(api.HrfdError, match="hrfd_audio_set_bus.*-32768"):
        d.set_bus(0, [0], [-32768])
    with pytest.raises(api.HrfdError, match="hrfd_audio_set_want.*channel 4"):
        d.set_want(0, 4)
    with pytest.raises(api.HrfdError, match="hrfd_audio_set_want.*want 128"):
        d.set_want(128)
    with pytest.raises(api.HrfdError, match="hrfd_audio_reset.*channel 4"):
        d.reset(4)
    with pytest.raises(api.HrfdError, match="hrfd_audio_set_taps.*65536"):
        d.set_taps([-32768, -32768])
    # out behind the first input row but inside the fourth
    with pytest.raises(api.HrfdError, match="hrfd_audio_process_device.*overlaps"):
        d.process_device(p, 1024, None, None, 1, p + 3 * 1024 + 1022, 1024, None, None)
    with pytest.raises(api.HrfdError, match="hrfd_audio_process_device.*no output"):
        d.process_device(p, 1024, None, None, 1, None, 1024, None, p + 8192)
    with pytest.raises(api.HrfdError, match="hrfd_audio_gate_device.*frames"):
        d.gate_device(p, p, 1024, 0, 3, p + 8192)
    x = np.arange(4 * 512, dtype=np.int16).reshape(4, 512)
    out, mix, clips = d.process(x)                         # the handle still works, with its defaults: identity, no list
    assert (out[:, 0, :64] == (x[:, :64].astype(np.int64) * (512 * (np.arange(64) + 1)) + (1 << 14)) >> 15).all()
    assert (out[:, 0, 64:] == x[:, 64:]).all() and (mix == 0).all() and (clips == 0).all()


# 11. the closed loop on the device
def test_closed_loop_transmit_receive_decode_listen(torch_dev, oracle):
    """tests/test_gpu_tone.py's closed loop with the audio bank behind it: two WBFM stations whose audio is a DTMF digit per
    64 ms block, a 1000 Hz pilot under the first, through Mod, Duc.transmit, Ddc.receive and Tones.process_device; then
    Audio.gate_device on the verdicts (want = the pilot's index for both channels, the pilot's group) and
    Audio.process_device (the high-pass helper's taps, one bus holding both channels at unity gain) on the d_pcm and d_n_pcm
    receive filled, no host copy between.  (a) open, out, mix and clips equal the model's on the PCM receive wrote, (b)
    channel 0 has open blocks, channel 1 has none, and the bus carries channel 0 alone.  The model gives this gate pattern
    on the CPU as well (every block of channel 0 open, none of channel 1), with the tone test's own group and want: nothing
    had to be picked."""
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
    pilot, pilot_group = len(steps) - 1, 2
    taps = api.audio_highpass_taps()
    bank, model = both(2, 1, taps, [([0, 1], [api.AUDIO_UNITY_GAIN] * 2)])
    bank.set_want(pilot)
    model.set_want(pilot)
    F = 512 * B // tm.LOOP_L
    d_pcm_in = torch.from_numpy(np.stack(audio).astype(np.int16)).to(dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((2, B), dtype=torch.int32, device=dev)
    d_best = torch.zeros((2, F, 4), dtype=torch.uint8, device=dev)
    d_present = torch.zeros((2, F, 4), dtype=torch.uint8, device=dev)
    d_open = torch.full((2, B), 77, dtype=torch.uint8, device=dev)
    d_out = torch.zeros((2, B, 512), dtype=torch.int16, device=dev)
    d_mix = torch.zeros((1, B, 512), dtype=torch.int16, device=dev)
    d_clips = torch.full((1,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_pcm_in.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    # one stream for the three calls behind receive: each reads what the one in front of it wrote
    st = torch.cuda.Stream()
    tones.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, None, None, None, d_best.data_ptr(), d_present.data_ptr(),
                         st.cuda_stream)
    bank.gate_device(d_best.data_ptr(), d_present.data_ptr(), tm.LOOP_L, pilot_group, B, d_open.data_ptr(), st.cuda_stream)
    bank.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), d_open.data_ptr(), B, d_out.data_ptr(), 0, d_mix.data_ptr(),
                        d_clips.data_ptr(), st.cuda_stream)
    st.synchronize()
    torch.cuda.synchronize()
    pcm = d_pcm.cpu().numpy().reshape(2, -1)
    n_pcm = d_n.cpu().numpy().view(np.uint32)
    best, present = tm.loop_model().process(pcm, n_pcm)[3:]
    assert (d_best.cpu().numpy() == best).all() and (d_present.cpu().numpy() == present).all()
    open_ = model.gate(best, present, tm.LOOP_L, pilot_group)
    assert (d_open.cpu().numpy() == open_).all()
    got = (d_out.cpu().numpy(), d_mix.cpu().numpy(), d_clips.cpu().numpy().view(np.uint32))
    same(got, model.process(pcm, n_pcm, open_), "the bank on the PCM receive wrote")
    assert open_[0].any() and not open_[1].any()
    assert (got[0][1] == 0).all() and (got[1][0] == got[0][0]).all() and got[2][0] == 0
