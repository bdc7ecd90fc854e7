"""The AFSK generator bank on the device (hrfd_afskgen_*) against the numpy model (tests/afskgen_model.py), bit for bit: channel
and block counts on both sides of the kernel's tile, messages that start and end on every lane, wave, block and tile edge,
messages shorter than their two ramps, four in one tile, the phase carried across calls with a cut and a queue between, every
modem of the model's tests and two on neighbouring channels, one tone against ToneGen on the device, saturation with its
count, generate-only, out of place and in place at every even residue with padded strides and guard bytes around every
buffer, the clock across 2^32 and up to 2^63, setters behind running calls, and what the bank exists for: its audio decoded by
Afsk on the device, and the closed loop AfskGen -> Mod -> Duc.transmit -> Ddc.receive -> Afsk.  No comparison has a
tolerance."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import afsk_model as am
from tests import afskgen_model as gm
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF
MODEMS = [(gm.step(1200), gm.step(2200), gm.step(1200)), (gm.step(1270), gm.step(1070), gm.step(300)), (gm.step(1200), gm.step(1800), 1 << 31),
          (0x5A5A5A5B, 0x13579BDF, gm.ODD_STEP)]              # Bell 202, Bell 103, 4000 baud, the odd step


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C):
    return api.AfskGen(C, device=0), gm.AfskGenModel(C)


def rbits(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


_reference = {}


def reference(C, n, seed=7):
    """random int16 over the full range, one array per shape, computed once and left unchanged"""
    key = (C, n, seed)
    if key not in _reference:
        x = np.random.default_rng(seed).integers(-32768, 32768, size=(C, n), dtype=np.int16)
        x.setflags(write=False)
        _reference[key] = x
    return _reference[key]


def scatter(hs, C, n, seed, base=0):
    """the same random queues on every handle of hs: every third channel idle, the others with one to four messages of any
    modem around the call's n samples"""
    rng = np.random.default_rng(seed)
    for c in range(C):
        if c % 3 == 2:
            continue
        start = base + int(rng.integers(0, max(n // 2, 2)))
        for i in range(int(rng.integers(1, 5))):
            bits = rbits(int(rng.choice([1, 3, 40, 200, 700])), seed + 10 * c + i)
            kw = dict(steps=MODEMS[int(rng.integers(4))], amplitude=int(rng.integers(0, 32768)), nrzi=bool(rng.integers(2)),
                      gap=int(rng.choice([0, 0, 1, 200, 700])))
            for h in hs:
                h.queue(c, bits, start=start if i == 0 else gm.APPEND, **kw)


def same_state(d, m, what):
    assert d.time() == m.time(), what
    for c in range(m.C):
        assert d.clips(c) == m.clips(c), f"{what}: clips of channel {c}: {d.clips(c)} against {m.clips(c)}"
        assert d.pending(c) == m.pending(c), f"{what}: pending({c})"


def run_device(torch_dev, d, m, pcm, n_blocks, what, mode="out", residue=0, pad=0, out_pad=0, want_active=True, stream=None):
    """process_device in one of three modes: "gen" (no input), "out" (input rows at `residue` modulo 16, 1024 n_blocks + pad
    bytes apart; out rows at 14 - residue, 1024 n_blocks + out_pad apart) or "in_place"; active at an odd address; every
    buffer between guards.  The model takes the same call; out, active, the guards, the input and the clips must be its"""
    torch, dev = torch_dev
    C, n = m.C, 512 * n_blocks
    stride = 2 * n + pad
    out_stride = stride if mode == "in_place" else 2 * n + out_pad
    src = None
    if mode != "gen":
        pcm = np.asarray(pcm).reshape(C, n)
        src = Guarded(torch_dev, stride * (C - 1) + 2 * n, residue, 16, 21)
        for c in range(C):
            src.host[src.off + c * stride:src.off + c * stride + 2 * n] = pcm[c].view(np.uint8)
        src.put(0, pcm[0])
    want, want_act = m.process(None if mode == "gen" else pcm, n_blocks, want_active=True)
    out = src if mode == "in_place" else Guarded(torch_dev, out_stride * (C - 1) + 2 * n, 14 - residue, 16, 22)
    act = Guarded(torch_dev, C * n_blocks, 1, 2, 23)
    torch.cuda.synchronize()
    d.process_device(None if src is None else src.ptr, stride, n_blocks, out.ptr, out_stride, act.ptr if want_active else None, stream)
    torch.cuda.synchronize()
    rows = out.host[out.off:out.off + out.n].copy()           # the rows of out as they must lie between what was there before
    for c in range(C):
        rows[c * out_stride:c * out_stride + 2 * n] = want[c].reshape(-1).view(np.uint8)
    if mode == "out":
        src.check(None, what + ": the input")
    out.check(rows, f"{what}: out")
    act.check(want_act if want_active else None, f"{what}: active")
    same_state(d, m, what)
    return want, want_act


# 1. sizes: the tile is 4 blocks: 1 block (a quarter tile), 4 and 5 (both sides of one tile), 16 (four tiles); one channel,
#    three, and 65
@pytest.mark.parametrize("C", [1, 3, 65])
@pytest.mark.parametrize("n_blocks", [1, 4, 5, 16])
def test_channel_and_block_counts(C, n_blocks):
    d, m = both(C)
    scatter((d, m), C, 512 * n_blocks, 100 * C + n_blocks)
    pcm = reference(C, 512 * n_blocks)
    got, act = d.process(pcm, want_active=True)
    want, want_act = m.process(pcm, want_active=True)
    assert got.dtype == want.dtype and got.shape == want.shape and (got == want).all(), np.argwhere(got != want)[:4].tolist()
    assert (act == want_act).all()
    got = d.process(None, n_blocks)                            # the second call: generate only, what is still in progress
    assert (got == m.process(None, n_blocks)).all()
    same_state(d, m, f"C={C}, {n_blocks} blocks")


# 2. edges, on the second of two calls of 5 blocks: per offset one channel whose message starts there and one whose message
#    ends there (its last sample lies one in front; those that began in the first call carry their phase across)
EDGES = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 2047, 2048, 2049)


def test_message_edges(torch_dev):
    n_blocks, N0 = 5, 2560
    C = 2 * len(EDGES)
    d, m = both(C)
    bits = rbits(45, 31)                                       # 301 samples at 1200 baud
    L = gm.length(45, gm.step(1200))
    for h in (d, m):
        for i, e in enumerate(EDGES):
            h.queue(2 * i, bits, amplitude=30000, start=N0 + e)
            h.queue(2 * i + 1, bits, amplitude=30000, nrzi=False, start=N0 + e - L)
    x = reference(C, 512 * n_blocks)
    run_device(torch_dev, d, m, x, n_blocks, "the call in front")
    assert d.pending(1) == (0, N0) and d.pending(3) == (1, N0 + 1)
    want, act = run_device(torch_dev, d, m, x, n_blocks, "edges", mode="in_place")
    assert act[0].tolist() == [1, 0, 0, 0, 0] and act[1].tolist() == [0] * 5 and act[2 * EDGES.index(2049)].tolist() == [0, 0, 0, 0, 1]
    assert act[2 * EDGES.index(2048) + 1].tolist() == [0, 0, 0, 1, 0] and act[2 * EDGES.index(2049) + 1].tolist() == [0, 0, 0, 1, 1]


# 3. short and crowded: messages of 2, 20 and 21 samples, whose ramps meet; four messages inside one tile; one that ends at
#    n - 1 with the next starting at n
def test_short_and_crowded(torch_dev):
    d, m = both(4)
    for h in (d, m):
        h.queue(0, [1], amplitude=32767, steps=(1 << 30, 1 << 29, 1 << 31), start=5)                      # L = 2
        h.queue(0, [0, 1, 0], amplitude=32767, gap=9)                                                      # L = 21 at 1200 baud
        h.queue(0, [0, 1, 0], amplitude=32767, steps=(gm.step(1200), gm.step(2200), gm.step(1200) + 1))    # L = 20, at once behind
        h.queue(1, rbits(60, 1), amplitude=20000, start=3)                                                 # [3, 404)
        for i, (n_bits, modem, gap) in enumerate(((20, 1, 0), (51, 2, 17), (3, 3, 34))):                   # 534, 102 and 676 samples
            h.queue(1, rbits(n_bits, 2 + i), amplitude=32767, nrzi=bool(i & 1), steps=MODEMS[modem], gap=gap)
        h.queue(2, rbits(77, 9), amplitude=32767, start=1)
        h.queue(2, rbits(300, 10), amplitude=32767, steps=MODEMS[3])                                       # starts where the first ends
    assert d.pending(0) == m.pending(0) == (3, 5 + 2 + 9 + 21 + 20) and d.pending(1)[0] == 4
    assert d.pending(2) == m.pending(2) and m.q[2][0].end == m.q[2][1].start
    want, act = run_device(torch_dev, d, m, None, 4, "short and crowded", mode="gen")
    row = want[0].reshape(-1)
    assert row[5] == 0 and row[6] == (32767 + 32) >> 6 and np.count_nonzero(row[:16]) == 1                # sin(pi / 2) at the top of one step
    assert m.q[1][-1].end < 2048 and act[1].tolist() == [1, 1, 1, 1] and act[3].tolist() == [0] * 4
    run_device(torch_dev, d, m, reference(4, 2048), 4, "what is left", mode="in_place")


# 4. the phase carried across calls
def test_carried_phase(torch_dev):
    C, cuts = 3, (1, 4, 5)
    pcm = reference(C, 512 * sum(cuts), 8).reshape(C, -1, 512)
    long, late = rbits(660, 41), rbits(80, 42)                 # 4400 samples: in progress across both cuts
    parts, mp = both(C)
    for h in (parts, mp):
        h.queue(ALL, long, amplitude=20000, start=100)
        h.queue(1, rbits(100, 43), steps=MODEMS[1], gap=50)
    got, at = [], 0
    for i, k in enumerate(cuts):
        out = parts.process(pcm[:, at:at + k])
        assert (out == mp.process(pcm[:, at:at + k])).all(), f"call {i}"
        got.append(out)
        at += k
        if i == 0:
            for h in (parts, mp):
                h.queue(0, late, amplitude=32767, nrzi=False, gap=30)      # behind the one in progress
                h.cut(2)                                       # the long one ends at 512 + 64
                h.cut(1)                                       # and drops what has not begun
            assert parts.pending(2) == mp.pending(2) == (1, 576) and parts.pending(1) == (1, 576) and parts.pending(0)[0] == 2
    same_state(parts, mp, "cut into calls")
    # one call of 10 blocks over the queues the cut stream ended up with, on the model
    whole, mw = both(C)
    for h in (whole, mw):
        h.queue(ALL, long, amplitude=20000, start=100)
        h.queue(0, late, amplitude=32767, nrzi=False, gap=30)
    for q in (mw.q[1], mw.q[2]):
        q[0].end = 576
    one, mo = both(C)                                          # the uncut stream in ONE call of 10 blocks on a third handle
    for h in (one, mo):
        h.queue(ALL, long, amplitude=20000, start=100)
        h.queue(0, late, amplitude=32767, nrzi=False, gap=30)
    other = one.process(pcm.reshape(C, -1))
    assert (other == mo.process(pcm.reshape(C, -1))).all()
    joined = np.concatenate(got, axis=1)
    want = mw.process(pcm.reshape(C, -1))
    assert (joined == want).all() and (other[0] == joined[0]).all()       # channel 0 was never cut: 1 + 4 + 5 against 10
    # another cut of the stream on the device, 1 + 9, with the same cuts of channels 1 and 2 between: two handles agree
    x0 = whole.process(pcm[:, :1])
    whole.cut(1)
    whole.cut(2)
    rest = whole.process(pcm[:, 1:])
    assert (np.concatenate([x0, rest], axis=1) == want).all()
    assert [whole.clips(c) for c in range(C)] == [parts.clips(c) for c in range(C)]


# 5. modems: 300, 1200 and 4000 baud and the odd step, NRZI off and on, on neighbouring channels of one call; 8192 bits
def test_modems_on_neighbouring_channels(torch_dev):
    C = 9
    d, m = both(C)
    for h in (d, m):
        for c in range(8):
            h.queue(c, rbits(150 + c, 50 + c), steps=MODEMS[c % 4], amplitude=8000 + c, nrzi=c >= 4, start=c)
        h.queue(8, rbits(8192, 59), steps=(gm.step(2200), gm.step(1200), 1 << 31), amplitude=32767, start=511)        # 16384 samples
    run_device(torch_dev, d, m, reference(C, 512 * 16), 16, "modems", residue=2, pad=2)
    run_device(torch_dev, d, m, reference(C, 512 * 20, 5), 20, "modems, the second call", mode="in_place")
    assert d.pending(8) == (0, d.time()) and d.pending(3)[0] == 1                                      # the odd step goes on


# 6. one tone: mark_step == space_step is ToneGen's segment, on the device, equal bytes
def test_one_tone_equals_tonegen_on_the_device(torch_dev):
    torch, dev = torch_dev
    C, n_blocks = 4, 6
    a, t = api.AfskGen(C, device=0), api.ToneGen(C, device=0)
    for c in range(C):
        tone, B, r, amp, start = (1 << 27) * (2 * c + 1) + c, (3, 90, 400, 1)[c], MODEMS[c][2], (32767, 9000, 1, 20000)[c], (0, 77, 511, 2047)[c]
        a.queue(c, rbits(B, 60 + c), amplitude=amp, start=start, steps=(tone, tone, r))
        t.queue(c, 0, [(0, gm.length(B, r), tone, 0, amp, 0)], start)
    x = torch.from_numpy(reference(C, 512 * n_blocks, 11).copy()).to(dev)
    ya, yt = torch.zeros_like(x), torch.zeros_like(x)
    torch.cuda.synchronize()
    a.process_device(x.data_ptr(), 1024 * n_blocks, n_blocks, ya.data_ptr())
    t.process_device(x.data_ptr(), 1024 * n_blocks, n_blocks, yt.data_ptr())
    torch.cuda.synchronize()
    assert (ya.cpu().numpy() == yt.cpu().numpy()).all() and (ya != x).any()
    assert [a.clips(c) for c in range(C)] == [t.clips(c) for c in range(C)]


# 7. the output: amp 0, 1 and 32767 under full-scale input with the clip count; the three modes at every even residue with
#    padded strides, with and without active; idle rows
def test_saturation_and_clips(torch_dev):
    d, m = both(4)
    for h in (d, m):
        for c, amp in enumerate((0, 1, 32767, 32767)):
            h.queue(c, rbits(250, 70 + c), amplitude=amp, start=10)
    x = np.zeros((4, 2048), dtype=np.int16)
    x[0], x[1], x[2], x[3] = 32767, -32768, 32767, -32768
    want, act = run_device(torch_dev, d, m, x, 4, "saturation", residue=6, pad=4)
    clips = [d.clips(c) for c in range(4)]
    assert clips == [m.clips(c) for c in range(4)] and clips[0] == 0 and min(clips[2:]) > 100 and (want[0] == 32767).all()
    assert want.max() == 32767 and want.min() == -32768 and act.tolist() == [[1, 1, 1, 1]] * 4
    for h in (d, m):
        h.reset()
    assert [d.clips(c) for c in range(4)] == [0] * 4 and d.time() == 0 and d.pending(0) == (0, 0)
    run_device(torch_dev, d, m, x, 4, "behind reset", mode="in_place")
    assert [d.clips(c) for c in range(4)] == [0] * 4


@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_modes_addresses_and_strides(torch_dev, residue):
    C, n_blocks = 5, 5
    d, m = both(C)
    scatter((d, m), C, 3 * 512 * n_blocks, 70 + residue)
    pcm = reference(C, 512 * n_blocks, 9)
    for i, (pad, out_pad) in enumerate(((2, 6), (6, 16), (16, 2))):
        what = f"residue {residue} pads {pad} {out_pad}"
        mode = ("out", "in_place", "gen")[(residue // 2 + i) % 3]
        run_device(torch_dev, d, m, pcm, n_blocks, f"{what} {mode}", mode, residue, pad, out_pad, want_active=i != 1)
    assert d.pending(2) == (0, d.time())                       # an idle row: in place its bytes were never written (the guards' check)


# 8. the clock
def test_clock_across_2_32_and_up_to_2_63(torch_dev):
    d, m = both(2)
    for h in (d, m):
        h.set_time((1 << 32) - 1024)
        h.queue(0, rbits(250, 81), amplitude=25000, start=(1 << 32) - 700)
        h.queue(1, rbits(60, 82), steps=MODEMS[1], start=(1 << 32) - 1)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_set_time.*channel 0 holds a message that has not ended"):
        d.set_time(5)
    run_device(torch_dev, d, m, reference(2, 1024), 2, "up to 2^32")
    run_device(torch_dev, d, m, reference(2, 1024), 2, "from 2^32", mode="in_place")
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_set_time.*channel 1"):
        d.set_time(1 << 40)
    run_device(torch_dev, d, m, None, 4, "the rest of the slow one", mode="gen")
    base = (1 << 63) - 3 * 512 - 1
    for h in (d, m):
        h.set_time(base)
        h.queue(ALL, rbits(91, 83), amplitude=32767, gap=3 * 512 - 607)       # ends on the last stream time there is
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_queue.*2\\^63"):
        d.queue(0, [1], gap=1)
    assert d.pending(0) == (1, (1 << 63) - 1)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_process.*below 2\\^63"):
        d.process(None, 4)
    run_device(torch_dev, d, m, reference(2, 512), 1, "below 2^63, the first block")
    want, act = run_device(torch_dev, d, m, None, 2, "below 2^63, the last two", mode="gen")
    assert d.time() == (1 << 63) - 1 and want[0, 1].any() and act.tolist() == [[1, 1]] * 2
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_process.*below 2\\^63"):
        d.process(None, 1)


# 9. ordering: the queues of a call are those set before it, whatever still runs; a call chained behind the copy that fills
#    its input; the blocking host entry between them
def test_setters_behind_running_calls(torch_dev):
    torch, dev = torch_dev
    C, n_blocks = 64, 16
    d, m = both(C)
    scatter((d, m), C, 512 * n_blocks * 3, 81)
    pcm = reference(C, 512 * n_blocks, 10)
    host = torch.from_numpy(pcm.copy()).pin_memory()
    calls = 7
    d_in = torch.zeros((calls, C, n_blocks * 512), dtype=torch.int16, device=dev)
    d_out = torch.zeros((calls, C, n_blocks, 512), dtype=torch.int16, device=dev)
    d_act = torch.zeros((calls, C, n_blocks), dtype=torch.uint8, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    want = []
    torch.cuda.synchronize()
    for i in range(calls):
        # four calls on one stream, then one on a second stream directly behind them, then the first stream again
        s = streams[1 if i == 4 else 0]
        gen = i % 3 == 2
        if not gen:
            with torch.cuda.stream(s):
                d_in[i].copy_(host, non_blocking=True)         # the call below is chained behind this copy on s
        d.process_device(None if gen else d_in[i].data_ptr(), 1024 * n_blocks, n_blocks, d_out[i].data_ptr(), 0, d_act[i].data_ptr(),
                         s.cuda_stream)
        want.append(m.process(None if gen else pcm, n_blocks, want_active=True))
        for h in (d, m):                                       # behind the call that now runs
            if i in (0, 3):
                h.cut(ALL)
            if i in (1, 4):
                h.queue(ALL, rbits(500 + i, 90 + i), amplitude=30000, steps=MODEMS[i % 4], gap=100)
            if i == 2:
                h.cut(5)
                h.queue(5, rbits(12, 99), amplitude=32767, start=h.time() + 64)
            if i == 5:
                h.reset()
                h.queue(ALL, rbits(450, 98), amplitude=32767, start=50)
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        out, act = d_out[i].cpu().numpy(), d_act[i].cpu().numpy()
        assert (out == want[i][0]).all(), f"call {i}: out differs at {np.argwhere(out != want[i][0])[:4].tolist()}"
        assert (act == want[i][1]).all(), f"call {i}: active"
    got = d.process(pcm)                                       # the blocking entry behind them
    assert (got == m.process(pcm)).all()
    same_state(d, m, "behind eight calls")


# what needs a handle to be refused; a refused queue changes nothing
def test_refusals_with_a_handle(torch_dev):
    torch, dev = torch_dev
    d, m = both(4)
    buf = torch.zeros(1 << 16, dtype=torch.int8, device=dev)
    p = buf.data_ptr()
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_queue.*channel 4"):
        d.queue(4, [1])
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_cut.*channel 4"):
        d.cut(4)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_pending.*channel 4"):
        d.pending(4)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_get_clips.*channel 4"):
        d.clips(4)
    for h in (d, m):
        h.queue(ALL, [1, 0, 1], start=1000)                    # [1000, 1021)
        for i in range(3):
            h.queue(3, [1, 0, 1], gap=i)
    for text, kw in (("would overlap", dict(channel=ALL, start=1020)), ("would overlap", dict(channel=2, start=980)),
                     ("5 messages", dict(channel=3)), ("5 messages", dict(channel=ALL, start=5000)),
                     ("2\\^63", dict(channel=1, start=(1 << 63) - 21))):
        channel = kw.pop("channel")
        with pytest.raises(api.HrfdError, match="hrfd_afskgen_queue.*" + text):
            d.queue(channel, [1, 0, 1], **kw)
        with pytest.raises(ValueError):
            m.queue(channel, [1, 0, 1], **kw)
    assert (d.process(None, 1) == m.process(None, 1)).all()
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_queue.*start 511 lies before the stream time 512"):
        d.queue(1, [1], start=511)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_process_device.*overlaps"):      # behind the first input row, inside the fourth
        d.process_device(p, 1024, 1, p + 3 * 1024 + 1022, 1024)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_process_device.*overlaps"):
        d.process_device(p, 1024, 1, p, 1026)
    with pytest.raises(api.HrfdError, match="hrfd_afskgen_process_device.*NULL argument"):
        d.process_device(p, 1024, 1, None, 1024)
    same_state(d, m, "behind the refusals")                    # every refused call left the queues and the clock alone
    x = reference(4, 1024)
    got, act = d.process(x, want_active=True)                  # the handle still works
    want, want_act = m.process(x, want_active=True)
    assert (got == want).all() and (act == want_act).all() and act[3].tolist() == [1, 1] and act[1].tolist() == [1, 0]


# 10. what the bank is for: its audio decoded by Afsk, both on the device
@pytest.mark.parametrize("modem", ["bell202", "bell103"])
def test_closed_loop_on_the_device(modem):
    """tests/test_afskgen_model.py's closed loop, seeds 1..3: api.AfskGen writes the audio, api.Afsk decodes it, api.hdlc_frames
    returns every frame; the audio is the model's"""
    mo = am.BELL202 if modem == "bell202" else am.BELL103
    gen, dec = api.AfskGen(1, device=0), api.Afsk(1, device=0, **mo)
    for amplitude, sigma in gm.LOOP_LEVELS:
        for seed in (1, 2, 3):
            gen.reset()
            dec.reset()
            payloads, pcm = gm.loop_case(mo, amplitude, sigma, seed, bank=gen)
            assert (pcm == gm.loop_case(mo, amplitude, sigma, seed)[1]).all()
            bits, _ = dec.process(pcm[None])
            assert api.hdlc_frames(bits[0]) == payloads, (modem, amplitude, sigma, seed)


# 11. the RF loop
def test_rf_loop_generate_transmit_receive_decode(torch_dev):
    """test_gpu_tonegen's chain with this bank in front and the AFSK bank behind: AfskGen -> Mod (FM) -> Duc.transmit ->
    Ddc.receive -> Rx (FM) -> Afsk -> hdlc_frames on the device, no host copy between: Bell 202 at amplitude 8000, one frame of 40
    bytes per channel on 3 channels 400 kHz apart, the tone generator test's R, block count and gain shift.  Every frame
    returns."""
    from tests import ddc_model as dm
    torch, dev = torch_dev
    R, B, FULL, C = dm.SEL_R, dm.SEL_BLOCKS, 262144, 3
    offsets = (-400_000.0, 0.0, 400_000.0)
    rng = np.random.default_rng(5)
    payloads = [am.random_payloads(rng, 1) for _ in range(C)]
    gen = api.AfskGen(C, device=0)
    for c in range(C):
        gen.send(c, payloads[c], start=300 + 100 * c)
    assert max(gen.pending(c)[1] for c in range(C)) < 512 * B - 1000
    mod = api.Mod(api.MOD_FM, C, device=0)
    duc = api.Duc(1, C, R, device=0)
    ddc = api.Ddc(1, C, R, device=0)
    rx = api.Rx(C, device=0)
    rx.set_mode(api.FM)
    for c, f in enumerate(offsets):
        duc.tune(c, 0, f)
        duc.set_amplitude(32768 // 5, c)
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(dm.SEL_GAIN_SHIFT[0], c)
    dec = api.Afsk(C, device=0)
    d_audio = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    d_pcm = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((C, B), dtype=torch.int32, device=dev)
    cap = dec.max_bits(B)
    d_bits = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(C, dtype=torch.int32, device=dev)
    d_hard = torch.zeros((C, B, 64), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(None, 0, B, d_audio.data_ptr())
    torch.cuda.synchronize()
    duc.transmit(mod, d_audio.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL)
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    dec.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_bits.data_ptr(), cap, d_count.data_ptr(), d_hard.data_ptr())
    torch.cuda.synchronize()
    bits, count = d_bits.cpu().numpy(), d_count.cpu().numpy()
    for c in range(C):
        got = api.hdlc_frames(bits[c, :count[c]])
        assert got == payloads[c], f"channel {c}: {len(got)} frames of 1 returned"
