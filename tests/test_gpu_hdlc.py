"""The HDLC bank on the device (hrfd_hdlc_*) against the model of tests/hdlc_model.py, bit for bit: the counts first (records,
bad frames, dropped), then the rows of records.  Every buffer lies between guard bytes, the rows of bits at an odd stride
from a misaligned base, and what lies behind a row's last record must stay as it was.  Channel counts 1, 3 and 65; rows of 1,
7, 8, 2047, 2048, 2049 and 5000 bits, the edges of the kernel's tile; d_n_bits at 0, below, at and above max_bits; every cut
of one stream in two launches; a frame across three calls and three tiles; P = 1, P = 1021 and m = P; a row of records one
record short; reset and set_limits between calls; n_bad; require_carrier; the host entry; a call chained behind the copy that
fills its input; the closed loop AfskGen -> Afsk -> Hdlc on the device; runs of 4..10 ones ending at every position of a
lane; and the carrier dropped on, behind and in front of closing flags at every alignment."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import hdlc_model as hm
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C, m=1, P=512, require_carrier=False):
    return api.Hdlc(C, m, P, require_carrier, device=0), hm.HdlcModel(C, m, P, require_carrier)


_pool = {}


def streams(C, n, P=24, seed=7):
    """C streams of n bits each (frames of up to P + 2 bytes, noise, runs, flipped bits), made once and left unchanged"""
    key = (C, n, P, seed)
    if key not in _pool:
        rng = np.random.default_rng(seed)
        rows = []
        for _ in range(C):
            parts, have = [], 0
            while have < n:
                parts.append(hm.mixed_stream(rng, 12, P=P))
                have += len(parts[-1])
            rows.append(np.concatenate(parts)[:n])
        x = np.stack(rows)
        x.setflags(write=False)
        _pool[key] = x
    return _pool[key]


def run_device(torch_dev, d, m, rows, what, max_bits=None, counts=None, residue=1, bits_pad=3, out_bytes=None, out_pad=4, want_bad=True,
               stream=None):
    """process_device over rows of bits at `residue` modulo 8, max_bits + bits_pad bytes apart, d_n_bits = counts (the rows'
    lengths unless given: the buffer holds max_bits bytes a row whatever the count says); rows of records out_bytes + out_pad
    apart; every buffer between guards.  The model takes the bytes the law uses.  Returns the model's frames"""
    torch, dev = torch_dev
    C = m.C
    assert len(rows) == C
    max_bits = max(1, max(len(r) for r in rows)) if max_bits is None else max_bits
    counts = np.array([len(r) for r in rows] if counts is None else counts, dtype=np.uint32)
    stride = max_bits + bits_pad
    src = Guarded(torch_dev, stride * (C - 1) + max_bits, residue, 8, 31)
    for c in range(C):
        k = min(len(rows[c]), max_bits)
        src.host[src.off + c * stride:src.off + c * stride + k] = rows[c][:k]
    src.put(0, np.zeros(0, dtype=np.uint8))
    used = [src.host[src.off + c * stride:src.off + c * stride + min(int(counts[c]), max_bits)].copy() for c in range(C)]
    d_n = Guarded(torch_dev, 4 * C, 4, 8, 32)
    d_n.put(0, counts)
    out_bytes = d.max_out(max_bits) if out_bytes is None else out_bytes
    out_stride = out_bytes + out_pad
    g_out = Guarded(torch_dev, out_stride * (C - 1) + out_bytes, 4, 8, 33)
    g_frames, g_bad, g_dropped = (Guarded(torch_dev, 4 * C, 4, 8, 34 + i) for i in range(3))
    torch.cuda.synchronize()
    d.process_device(src.ptr, stride, d_n.ptr, max_bits, g_out.ptr, out_stride, out_bytes, g_frames.ptr, g_bad.ptr if want_bad else None,
                     g_dropped.ptr, stream)
    torch.cuda.synchronize()
    frames, n_frames, n_bad, dropped, outs = m.process(used, out_bytes)
    g_frames.check(n_frames, f"{what}: n_frames")
    g_bad.check(n_bad if want_bad else None, f"{what}: n_bad")
    g_dropped.check(dropped, f"{what}: dropped")
    want = g_out.host[g_out.off:g_out.off + g_out.n].copy()
    for c in range(C):
        want[c * out_stride:c * out_stride + len(outs[c])] = np.frombuffer(outs[c], dtype=np.uint8)
    g_out.check(want, f"{what}: the records, or the bytes behind a row's last")
    src.check(None, f"{what}: the bits")
    d_n.check(None, f"{what}: n_bits")
    return frames


# 1. channel counts and the tile's edges, two calls each so that the state is carried across every length
@pytest.mark.parametrize("n", [1, 7, 8, 2047, 2048, 2049, 5000])
@pytest.mark.parametrize("C", [1, 3, 65])
def test_channel_counts_and_tile_edges(torch_dev, C, n):
    d, m = both(C, 1, 24)
    x = streams(C, 13000)
    total = 0
    for call, part in enumerate((x[:, :n], x[:, n:2 * n], x[:, 2 * n:2 * n + 2049])):
        total += sum(len(f) for f in run_device(torch_dev, d, m, list(part), f"C={C} n={n} call {call}"))
    assert total >= C


# 2. every residue of the base, odd and even strides
@pytest.mark.parametrize("residue", range(8))
def test_misaligned_rows_of_bits(torch_dev, residue):
    d, m = both(3, 2, 24)
    x = streams(3, 10000)
    frames = run_device(torch_dev, d, m, list(x[:, :2049 + residue]), f"residue {residue}", residue=residue, bits_pad=residue % 3,
                        out_pad=4 * (residue % 2))
    assert sum(len(f) for f in frames) >= 3


# 3. the counts the kernel reads on the device
def test_n_bits_at_zero_below_at_and_above_max_bits(torch_dev):
    d, m = both(5, 1, 24)
    x = streams(5, 10000)
    max_bits = 3000
    for call, counts in enumerate(([0, 100, 3000, 3050, 2999], [3000, 0, 0xFFFFFFFF, 1, 2048], [0, 0, 0, 0, 0])):
        run_device(torch_dev, d, m, list(x[:, call * 3000:(call + 1) * 3000]), f"counts {counts}", max_bits=max_bits, counts=counts)


# 4. every cut of one stream in two launches
def three_frames_600():
    rng = np.random.default_rng(11)
    p = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (18, 15, 20)]
    bits = hm.FLAG * 2 + hm.frame_bits(p[0]) + hm.FLAG + hm.frame_bits(p[1]) + hm.FLAG + hm.frame_bits(p[2]) + hm.FLAG
    assert len(bits) <= 600
    bits += [1, 0] * 300
    return np.array(bits[:600], dtype=np.uint8) | hm.CARRIER, p


def test_every_cut_of_one_stream_in_two_launches(torch_dev):
    stream, payloads = three_frames_600()
    uncut = hm.HdlcModel(1).process([stream])[0][0]
    assert [p for _, p, _ in uncut] == payloads == api.hdlc_frames(stream)
    C = 600
    d, m = both(C)
    first = run_device(torch_dev, d, m, [stream[:c] for c in range(C)], "the first c bits", max_bits=600)
    second = run_device(torch_dev, d, m, [stream[c:] for c in range(C)], "the rest", max_bits=600)
    for c in range(C):
        joined = first[c] + [(c + e, p, fcs) for e, p, fcs in second[c]]
        assert joined == uncut, f"cut at {c}"


# 5. a frame across three calls and three tiles
def test_a_frame_across_three_calls_and_three_tiles(torch_dev):
    rng = np.random.default_rng(12)
    long = rng.integers(0, 256, size=800, dtype=np.uint8).tobytes()
    stream = np.array(hm.FLAG + hm.frame_bits(b"before") + hm.FLAG + hm.frame_bits(long) + hm.FLAG + hm.frame_bits(b"behind") + hm.FLAG,
                      dtype=np.uint8)
    assert len(stream) > 3 * 2048
    shifted = np.concatenate([np.ones(5, dtype=np.uint8), stream])[:len(stream)]
    d, m = both(2, 1, 1021)
    got = [[], []]
    for call, (a, b) in enumerate(((0, 2500), (2500, 4600), (4600, len(stream)))):
        f = run_device(torch_dev, d, m, [stream[a:b], shifted[a:b]], f"call {call}")
        for c in range(2):
            got[c] += [p for _, p, _ in f[c]]
    assert got[0] == [b"before", long, b"behind"] and got[1] == [b"before", long]
    d, m = both(2, 1, 1021)
    whole = run_device(torch_dev, d, m, [stream, shifted], "one call of four tiles")
    assert [p for _, p, _ in whole[0]] == got[0]


# 6. the limits of the limits
@pytest.mark.parametrize("m_,P", [(1, 1), (1021, 1021), (1, 1021), (5, 5)])
def test_shortest_and_longest_payloads(torch_dev, m_, P):
    ok, over, under = bytes([0x5A] * P), bytes([0xC3] * (P + 1)), bytes([0x3C] * (P - 1))
    parts = hm.FLAG + hm.frame_bits(ok) + hm.FLAG + hm.frame_bits(over) + hm.FLAG
    if P > 1:
        parts += hm.frame_bits(under) + hm.FLAG
    parts += hm.frame_bits(bytes([0xFF] * P)) + hm.FLAG
    stream = np.array(parts, dtype=np.uint8)
    want = [ok] + ([under] if P > 1 and m_ < P else []) + [bytes([0xFF] * P)]
    d, m = both(1, m_, P)
    assert [p for _, p, _ in run_device(torch_dev, d, m, [stream], f"m={m_} P={P}")[0]] == want
    d.reset()
    m.reset()
    cut = len(stream) // 2 + 3
    got = run_device(torch_dev, d, m, [stream[:cut]], f"m={m_} P={P} first")[0] + run_device(torch_dev, d, m, [stream[cut:]], f"m={m_} P={P} second")[0]
    assert [p for _, p, _ in got] == want


# 7. a row of records one record short, exactly full, and far too small
def test_a_row_too_small_by_one_record(torch_dev):
    frames = [bytes([i + 1] * (3 + i)) for i in range(6)]
    sizes = [8 + ((len(p) + 3) & ~3) for p in frames]
    rows = [np.array(hm.shared_flag_frames(frames[:k]), dtype=np.uint8) for k in (6, 5, 4, 6)]
    d, m = both(4)
    out_bytes = sum(sizes[:5])
    run_device(torch_dev, d, m, rows, "one record short on channels 0 and 3", out_bytes=out_bytes)
    want = m.process([r for r in rows], out_bytes)
    assert want[1].tolist() == [5, 5, 4, 5] and want[3].tolist() == [1, 0, 0, 1]
    d, m = both(4)
    run_device(torch_dev, d, m, rows, "four bytes less: two dropped", out_bytes=out_bytes - 4)
    d, m = both(4)
    run_device(torch_dev, d, m, rows, "a row of one dword: all dropped", out_bytes=4, out_pad=0)
    assert hm.HdlcModel(4).process(rows, 4)[3].tolist() == [6, 5, 4, 6]


# 8. reset and set_limits between calls
def test_reset_and_set_limits_between_calls(torch_dev):
    d, m = both(3, 1, 24)
    x = streams(3, 10000)
    run_device(torch_dev, d, m, list(x[:, :1500]), "before")
    d.reset(1)
    m.reset(1)
    run_device(torch_dev, d, m, list(x[:, 1500:3000]), "channel 1 reset")
    d.reset()
    m.reset()
    run_device(torch_dev, d, m, list(x[:, 3000:4500]), "all reset")
    d.set_limits(3, 10)
    m.set_limits(3, 10)
    assert d.max_out(1500) == m.max_out(1500)
    run_device(torch_dev, d, m, list(x[:, 4500:6000]), "other limits")
    run_device(torch_dev, d, m, list(x[:, 6000:7500]), "other limits, carried")
    with pytest.raises(api.HrfdError, match="channel 3"):
        d.reset(3)
    with pytest.raises(api.HrfdError, match="min_payload 11"):
        d.set_limits(11, 10)


# 9. the link-quality meter
def test_n_bad_on_a_frame_with_one_flipped_bit(torch_dev):
    body = hm.frame_bits(b"link quality")
    body[20] ^= 1
    stream = np.array(hm.FLAG + body + hm.FLAG + hm.frame_bits(b"fine") + hm.FLAG, dtype=np.uint8)
    d, m = both(2)
    frames = run_device(torch_dev, d, m, [stream, stream[::-1].copy()], "one flipped bit")
    assert [p for _, p, _ in frames[0]] == [b"fine"]
    assert hm.HdlcModel(1).process([stream])[2][0] == 1
    run_device(torch_dev, d, m, [stream, stream], "without n_bad", want_bad=False)


# 10. the carrier
def test_require_carrier_on_and_off(torch_dev):
    rng = np.random.default_rng(13)
    x = streams(4, 10000)[:, :6000].copy()
    for c in range(4):
        x[c, rng.integers(0, 6000, size=(0, 3, 40, 6000)[c])] &= ~np.uint8(hm.CARRIER)
    d, m = both(4, 1, 24, require_carrier=True)
    on = run_device(torch_dev, d, m, list(x[:, :3000]), "carrier required")
    d.set_require_carrier(False)
    m.require_carrier = False
    run_device(torch_dev, d, m, list(x[:, 3000:]), "no longer required: the state stays")
    d2, m2 = both(4, 1, 24)
    off = run_device(torch_dev, d2, m2, list(x[:, :3000]), "carrier ignored")
    assert on[0] == off[0] and len(on[2]) < len(off[2]) and on[3] == []


# 11. the blocking host entry
def test_the_host_entry(torch_dev):
    d, m = both(3, 1, 24)
    x = streams(3, 10000)
    for rows in ([x[0, :3000], x[1, :0], x[2, :2049]], [x[0, 3000:3001], x[1, :5000], x[2, 2049:4000]]):
        frames, (n_frames, n_bad, dropped) = d.process(rows, want_counts=True)
        want, w_frames, w_bad, w_dropped, _ = m.process(rows)
        assert (n_frames == w_frames).all() and (n_bad == w_bad).all() and (dropped == w_dropped).all() and not dropped.any()
        assert frames == [[(e, p) for e, p, _ in f] for f in want]
    assert sum(len(f) for f in frames) >= 3


# 12. chained on one stream behind the copy that fills its input
def test_chained_on_one_stream_behind_the_copy(torch_dev):
    torch, dev = torch_dev
    C, n = 5, 5000
    d, m = both(C, 1, 24)
    x = streams(C, 10000)[:, :n]
    host = torch.from_numpy(x.copy()).pin_memory()
    d_bits = torch.zeros((C, n), dtype=torch.uint8, device=dev)
    d_n = torch.full((C,), n, dtype=torch.int32, device=dev)
    ob = d.max_out(n)
    d_out = torch.zeros((C, ob), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((3, C), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_bits.copy_(host, non_blocking=True)
    d.process_device(d_bits.data_ptr(), n, d_n.data_ptr(), n, d_out.data_ptr(), ob, ob, d_cnt[0].data_ptr(), d_cnt[1].data_ptr(),
                     d_cnt[2].data_ptr(), st.cuda_stream)
    st.synchronize()
    want, n_frames, n_bad, dropped, _ = m.process(list(x))
    cnt = d_cnt.cpu().numpy().view(np.uint32)
    assert (cnt[0] == n_frames).all() and (cnt[1] == n_bad).all() and (cnt[2] == dropped).all()
    out = d_out.cpu().numpy()
    assert [api.Hdlc.parse(out[c], cnt[0][c]) for c in range(C)] == want


# 13. what the bank is for: packets from the generator to the frames, all on the device
def test_closed_loop_on_the_device(torch_dev):
    """AfskGen.send -> Afsk.process_device -> Hdlc.process_device chained on one stream, no host copy between: 65 channels x
    16 blocks, two frames of a channel's own on each.  The frames are those sent, and those of api.hdlc_frames over the bits"""
    torch, dev = torch_dev
    C, B = 65, 16
    rng = np.random.default_rng(14)
    payloads = [[bytes([c]) + rng.integers(0, 256, size=int(rng.integers(5, 30)), dtype=np.uint8).tobytes() for _ in range(2)] for c in range(C)]
    gen, dec, hd = api.AfskGen(C, device=0), api.Afsk(C, device=0), api.Hdlc(C, device=0)
    for c in range(C):
        gen.send(c, payloads[c], start=100 + 7 * c)
    assert max(gen.pending(c)[1] for c in range(C)) < 512 * B - 200
    cap = dec.max_bits(B)
    ob = hd.max_out(cap)
    d_audio = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    d_bits = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(C, dtype=torch.int32, device=dev)
    d_out = torch.zeros((C, ob), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((3, C), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    gen.process_device(None, 0, B, d_audio.data_ptr(), stream=st.cuda_stream)
    dec.process_device(d_audio.data_ptr(), 1024 * B, None, B, d_bits.data_ptr(), cap, d_count.data_ptr(), None, st.cuda_stream)
    hd.process_device(d_bits.data_ptr(), cap, d_count.data_ptr(), cap, d_out.data_ptr(), ob, ob, d_cnt[0].data_ptr(), d_cnt[1].data_ptr(),
                      d_cnt[2].data_ptr(), st.cuda_stream)
    st.synchronize()
    cnt, out, bits, count = d_cnt.cpu().numpy(), d_out.cpu().numpy(), d_bits.cpu().numpy(), d_count.cpu().numpy()
    assert (cnt[0] == 2).all() and (cnt[2] == 0).all()
    for c in range(C):
        got = [p for _, p, _ in api.Hdlc.parse(out[c], cnt[0][c])]
        assert got == payloads[c], f"channel {c}"
        assert got == api.hdlc_frames(bits[c, :count[c]]), f"channel {c}: the host's walk over the same bits"


# 14. runs of ones across the lanes' boundaries: the run in front of a lane comes from the lane before it alone
def test_runs_of_ones_at_every_alignment(torch_dev):
    """a good frame, 1..8 zeros, a run of 4..10 ones, a zero and then a frame's bits without a flag of their own: behind six
    ones that zero is a flag and the frame counts, behind five it is stuffing, behind seven and more the run was an abort and
    nothing is open.  Every run length ends at every position of a lane's eight bits, also where the run fills the lane in
    front to its end"""
    bits = []
    for r in range(4, 11):
        for z in range(1, 9):
            bits += hm.FLAG + hm.frame_bits(bytes([r, z])) + hm.FLAG + [0] * z + [1] * r + [0] + hm.frame_bits(bytes([z, r, 0xFF])) + hm.FLAG
    stream = np.array(bits, dtype=np.uint8)
    assert len(stream) > 2 * 2048
    want = api.hdlc_frames(stream)
    assert len(want) == 56 + 8 and [p for p in want if len(p) == 3] == [bytes([z, 6, 0xFF]) for z in range(1, 9)]
    d, m = both(8, 1, 24)
    frames = run_device(torch_dev, d, m, [stream[s:] for s in range(8)], "runs at eight shifts")
    assert min(len(f) for f in frames) >= 63
    assert [p for _, p, _ in frames[0]] == want


# 15. the carrier dropped on a closing flag's last bit, on the bit behind it and on a data bit, at every alignment
def test_the_carrier_on_and_around_a_closing_flag(torch_dev):
    bits, lost = [], []
    for i in range(24):
        bits += [0] * (i % 8) + hm.FLAG + hm.frame_bits(bytes([i, i + 1, i + 2])) + hm.FLAG
        lost.append(len(bits) - 1 if i % 3 == 0 else (len(bits) - 20 if i % 3 == 1 else None))
    stream = np.array(bits, dtype=np.uint8) | hm.CARRIER
    behind = stream.copy()
    for i, at in enumerate(lost):
        if at is not None:
            stream[at] &= ~np.uint8(hm.CARRIER)
        if i % 3 == 0:
            behind[lost[i] + 1] &= ~np.uint8(hm.CARRIER)       # the first bit of the next segment: nothing is open there to lose
    d, m = both(2, 1, 24, require_carrier=True)
    frames = run_device(torch_dev, d, m, [stream, behind], "the carrier around closing flags")
    assert [p[0] for _, p, _ in frames[0]] == [i for i in range(24) if i % 3 == 2]
    assert [p[0] for _, p, _ in frames[1]] == list(range(24))
