"""The HDLC framer bank on the device (hrfd_hdlcgen_*) against the model of tests/hdlcgen_model.py, bit for bit and with no
tolerance: the counts first (n_bits, n_sent, dropped), then the rows of bits.  Every buffer lies between guard bytes, the rows
of bits at an odd stride from a misaligned base, the rows of records at a stride of their own, and what lies behind a row's
n_bits must stay as it was.  Channel counts 1, 3 and 65; the edge payloads of the CPU suite (runs of ones across lane, wave
and tile boundaries, runs of 4..11 ones ending at every bit of a lane, a stuffed zero directly in front of the closing flag,
a run that goes on into the check sequence, zeros, one byte); rows of several frames, rows of none, malformed records;
max_bits one short of, at and one above a row's length; 0 and 255 lead flags; the host entry; a call chained behind the copy
that fills its input; and the two closed loops on the device: Hdlc -> HdlcGen -> Hdlc (the digipeater) and HdlcGen ->
AfskGen -> Afsk -> Hdlc."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import hdlcgen_model as M
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

EDGES = M.edge_payloads()


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def run_device(torch_dev, g, rows, n_frames, what, flags=(12, 2, 3), max_bits=None, in_bytes=None, in_pad=4, residue=1, bits_pad=3,
               want_counts=True, stream=None):
    """process_device over rows of records (per channel a uint8 array) in_bytes + in_pad apart at a 4-byte aligned base, rows
    of bits at `residue` modulo 8, max_bits + bits_pad bytes apart; every buffer between guards, random bytes wherever no
    record lies.  Returns per channel (bits, n_sent, dropped) of the model"""
    torch, dev = torch_dev
    C = g.n
    assert len(rows) == C
    in_bytes = max(4, max(len(r) for r in rows)) if in_bytes is None else in_bytes
    in_stride = in_bytes + in_pad
    src = Guarded(torch_dev, in_stride * (C - 1) + in_bytes, 4, 8, 41)
    for c in range(C):
        k = min(len(rows[c]), in_bytes)
        src.host[src.off + c * in_stride:src.off + c * in_stride + k] = rows[c][:k]
    src.put(0, np.zeros(0, dtype=np.uint8))
    used = [src.host[src.off + c * in_stride:src.off + c * in_stride + in_bytes].copy() for c in range(C)]
    want = [M.row_bits(used[c], in_bytes, int(n_frames[c]), *flags, max_bits=M.MAX_BITS if max_bits is None else max_bits) for c in range(C)]
    max_bits = max(1, max(w[0].size for w in want)) if max_bits is None else max_bits
    d_nf = Guarded(torch_dev, 4 * C, 4, 8, 42)
    d_nf.put(0, np.asarray(n_frames, dtype=np.uint32))
    stride = max_bits + bits_pad
    g_bits = Guarded(torch_dev, stride * (C - 1) + max_bits, residue, 8, 43)
    g_n, g_sent, g_dropped = (Guarded(torch_dev, 4 * C, 4, 8, 44 + i) for i in range(3))
    torch.cuda.synchronize()
    g.process_device(src.ptr, in_stride, in_bytes, d_nf.ptr, g_bits.ptr, stride, max_bits, g_n.ptr, g_sent.ptr if want_counts else None,
                     g_dropped.ptr if want_counts else None, stream)
    torch.cuda.synchronize()
    u = lambda v: np.array(v, dtype=np.uint32)
    g_n.check(u([w[0].size for w in want]), f"{what}: n_bits")
    g_sent.check(u([w[1] for w in want]) if want_counts else None, f"{what}: n_sent")
    g_dropped.check(u([w[2] for w in want]) if want_counts else None, f"{what}: dropped")
    image = g_bits.host[g_bits.off:g_bits.off + g_bits.n].copy()
    for c in range(C):
        image[c * stride:c * stride + want[c][0].size] = want[c][0]
    g_bits.check(image, f"{what}: the bits, or the bytes behind a row's n_bits")
    src.check(None, f"{what}: the records")
    d_nf.check(None, f"{what}: n_frames")
    return want


def spread(items, C):
    """every item on some channel: channel c takes items c, c + C, .."""
    return [[items[i] for i in range(c, len(items), C)] or [items[c % len(items)]] for c in range(C)]


# 1. the edge payloads at the three channel counts: every one at a frame's first bit, alone and behind other frames
@pytest.mark.parametrize("C", [1, 3, 65])
def test_edge_payloads(torch_dev, C):
    g = api.HdlcGen(C, device=0)
    per = spread([p for _, p in EDGES], C)
    want = run_device(torch_dev, g, [M.record_row(p) for p in per], [len(p) for p in per], f"edges on {C} channels")
    for c in range(C):
        assert want[c][1] == len(per[c]) and np.array_equal(want[c][0], api.hdlc_encode(per[c]))


# 2. the rows of bits at every residue: the single bytes in front of and behind the dword stores
@pytest.mark.parametrize("residue", range(8))
def test_rows_of_bits_at_every_residue(torch_dev, residue):
    g = api.HdlcGen(3, device=0)
    per = [[b"\xff" * 65, b"ab"], [b"\x1f" * (3 + residue)], [b"\0", b"\xfe\xff\xff\x01", b"xyz"]]
    for pad in (0, 1):
        run_device(torch_dev, g, [M.record_row(p) for p in per], [2, 1, 3], f"residue {residue}, pad {pad}", residue=residue, bits_pad=pad)


# 3. rows of several frames, of none, and with a malformed record in the middle
def test_rows_and_counts(torch_dev):
    C = 65
    g = api.HdlcGen(C, device=0)
    per = [M.random_payloads(100 + c, 1 + c % 5, 1, 70) for c in range(C)]
    rows = [M.record_row(p) for p in per]
    n_frames = [len(p) for p in per]
    for c in range(0, C, 7):
        n_frames[c] = 0                                    # a row of records that does not count
    for c in range(1, C, 7):
        n_frames[c] += 3                                   # more than the row holds: the walk meets random bytes or the row's end
    rows[2] = M.record_row([b"good", b"", b"never"])                   # n_payload 0
    rows[3] = M.record_row([b"good", b"\x33" * 1022, b"never"])        # n_payload 1022
    n_frames[2] = n_frames[3] = 3
    want = run_device(torch_dev, g, rows, n_frames, "rows and counts", in_bytes=max(len(r) for r in rows[:2] + rows[4:]))
    assert want[0][0].size == 0 and want[2][1:] == (1, 2) and want[3][1:] == (1, 2)
    assert sum(w[1] for w in want) > 100
    # a record that runs past in_bytes: the row is cut inside the third record's payload, at its header, and at the second's
    per = [[b"one1", b"two22222", b"three"]] * 3
    rows = [M.record_row(p) for p in per]
    for in_bytes, sent in ((12 + 16 + 12, 2), (12 + 16 + 4, 2), (12 + 12, 1), (8, 0), (4, 0)):
        want = run_device(torch_dev, api.HdlcGen(3, device=0), rows, [3, 3, 3], f"in_bytes {in_bytes}", in_bytes=in_bytes, want_counts=in_bytes != 8)
        assert [w[1] for w in want] == [sent] * 3


# 4. max_bits one short of, at and one above a row's exact length, for a row of one, two and three frames
def test_max_bits_around_the_exact_length(torch_dev):
    g = api.HdlcGen(3, device=0)
    batch = [b"\xff" * 9, b"hello", b"\xff" * 300]
    rows = [M.record_row(batch), M.record_row(batch[1:]), M.record_row(batch[2:] + batch[:1])]
    for k in (1, 2, 3):
        exact = M.encode(batch[:k])[0].size
        for max_bits, sent in ((exact - 1, k - 1), (exact, k), (exact + 1, k)):
            want = run_device(torch_dev, g, rows, [3, 2, 2], f"{k} frames, max_bits {max_bits}", max_bits=max_bits)
            assert want[0][1:] == (sent, 3 - sent)
    want = run_device(torch_dev, g, rows, [3, 2, 2], "max_bits 1", max_bits=1)
    assert [w[0].size for w in want] == [0, 0, 0]


# 5. the flag counts
@pytest.mark.parametrize("flags", [(0, 1, 1), (255, 255, 255), (1, 7, 2)])
def test_set_flags(torch_dev, flags):
    g = api.HdlcGen(3, device=0)
    g.set_flags(*flags)
    per = [[b"\xff" * 64, b"q"], [b"zz"], [b"a", b"b", b"\xf8" * 9]]
    want = run_device(torch_dev, g, [M.record_row(p) for p in per], [2, 1, 3], f"flags {flags}", flags=flags)
    for c in range(3):
        assert np.array_equal(want[c][0], api.hdlc_encode(per[c], *flags))
    assert g.max_bits(2, 65) == M.bound(2, 65, *flags)
    g.set_flags()
    run_device(torch_dev, g, [M.record_row(p) for p in per], [2, 1, 3], "the default flags again")
    h = api.HdlcGen(3, *flags, device=0)
    run_device(torch_dev, h, [M.record_row(p) for p in per], [2, 1, 3], f"flags {flags} at create", flags=flags)


# 6. the blocking host entry
def test_the_host_entry(torch_dev):
    g = api.HdlcGen(3, device=0)
    per = [[p for _, p in EDGES[:12]], [], [b"only"]]
    bits, (n_sent, dropped) = g.process(per, want_counts=True)
    assert n_sent.tolist() == [12, 0, 1] and dropped.tolist() == [0, 0, 0]
    for c in range(3):
        assert np.array_equal(bits[c], api.hdlc_encode(per[c]) if per[c] else np.zeros(0, dtype=np.uint8))
    rows, n_frames = g.pack(per)
    # bytes behind n_bits come back as they went up: process_rows sends zeros
    out, (n_bits, n_sent, dropped) = g.process_rows(rows, n_frames, 500)
    want = [M.row_bits(rows[c], rows.shape[1], n_frames[c], max_bits=500) for c in range(3)]
    assert n_bits.tolist() == [w[0].size for w in want] and n_sent.tolist() == [w[1] for w in want] and dropped.tolist() == [w[2] for w in want]
    for c in range(3):
        assert np.array_equal(out[c, :n_bits[c]], want[c][0]) and not out[c, n_bits[c]:].any()
    assert dropped[0] > 0


# 7. chained on one stream behind the copy that fills its input
def test_chained_on_one_stream_behind_the_copy(torch_dev):
    torch, dev = torch_dev
    C = 5
    g = api.HdlcGen(C, device=0)
    per = [M.random_payloads(70 + c, 3, 1, 300) for c in range(C)]
    rows, n_frames = g.pack(per)
    max_bits = max(g.max_bits(3, sum(map(len, p))) for p in per)
    host = torch.from_numpy(rows.copy()).pin_memory()
    host_n = torch.from_numpy(n_frames.view(np.int32).copy()).pin_memory()
    d_rows = torch.zeros(rows.shape, dtype=torch.uint8, device=dev)
    d_nf = torch.zeros(C, dtype=torch.int32, device=dev)
    d_bits = torch.full((C, max_bits), 7, dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((3, C), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_rows.copy_(host, non_blocking=True)
        d_nf.copy_(host_n, non_blocking=True)
    g.process_device(d_rows.data_ptr(), rows.shape[1], rows.shape[1], d_nf.data_ptr(), d_bits.data_ptr(), max_bits, max_bits,
                     d_cnt[0].data_ptr(), d_cnt[1].data_ptr(), d_cnt[2].data_ptr(), st.cuda_stream)
    st.synchronize()
    cnt, bits = d_cnt.cpu().numpy(), d_bits.cpu().numpy()
    assert (cnt[1] == 3).all() and (cnt[2] == 0).all()
    for c in range(C):
        want = api.hdlc_encode(per[c])
        assert cnt[0][c] == want.size and np.array_equal(bits[c, :want.size], want) and (bits[c, want.size:] == 7).all()


# 8. the digipeater: the frames a receive bank found are said again where they lie, and heard again by a second one
def test_closed_loop_hdlc_to_framer_to_hdlc(torch_dev):
    """Hdlc.process_device -> HdlcGen.process_device -> Hdlc.process_device (a second handle) on one stream: the framer reads
    the first bank's rows of records and its d_n_frames as they are, end_bit and fcs included, and no byte visits the host"""
    torch, dev = torch_dev
    C = 65
    per = [M.random_payloads(200 + c, 1 + c % 4, 1, 60) + ([EDGES[c % len(EDGES)][1]] if len(EDGES[c % len(EDGES)][1]) <= 400 else []) for c in range(C)]
    sent = [api.hdlc_encode(p, 3, 1, 2) for p in per]
    n_in = max(s.size for s in sent)
    hd1, gen, hd2 = api.Hdlc(C, 1, 1021, device=0), api.HdlcGen(C, 2, 1, 2, device=0), api.Hdlc(C, 1, 1021, device=0)
    bits_in = np.zeros((C, n_in), dtype=np.uint8)
    for c in range(C):
        bits_in[c, :sent[c].size] = sent[c]
    d_in = torch.from_numpy(bits_in).to(dev)
    d_n_in = torch.from_numpy(np.array([s.size for s in sent], dtype=np.int32)).to(dev)
    ob = hd1.max_out(n_in)
    mid_bits = max(gen.max_bits(len(p), sum(map(len, p))) for p in per)
    ob2 = hd2.max_out(mid_bits)
    d_rec = torch.zeros((C, ob), dtype=torch.uint8, device=dev)
    d_mid = torch.zeros((C, mid_bits), dtype=torch.uint8, device=dev)
    d_rec2 = torch.zeros((C, ob2), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((9, C), dtype=torch.int32, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    p = lambda i: d_cnt[i].data_ptr()
    hd1.process_device(d_in.data_ptr(), n_in, d_n_in.data_ptr(), n_in, d_rec.data_ptr(), ob, ob, p(0), p(1), p(2), st.cuda_stream)
    gen.process_device(d_rec.data_ptr(), ob, ob, p(0), d_mid.data_ptr(), mid_bits, mid_bits, p(3), p(4), p(5), st.cuda_stream)
    hd2.process_device(d_mid.data_ptr(), mid_bits, p(3), mid_bits, d_rec2.data_ptr(), ob2, ob2, p(6), p(7), p(8), st.cuda_stream)
    st.synchronize()
    cnt, mid, rec2 = d_cnt.cpu().numpy(), d_mid.cpu().numpy(), d_rec2.cpu().numpy()
    for c in range(C):
        assert cnt[0][c] == cnt[4][c] == cnt[6][c] == len(per[c]) and cnt[5][c] == cnt[7][c] == cnt[8][c] == 0, f"channel {c}"
        assert np.array_equal(mid[c, :cnt[3][c]], api.hdlc_encode(per[c], 2, 1, 2)), f"channel {c}: the bits said again"
        assert [q for _, q, _ in api.Hdlc.parse(rec2[c], cnt[6][c])] == per[c], f"channel {c}"


# 9. what the bank is for: UI frames from the framer through the modem and back
def test_closed_loop_framer_to_afsk_and_back(torch_dev):
    """HdlcGen -> AfskGen.send_all -> AfskGen / Afsk / Hdlc chained on one stream: the payloads of ax25_ui_frame come back"""
    torch, dev = torch_dev
    C, B = 5, 16
    per = [[api.ax25_ui_frame("APRS", f"N0CALL-{c}", b"!4903.50N/07201.75W-ch%d" % c, path=["WIDE1-1"]),
            api.ax25_ui_frame(("CQ", 0), ("DL1ABC", c), bytes([0xFF] * (c + 1)))] for c in range(C)]
    per[3] = []                                            # a channel with nothing to say: nothing is queued on it
    framer, gen, dec, hd = api.HdlcGen(C, device=0), api.AfskGen(C, device=0), api.Afsk(C, device=0), api.Hdlc(C, device=0)
    gen.send_all(framer, per, start=100)
    assert [gen.pending(c)[0] for c in range(C)] == [1, 1, 1, 0, 1]
    assert max(gen.pending(c)[1] for c in range(C)) < 512 * B - 200
    with pytest.raises(ValueError):
        gen.send_all(framer, [[bytes(1021)]] * C)          # 8184 data bits and the flags pass 8192: refused, nothing queued
    assert [gen.pending(c)[0] for c in range(C)] == [1, 1, 1, 0, 1]
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
    cnt, out = d_cnt.cpu().numpy(), d_out.cpu().numpy()
    for c in range(C):
        got = [p for _, p, _ in api.Hdlc.parse(out[c], cnt[0][c])]
        assert got == per[c], f"channel {c}"
        if got:
            assert api.ax25_parse(got[0])["src"] == ("N0CALL", c) and api.ax25_parse(got[1])["info"] == bytes([0xFF] * (c + 1))


# 10. what depends on a handle
def test_refusals_that_need_a_handle(torch_dev):
    g = api.HdlcGen(3, device=0)
    with pytest.raises(api.HrfdError, match="n_between 0"):
        g.set_flags(12, 0, 3)
    g.set_flags(255, 255, 255)
    with pytest.raises(api.HrfdError, match="more than one call"):
        g.max_bits(500, 500 * 200)
    # rows of bits that overlap the records: only the handle knows how many rows there are
    with pytest.raises(api.HrfdError, match="overlaps"):
        g.process_device(0x10000, 64, 64, 0x1000, 0x10000 + 3 * 64 - 1, 100, 100, 0x2000, None, None)
