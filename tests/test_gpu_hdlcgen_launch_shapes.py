"""The HDLC framer bank (k_hdlcgen) in the launch shapes and payloads its own suite does not reach, tolerance 0 everywhere.

F1. payloads of 253 .. 1021 bytes that are not all ones: the per-byte CRC term at every distance from the check sequence, the
    check sequence across a tile edge, a run of ones carried from tile to tile, `len` summed over tiles of different lengths
F2. the most `ob` holds in LDS: 255 flags in front of the longest frame, max_bits one short of, at and above the exact length
F3. a row that fills max_bits = 2^20, one whose frames all fit, one of 4000 frames
F4. 1300 channels, and 65 536: the most the bank takes
F5. rows of records and rows of bits more than 4 GiB apart
F6. the digipeater loop with frames of 1021 bytes

Everything but F4's second half, F5 and F6 goes through tests/test_gpu_hdlcgen.py's run_device, which compares with the model
of tests/hdlcgen_model.py between guards and at odd strides; F1 also holds the C slow loop (api.hdlc_encode_c) against the
same bits.  The payloads are built in tests/test_key_launch_shapes_model.py, which states without a device what each of them
reaches; the same figures are asserted here next to the calls."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import hdlcgen_model as M
from tests import test_gpu_hdlcgen as tg
from tests import test_key_launch_shapes_model as ks
from tests.test_gpu_bank_launch_shapes import big, equal, far_equals_dense, far_rows, host, torch_dev, zeros      # noqa: F401

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- F1
@pytest.mark.parametrize("C", [3, 65])
def test_long_payloads_that_are_not_all_ones(torch_dev, C):
    """F1: on 3 channels every row holds 15 of the 45 payloads one behind the other, on 65 every payload stands alone"""
    items = ks.f1_items()
    assert len(items) == 3 * len(ks.F1_N) == 45 and sorted({ks.tiles(len(p)) for p in items}) == [1, 2, 3, 4]
    assert [ks.fcs_lanes(n) for n in (255, 511, 767)] == [[(t, 255), (t + 1, 0)] for t in range(3)]
    for n, (_, _, crossing) in zip(ks.F1_N, ks.f1_payloads()):
        edge = ks.f1_edge(n)
        assert edge is None or 7 <= ks.run_across(crossing, edge)[1] <= 11
    per = tg.spread(items, C)
    assert all(len(p) == (15 if C == 3 else 1) for p in per)
    want = tg.run_device(torch_dev, api.HdlcGen(C, device=0), [M.record_row(p) for p in per], [len(p) for p in per], f"F1 on {C} channels")
    for c in range(C):
        assert want[c][1:] == (len(per[c]), 0)
        slow = api.hdlc_encode_c(per[c])
        assert np.array_equal(want[c][0], slow), f"channel {c}: the C slow loop differs at {np.flatnonzero(want[c][0][:slow.size] != slow[:want[c][0].size])[:4]}"


# ---------------------------------------------------------------- F2
@pytest.mark.parametrize("flags", ks.F2_FLAGS, ids=["255_255_255", "0_255_1"])
def test_the_most_ob_holds(torch_dev, flags):
    """F2: ob starts with the flags in front of a frame: 255 of them and 9819 bits of 1021 x 0xFF, lead and between alike"""
    g = api.HdlcGen(3, device=0)
    g.set_flags(*flags)
    per = ks.f2_rows()
    rows, n_frames = [M.record_row(p) for p in per], [len(p) for p in per]
    exact = M.encode(per[0], *flags)[0].size
    assert exact == 8 * sum(flags) + 2 * 9819 and M.frame_bits(ks.FF).size == 9819
    assert 8 * max(flags[:2]) + 9819 == 8 * ks.HDLCGEN_MAX_FLAGS + 9819 <= 8 * api.HDLCGEN_MAX_FLAGS + ks.HDLCGEN_MAX_FRAME
    for max_bits, sent in ((exact, 2), (exact - 1, 1), (exact + 1, 2)):
        want = tg.run_device(torch_dev, g, rows, n_frames, f"F2, flags {flags}, max_bits {max_bits}", flags=flags, max_bits=max_bits)
        assert want[0][1:] == (sent, 2 - sent) and want[1][1:] == (1, 0) and want[2][1:] == (2, 0)
        for c in range(3):
            slow = api.hdlc_encode_c(per[c], *flags, max_bits=max_bits)
            assert np.array_equal(want[c][0], slow), f"channel {c}"


# ---------------------------------------------------------------- F3
def test_a_row_that_fills_max_bits(torch_dev):
    """F3: max_bits = 2^20.  Channel 0's 106 frames of 1021 bytes all fit (106 is the most max_bits() promises), channel 1
    has 130 and drops those that no longer fit, channel 2 walks 4000 records"""
    per = ks.f3_rows()
    assert tuple(len(p) for p in per) == ks.F3_FRAMES
    g = api.HdlcGen(3, device=0)
    assert g.max_bits(106, 106 * 1021) == M.bound(106, 106 * 1021) <= M.MAX_BITS == api.HDLCGEN_MAX_BITS
    with pytest.raises(api.HrfdError, match="more than one call"):
        g.max_bits(107, 107 * 1021)
    in_bytes = 130 * (8 + 1024)
    rows = [M.record_row(p) for p in per]
    assert max(r.size for r in rows) == rows[1].size == in_bytes
    want = tg.run_device(torch_dev, g, rows, list(ks.F3_FRAMES), "F3", max_bits=M.MAX_BITS, in_bytes=in_bytes, bits_pad=1)
    model = ks.f3_want()
    for c in range(3):
        assert want[c][1:] == model[c][1:] and np.array_equal(want[c][0], model[c][0])
    assert want[0][1:] == (106, 0) and want[2][1:] == (4000, 0)
    n_bits, sent, dropped = want[1][0].size, want[1][1], want[1][2]
    assert sent + dropped == 130 and dropped > 0 and M.MAX_BITS - ks.HDLCGEN_MAX_FRAME - 8 * (2 + 3) < n_bits <= M.MAX_BITS


# ---------------------------------------------------------------- F4
def test_1300_channels(torch_dev):
    """F4: 1..3 short frames a channel"""
    C = 1300
    per = [M.random_payloads(5000 + c, 1 + c % 3, 1, 40) for c in range(C)]
    want = tg.run_device(torch_dev, api.HdlcGen(C, device=0), [M.record_row(p) for p in per], [len(p) for p in per], "F4, 1300 channels")
    assert [w[1] for w in want] == [1 + c % 3 for c in range(C)] and sum(w[2] for w in want) == 0


F4_MOST = 65536
F4_POOL = 61


def test_the_most_channels(torch_dev):
    """F4: 65 536 channels, the limit of the channel count and the grid's bound.  Every channel takes one of 61 payloads of
    1..8 bytes, a few take none; the model frames the 61 once and every channel's counts and bits are compared against its
    own, as arrays.  The rows lie dense between guard rows"""
    torch, dev = torch_dev
    C = F4_MOST
    with pytest.raises(Exception, match="channel"):
        api.HdlcGen(C + 1, device=0)
    rng = np.random.default_rng(65)
    pool = [bytes(rng.integers(0, 256, 1 + i % 8, dtype=np.uint8)) for i in range(F4_POOL - 1)] + [b"\xff" * 8]
    framed = [M.encode([p]) for p in pool]
    max_bits = max(b.size for b, _, _ in framed)
    assert max_bits == framed[-1][0].size <= M.bound(1, 8) and all(s == 1 for _, s, _ in framed)
    which = rng.integers(0, F4_POOL, size=C)
    n_frames = np.ones(C, dtype=np.uint32)
    n_frames[rng.choice(C, size=40, replace=False)] = 0
    n_frames[[0, C - 1]] = 1                                   # the first and the last channel speak
    in_bytes = 16
    recs = np.stack([np.pad(M.record_row([p]), (0, in_bytes - M.record_row([p]).size)) for p in pool])
    image = np.zeros((F4_POOL, max_bits), dtype=np.uint8)
    fill = 0xA5
    image[:] = fill
    for i, (b, _, _) in enumerate(framed):
        image[i, :b.size] = b
    sizes = np.array([b.size for b, _, _ in framed], dtype=np.uint32)
    want_bits = np.where((n_frames != 0)[:, None], image[which], np.uint8(fill))
    want_n = np.where(n_frames != 0, sizes[which], 0).astype(np.uint32)
    # one guard row in front of and behind everything the kernel writes
    d_in = torch.from_numpy(recs[which]).to(dev)
    d_nf = torch.from_numpy(n_frames.view(np.int32)).to(dev)
    d_bits = torch.full((C + 2, max_bits), fill, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((3, C + 2), -7, dtype=torch.int32, device=dev)
    g = api.HdlcGen(C, device=0)
    torch.cuda.synchronize()
    g.process_device(d_in.data_ptr(), in_bytes, in_bytes, d_nf.data_ptr(), d_bits[1].data_ptr(), max_bits, max_bits, d_cnt[0, 1:].data_ptr(),
                     d_cnt[1, 1:].data_ptr(), d_cnt[2, 1:].data_ptr())
    torch.cuda.synchronize()
    bits, cnt = d_bits.cpu().numpy(), d_cnt.cpu().numpy()
    assert (cnt[:, 0] == -7).all() and (cnt[:, -1] == -7).all() and (bits[0] == fill).all() and (bits[-1] == fill).all(), "the guards"
    equal(cnt[0, 1:-1].view(np.uint32), want_n, "n_bits")
    equal(cnt[1, 1:-1].view(np.uint32), n_frames, "n_sent")
    equal(cnt[2, 1:-1].view(np.uint32), np.zeros(C, dtype=np.uint32), "dropped")
    equal(bits[1:-1], want_bits, "the bits, or the bytes behind a row's n_bits")
    assert torch.equal(d_in.cpu(), torch.from_numpy(recs[which])), "the records"
    # the model's bits are the slow loop's as well
    for i in (0, 7, F4_POOL - 1):
        assert np.array_equal(framed[i][0], api.hdlc_encode_c([pool[i]]))


# ---------------------------------------------------------------- F5
def test_far_rows_hdlcgen(torch_dev, big):
    """F5: the rows of records and the rows of bits each more than 4 GiB apart; frames of three tiles on both rows"""
    per = [M.random_payloads(81, 2, 600, 700), M.random_payloads(82, 3, 300, 700)]
    n_frames = np.array([len(p) for p in per], dtype=np.uint32)
    recs = [M.record_row(p) for p in per]
    in_bytes = max(r.size for r in recs)
    filler = np.random.default_rng(83).integers(0, 256, size=(2, in_bytes), dtype=np.uint8)
    for c in range(2):
        filler[c, :recs[c].size] = recs[c]
    model = [M.row_bits(filler[c], in_bytes, n_frames[c]) for c in range(2)]
    max_bits = max(m[0].size for m in model) + 5
    assert all(ks.tiles(len(p)) == 3 for p in per[0]) and [m[1] for m in model] == [2, 3]

    def call(far):
        torch = torch_dev[0]
        g = api.HdlcGen(2, device=0)
        src, out = far_rows(torch_dev, in_bytes, 84, filler, far), far_rows(torch_dev, max_bits, 85, None, far)
        assert src.stride % 4 == 0 and (not far or min(src.stride, out.stride) > 1 << 32)
        d_nf = torch.from_numpy(n_frames.view(np.int32)).to(torch_dev[1])
        cnt = zeros(torch_dev, (3, 2), "int32")
        torch.cuda.synchronize()
        g.process_device(src.ptr, src.stride, in_bytes, d_nf.data_ptr(), out.ptr, out.stride, max_bits, cnt[0].data_ptr(), cnt[1].data_ptr(),
                         cnt[2].data_ptr())
        torch.cuda.synchronize()
        src.check("the records", unchanged=True)
        return {"bits": out.check("the bits"), "counts": host(cnt)[0], "before": out.rows.copy()}

    got = far_equals_dense(torch_dev, call, "HdlcGen")
    assert got["counts"].tolist() == [[m[0].size for m in model], [2, 3], [0, 0]]
    for c in range(2):
        n = model[c][0].size
        equal(got["bits"][c, :n], model[c][0], f"the far rows against the model, channel {c}")
        equal(got["bits"][c, n:], got["before"][c, n:], f"the bytes behind n_bits, channel {c}")
    assert not np.array_equal(got["bits"][0, :4000], got["bits"][1, :4000])


# ---------------------------------------------------------------- F6
def test_closed_loop_with_the_longest_frames(torch_dev):
    """F6: Hdlc -> HdlcGen -> Hdlc on one stream, as test_gpu_hdlcgen's digipeater, with frames of 1021 bytes, four tiles each,
    on 3 channels: 1021 x 0xFF among them, and a frame of one byte between two long ones"""
    torch, dev = torch_dev
    C = 3
    per = [M.random_payloads(90, 2, 1021, 1021), [ks.FF, b"\x7e", M.random_payloads(91, 1, 1021, 1021)[0]], [M.random_payloads(92, 2, 1021, 1021)[1]]]
    assert all(len(p) in (1, 1021) for q in per for p in q) and ks.tiles(1021) == 4
    sent = [M.encode(p, 3, 1, 2)[0] for p in per]
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
    d_mid = torch.full((C, mid_bits), 9, dtype=torch.uint8, device=dev)
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
        again = M.encode(per[c], 2, 1, 2)[0]
        assert cnt[3][c] == again.size and np.array_equal(mid[c, :again.size], again), f"channel {c}: the bits said again"
        assert (mid[c, again.size:] == 9).all(), f"channel {c}: the bytes behind n_bits"
        assert np.array_equal(again, api.hdlc_encode_c(per[c], 2, 1, 2)), f"channel {c}: the C slow loop"
        assert [q for _, q, _ in api.Hdlc.parse(rec2[c], cnt[6][c])] == per[c], f"channel {c}"
