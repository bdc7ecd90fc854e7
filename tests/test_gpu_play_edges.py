"""hrfd_play_* at its edges: k_play's two paths (16-byte groups without a wrap on a 16-aligned layout, the byte loop for
everything else) against tests.toolsupport.playback_model -- DataProvider::retrieveIqDataFromBuffer as index arithmetic --
over every small image length, start and count, every destination layout, every placement of the wrap, a reload, and two
calls on two caller streams.  Bit-exact."""
import numpy as np
import pytest

from hackrfdiags_amd import api, synth
from tests import toolsupport as T

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A


def _model(image, starts, n):
    """playback_model for every channel: (want [C, n], the positions after the call)"""
    rows = [T.playback_model(image, int(s), n) for s in starts]
    return np.stack([r[0] for r in rows]), [r[1] for r in rows]


def _set_positions(p, starts):
    for c, s in enumerate(starts):
        p.set_position(int(s), c)


def _get_device(p, torch, n, stride, offset=0, stream=None):
    """one hrfd_play_get_device into a sentinel-filled buffer: -> (rows [C, n], the whole buffer) on the host"""
    size = offset + p.C * stride + 64
    buf = torch.full((size,), SENTINEL, dtype=torch.int8, device="cuda:0")
    torch.cuda.synchronize()
    p.get_device(buf.data_ptr() + offset, stride, n, stream)
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    rows = np.stack([whole[offset + c * stride: offset + c * stride + n] for c in range(p.C)])
    return rows, whole


def _assert_guards(whole, offset, stride, n, C):
    keep = np.ones(whole.size, dtype=bool)
    for c in range(C):
        keep[offset + c * stride: offset + c * stride + n] = False
    assert (whole[keep] == SENTINEL).all(), "bytes outside the rows were written"


LENGTHS = list(range(1, 41)) + [63, 64, 65]


@pytest.mark.parametrize("through", ["get", "get_device"])
def test_small_images_every_start_every_count(through):
    """image lengths 1..40, 63, 64, 65 (shorter than one 16-byte group, equal to whole groups, one off), EVERY start (one
    channel per start, at least three), 1..50 bytes per channel, and the same call a second time from the carried position.
    hrfd_play_get stages on a 16-aligned layout (the group path where a group fits); get_device here writes rows `count`
    bytes apart (the byte loop unless count is a multiple of 16)"""
    import torch
    for L in LENGTHS:
        image = synth.lcg_bytes(1000 + L, L)
        C = max(L, 3)
        p = api.Play(C)
        p.load(image)
        for n in range(1, 51):
            starts = [c % L for c in range(C)]
            _set_positions(p, starts)
            for call in range(2):
                want, after = _model(image, starts, n)
                if through == "get":
                    got = p.get(n)
                else:
                    got, whole = _get_device(p, torch, n, n)
                    _assert_guards(whole, 0, n, n, C)
                assert (got == want).all(), (L, n, call)
                assert [p.position(c) for c in range(C)] == after, (L, n, call)
                starts = after
        p.close()


def test_get_device_layouts_and_guard_bytes():
    """d_out 0..15 bytes into a larger buffer, rows a multiple of 16 apart and not, counts that are no multiple of 16 on
    the aligned layout (the last group of a row is partial): the rows equal the model and every byte before, between and
    behind them keeps its sentinel"""
    import torch
    L = 301
    image = synth.lcg_bytes(77, L)
    C = 3
    p = api.Play(C)
    p.load(image)
    starts = [0, 290, 150]                                  # channel 1 wraps in its first group
    for offset in range(16):
        for stride, n in [(64, 64), (64, 50), (80, 33), (96, 81), (67, 67), (67, 50), (50, 50), (49, 48), (112, 100), (17, 16),
                          (16, 16), (32, 17), (16, 1), (1, 1)]:
            _set_positions(p, starts)
            want, after = _model(image, starts, n)
            got, whole = _get_device(p, torch, n, stride, offset)
            assert (got == want).all(), (offset, stride, n)
            _assert_guards(whole, offset, stride, n, C)
            assert [p.position(c) for c in range(C)] == after
    with pytest.raises(api.HrfdError):
        p.get_device(1 << 20, 15, 16)                       # rows that overlap: refused before anything is launched
    p.close()


@pytest.mark.parametrize("through", ["get", "get_device_unaligned"])
def test_wrap_placement(through):
    """a 16-byte group that ends exactly at the image's end, one and two bytes before it and behind it, for each of the four
    groups of a 64-byte call, image lengths of every residue modulo 4: every (length % 4, start % 4) pair, so every shift
    of the unaligned dword reads against the 8 pad bytes behind the image; two calls, the second from the carried position"""
    import torch
    seen = set()
    for L in (300, 301, 302, 303):
        image = synth.lcg_bytes(300 + L, L)
        starts = [L - 16 * (g + 1) + d for g in range(4) for d in (-2, -1, 0, 1, 2)]
        seen |= {(L % 4, s % 4) for s in starts}
        p = api.Play(len(starts))
        p.load(image)
        _set_positions(p, starts)
        for call in range(2):
            want, after = _model(image, starts, 64)
            if through == "get":
                got = p.get(64)
            else:
                got, whole = _get_device(p, torch, 64, 67, 3)
                _assert_guards(whole, 3, 67, 64, p.C)
            assert (got == want).all(), (L, call, np.argwhere(got != want)[:4])
            assert [p.position(c) for c in range(p.C)] == after
            starts = after
        p.close()
    assert len(seen) == 16


def test_reload_replaces_the_image_and_restarts_every_position():
    long_image, short_image = synth.lcg_bytes(5, 1000), synth.lcg_bytes(6, 10)
    C = 3
    p = api.Play(C)
    with pytest.raises(api.HrfdError):
        p.set_position(0)                                   # nothing loaded
    p.load(long_image)
    _set_positions(p, [999, 500, 17])
    want, after = _model(long_image, [999, 500, 17], 40)
    assert (p.get(40) == want).all()
    p.load(short_image)                                     # DataProvider::loadIqFile: the index restarts
    assert [p.position(c) for c in range(C)] == [0, 0, 0]
    want, after = _model(short_image, [0, 0, 0], 37)
    assert (p.get(37) == want).all() and [p.position(c) for c in range(C)] == after
    for bad in (10, 11, 999, 0xFFFFFFFE):                   # at or beyond the NEW length (999 was fine for the old image)
        with pytest.raises(api.HrfdError):
            p.set_position(bad, 1)
        with pytest.raises(api.HrfdError):
            p.set_position(bad)
    with pytest.raises(api.HrfdError):
        p.set_position(0, C)
    assert [p.position(c) for c in range(C)] == after
    p.set_position(9)                                       # HRFD_ALL_CHANNELS
    assert [p.position(c) for c in range(C)] == [9, 9, 9]
    want, after = _model(short_image, [9, 9, 9], 5)
    assert (p.get(5) == want).all() and [p.position(c) for c in range(C)] == after
    p.close()


def test_two_calls_on_two_caller_streams_keep_their_own_positions():
    """two hrfd_play_get_device calls back to back on two caller streams, the first stream held up behind a large fill and
    its k_play long enough (64 MiB per channel) to be still running when the second call hands over ITS positions: the
    first kernel must go on reading the positions of its own call.  Both outputs equal the model, compared on the device"""
    import torch
    dev = torch.device("cuda:0")
    L, C, n = 1000003, 4, 64 << 20
    image = synth.lcg_bytes(9, L)
    starts = [0, 1, 999999, 500001]
    p = api.Play(C)
    p.load(image)
    _set_positions(p, starts)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    out1 = torch.zeros((C, n), dtype=torch.int8, device=dev)
    out2 = torch.zeros((C, n), dtype=torch.int8, device=dev)
    ballast = torch.empty(1 << 30, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        ballast.fill_(1)
    p.get_device(out1.data_ptr(), n, n, s1.cuda_stream)
    p.get_device(out2.data_ptr(), n, n, s2.cuda_stream)
    torch.cuda.synchronize()
    mid = [(s + n) % L for s in starts]
    assert [p.position(c) for c in range(C)] == [(s + 2 * n) % L for s in starts]
    img = torch.from_numpy(image).to(dev)
    step = 8 << 20
    for out, first in ((out1, starts), (out2, mid)):
        for c in range(C):
            for lo in range(0, n, step):
                idx = (torch.arange(lo, lo + step, device=dev, dtype=torch.int64) + first[c]) % L
                assert torch.equal(out[c, lo:lo + step], img[idx]), (c, lo)
    p.close()
