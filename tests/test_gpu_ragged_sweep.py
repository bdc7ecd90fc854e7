"""k_rx_ragged (csrc/hrfd_rx_ragged.hip) over every commutator position: the walks of
tests/ragged_walks.py on the device against the CPU oracle, bit for bit -- the oracle itself is held to the compiled
reference on the same walks by tests/test_ragged_walks_model.py.  And k_rag_expand, the one-way conversion from ChanState to
RagState, behind every producer of ChanState and for the demodulators that are NOT active when the handle leaves the grid."""
import numpy as np
import pytest

from hackrfdiags_amd import api, synth
from tests import ragged_walks as W
from tests.ragged_walks import MODES, AM, FM, WBFM, LSB, USB

pytestmark = pytest.mark.gpu
BLK = synth.BLOCK_BYTES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path cannot run (and there is no CPU fallback)")


_WANT = {}


def _want(oracle, key, walk, xs):
    """the oracle's answers to a walk, per channel and block: computed once"""
    if key not in _WANT:
        _WANT[key] = [W.replay_outer(oracle.rx(), walk, xs[c], c) for c in range(xs.shape[0])]
    return _WANT[key]


def _apply(rx, events):
    """-> the call is a reduce_sample_rate call"""
    reduce = False
    for e in events:
        if e[0] == "mode":
            rx.set_mode(e[1])
        elif e[0] == "gain":
            rx.set_gain(e[1], e[2])
        elif e[0] == "reset":
            rx.reset_demod(e[1])
        elif e[0] == "threshold":
            rx.set_threshold(e[1])
        elif e[0] == "reduce":
            reduce = True
    return reduce


def _check_unit(got, want, where):
    """one block of one channel: got = (pcm row, n_pcm, magnitude, allowed, dump row); every sample and byte up to the
    count, zeros behind it (the entry clears its rows: nothing may be written past the count)"""
    pcm, n_pcm, mag, allowed, dump = got
    wp, wm, wa, wd = want
    assert int(n_pcm) == len(wp), (where, int(n_pcm), len(wp))
    assert (pcm[:len(wp)] == wp).all() and not pcm[len(wp):].any(), where
    assert int(mag) == wm and bool(allowed) == wa, (where, int(mag), wm, bool(allowed), wa)
    assert (dump[:len(wd)] == wd).all() and not dump[len(wd):].any(), where


def _run_outer(rx, walk, xs, want):
    """the walk on the handle, call by call, every channel against `want`"""
    C = xs.shape[0]
    off = k = held = 0
    for i, (bb, nb, events) in enumerate(walk):
        reduce = _apply(rx, events)
        x = xs[:, off:off + bb * nb]
        off += bb * nb
        if reduce:
            out = rx.reduce_sample_rate(x)
            assert out.shape == (C, api.iq256_capacity(bb))
            for c in range(C):
                wd = want[c][k][3]
                assert (out[c, :len(wd)] == wd).all() and not out[c, len(wd):].any(), (i, c)
        else:
            pcm, n_pcm, mag, allowed, dump = rx.process_block(x.reshape(C, nb, bb), nb, want_iq256=True)
            assert pcm.shape[2] == api.pcm_capacity(bb) and dump.shape[2] == api.iq256_capacity(bb)
            for c in range(C):
                for b in range(nb):
                    _check_unit((pcm[c, b], n_pcm[c, b], mag[c, b], allowed[c, b], dump[c, b]), want[c][k + b], (i, bb, c, b))
        k += nb
        held = (held + nb * (bb // 2)) % 8
        assert rx.pending_samples() == held, (i, bb, nb)
    return k


@pytest.mark.parametrize("mode", MODES)
def test_phase_sweep(oracle, mode):
    """every length class from every one of the 256 positions of a plain stream, a full block from position 255 (every
    LDS array and every output row at its capacity at once) and from 1, even classes at a non-zero position, a call
    that completes nothing: three channels with inputs of their own, everything exact after every call"""
    w = W.phase_sweep(mode)
    xs = W.sweep_inputs(w, 900 + mode)
    want = _want(oracle, ("sweep", mode), w, xs)
    rx = api.Rx(xs.shape[0])
    n = _run_outer(rx, w, xs, want)
    assert n == len(w.blocks)
    assert rx.debug_ragged() == (True, len(w))


@pytest.mark.parametrize("mode", MODES)
def test_gated_walk(oracle, mode):
    """eight channels, each with gates of its own: one front-end position, eight demodulator positions.  With a gain
    change, a mode excursion, resets of the active and of an inactive demodulator (the bank then switches to that one),
    a call that completes nothing, and reduce_sample_rate calls that advance the front end only"""
    w = W.gated_walk(mode, W.GATED_SEED + mode)
    xs = W.gated_inputs(w, 300 + mode)
    want = _want(oracle, ("gated", mode), w, xs)
    rx = api.Rx(w.n_channels)
    _run_outer(rx, w, xs, want)
    assert rx.debug_ragged()[0] is True
    shut = sum(1 for c in range(w.n_channels) for u in want[c] if u[2] is False)
    assert shut > 400                                       # the gates really closed (the oracle's `allowed`)


@pytest.mark.parametrize("mode", MODES)
def test_inner_sweep(oracle, mode):
    """the inner API: every class from every one of the 32 positions, resets at non-zero positions, 16384 samples from
    position 15 (512 PCM samples: the row's capacity); a bank of three"""
    w = W.inner_sweep(mode)
    xs = W.inner_inputs(w, 500 + mode)
    C = xs.shape[0]
    want = [W.replay_inner(oracle.demod(mode), w, xs[c]) for c in range(C)]
    d = api.Demod(mode, C)
    off = 0
    for i, (nbytes, _, events) in enumerate(w):
        if events:
            d.reset()
        got = d.process(xs[:, off:off + nbytes])
        off += nbytes
        assert got.shape[1] == w.blocks[i].n_pcm <= W.demod_pcm_capacity(nbytes), (i, nbytes)
        for c in range(C):
            assert (got[c] == want[c][i]).all(), (i, nbytes, c)


# ---------------------------------------------------------------- ChanState -> RagState
PAIRS = [(a, b) for a in MODES for b in MODES if a != b]
NAMES = {AM: "am", FM: "fm", WBFM: "wbfm", LSB: "lsb", USB: "usb"}


@pytest.mark.parametrize("producer", ["default", "block_kernels", "flow_kernels"])
@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{NAMES[a]}_to_{NAMES[b]}" for a, b in PAIRS])
def test_hand_over_to_the_ragged_kernel(oracle, a, b, producer):
    """The handle leaves the grid while B is active and A is not: k_rag_expand rebuilds A's pipelines from the input tail
    (fm_tail / am_tail / ssb_tail, ssb_i / ssb_q, the WBFM pipelines) that blocks of mode A left in ChanState on the
    streaming kernels -- the block kernels, the flow kernel's FIR modes and both WBFM kernels, each in turn -- and B's from
    what rag_store_chan wrote in an on-grid passage of 512 and 1536-byte blocks.  Then uneven blocks in B, the switch
    back to A off the grid, uneven blocks in A: every channel the sequential oracle's."""
    C = 3
    rx = api.Rx(C)
    if producer == "block_kernels":
        rx.debug_set_fir_flow(0)
        rx.debug_set_stream(0)
    elif producer == "flow_kernels":
        rx.debug_set_fir_flow(1)
        rx.debug_set_stream(1)
    # (mode, block bytes, blocks)
    seq = [(a, 32768, 4), (a, 32768, 3), (b, 32768, 2), (b, 512, 1), (b, 1536, 2), (b, 1000, 1), (b, 4098, 1), (b, 30, 2),
           (a, 2050, 1), (a, 18, 3), (a, 262142, 1), (a, 514, 2), (b, 1026, 1)]
    total = sum(bb * nb for _, bb, nb in seq)
    need = (total + BLK - 1) // BLK
    xs = np.stack([synth.make_input(kind, 40 + 10 * a + b + c, need)[:total] for c, kind in enumerate(("fmtone", "amtone", "lcg"))])
    orcs = [oracle.rx() for _ in range(C)]
    for h in [rx] + orcs:
        h.set_gain(a, 700.0)
        h.set_gain(b, 2100.0)                              # (LSB and USB share one demodulator: the later value holds)
    off = ragged = 0
    offgrid = False
    mode = None
    for i, (m, bb, nb) in enumerate(seq):
        if m != mode:
            mode = m
            for h in [rx] + orcs:
                h.set_mode(m)
        offgrid = offgrid or bb % 512 != 0
        on_ragged = offgrid or bb % 1024 != 0
        ragged += on_ragged
        x = xs[:, off:off + bb * nb].reshape(C, nb, bb)
        off += bb * nb
        pcm, n_pcm, mag, allowed, dump = rx.process_block(x, nb, want_iq256=on_ragged)
        for c in range(C):
            for k in range(nb):
                wp, wm, wa, wd = orcs[c].process(x[c, k])
                row = dump[c, k] if on_ragged else np.concatenate([wd, np.zeros(api.iq256_capacity(bb) - len(wd), np.int8)])
                _check_unit((pcm[c, k], n_pcm[c, k], mag[c, k], allowed[c, k], row), (wp, wm, wa, wd), (i, m, bb, c, k))
    assert rx.debug_ragged() == (True, ragged)


# ---------------------------------------------------------------- the device entry
def test_device_entry_with_a_padded_unaligned_stride(oracle):
    """one class of the phase sweep (257 samples: one or two PCM samples per block, 32 or 33 samples at 256 kS/s) from
    all 256 positions in one process_device call: a channel stride of n_blocks * block_bytes + 6 (padded, not 16-byte
    aligned), output rows of the documented capacities filled with a pattern in front -- it must survive behind every
    unit's count and around the buffers"""
    import torch
    C, nb, n = 3, 256, 257
    bb = 2 * n
    stride = nb * bb + 6
    kinds = ("fmtone", "lcg", "fullscale")
    xs = np.stack([W._stream(k, 70 + c, nb * bb) for c, k in enumerate(kinds)])
    dev = torch.device("cuda:0")
    raw = np.full((C, stride), 0x55, dtype=np.int8)
    raw[:, :nb * bb] = xs
    d_iq = torch.from_numpy(raw).to(dev)
    pcap, qcap, G = api.pcm_capacity(bb), api.iq256_capacity(bb), 64
    assert (pcap, qcap) == (2, 66)
    units = C * nb
    d_pcm = torch.full((units * pcap + 2 * G,), 0x5A5A, dtype=torch.int16, device=dev)
    d_dump = torch.full((units * qcap + 2 * G,), 0x5A, dtype=torch.int8, device=dev)
    d_np = torch.full((units + 2 * G,), -7, dtype=torch.int32, device=dev)
    d_mag = torch.full((units + 2 * G,), -7, dtype=torch.int32, device=dev)
    d_alw = torch.full((units + 2 * G,), 0x5A, dtype=torch.uint8, device=dev)
    rx = api.Rx(C)
    rx.set_mode(WBFM, 0)
    rx.set_mode(AM, 1)
    rx.set_mode(USB, 2)
    rx.process_device(d_iq.data_ptr(), stride, bb, nb, d_pcm.data_ptr() + 2 * G, d_np.data_ptr() + 4 * G, d_mag.data_ptr() + 4 * G,
                      d_alw.data_ptr() + G, d_dump.data_ptr() + G)
    assert rx.sync() == 0
    pcm, dump = d_pcm.cpu().numpy(), d_dump.cpu().numpy()
    n_pcm, mag, alw = d_np.cpu().numpy(), d_mag.cpu().numpy(), d_alw.cpu().numpy()
    for a, poison in ((pcm, 0x5A5A), (dump, 0x5A), (n_pcm, -7), (mag, -7), (alw, 0x5A)):
        assert (a[:G] == poison).all() and (a[-G:] == poison).all()
    pcm = pcm[G:-G].reshape(C, nb, pcap)
    dump = dump[G:-G].reshape(C, nb, qcap)
    n_pcm, mag, alw = (v[G:-G].reshape(C, nb) for v in (n_pcm, mag, alw))
    held = 0
    seen = set()
    for c, m in enumerate((WBFM, AM, USB)):
        o = oracle.rx()
        o.set_mode(m)
        for k in range(nb):
            wp, wm, wa, wd = o.process(xs[c, k * bb:(k + 1) * bb])
            assert n_pcm[c, k] == len(wp) and mag[c, k] == wm and bool(alw[c, k]) == wa, (c, k)
            assert (pcm[c, k, :len(wp)] == wp).all() and (pcm[c, k, len(wp):] == 0x5A5A).all(), (c, k)
            assert (dump[c, k, :len(wd)] == wd).all() and (dump[c, k, len(wd):] == 0x5A).all(), (c, k)
            seen.add((len(wp), len(wd)))
    assert seen == {(1, 64), (1, 66), (2, 66)}              # rows filled to their capacity (from position 255: both), and not
    assert rx.pending_samples() == (nb * n) % 8 == held
    assert (d_iq.cpu().numpy() == raw).all()
