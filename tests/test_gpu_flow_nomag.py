"""k_rx_wbfm_flow<.., MAG = false>: a WBFM batch given no magnitude buffer, on a bank whose gates cannot close, leaves
the squelch magnitude out (rx_magnitude_unobservable, hrfd_rx_plan.h) -- and nothing a caller can see may differ.

Per shape two fresh handles over the same input: N passes no magnitude buffer, M passes one.  hrfd_rx_debug_mag_skipped
proves that N ran the new instantiation and M the old one (so the comparison is not of a kernel with itself); PCM, n_pcm
and signal_allowed are equal bit for bit over EVERY channel, eight channels (the four quiet ones among them) equal the
sequential CPU oracle exactly.  Then the state must carry over: threshold -30 on both, a second call over the next blocks
WITH a magnitude buffer -- N is back on the old kernel, the quiet channels' gates close, the gated pass follows -- equal
between N and M and equal to the oracle, which was fed both calls.  A third call on N without a buffer under the -30
threshold must not skip either.

Shapes: the smallest that reach each path (32 KiB is the shortest block the flow shape takes)."""
import pytest

from hackrfdiags_amd import api

pytestmark = pytest.mark.gpu

SHAPES = [
    (256, 2, 32768),      # one run per channel, finished from LDS (the bench's shape)
    (256, 20, 32768),     # more than 16 blocks: the block slots are reused
    (8, 3, 32768),        # the plan cuts the channels into runs: the last workgroup to arrive finishes from P.present
    (9, 2, 262144),       # the bench's block size; 9 channels in a grid of whole rounds of 8: some workgroups are empty
]


def _input(C, B, bb, calls, dev):
    """[C][calls * B][bb] int8: the FM test signal, four channels replaced by noise in [-1, 1] (no signal)"""
    import torch
    from hackrfdiags_amd.synth_torch import BLOCK, make_fm_batch
    total = calls * B * bb
    x = make_fm_batch(C, (total + BLOCK - 1) // BLOCK, dev).reshape(C, -1)[:, :total].reshape(C, calls * B, bb).contiguous()
    quiet = sorted({1, C // 2, C - 2, C - 1})
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    x[torch.tensor(quiet, device=dev)] = torch.randint(-1, 2, (len(quiet), calls * B, bb), dtype=torch.int8, device=dev, generator=gen)
    return x, quiet


def _call(rx, xs, C, B, bb, want_mag):
    """one process_device call; -> (violations, pcm, n_pcm, allowed, magnitude | None) as numpy"""
    import torch
    dev = xs.device
    npcm = api.pcm_capacity(bb)
    pcm = torch.full((C, B, npcm), 77, dtype=torch.int16, device=dev)
    n_pcm = torch.full((C, B), 77, dtype=torch.int32, device=dev)
    alw = torch.full((C, B), 77, dtype=torch.uint8, device=dev)
    mag = torch.full((C, B), 77, dtype=torch.int32, device=dev) if want_mag else None
    torch.cuda.synchronize()                               # torch fills on its own stream, the handle runs on another
    rx.process_device(xs.data_ptr(), B * bb, bb, B, pcm.data_ptr(), d_n_pcm=n_pcm.data_ptr(),
                      d_magnitude=mag.data_ptr() if want_mag else None, d_allowed=alw.data_ptr())
    bad = rx.sync()
    return bad, pcm.cpu().numpy(), n_pcm.cpu().numpy(), alw.cpu().numpy(), mag.cpu().numpy() if want_mag else None


@pytest.mark.parametrize("C,B,bb", SHAPES, ids=[f"{c}x{b}x{n}" for c, b, n in SHAPES])
def test_no_magnitude_buffer_changes_nothing_a_caller_sees(oracle, C, B, bb):
    import torch
    dev = torch.device("cuda:0")
    x, quiet = _input(C, B, bb, 2, dev)
    x1, x2 = x[:, :B].contiguous(), x[:, B:].contiguous()
    rn, rm = api.Rx(C), api.Rx(C)
    rn.set_mode(api.WBFM)
    rm.set_mode(api.WBFM)
    assert rn.debug_mag_skipped() == 0 and rm.debug_mag_skipped() == 0

    # ---- call 1: default threshold (-200), N without a magnitude buffer, M with one
    bad_n, pcm_n, np_n, al_n, _ = _call(rn, x1, C, B, bb, False)
    bad_m, pcm_m, np_m, al_m, mg_m = _call(rm, x1, C, B, bb, True)
    assert rn.debug_mag_skipped() == 1, "the handle without a magnitude buffer did not run the MAG = false instantiation"
    assert rm.debug_mag_skipped() == 0, "a caller who passed a magnitude buffer must run the kernel that computes it"
    assert bad_n == 0 and bad_m == 0, (bad_n, bad_m)
    assert (pcm_n == pcm_m).all() and (np_n == np_m).all() and (al_n == al_m).all()
    assert (np_n == bb // 512).all() and (al_n == 1).all()

    # ---- call 2: gates that can close; both with a magnitude buffer -- N on the old kernel, from the state call 1 left
    rn.set_threshold(-30)
    rm.set_threshold(-30)
    bad_n2, pcm_n2, np_n2, al_n2, mg_n2 = _call(rn, x2, C, B, bb, True)
    bad_m2, pcm_m2, np_m2, al_m2, mg_m2 = _call(rm, x2, C, B, bb, True)
    assert rn.debug_mag_skipped() == 1 and rm.debug_mag_skipped() == 0
    assert bad_n2 == 0 and bad_m2 == 0, (bad_n2, bad_m2)
    assert (pcm_n2 == pcm_m2).all() and (np_n2 == np_m2).all() and (al_n2 == al_m2).all() and (mg_n2 == mg_m2).all()
    assert (al_n2[quiet] == 0).any(), "no gate of a quiet channel closed under the -30 dBFS threshold"

    # ---- call 3 on N: no buffer again, but a gate can close -- the sums are needed
    _call(rn, x2, C, B, bb, False)
    assert rn.debug_mag_skipped() == 1

    # ---- eight channels, the quiet ones among them, through the sequential oracle: both calls, tolerance 0
    sel = sorted(set(quiet) | {0, 2, 3, C - 3})
    assert len(sel) == 8
    xs = x[torch.tensor(sel, device=dev)].cpu().numpy()
    for i, c in enumerate(sel):
        o = oracle.rx()
        o.set_mode(api.WBFM)
        for b in range(2 * B):
            if b == B:
                o.set_threshold(-30)
            p, m, a, _ = o.process(xs[i, b])
            if b < B:
                assert len(p) == np_n[c, b] == np_m[c, b] and (pcm_n[c, b, :len(p)] == p).all() and (pcm_m[c, b, :len(p)] == p).all(), (c, b)
                assert bool(al_n[c, b]) == a and bool(al_m[c, b]) == a and int(mg_m[c, b]) == m, (c, b)
            else:
                k = b - B
                assert len(p) == np_n2[c, k] and bool(al_n2[c, k]) == a and int(mg_n2[c, k]) == m, (c, k)
                assert (pcm_n2[c, k, :len(p)] == p).all(), (c, k)
