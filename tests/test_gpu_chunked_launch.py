"""The chunked launch of the tone, audio and resampler banks (bank_launch_chunked in hackrfdiags_amd/csrc/hrfd_bank.hip) with
a chunk boundary in every place that matters, tolerance 0.

A call of more than 2^22 workgroups is cut into several launches, and k_tone, k_audio_fir and k_resamp take their workgroup
number as P.first_wg + blockIdx.x.  The smallest call that chunks on its own needs 9 to 17 GB of PCM, so
hrfd_<bank>_debug_set_max_wgs (include/hrfd_debug.h, inert without HRFD_DEBUG_HOOKS=1) lowers the workgroups of one launch
and a call of 2 to 9 workgroups runs with first_wg != 0: with the boundary inside a channel, between channels, directly in
front of the workgroup that writes the ping-pong history (audio, resampler) and in front of a partial last tile (tone).
For a call of n workgroups the limits are 1, 2, a value that splits a channel in the middle, n - 1, n and n + 1.

Every call is compared bit for bit with the numpy model (tests/tone_model.py, audio_model.py, resamp_model.py) through the
guarded device buffers of the banks' own suites -- nothing outside the rows may be written, the input stays unchanged --
and with a twin handle that never had the hook called and is given the same calls through its host path."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import test_gpu_audio as ta
from tests import test_gpu_resamp as tr
from tests import test_gpu_tone as tt
from tests import tone_model as tm
from tests.hooks import HOOKS_ON

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not HOOKS_ON, reason="debug_set_max_wgs needs HRFD_DEBUG_HOOKS=1 (this run is the shipped state)")]

ALL = 0xFFFFFFFF
MOST = 1 << 22
NINE = (1, 2, 4, 8, 9, 10)             # for a call of 3 channels x 3 workgroups: 4 splits channel 1 in the middle


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def rows_equal(got, want, what):
    assert got.shape == want.shape and (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:4].tolist()}"


# ---------------------------------------------------------------- the resampler
def resamplers(C, L, M, taps, max_wgs):
    """the hooked handle, its model, and the twin without the hook"""
    d, m = tr.both(C, L, M, taps)
    d.debug_set_max_wgs(max_wgs)
    twin, _ = tr.both(C, L, M, taps)
    return d, m, twin


def resamp_call(torch_dev, d, m, twin, pcm, n_pcm, what, **kw):
    want = tr.run_device(torch_dev, d, m, pcm, n_pcm, what, **kw)
    rows_equal(twin.process(pcm, n_pcm), want, what + ": the twin without the hook")
    return want


def resamp_taps_3(max_wgs, odd):
    """taps for up = 3 with K = 33 taps per branch (the last branch one short) or K = 34"""
    return tr.random_taps(3 * 33 - 1 if odd else 3 * 34, 3, 70 + max_wgs)


@pytest.mark.parametrize("max_wgs", NINE)
@pytest.mark.parametrize("parity", ["odd_K", "even_K"])
def test_resampler_two_calls(torch_dev, parity, max_wgs):
    """3 channels x 3 tiles (2126 outputs, the last tile of 78).  The second call reads the history the chunked first call
    wrote: with 8 workgroups per launch the history writer of the last channel is alone in its launch, with 2 and 4 the
    writers of channels 0 and 1 are the first workgroup of theirs."""
    d, m, twin = resamplers(3, 3, 2, resamp_taps_3(max_wgs, parity == "odd_K"), max_wgs)
    pcm = tr.reference(3, 1417)
    want = resamp_call(torch_dev, d, m, twin, pcm, None, f"{parity}, {max_wgs} per launch")
    assert want.shape[1] == 2126 and m.d == 1
    # shorter, rows that are not 4-byte aligned, padded strides on both sides
    resamp_call(torch_dev, d, m, twin, pcm[:, :777], None, f"{parity}, {max_wgs} per launch, the second call", residue=2, out_residue=6,
                pad=6, out_pad=2, spare=3)


@pytest.mark.parametrize("max_wgs", NINE)
def test_resampler_n_pcm(torch_dev, max_wgs):
    """the same with short and empty blocks, the last block among them: the masked samples go into the history too"""
    d, m, twin = resamplers(3, 3, 2, resamp_taps_3(max_wgs, max_wgs % 2 == 1), max_wgs)
    pcm = tr.reference(3, 1536)
    n_pcm = np.array([[512, 0, 511], [1, 0xFFFFFFFF, 0], [0xFFFFFFFF, 511, 1]], dtype=np.uint32)
    want = resamp_call(torch_dev, d, m, twin, pcm, n_pcm, f"n_pcm, {max_wgs} per launch")
    assert want.shape[1] == 2304
    resamp_call(torch_dev, d, m, twin, pcm[:, :777], None, f"n_pcm, {max_wgs} per launch, the second call", residue=6, out_residue=2,
                pad=2, out_pad=6, spare=1)


@pytest.mark.parametrize("max_wgs", [1, 2])
def test_resampler_history_only_workgroups(torch_dev, max_wgs):
    """1 / 6: behind a first call of 6 x 236 + 1 samples a call of one sample gives no output and launches one history-only
    workgroup per channel, here in launches of 1 and 2; the call behind it reads what they wrote"""
    d, m, twin = resamplers(3, 1, 6, tr.random_taps(100, 1, 75), max_wgs)
    pcm = tr.reference(3, 1417)
    resamp_call(torch_dev, d, m, twin, pcm, None, f"1/6, {max_wgs} per launch")
    assert d.out_count(1) == 0 and m.out_count(1) == 0
    none = resamp_call(torch_dev, d, m, twin, pcm[:, 700:701], None, f"1/6, {max_wgs} per launch, one sample", out_residue=2, spare=2)
    assert none.shape == (3, 0)
    resamp_call(torch_dev, d, m, twin, pcm, None, f"1/6, {max_wgs} per launch, behind the call without outputs")


@pytest.mark.parametrize("max_wgs", [1, 4])
def test_resampler_widest_tile(torch_dev, max_wgs):
    """1 / 8 with 512 taps: every tile reads the widest span of input; 2 channels x 3 tiles"""
    d, m, twin = resamplers(2, 1, 8, tr.random_taps(512, 1, 3), max_wgs)
    pcm = tr.reference(2, 8 * 2048 + 803)
    want = resamp_call(torch_dev, d, m, twin, pcm, None, f"1/8, {max_wgs} per launch")
    assert want.shape[1] == 2149
    resamp_call(torch_dev, d, m, twin, pcm, None, f"1/8, {max_wgs} per launch, the second call")


def test_resampler_reset_and_set_taps_between_chunked_calls(torch_dev):
    """the reset flags and new taps reach every launch of a call, not the first alone"""
    C, L, M = 3, 3, 2
    taps = tr.random_taps(3 * 200, L, 51)
    d, m, twin = resamplers(C, L, M, taps, 2)
    pcm = tr.reference(C, 1417)
    first = resamp_call(torch_dev, d, m, twin, pcm, None, "first call")
    for h in (d, m, twin):
        h.reset(1)
    nxt = resamp_call(torch_dev, d, m, twin, pcm, None, "behind reset(1)")
    assert (nxt[0] != first[0][1:]).any() and (nxt[2] != first[2][1:]).any()      # the others go on, one output later in phase
    for h in (d, m, twin):
        h.reset()
    rows_equal(resamp_call(torch_dev, d, m, twin, pcm, None, "behind reset()"), first, "behind reset(), against the first call")
    other = tr.random_taps(3 * 7 + 1, L, 52)
    for h in (d, m, twin):
        h.set_taps(other)
    resamp_call(torch_dev, d, m, twin, pcm, None, "behind other taps")
    resamp_call(torch_dev, d, m, twin, pcm[:, :777], None, "behind other taps, the second call", out_residue=2)


# ---------------------------------------------------------------- the audio bank
AUDIO_BUSES = [([0, 1, 2], [32767, 32767, -20000]), ([2, 0], [4096, -4096])]      # bus 0 clips


def audios(C, T, max_wgs, buses=AUDIO_BUSES):
    taps = ta.random_taps(T, 60 + T)
    d, m = ta.both(C, len(buses), taps, buses)
    d.debug_set_max_wgs(max_wgs)
    twin, _ = ta.both(C, len(buses), taps, buses)
    return d, m, twin


def audio_call(torch_dev, d, m, twin, pcm, n_pcm, open_, what, **kw):
    want = ta.run_device(torch_dev, d, m, pcm, n_pcm, open_, what, **kw)
    ta.same(twin.process(pcm, n_pcm, open_), [want[k] for k in ta.OUTPUTS], what + ": the twin without the hook")
    return want


@pytest.mark.parametrize("max_wgs", NINE)
@pytest.mark.parametrize("T", [63, 64])
def test_audio_three_runs_per_channel(torch_dev, T, max_wgs):
    """3 channels x 9 blocks: runs of 4, 4 and 1 blocks, so the workgroup that writes the history and the previous gate is
    the third of its channel.  Gates that change across the run boundaries (blocks 3 | 4 and 7 | 8) and across the call
    boundary, short and empty blocks, both parities of the window start.  k_audio_mix runs behind the last launch and reads
    every row of z.  Three calls: the second reads the history and gate a chunked call wrote, the third follows reset(1)."""
    d, m, twin = audios(3, T, max_wgs)
    n = 512 * 9
    n_pcm = np.array([[512, 7, 512, 0, 512, 600, 511, 512, 300],
                      [0, 512, 512, 511, 7, 512, 512, 0, 512],
                      [512, 512, 0, 512, 512, 1, 512, 512, 0]], dtype=np.uint32)
    opens = [np.array([[1, 1, 1, 0, 1, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, 0, 0, 1], [1, 0, 1, 1, 0, 0, 1, 0, 0]], dtype=np.uint8),
             np.array([[1, 0, 0, 1, 0, 1, 1, 0, 1], [1, 1, 1, 1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 1, 1, 1, 1]], dtype=np.uint8),
             np.array([[1, 1, 0, 0, 1, 1, 0, 0, 1], [1, 0, 1, 1, 1, 1, 1, 0, 1], [0, 1, 1, 0, 1, 0, 0, 1, 1]], dtype=np.uint8)]
    what = f"T={T}, {max_wgs} per launch"
    want = audio_call(torch_dev, d, m, twin, ta.reference(3, n), n_pcm, opens[0], what)
    assert want["clips"][0] > 0 and want["mix"].any()
    audio_call(torch_dev, d, m, twin, ta.reference(3, n, seed=8), np.roll(n_pcm, 4, axis=1), opens[1], what + ", the second call",
               residue=2, pad=6, out_pad=2)
    for h in (d, m, twin):
        h.reset(1)
    audio_call(torch_dev, d, m, twin, ta.reference(3, n, seed=9), None, opens[2], what + ", behind reset(1)", residue=4, pad=2, out_pad=6)


@pytest.mark.parametrize("max_wgs", [1, 2, 4])
def test_audio_one_run_per_channel(torch_dev, max_wgs):
    """5 channels x 4 blocks: one workgroup per channel, each the history writer of its own"""
    buses = [([0, 1, 2, 3, 4], [4096, -4096, 3000, 77, 32767]), ([4], [4096])]
    d, m, twin = audios(5, 511, max_wgs, buses)
    rng = np.random.default_rng(max_wgs)
    for call in range(2):
        n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(5, 4))
        open_ = rng.integers(0, 2, size=(5, 4), dtype=np.uint8)
        audio_call(torch_dev, d, m, twin, ta.reference(5, 2048, seed=7 + call), n_pcm, open_, f"{max_wgs} per launch, call {call}")


def test_audio_second_stream_behind_a_chunked_call(torch_dev):
    """16 channels x 16 blocks in launches of 5 workgroups (13 launches) on one stream, the next call directly behind it on a
    second stream, the third on the first again: the hand-over orders a call behind the last launch of the one before, whose
    history and gate it reads and whose other history side it overwrites"""
    torch, dev = torch_dev
    C, M, n_blocks = 16, 2, 16
    buses = [(list(range(C)), [300] * C), ([C - 1, 0], [4096, -4096])]
    d, m, twin = audios(C, 512, 5, buses)
    pcm = ta.reference(C, 512 * n_blocks)
    d_pcm = torch.from_numpy(pcm.copy()).to(dev)
    calls = 3
    opens = np.random.default_rng(16).integers(0, 2, size=(calls, C, n_blocks), dtype=np.uint8)
    d_open = torch.from_numpy(opens).to(dev)
    d_out = torch.zeros((calls, C, n_blocks, 512), dtype=torch.int16, device=dev)
    d_mix = torch.zeros((calls, M, n_blocks, 512), dtype=torch.int16, device=dev)
    d_clips = torch.zeros((calls, M), dtype=torch.int32, device=dev)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for i in range(calls):
        d.process_device(d_pcm.data_ptr(), 1024 * n_blocks, None, d_open[i].data_ptr(), n_blocks, d_out[i].data_ptr(), 0,
                         d_mix[i].data_ptr(), d_clips[i].data_ptr(), streams[i % 2].cuda_stream)
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i in range(calls):
        want = m.process(pcm, None, opens[i])
        got = (d_out[i].cpu().numpy(), d_mix[i].cpu().numpy(), d_clips[i].cpu().numpy().view(np.uint32))
        ta.same(got, want, f"call {i}")
        ta.same(twin.process(pcm, None, opens[i]), want, f"call {i}: the twin without the hook")


# ---------------------------------------------------------------- the tone bank
# (frame length, channels, blocks, limits): G = C F frames in workgroups of FT = 16384 / L (at most 16); in every case G is
# no multiple of FT and a workgroup holds frames of two channels
TONE_CASES = [(128, 3, 3, (1, 2, 3, 4)),       # F = 12, G = 36, FT = 16: 3 workgroups, the last with 4 frames
              (2048, 5, 12, (1, 2)),           # F = 3, G = 15, FT = 8: 2 workgroups, the last with 7 frames
              (4096, 7, 8, (1, 2)),            # F = 1, G = 7, FT = 4: 2 workgroups, the last with 3 frames
              (8192, 3, 16, (1, 2))]           # F = 1, G = 3, FT = 2: 2 workgroups, the last with 1 frame
TONE_STEPS = [tm.tone_step(f) for f in (67.0, 697.0, 1000.0, 1633.0, 2400.0, 3999.0)]
TONE_GROUPS = [0, 1, 2, 3, 0, 1]


def tones(C, L, max_wgs, ratio_q8):
    d, m = tt.both(C, L, TONE_STEPS, TONE_GROUPS)
    twin, _ = tt.both(C, L, TONE_STEPS, TONE_GROUPS)
    for h in (d, twin):
        h.set_threshold(ALL, ratio_q8=ratio_q8, min_energy=0)
    m.set_threshold(ALL, ratio_q8, 0)
    d.debug_set_max_wgs(max_wgs)
    return d, m, twin


@pytest.mark.parametrize("L,C,n_blocks,max_wgs", [(L, C, b, w) for L, C, b, ws in TONE_CASES for w in ws])
def test_tone_every_instantiation(torch_dev, L, C, n_blocks, max_wgs):
    """k_tone<16>, <8>, <4> and <2>, each with a boundary in front of its partial last workgroup: g0 and the g0 K output
    offsets of every output, the channel and frame a frame number splits into, n_pcm rows with short and empty blocks.  The
    ratio threshold is the median of the model's own P_max / E, so that `present` holds both verdicts."""
    pcm = tt.reference(C, 512 * n_blocks)
    n_pcm = np.random.default_rng(L).choice(np.array([512, 512, 512, 600, 100, 0], dtype=np.uint32), size=(C, n_blocks))
    n_pcm[0, 0], n_pcm[C - 1, n_blocks - 1], n_pcm[C // 2, 1] = 0, 100, 512
    _, probe = tt.both(C, L, TONE_STEPS, TONE_GROUPS)
    P, E = probe.process(pcm)[:2]
    ratios = sorted(int(p) * 256 // max(int(e), 1) for p, e in zip(P.max(axis=2).ravel(), E.ravel()))
    d, m, twin = tones(C, L, max_wgs, ratios[len(ratios) // 2])
    assert (C * (512 * n_blocks // L)) % min(16, 16384 // L) != 0
    what = f"L={L}, {max_wgs} per launch"
    for rows, outputs in ((None, tt.OUTPUTS), (n_pcm, tt.OUTPUTS), (n_pcm, ("energy", "best")), (None, ("power", "present"))):
        label = f"{what}, n_pcm {rows is not None}, outputs {outputs}"
        want = tt.run_device(torch_dev, d, m, pcm, rows, label, residue=2 if rows is None else 0, pad=6 if rows is None else 0,
                             outputs=outputs)
        tt.same(twin.process(pcm, rows), [want[k] for k in tt.OUTPUTS], label + ": the twin without the hook")
        if rows is None:
            assert 0 < int(want["present"].sum()) < want["present"].size
        else:
            assert (want["valid"] < L).any() and (want["valid"] > 0).any()


# ---------------------------------------------------------------- the hook's own arguments
@pytest.mark.parametrize("bank", ["tone", "audio", "resamp"])
def test_hook_refuses_limits_outside_its_range(torch_dev, bank):
    """0 and 2^22 + 1 are refused under the function's name and change nothing: the handle goes on in launches of 2; 2^22
    itself, the default, is taken"""
    if bank == "tone":
        d, m, twin = tones(3, 128, 2, 1 << 12)
        pcm = tt.reference(3, 1536)
        call = lambda what: tt.same(twin.process(pcm), [tt.run_device(torch_dev, d, m, pcm, None, what)[k] for k in tt.OUTPUTS], what)
    elif bank == "audio":
        d, m, twin = audios(3, 64, 2)
        pcm = ta.reference(3, 512 * 9)
        call = lambda what: audio_call(torch_dev, d, m, twin, pcm, None, None, what)
    else:
        d, m, twin = resamplers(3, 3, 2, resamp_taps_3(2, True), 2)
        pcm = tr.reference(3, 1417)
        call = lambda what: resamp_call(torch_dev, d, m, twin, pcm, None, what)
    call("in launches of 2")
    for n in (0, MOST + 1):
        with pytest.raises(api.HrfdError, match=f"hrfd_{bank}_debug_set_max_wgs"):
            d.debug_set_max_wgs(n)
        call(f"behind the refused limit {n}")
    d.debug_set_max_wgs(MOST)
    call("at the default limit")
