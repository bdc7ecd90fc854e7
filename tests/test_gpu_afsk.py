"""The AFSK bank on the device (hrfd_afsk_*) against the numpy model (tests/afsk_model.py), bit for bit.  `hard`, the
discriminator's decisions, is compared first, so a failure says which stage it is in: the dense one (filters, powers,
decision) or the serial one (clock, NRZI, carrier flag, count).  Channel and block counts on both sides of the kernel's step
of 4 blocks, odd and even windows and the longest, both ends of the loop shift, three baud rates, NRZI off and on, a stream
cut into calls, resets and a new modem between calls, n_pcm at its edges with other bytes behind it, rows at every even
residue with padded strides and guard bytes around every buffer and behind every row's bits, full-scale input that follows
the taps' signs, the carrier threshold on both sides of a constant tone's power, a call with only `hard`, a call chained on
one stream behind the copy that fills its input, the blocking host entry, and HDLC frames end to end."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import afsk_model as am
from tests.test_gpu_tone import Guarded

pytestmark = pytest.mark.gpu

ALL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def both(C, nrzi=True, **modem):
    modem = {**am.BELL202, **modem}
    return api.Afsk(C, nrzi=nrzi, device=0, **modem), am.AfskModel(C, nrzi=nrzi, **modem), modem


_signals = {}


def signal(C, n_blocks, modem, seed=3):
    """noisy AFSK on the modem's tones, one array per shape and modem, computed once and left unchanged: [C, n_blocks, 512]"""
    key = (C, n_blocks, modem["mark_hz"], modem["space_hz"], modem["baud"], seed)
    if key not in _signals:
        rng = np.random.default_rng(seed)
        x = np.stack([am.noisy_afsk(rng, modem, n_blocks) for _ in range(C)])
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


def same_bits(got, want, what):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), f"{what}: channel {c} gave {len(g)} bits, the model {len(w)}"
        assert (g == w).all(), f"{what}: channel {c}'s bits differ first at {np.argwhere(g != w)[:4].ravel().tolist()}"


def run_device(torch_dev, d, m, pcm, n_pcm, what, residue=0, pad=0, bits_pad=0, want_bits=True, want_hard=True, stream=None):
    """process_device over rows at `residue` modulo 16, 1024 n_blocks + pad bytes apart; rows of bits max_bits + bits_pad
    apart at an odd address, n_bits at 4 modulo 8, hard at an odd address; every buffer between guards, and what lies behind
    n_bits[c] in a row must stay.  The model takes the same call.  Returns the model's (bits, hard)"""
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
    cap = d.max_bits(n_blocks)
    assert cap == m.max_bits(n_blocks)
    bits_stride = cap + bits_pad
    g_bits = Guarded(torch_dev, bits_stride * (C - 1) + cap, 1, 2, 22)
    g_count = Guarded(torch_dev, 4 * C, 4, 8, 23)
    g_hard = Guarded(torch_dev, C * n // 8, 1, 2, 24)
    torch.cuda.synchronize()
    d.process_device(src.ptr, stride, None if d_n is None else d_n.data_ptr(), n_blocks, g_bits.ptr if want_bits else None, bits_stride,
                     g_count.ptr if want_bits else None, g_hard.ptr if want_hard else None, stream)
    torch.cuda.synchronize()
    bits, hard = m.process(pcm.reshape(C, n_blocks, 512), n_pcm, want_bits=want_bits)
    g_hard.check(hard if want_hard else None, f"{what}: hard (the dense stage)")
    if not want_bits:
        g_count.check(None, f"{what}: n_bits without bits")
        g_bits.check(None, f"{what}: bits not asked for")
    else:
        g_count.check(np.array([len(b) for b in bits], dtype=np.uint32), f"{what}: n_bits (the serial stage)")
        rows = g_bits.host[g_bits.off:g_bits.off + g_bits.n].copy()
        for c in range(C):
            rows[c * bits_stride:c * bits_stride + len(bits[c])] = bits[c]
        g_bits.check(rows, f"{what}: bits (the serial stage), or the bytes behind n_bits")
    src.check(None, f"{what}: the input")
    return bits, hard


# 1. channel and block counts on both sides of the kernel's step
@pytest.mark.parametrize("n_blocks", [1, 4, 5, 16])
@pytest.mark.parametrize("C", [1, 3, 65])
def test_channel_and_block_counts(torch_dev, C, n_blocks):
    d, m, modem = both(C)
    bits, _ = run_device(torch_dev, d, m, signal(C, n_blocks, modem), None, f"C={C} B={n_blocks}")
    assert min(len(b) for b in bits) > 60 * n_blocks           # 76.8 a block


# 2. windows, loop shifts, baud rates, NRZI: every value of each, two calls so that the state of every kind is carried
@pytest.mark.parametrize("baud", [300, 1200, 4000])
@pytest.mark.parametrize("W", [2, 7, 8, 32])
def test_windows_shifts_bauds_and_nrzi(torch_dev, W, baud):
    i = [2, 7, 8, 32].index(W) + [300, 1200, 4000].index(baud)
    A, nrzi = (1, 8)[i % 2], bool((i // 2) % 2)
    d, m, modem = both(2, nrzi=nrzi, window=W, loop_shift=A, baud=baud)
    x = signal(2, 10, modem)
    for call, part in enumerate((x[:, :5], x[:, 5:])):
        run_device(torch_dev, d, m, part, None, f"W={W} A={A} baud={baud} nrzi={nrzi} call {call}")


@pytest.mark.parametrize("A,nrzi", [(1, True), (8, False), (8, True), (1, False)])
def test_both_shifts_with_nrzi_off_and_on(torch_dev, A, nrzi):
    d, m, modem = both(3, nrzi=nrzi, loop_shift=A, window=7)
    run_device(torch_dev, d, m, signal(3, 5, modem), None, f"A={A} nrzi={nrzi}")


# 3. the 1 + 4 + 5 + 6 cut against one call
def test_a_stream_cut_into_calls_equals_one_call(torch_dev):
    C = 3
    d1, m1, modem = both(C)
    d2, m2, _ = both(C)
    x = signal(C, 16, modem)
    n_pcm = np.random.default_rng(4).choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C, 16))
    n_pcm[0] = 512
    bits, hard = run_device(torch_dev, d1, m1, x, n_pcm, "one call")
    parts, at = [], 0
    for k in (1, 4, 5, 6):
        parts.append(run_device(torch_dev, d2, m2, x[:, at:at + k], n_pcm[:, at:at + k], f"blocks {at}..{at + k}"))
        at += k
    assert (np.concatenate([p[1] for p in parts], axis=1) == hard).all()
    same_bits([np.concatenate([p[0][c] for p in parts]) for c in range(C)], bits, "the cut against one call")


# 4. a reset of one channel, of all, and set_modem between calls
def test_reset_and_set_modem_between_calls(torch_dev):
    C = 3
    d, m, modem = both(C)
    x = signal(C, 8, modem)
    run_device(torch_dev, d, m, x[:, :3], None, "before the reset")
    d.reset(1)
    m.reset(1)
    with pytest.raises(api.HrfdError, match="channel 3"):
        d.reset(C)
    run_device(torch_dev, d, m, x[:, 3:5], None, "behind the reset of channel 1")
    d.reset()
    m.reset()
    run_device(torch_dev, d, m, x[:, 5:6], None, "behind the reset of all")
    new = dict(mark_hz=1270, space_hz=1070, baud=300, window=27, loop_shift=3, nrzi=False)
    d.set_modem(**new)
    m.set_modem(**new)
    assert d.max_bits(2) == m.max_bits(2) == api.afsk_max_bits(am.step(300), 3, 2)
    run_device(torch_dev, d, m, x[:, 6:], None, "behind set_modem")
    d.set_modem(steps=(1 << 31, 1, 1 << 31), window=32, loop_shift=1)       # the limits of every step
    m.set_modem(steps=(1 << 31, 1, 1 << 31), window=32, loop_shift=1)
    run_device(torch_dev, d, m, x[:, :2], None, "steps at their limits")


# 5. n_pcm at its edges, other bytes behind it
def test_n_pcm_edges(torch_dev):
    C, B = 4, 6
    d, m, modem = both(C)
    x = signal(C, B, modem)
    n_pcm = np.array([[0, 1, 511, 512, 513, 0xFFFFFFFF], [512, 0, 0, 1, 511, 2], [1, 1, 1, 1, 1, 1], [511, 512, 0, 510, 7, 8]], dtype=np.uint32)
    _, hard = run_device(torch_dev, d, m, x, n_pcm, "n_pcm edges")
    d2, m2, _ = both(C)
    y = x.copy()
    lim = np.minimum(n_pcm, 512)
    y[np.arange(512)[None, None, :] >= lim[:, :, None]] ^= 0x5A5A
    _, hard2 = run_device(torch_dev, d2, m2, y, n_pcm, "n_pcm edges, other bytes behind")
    assert (hard == hard2).all()


# 6. rows at every even residue, padded strides of the PCM and of the bits
@pytest.mark.parametrize("residue", range(0, 16, 2))
def test_every_even_residue_with_padded_strides(torch_dev, residue):
    d, m, modem = both(3, window=(7, 8, 32, 2)[residue // 2 % 4])
    run_device(torch_dev, d, m, signal(3, 5, modem), None, f"residue {residue}", residue=residue, pad=2 + 4 * (residue % 4),
               bits_pad=1 + residue)


# 7. the stride of a row of bits against the handle's own modem
def test_a_bits_stride_below_the_bound_is_refused(torch_dev):
    torch, dev = torch_dev
    d, m, _ = both(2)
    buf = torch.zeros(8192, dtype=torch.uint8, device=dev)
    cap = d.max_bits(2)
    assert cap == ((1024 * (am.step(1200) + (1 << 29))) >> 32) + 1 == 282
    with pytest.raises(api.HrfdError, match="bits_stride_bytes 281 is below hrfd_afsk_max_bits = 282"):
        d.process_device(buf.data_ptr(), 2048, None, 2, buf.data_ptr() + 4096, cap - 1, buf.data_ptr() + 6000, None)
    d.set_modem(baud=4000, loop_shift=1)
    with pytest.raises(api.HrfdError, match="is below hrfd_afsk_max_bits = 769"):
        d.process_device(buf.data_ptr(), 2048, None, 2, buf.data_ptr() + 4096, cap, buf.data_ptr() + 6000, None)
    torch.cuda.synchronize()
    assert int(buf.max()) == 0                                 # a refused call writes nothing


# 8. full scale, the signs following the taps: |I| at its bound, squares that need their 64 bits
def test_full_scale_input_that_follows_the_taps(torch_dev):
    C, B = 3, 2
    steps = (1 << 31, am.step(2200), am.step(1200))           # a 4 kHz mark: every cosine tap of it is +-2047
    d = api.Afsk(C, device=0)
    d.set_modem(steps=steps, window=32)
    m = am.AfskModel(C, steps=steps, window=32)
    t = am.taps(steps[0], steps[1], 32)
    assert (np.abs(t[0]) == 2047).all()
    x = np.zeros((C, B * 512), dtype=np.int16)
    for c, f in enumerate((0, 2, 3)):                          # the window that ends at n = 31 mod 32 sees -32768 sign(tap k) at n - k
        period = np.where(t[f][::-1] >= 0, -32768, 32767).astype(np.int16)
        x[c] = np.tile(period, B * 512 // 32)
    x[2, 512:] = np.where(np.arange(512) % 2 == 0, 32767, -32768)
    run_device(torch_dev, d, m, x, None, "full scale")
    assert m.max_abs_i >= 32 * 2047 * 32768 - 32 * 2047 and m.max_power > 1 << 61, (m.max_abs_i, m.max_power)


# 9. the carrier flag just below and just above a constant tone's power
def test_the_carrier_threshold_on_both_sides_of_a_tones_power(torch_dev):
    steps = (1 << 30, 1 << 29, 1 << 30)                        # a 2 kHz mark, sampled every 4 samples: one power at every bit
    x = np.tile(np.array([8000, 0, -8000, 0], dtype=np.int16), 256)[None]
    probe = am.AfskModel(1, steps=steps, window=8, nrzi=False)
    bits, _ = probe.process(x.reshape(1, 2, 512))
    power = int(probe.total_power[0, 511])
    assert (probe.total_power[0, 35::4] == power).all() and power > 1 << 40 and len(bits[0]) >= 255
    for min_power, flagged in ((power - 1, True), (power, False)):
        d = api.Afsk(1, device=0)
        d.set_modem(steps=steps, window=8, nrzi=False)
        m = am.AfskModel(1, steps=steps, window=8, nrzi=False)
        d.set_carrier(min_power)
        m.set_carrier(min_power)
        bits, _ = run_device(torch_dev, d, m, x, None, f"min_power {min_power}")
        assert ((bits[0][10:] & 2) != 0).all() == flagged and ((bits[0][10:] & 2) != 0).any() == flagged
        assert (bits[0][10:] & 1).all()                        # mark


# 10. a call with only hard: the clock waits, the samples and h[n-1] move on
def test_a_call_with_only_hard(torch_dev):
    d, m, modem = both(2)
    x = signal(2, 9, modem)
    run_device(torch_dev, d, m, x[:, :4], None, "bits and hard")
    run_device(torch_dev, d, m, x[:, 4:5], None, "only hard", want_bits=False)
    run_device(torch_dev, d, m, x[:, 5:], None, "only bits, behind the call without", want_hard=False)
    with pytest.raises(api.HrfdError, match="no output"):
        d.process_device(1 << 20, 1024, None, 1, None, 0, None, None)


# 11. chained on one stream behind the copy that fills its input
def test_chained_on_one_stream_behind_the_copy(torch_dev):
    torch, dev = torch_dev
    C, B = 5, 16
    d, m, modem = both(C)
    x = signal(C, B, modem)
    host = torch.from_numpy(x.copy()).pin_memory()
    d_pcm = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    cap = d.max_bits(B)
    d_bits = torch.zeros((C, cap), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(C, dtype=torch.int32, device=dev)
    d_hard = torch.zeros((C, B, 64), dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_pcm.copy_(host, non_blocking=True)
    d.process_device(d_pcm.data_ptr(), 1024 * B, None, B, d_bits.data_ptr(), 0, d_count.data_ptr(), d_hard.data_ptr(), st.cuda_stream)
    st.synchronize()
    bits, hard = m.process(x)
    assert (d_hard.cpu().numpy() == hard).all()
    count = d_count.cpu().numpy()
    same_bits([d_bits[c, :count[c]].cpu().numpy() for c in range(C)], bits, "chained")


# 12. the blocking host entry
def test_the_host_entry(torch_dev):
    d, m, modem = both(3, window=7)
    x = signal(3, 5, modem)
    n_pcm = np.array([[512] * 5, [0, 511, 512, 1, 600], [512, 512, 0, 0, 512]], dtype=np.uint32)
    for call, (want_bits, want_hard) in enumerate(((True, True), (False, True), (True, False))):
        got_bits, got_hard = d.process(x, n_pcm, want_bits=want_bits, want_hard=want_hard)
        bits, hard = m.process(x, n_pcm, want_bits=want_bits)
        if want_hard:
            assert (got_hard == hard).all(), call
        else:
            assert got_hard is None
        if want_bits:
            same_bits(got_bits, bits, f"host call {call}")
        else:
            assert got_bits is None


# 13. frames end to end: the cases of tests/test_afsk_model.py through the device and hdlc_frames, cut into two calls
@pytest.mark.parametrize("name", ["bell202", "bell103"])
def test_frames_end_to_end(torch_dev, name):
    cases = [(c, s) for c in am.E2E_CASES if c[0].startswith(name) for s in am.E2E_SEEDS]
    made = [am.e2e_signal(c[1], c[2], c[3], s) for c, s in cases]
    C, B = len(made), max(pcm.shape[0] for _, pcm in made)
    x = np.zeros((C, B, 512), dtype=np.int16)
    for c, (_, pcm) in enumerate(made):
        x[c, :pcm.shape[0]] = pcm
    d, m, _ = both(C, **cases[0][0][1])
    cut = B // 2 + 1
    first, _ = run_device(torch_dev, d, m, x[:, :cut], None, f"{name}: first call")
    second, _ = run_device(torch_dev, d, m, x[:, cut:], None, f"{name}: second call")
    for c, (payloads, _) in enumerate(made):
        assert api.hdlc_frames(np.concatenate([first[c], second[c]])) == payloads, (name, cases[c][0][0], cases[c][1])
