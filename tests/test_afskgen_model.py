"""tests/afskgen_model.py against the library's own statement of the AFSK generator bank's law (hrfd_afskgen.h, reached on the
host through hrfd_afskgen_debug_levels, _length and _slow: no device), against the tone generator's model where mark and
space are one tone, against every cut of a stream into calls, and in a closed loop: HDLC frames through the model, the AFSK
bank's model and api.hdlc_frames.  No GPU; no comparison has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import afsk_model as am
from tests import afskgen_model as gm
from tests import tonegen_model as tm

BAUD_STEPS = {"300": gm.step(300), "1200": gm.step(1200), "4000": 1 << 31, "odd": gm.ODD_STEP}
BIT_COUNTS = (1, 2, 31, 32, 33, 8192)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def lib_levels(lib, bits, nrzi):
    words = np.full((len(bits) + 31) // 32 + 1, 0xEEEEEEEE, dtype=np.uint32)
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    assert lib.hrfd_afskgen_debug_levels(p(b), b.size, 1 if nrzi else 0, p(words)) == 0, lib.hrfd_last_error().decode()
    assert words[-1] == 0xEEEEEEEE
    return words[:-1]


def lib_length(lib, n_bits, baud_step):
    v = C.c_uint64(0)
    rc = lib.hrfd_afskgen_debug_length(n_bits, baud_step, C.byref(v))
    return int(v.value) if rc == 0 else None


def lib_slow(lib, model, c, pcm, n_blocks, in_place=False):
    """hrfd_afskgen.h's loop over channel c of the model's queues and clock as they stand: (out [n_blocks, 512], active, clips)"""
    q = [m for m in model.q[c] if m.end > model.N]
    msgs = np.array([[0, len(m.lv), m.mark_step, m.space_step, m.baud_step, m.amp, 0, 0] for m in q], dtype=np.uint32).reshape(-1, 8)
    bits = np.concatenate([m.lv for m in q]).astype(np.uint8) if q else None       # the levels as data, NRZI off
    starts = np.array([m.start for m in q], dtype=np.uint64)
    ends = np.array([m.end for m in q], dtype=np.uint64)
    x = None if pcm is None else np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1).copy()
    out = x if in_place else np.full(512 * n_blocks, 0x7777, dtype=np.int16)
    active = np.full(n_blocks, 9, dtype=np.uint8)
    clips = C.c_uint64(77)
    rc = lib.hrfd_afskgen_debug_slow(p(msgs) if q else None, p(bits), p(starts) if q else None, p(ends) if q else None, len(q), model.N,
                                     p(x), n_blocks, p(out), p(active), C.byref(clips))
    assert rc == 0, lib.hrfd_last_error().decode()
    return out.reshape(n_blocks, 512), active, int(clips.value)


def random_bits(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8)       # only bit 0 counts


# ---- the laws
@pytest.mark.parametrize("nrzi", [False, True])
def test_levels_equal_the_library_and_the_decoders_inverse(lib, nrzi):
    rng = np.random.default_rng(3 + nrzi)
    for n in BIT_COUNTS + (7, 100, 4097):
        bits = random_bits(rng, n)
        lv = gm.levels(bits, nrzi)
        assert (lib_levels(lib, bits, nrzi) == gm.pack_levels(lv)).all(), n
        if nrzi:
            assert (lv == am.nrzi_levels(bits & 1, start=1)).all()
            h = np.concatenate([[1], lv]).astype(np.int64)     # the decoder from a level of mark: 1 - (h ^ last)
            assert (1 - (h[1:] ^ h[:-1]) == (bits & 1)).all()
        else:
            assert (lv == (bits & 1)).all()
    assert gm.levels([0, 0, 1, 0], True).tolist() == [0, 1, 1, 0] and gm.levels([1, 1], True).tolist() == [1, 1]


def test_length_at_its_edges(lib):
    """(three bits at 1200 baud are 21 samples, not 20: round(0.15 x 2^32) = 644245094 lies below 0.15 x 2^32, so 20 steps stay
    8 short of 3 x 2^32, and L is the least k with (k baud_step) >> 32 >= B)"""
    for n_bits, baud_step, want in ((8192, 1 << 31, 16384), (3, gm.step(1200), 21), (3, gm.step(1200) + 1, 20), (1, 1 << 31, 2), (1, 1, None), (1, 2, None), (1, 3, 1431655766),
                                    (3 << 28, (3 << 29) + 1, (1 << 31) - 1), (3 << 28, 3 << 29, None),
                                    (8192, gm.step(300), -((-8192 << 32) // gm.step(300))),
                                    (0, 5, None), (5, 0, None), (5, (1 << 31) + 1, None)):
        got = lib_length(lib, n_bits, baud_step)
        assert got == want, (n_bits, baud_step, got)
        if want is not None:
            assert gm.length(n_bits, baud_step) == want
            assert ((want - 1) * baud_step) >> 32 == n_bits - 1 and (want * baud_step) >> 32 >= n_bits      # the bit bound at the end
        elif n_bits and 0 < baud_step <= 1 << 31:
            with pytest.raises(ValueError):
                gm.length(n_bits, baud_step)


@pytest.mark.parametrize("baud", sorted(BAUD_STEPS))
def test_bit_bound(lib, baud):
    """bit(L - 1) == B - 1, bit(k) < B for every k < L and the bits rise by at most one a sample"""
    r = BAUD_STEPS[baud]
    for B in BIT_COUNTS:
        L = gm.length(B, r)
        assert lib_length(lib, B, r) == L
        k = np.arange(L, dtype=np.int64)
        bit = (k * r) >> 32
        assert bit[-1] == B - 1 and bit.max() < B and bit[0] == 0 and (np.diff(bit) <= 1).all() and (np.diff(bit) >= 0).all()
        assert L == 1 or ((L - 2) * r) >> 32 <= B - 1


# ---- the model against the slow loop
@pytest.mark.parametrize("nrzi", [False, True])
@pytest.mark.parametrize("baud", sorted(BAUD_STEPS))
def test_model_equals_the_library_slow_loop(lib, baud, nrzi):
    r = BAUD_STEPS[baud]
    rng = np.random.default_rng(100 * nrzi + len(baud))
    for B in BIT_COUNTS:
        L = gm.length(B, r)
        n_blocks = min(-(-(L + 700) // 512), 6)
        g = gm.AfskGenModel(1)
        start = int(rng.integers(0, 600))
        g.queue(0, random_bits(rng, B), amplitude=int(rng.choice([1, 8000, 32767])), nrzi=nrzi, start=start,
                steps=(int(rng.integers(1, (1 << 31) + 1)), int(rng.integers(1, (1 << 31) + 1)), r))
        if L < 300:
            g.queue(0, random_bits(rng, 3), amplitude=32767, nrzi=nrzi, gap=int(rng.integers(0, 3)), steps=(gm.step(1200), gm.step(2200), 1 << 31))
        x = rng.integers(-32768, 32768, size=(1, 512 * n_blocks), dtype=np.int16)
        for call in range(2):                                  # the second call starts inside a long message
            want_out, want_act, want_clips = lib_slow(lib, g, 0, x, n_blocks)
            again, _, _ = lib_slow(lib, g, 0, x, n_blocks, in_place=True)
            gen, _, gen_clips = lib_slow(lib, g, 0, None, n_blocks)
            before = g.clips(0)
            out, act = g.process(x, want_active=True)
            assert (out[0] == want_out).all(), (B, call, np.argwhere(out[0] != want_out)[:4].tolist())
            assert (again == want_out).all() and (act[0] == want_act).all() and g.clips(0) - before == want_clips
            assert gen_clips == 0 and (np.abs(gen) <= 32767).all()
        assert act.max() <= 1


def test_random_queues_equal_the_slow_loop(lib):
    rng = np.random.default_rng(11)
    for trial in range(6):
        g = gm.AfskGenModel(1)
        g.set_time(int(rng.choice([0, (1 << 32) - 900, (1 << 40) + 3])))
        for i in range(4):
            g.queue(0, random_bits(rng, int(rng.integers(1, 200))), amplitude=int(rng.integers(0, 32768)), nrzi=bool(i & 1), gap=int(rng.choice([0, 1, 100, 700])),
                    steps=(int(rng.integers(1, 1 << 31)), int(rng.integers(1, 1 << 31)), int(rng.choice(list(BAUD_STEPS.values())))))
        with pytest.raises(ValueError, match="5 messages"):
            g.queue(0, [1], gap=5)
        for n_blocks in (1, 2, 3):
            x = rng.integers(-32768, 32768, size=(1, 512 * n_blocks), dtype=np.int16)
            want_out, want_act, want_clips = lib_slow(lib, g, 0, x, n_blocks)
            before = g.clips(0)
            out, act = g.process(x, want_active=True)
            assert (out[0] == want_out).all() and (act[0] == want_act).all() and g.clips(0) - before == want_clips, (trial, n_blocks)


# ---- a second, independent check: one tone is the tone generator's segment
@pytest.mark.parametrize("start", [0, 5, 511, (1 << 32) - 700])
def test_pure_tone_equals_the_tone_generator(start):
    rng = np.random.default_rng(start % 1000)
    for B, r in ((3, gm.step(1200)), (1, 1 << 31), (40, gm.step(300)), (700, gm.ODD_STEP)):
        L = gm.length(B, r)
        tone, amp = int(rng.integers(1, (1 << 31) + 1)), int(rng.choice([1, 9000, 32767]))
        a, t = gm.AfskGenModel(1), tm.ToneGenModel(1)
        base = start - start % 512
        t.set_time(base)
        a.set_time(base)
        a.queue(0, random_bits(rng, B), amplitude=amp, start=start, steps=(tone, tone, r))
        t.queue(0, 0, [(0, L, tone, 0, amp, 0)], start)
        n_blocks = -(-(start - base + L) // 512) + 1
        x = rng.integers(-32768, 32768, size=(1, 512 * n_blocks), dtype=np.int16)
        assert (a.process(x) == t.process(x)).all(), (B, r)
        assert a.clips(0) == t.clips(0) and a.pending(0) == (0, a.time())


# ---- invariance to the cut
@pytest.mark.parametrize("base", [0, (1 << 32) - 700])
def test_a_stream_cut_into_calls(base):
    """calls of 1 + 4 + 5 + 6 + 4 blocks against one of 20, a queue and a cut between the calls"""
    cuts = (1, 4, 5, 6, 4)
    rng = np.random.default_rng(21)
    x = rng.integers(-32768, 32768, size=(2, 512 * sum(cuts)), dtype=np.int16).reshape(2, -1, 512)
    first, late, third = random_bits(rng, 600), random_bits(rng, 90), random_bits(rng, 1200)
    parts = gm.AfskGenModel(2)
    parts.set_time(base)
    parts.queue(gm.ALL, first, start=base + 300)                            # 4000 samples: across the first three calls
    parts.queue(1, third, baud=300, mark_hz=1270, space_hz=1070, gap=7)     # 32000: to the end and beyond
    got, at = [], 0
    for i, k in enumerate(cuts):
        got.append(parts.process(x[:, at:at + k]))
        at += k
        if i == 1:
            parts.queue(0, late, amplitude=32767, nrzi=False, gap=33)       # behind the first, which is still in progress
        if i == 3:
            parts.cut(1)                                                    # the long one ramps down
    whole = gm.AfskGenModel(2)
    whole.set_time(base)
    whole.queue(gm.ALL, first, start=base + 300)
    whole.queue(0, late, amplitude=32767, nrzi=False, gap=33)
    whole.queue(1, third, baud=300, mark_hz=1270, space_hz=1070, gap=7)
    whole.q[1][-1].end = base + 512 * 16 + 64                               # what the cut left
    want = whole.process(x)
    assert (np.concatenate(got, axis=1) == want).all()
    assert [parts.clips(c) for c in range(2)] == [whole.clips(c) for c in range(2)] and parts.time() == whole.time() == base + 512 * 20
    whole.queue(0, [1, 0])
    with pytest.raises(ValueError, match="not ended"):
        whole.set_time(5)


def test_the_last_three_blocks_below_2_63():
    """a clock started at 2^63 - 3 x 512 - 1: calls of 1 + 2 blocks and 1 + 1 + 1 against one of 3, the message ending on the
    last stream time there is"""
    base = (1 << 63) - 3 * 512 - 1
    bits = random_bits(np.random.default_rng(41), 91)           # L = 607
    outs = []
    for cuts in ((3,), (1, 2), (1, 1, 1)):
        g = gm.AfskGenModel(1)
        g.set_time(base)
        g.queue(0, bits, amplitude=32767, gap=3 * 512 - 607)
        assert g.pending(0) == (1, (1 << 63) - 1)
        outs.append(np.concatenate([g.process(None, k) for k in cuts], axis=1))
        assert g.time() == (1 << 63) - 1 and g.pending(0) == (0, g.time())
    assert (outs[0] == outs[1]).all() and (outs[0] == outs[2]).all() and outs[0][0, 2, -2] != 0 and outs[0][0, 0, 0] == 0
    g = gm.AfskGenModel(1)
    g.set_time(base)
    with pytest.raises(ValueError, match="2\\^63"):
        g.queue(0, bits, amplitude=32767, gap=3 * 512 - 606)


def test_the_queue_rules():
    g = gm.AfskGenModel(2)
    g.queue(0, [1] * 3, start=1000)                            # L = 21
    assert g.pending(0) == (1, 1021) and g.pending(1) == (0, 0)
    for s in (980, 1000, 1020):
        with pytest.raises(ValueError, match="overlap"):
            g.queue(gm.ALL, [1] * 3, start=s)
    assert g.pending(1) == (0, 0)                              # refused whole
    g.queue(gm.ALL, [1] * 3, start=979)
    g.queue(0, [1] * 3)                                        # appended at 1021
    assert g.pending(0) == (3, 1042) and g.pending(1) == (1, 1000)
    g.process(None, 1)
    with pytest.raises(ValueError, match="before the stream time"):
        g.queue(1, [1], start=511)
    g.process(None, 1)                                         # N = 1024: two of channel 0 have ended, the third is in progress
    assert g.pending(0) == (1, 1042)
    g.cut(0)
    assert g.pending(0) == (1, 1042)                           # 18 samples were left: the end stays
    with pytest.raises(ValueError, match="not ended"):
        g.set_time(0)
    g.process(None, 1)
    g.set_time((1 << 63) - 512)
    with pytest.raises(ValueError, match="2\\^63"):
        g.queue(0, [1] * 3, gap=491)
    g.queue(0, [1] * 3, gap=490)
    assert g.pending(0) == (1, (1 << 63) - 1)


# ---- HDLC
def test_hdlc_encode_is_the_test_models_and_the_decoders_inverse():
    rng = np.random.default_rng(31)
    for trial in range(40):
        payloads = [rng.integers(0, 256, size=int(rng.integers(1, 60)), dtype=np.uint8).tobytes() for _ in range(int(rng.integers(1, 4)))]
        if trial % 5 == 0:
            payloads[0] = bytes([0xFF] * 9 + [0x7E, 0x3F])     # runs of ones: stuffing
        counts = (int(rng.integers(1, 20)), int(rng.integers(1, 4)), int(rng.integers(1, 5)))
        bits = api.hdlc_encode(payloads, *counts)
        want = am.hdlc_bits(payloads, *counts)
        assert bits.dtype == want.dtype and bits.tobytes() == want.tobytes()
        assert api.hdlc_frames(bits) == payloads
    assert api.hdlc_encode([b"A"]).tobytes() == am.hdlc_bits([b"A"]).tobytes()


# ---- the closed loop on the CPU
@pytest.mark.parametrize("modem", ["bell202", "bell103"])
def test_closed_loop_generate_decode(modem):
    """AfskGenModel -> AfskModel -> api.hdlc_frames: two frames of 40 random bytes at amplitudes 300, 8000 and 32767 without
    noise and 8000 under Gaussian noise of sigma 500, 0..299 samples of silence in front and 100 behind, seeds 1..20, the
    decoder cut into calls of 1, 4, 5, 6 blocks and the rest.  The 80 cases of a modem are the 80 channels of one decoder
    model (the shorter ones with digital silence behind them up to the longest).  Every frame of every case returns."""
    m = am.BELL202 if modem == "bell202" else am.BELL103
    cases = [(amplitude, sigma, seed) for amplitude, sigma in gm.LOOP_LEVELS for seed in gm.LOOP_SEEDS]
    made = [gm.loop_case(m, *case) for case in cases]
    n_blocks = max(pcm.shape[0] for _, pcm in made)
    x = np.zeros((len(cases), n_blocks, 512), dtype=np.int16)
    for c, (_, pcm) in enumerate(made):
        x[c, :pcm.shape[0]] = pcm
    dec = am.AfskModel(len(cases), **m)
    rows, at = [[] for _ in cases], 0
    for k in (1, 4, 5, 6, n_blocks):
        k = min(k, n_blocks - at)
        if k > 0:
            bits, _ = dec.process(x[:, at:at + k])
            for c in range(len(cases)):
                rows[c].append(bits[c])
            at += k
    lost = [case for c, case in enumerate(cases) if api.hdlc_frames(np.concatenate(rows[c])) != made[c][0]]
    assert not lost, f"{modem}: the frames of {len(lost)} of {len(cases)} cases did not return: {lost[:8]}"
