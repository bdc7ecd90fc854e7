"""tests/afsk_model.py against the library's own statement of the AFSK bank's law (hrfd_afsk.h, reached on the host through
hrfd_afsk_debug_taps and hrfd_afsk_debug_slow: no device), against the bounds the contract states, against every cut of a
stream into calls, and end to end: HDLC frames through a floating-point AFSK generator, the model and api.hdlc_frames.
No GPU."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import afsk_model as am

MODEMS = [dict(am.BELL202), dict(am.BELL103), dict(mark_hz=1200, space_hz=2200, baud=1200, window=7, loop_shift=1),
          dict(mark_hz=1200, space_hz=1800, baud=4000, window=2, loop_shift=8),
          dict(mark_hz=3999.9, space_hz=0.01, baud=300, window=32, loop_shift=3)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def slow(lib, model_args, nrzi, min_power, pcm, n_pcm, state, want_bits=True):
    """hrfd_afsk.h's loop over one channel: (bits or None, hard [n_blocks, 64]); state (18 dwords) is replaced"""
    m = np.array([am.step(model_args["mark_hz"]), am.step(model_args["space_hz"]), am.step(model_args["baud"]),
                  model_args["window"], model_args["loop_shift"], 1 if nrzi else 0], dtype=np.uint32)
    x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1, 512)
    n_blocks = x.shape[0]
    npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32)
    bits = np.full(am.max_bits(int(m[2]), int(m[4]), n_blocks) + 8, 0xEE, dtype=np.uint8)
    n_bits = np.zeros(1, dtype=np.uint32)
    hard = np.zeros((n_blocks, 64), dtype=np.uint8)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = lib.hrfd_afsk_debug_slow(m.ctypes.data_as(C.POINTER(C.c_uint32)), min_power, p(x), p(npc), n_blocks,
                                  state.ctypes.data_as(C.POINTER(C.c_uint32)), p(bits) if want_bits else None,
                                  p(n_bits) if want_bits else None, p(hard))
    assert rc == 0, lib.hrfd_last_error().decode()
    if not want_bits:
        return None, hard
    assert (bits[n_bits[0]:] == 0xEE).all() and n_bits[0] <= bits.size - 8
    return bits[:n_bits[0]].copy(), hard


@pytest.mark.parametrize("index", range(len(MODEMS)))
def test_taps_match_the_library_entry_for_entry(lib, index):
    m = MODEMS[index]
    out = np.full(128, 77, dtype=np.int16)
    rc = lib.hrfd_afsk_debug_taps(am.step(m["mark_hz"]), am.step(m["space_hz"]), m["window"], out.ctypes.data_as(C.POINTER(C.c_int16)))
    assert rc == 0, lib.hrfd_last_error().decode()
    got = out.reshape(4, 32)
    want = am.taps(am.step(m["mark_hz"]), am.step(m["space_hz"]), m["window"])
    assert (got[:, :m["window"]] == want).all() and (got[:, m["window"]:] == 0).all()
    assert np.abs(want).max() <= 2047 and want[0, 0] == 2047 and want[1, 0] == 0          # cos 0 clamps to 2047, sin 0 = 0


@pytest.mark.parametrize("nrzi", [False, True])
@pytest.mark.parametrize("index", range(len(MODEMS)))
def test_model_equals_the_library_slow_loop(lib, index, nrzi):
    """two channels, two calls (the second starts from the first one's state), n_pcm of every kind, a carrier threshold"""
    m = MODEMS[index]
    rng = np.random.default_rng(10 * index + nrzi)
    C_, B = 2, 3
    model = am.AfskModel(C_, nrzi=nrzi, **m)
    min_power = [0, 1 << 40, (1 << 64) - 1][(index + nrzi) % 3]
    model.set_carrier(min_power)
    states = [np.zeros(18, dtype=np.uint32) for _ in range(C_)]
    for call in range(2):
        pcm = np.stack([am.noisy_afsk(rng, m, B) for _ in range(C_)])
        n_pcm = rng.choice(np.array([0, 1, 300, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32), size=(C_, B)) if call else None
        bits, hard = model.process(pcm, n_pcm)
        for c in range(C_):
            b, h = slow(lib, m, nrzi, min_power, pcm[c], None if n_pcm is None else n_pcm[c], states[c])
            assert (h == hard[c]).all(), (index, call, c, "hard")
            assert b.tolist() == bits[c].tolist(), (index, call, c, "bits")
            assert states[c][16] == model.phi[c] and states[c][17] == model.h_prev[c] | (model.last[c] << 1)
            kept = states[c][:16].view(np.int16)[32 - (m["window"] - 1):]
            assert kept.tolist() == model.hist[c].tolist()
        assert len(bits[0]) > 0


def test_a_call_without_bits_leaves_the_clock_alone(lib):
    rng = np.random.default_rng(5)
    m = am.BELL202
    pcm = np.stack([am.noisy_afsk(rng, m, 2) for _ in range(3)])
    model = am.AfskModel(1, **m)
    state = np.zeros(18, dtype=np.uint32)
    for call, want_bits in enumerate((True, False, True)):
        bits, hard = model.process(pcm[call][None], want_bits=want_bits)
        b, h = slow(lib, m, True, 0, pcm[call], None, state, want_bits=want_bits)
        assert (h == hard[0]).all() and (bits is None) == (b is None)
        if want_bits:
            assert b.tolist() == bits[0].tolist()
        assert state[16] == model.phi[0] and state[17] == model.h_prev[0] | (model.last[0] << 1)


@pytest.mark.parametrize("baud,A", [(1200, 1), (4000, 1), (300, 8)])
def test_max_bits_holds_on_full_scale_random_input(baud, A):
    """full-scale noise flips the decision as often as anything can: the count stays within the bound, and within one bit per
    sample; the int32 and 64-bit bounds hold with it"""
    rng = np.random.default_rng(baud + A)
    C_, B = 4, 4
    model = am.AfskModel(C_, baud=baud, window=32, loop_shift=A, nrzi=False)
    pcm = rng.choice(np.array([-32768, 32767], dtype=np.int16), size=(C_, B, 512))
    pcm[1] = rng.integers(-32768, 32768, size=(B, 512))
    bits, hard = model.process(pcm)                          # (the model asserts count < max_bits as it goes)
    cap = model.max_bits(B)
    assert cap == api.afsk_max_bits(am.step(baud), A, B) == ((512 * B * (am.step(baud) + ((1 << 31) >> A))) >> 32) + 1
    nominal = 512 * B * baud / 8000
    for c in range(C_):
        assert nominal / 4 < len(bits[c]) <= min(cap, 512 * B), (c, len(bits[c]), cap)
    assert model.max_abs_i < 1 << 31 and model.max_power < 1 << 63
    flips = np.abs(np.diff(am.unpack_hard(hard).astype(np.int64), axis=1)).sum(axis=1)
    assert (flips > 100).all()                               # the nudge was exercised


@pytest.mark.parametrize("index", range(len(MODEMS)))
def test_a_stream_cut_1_4_5_6_gives_the_bits_and_hard_of_one_call(index):
    m = MODEMS[index]
    rng = np.random.default_rng(200 + index)
    C_, B = 2, 16
    pcm = np.stack([am.noisy_afsk(rng, m, B) for _ in range(C_)])
    n_pcm = rng.choice(np.array([0, 100, 512, 600], dtype=np.uint32), size=(C_, B))
    n_pcm[0] = 512
    whole = am.AfskModel(C_, **m)
    bits, hard = whole.process(pcm, n_pcm)
    cut = am.AfskModel(C_, **m)
    parts, at = [], 0
    for k in (1, 4, 5, 6):
        parts.append(cut.process(pcm[:, at:at + k], n_pcm[:, at:at + k]))
        at += k
    assert (np.concatenate([p[1] for p in parts], axis=1) == hard).all()
    for c in range(C_):
        assert np.concatenate([p[0][c] for p in parts]).tolist() == bits[c].tolist()
    assert (cut.phi == whole.phi).all() and (cut.last == whole.last).all() and (cut.hist == whole.hist).all()


def test_hdlc_frames_on_a_clean_bit_stream():
    rng = np.random.default_rng(9)
    payloads = [bytes([0xFF] * 7), bytes([0x7E, 0x7E, 0x3F, 0xFC]), b"\x00", rng.integers(0, 256, 40, dtype=np.uint8).tobytes()]
    bits = am.hdlc_bits(payloads)
    assert api.crc16_x25(b"123456789") == 0x906E
    assert api.hdlc_frames(bits) == payloads
    assert api.hdlc_frames(bits | 2) == payloads             # the carrier flag does not count
    cut = len(bits) // 2                                     # joined streams: a frame may span calls
    assert api.hdlc_frames(np.concatenate([bits[:cut], bits[cut:]])) == payloads
    bad = bits.copy()
    bad[12 * 8 + 20] ^= 1                                    # one bit of the first frame
    assert api.hdlc_frames(bad) == payloads[1:]
    assert api.hdlc_frames(np.ones(100, dtype=np.uint8)) == [] and api.hdlc_frames([]) == []


@pytest.mark.parametrize("seed", am.E2E_SEEDS)
@pytest.mark.parametrize("name,modem,amplitude,sigma", am.E2E_CASES, ids=[c[0] for c in am.E2E_CASES])
def test_frames_come_back_end_to_end(name, modem, amplitude, sigma, seed):
    payloads, pcm = am.e2e_signal(modem, amplitude, sigma, seed)
    model = am.AfskModel(1, **modem)
    bits, _ = model.process(pcm[None])
    assert api.hdlc_frames(bits[0]) == payloads, name
