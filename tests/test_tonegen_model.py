"""The tone generator bank's model (tests/tonegen_model.py) against the contract restated sample by sample in Python integers,
and what the bank is for, decoded by the tone bank's model (tests/tone_model.py): every DTMF key over a range of amplitudes,
every CTCSS tone clean and under noise, and the closed loop of tests/test_tone_model.py with the generator's audio.  CPU only."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import tone_model as tm
from tests import tonegen_model as gm


def seg(length, step_a=0, amp_a=0, step_b=0, amp_b=0, gap=0):
    return (gap, length, step_a, step_b, amp_a, amp_b)


def agree(m, x, n_blocks, what):
    """one call of the model against the slow restatement from the same state"""
    clips_before = [m.clips(c) for c in range(m.C)]
    want, want_active, want_clips = gm.slow(m, x, n_blocks)
    out, active = m.process(x, n_blocks, want_active=True)
    assert out.dtype == np.int16 and out.shape == (m.C, n_blocks, 512) and active.shape == (m.C, n_blocks)
    assert out.reshape(m.C, -1).tolist() == want, what
    assert active.tolist() == want_active, what
    assert [m.clips(c) - clips_before[c] for c in range(m.C)] == want_clips, what
    return out


# 1. the model equals the contract sample by sample
def test_model_equals_the_contract_sample_by_sample():
    rng = np.random.default_rng(5)
    m = gm.ToneGenModel(3)
    steps = [int(v) for v in rng.integers(0, 1 << 32, size=8, dtype=np.uint64)]
    # channel 0: lengths around the ramp, back to back and with gaps, from sample 1; a tone without an end on track 1
    m.queue(0, 0, [seg(n, steps[i % 8], 32767, steps[(i + 3) % 8], 32767, gap=i % 3) for i, n in enumerate((1, 2, 63, 64, 65, 127, 128, 129))], 1)
    m.queue(0, 1, [seg(gm.FOREVER, steps[2], 32767, steps[5], 20000)], 511)
    # channel 1: 32 segments of 64 samples, gap 0; track 1 overlaps them and ends on the call's last sample
    m.queue(1, 0, [seg(64, steps[i % 8], 9000 + i, 0, 0) for i in range(32)], 0)
    m.queue(1, 1, [seg(1536 - 700, steps[7], 12345, steps[1], 4321)], 700)
    # channel 2 idle
    x = rng.integers(-32768, 32768, size=(3, 1536), dtype=np.int16)
    x[0, 600:900] = 32767
    x[0, 900:1200] = -32768
    first = agree(m, x, 3, "the first call")
    assert (first[2].reshape(-1) == x[2]).all() and m.clips(0) > 0 and m.clips(2) == 0
    assert m.pending(0, 0) == (0, 1536) and m.pending(0, 1) == (1, gm.NO_END) and m.pending(1, 1) == (0, 1536)
    # the call behind: a cut ramps the endless tone down, a queue in front of the clock is refused and changes nothing
    m.cut(0, 1)
    assert m.pending(0, 1) == (1, 1536 + 64)
    with pytest.raises(ValueError, match="before the stream time"):
        m.queue(2, 0, [seg(10)], 1535)
    m.queue(2, 0, [seg(100, steps[0], 100, steps[1], 200, gap=5)])
    assert m.pending(2, 0) == (1, 1536 + 105)
    agree(m, None, 1, "generate only behind a cut")
    assert m.time() == 2048 and m.pending(0, 1) == (0, 2048)
    # across 2^32, and k at and above 2^32 under an endless segment queued long before
    m.reset()
    assert m.time() == 0 and m.clips(0) == 0
    m.queue(1, 1, [seg(gm.FOREVER, steps[4], 30000, steps[6], 1)], 0)
    m.set_time((1 << 32) - 1024)
    m.queue(0, 0, [seg(1500, steps[3], 25000, steps[0], 7000)], (1 << 32) - 700)
    agree(m, x[:, :1024], 2, "up to 2^32")
    agree(m, x[:, :1024], 2, "from 2^32")
    m.set_time((1 << 32) + 5)
    agree(m, x[:, :512], 1, "k above 2^32")


def test_queue_rules():
    m = gm.ToneGenModel(2)
    m.queue(gm.ALL, 0, [seg(100), seg(50, gap=10)], 1000)
    assert m.pending(0, 0) == m.pending(1, 0) == (2, 1160)
    m.queue(0, 0, [seg(10)], 1100)                                         # into the gap
    m.queue(0, 0, [seg(1000)], 0)                                          # in front
    assert m.pending(0, 0) == (4, 1160)
    for start in (999, 1099, 1101, 1159, 1):
        with pytest.raises(ValueError, match="overlap"):
            m.queue(0, 0, [seg(2 if start > 1 else 1000)], start)
    with pytest.raises(ValueError, match="overlap"):                       # refused whole: channel 1 would have taken it
        m.queue(gm.ALL, 0, [seg(1000)], 0)
    assert m.pending(1, 0) == (2, 1160)
    m.queue(0, 0, [seg(gm.FOREVER)])
    assert m.pending(0, 0) == (5, gm.NO_END)
    for start in (gm.APPEND, 5000):
        with pytest.raises(ValueError, match="FOREVER"):
            m.queue(0, 0, [seg(1)], start)
    with pytest.raises(ValueError, match="FOREVER"):
        m.queue(1, 0, [seg(gm.FOREVER), seg(1)])
    with pytest.raises(ValueError, match="amp"):
        m.queue(1, 0, [seg(1, 0, 32768)])
    with pytest.raises(ValueError, match="length 0"):
        m.queue(1, 0, [seg(0)])
    m.queue(1, 1, [seg(1)] * 32)
    with pytest.raises(ValueError, match="33 segments"):
        m.queue(1, 1, [seg(1)])
    m.process(None, 1)                                                     # 32 samples on: all have ended
    m.queue(1, 1, [seg(1)] * 32)
    assert m.pending(1, 1) == (32, 512 + 32)
    # cut: in progress -> 64 samples more at the most; not yet begun -> gone
    m.set_time(1050)
    m.cut(gm.ALL, 0)
    assert m.pending(1, 0) == (1, 1100) and m.pending(0, 0) == (1, 1100)
    m.reset()
    m.queue(0, 0, [seg(5000)], 0)
    m.set_time(100)
    m.cut(0, 0)
    assert m.pending(0, 0) == (1, 164)


# 2. every DTMF key, 96 ms on and 32 ms off, at five amplitudes: decoded by the tone bank's model under its default thresholds
DTMF_AMPS = (64, 200, 1000, 8000, 16383)
DTMF_ORDER = "123A456B789C*0#D"


def dtmf_queue(bank, channel, amp):
    segs = []
    for j, key in enumerate(DTMF_ORDER):
        lo, hi = api.tonegen_dtmf(key)
        segs.append(api.tonegen_segment(768, lo, amp, hi, amp, gap=256 if j else 0))
    bank.queue(channel, 0, segs, 0)


def dtmf_decoder(m):
    m.set_tones([api.tone_step(f) for f in api.DTMF_LOW_HZ + api.DTMF_HIGH_HZ], [0] * 4 + [1] * 4)


def dtmf_check(best, present, what):
    for j in range(16):
        r, col = divmod(j, 4)
        for f in (4 * j + 1, 4 * j + 2):
            assert (best[f, 0], best[f, 1]) == (r, 4 + col) and present[f, 0] == 1 and present[f, 1] == 1, (what, j, f, best[f], present[f])
            assert api.dtmf_digit(best[f, 0], best[f, 1] - 4) == DTMF_ORDER[j]
        assert present[4 * j + 3, 0] == 0 and present[4 * j + 3, 1] == 0, (what, j, present[4 * j + 3])


def test_every_dtmf_key_is_decoded():
    gen = gm.ToneGenModel(len(DTMF_AMPS))
    for c, amp in enumerate(DTMF_AMPS):
        dtmf_queue(gen, c, amp)
    pcm, active = gen.process(None, 32, want_active=True)
    assert (active == 1).all() and all(gen.clips(c) == 0 for c in range(gen.C))
    dec = tm.ToneModel(gen.C, 256)
    dtmf_decoder(dec)
    P, E, V, B, Pr = dec.process(pcm)
    for c, amp in enumerate(DTMF_AMPS):
        dtmf_check(B[c], Pr[c], f"amp {amp}")


# 3. every CTCSS tone as a segment without an end, decoded among all 50
def ctcss_pcm(amp):
    gen = gm.ToneGenModel(len(api.CTCSS_HZ))
    for c, f in enumerate(api.CTCSS_HZ):
        gen.ctcss(c, f, amplitude=amp)
    return gen.process(None, 24).reshape(gen.C, -1)


def ctcss_decoder():
    dec = tm.ToneModel(len(api.CTCSS_HZ), 4096)
    dec.set_tones([api.tone_step(f) for f in api.CTCSS_HZ], [2] * len(api.CTCSS_HZ))
    return dec


def test_every_ctcss_tone_is_decoded():
    K = len(api.CTCSS_HZ)
    P, E, V, B, Pr = ctcss_decoder().process(ctcss_pcm(300))
    assert B.shape == (K, 3, 4)
    assert (B[:, :, 2] == np.arange(K)[:, None]).all() and (Pr[:, :, 2] == 1).all(), (B[:, :, 2].tolist(), Pr[:, :, 2].tolist())
    noise = np.random.default_rng(11).normal(0.0, 3000.0, size=(K, 3 * 4096))
    noisy = np.clip(np.round(ctcss_pcm(1000) + noise), -32768, 32767).astype(np.int16)
    P, E, V, B, Pr = ctcss_decoder().process(noisy)
    assert (B[:, :, 2] == np.arange(K)[:, None]).all(), B[:, :, 2].tolist()


def test_helpers():
    m = gm.ToneGenModel(2)
    m.dial(0, "5#")
    assert m.pending(0, 0) == (2, 2 * (256 + 768))
    s = m.track[0][0][1]
    assert (s.start, s.step_a, s.step_b, s.amp_a, s.amp_b) == (1024 + 256, api.tone_step(941.0), api.tone_step(1477.0), 8000, 8000)
    with pytest.raises(ValueError, match="33 segments"):                  # a track holds 32: refused whole
        m.dial(0, "1" * 31)
    m.dial(0, "1" * 30)
    assert m.pending(0, 0) == (32, 32 * 1024)
    m.ctcss(gm.ALL, 100.0)
    assert m.pending(1, 1) == (1, gm.NO_END) and m.track[1][1][0].amp_a == 1000
    m.burst(1)
    assert m.pending(1, 0) == (1, 4000) and m.track[1][0][0].step_a == api.tone_step(1750.0)
    m.tones(1, [1000.0, 2000.0, 1500.0], 70, gap_ms=10)
    assert m.pending(1, 0) == (4, 4000 + 3 * 560 + 2 * 80)
    with pytest.raises(ValueError, match="DTMF"):
        m.dial(0, "x")
    assert api.tonegen_samples(96) == 768 and api.tonegen_segment(5, 1000.0, 7, gap=2) == (2, 5, 1 << 29, 0, 7, 0)
    assert api.TONEGEN_APPEND == gm.APPEND and api.TONEGEN_FOREVER == gm.FOREVER


# 4. the closed loop of tests/test_tone_model.py on the models and the CPU oracle, with the generator's audio
def test_closed_loop_dtmf_over_two_wbfm_stations(oracle):
    audio, amps, duc_clips, pcm, gen_clips = gm.loop_reference(oracle)
    assert duc_clips == 0 and gen_clips == 0
    m = tm.loop_model()
    P, E, V, B, Pr = m.process(pcm)
    frac = api.tone_fraction(P, E, m.window)
    print("fractions of the decoded frames: rows", frac[:, 1::2, :4].max(axis=2).min(), "columns", frac[:, 1::2, 4:8].max(axis=2).min(),
          "pilot", frac[0, 1::2, 8].min(), "against", frac[1, 1::2, 8].max())
    tm.loop_check(B, Pr)
