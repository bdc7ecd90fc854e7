"""The DUC bank's default filters, the properties of its numpy model (tests/duc_model.py), and the closed loop that
shows the defaults fit for purpose: WBFM stations through the modulator, the DUC model, the DDC model and the CPU
oracle's receive chain."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ddc_model as dm
from tests import duc_model as um
from tools import duc_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- design
def test_design_tool_regenerates_the_committed_header():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "duc_design.py"), "--check"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", ["DUC_A2", "DUC_A4", "DUC_A8"])
def test_default_filters_meet_their_specification(name):
    """quantised taps: ripple <= 0.1 dB, >= 60 dB from 2.048 MHz - 220 kHz, every branch sum |h| <= 65535, DC gain R"""
    q = duc_design.tables()[name]
    R = duc_design.SPECS[name][0]
    ripple, atten = duc_design.response(q, name)
    assert ripple <= 0.1 and atten >= 60.0, (ripple, atten)
    assert q.size <= 64 and (duc_design.branch_sums(q, R) <= 65535).all()
    for p in range(R):
        assert abs(int(q[p::R].astype(np.int64).sum()) - 32768) < 1200, (p, "each branch passes DC at about unity")


# ---- the model's properties
def lcg(C, n, seed):
    return np.random.default_rng(seed).integers(-128, 128, size=(C, n)).astype(np.int8)


def tuned(W, C, R):
    m = um.DucModel(W, C, R)
    for c in range(C):
        m.set_tuning(c, c % W, um.duc_step(-600_000 + 250_000 * c, R))
    return m


@pytest.mark.parametrize("R", [1, 4, 8])
def test_any_split_of_the_stream_gives_the_same_output(R):
    x = lcg(3, 2 * 3000, R)
    whole = tuned(2, 3, R).process(x, 6000)
    m = tuned(2, 3, R)
    parts, o = [], 0
    for n in (2, 318, 1000, 2, 1678):
        parts.append(m.process(x[:, o:o + 2 * n], 2 * n))
        o += 2 * n
    assert o == 6000 and (np.concatenate(parts, axis=1) == whole).all()


def test_retuning_is_phase_continuous():
    R = 4
    m = um.DucModel(1, 1, R)
    m.set_tuning(0, 0, um.duc_step(100_000, R))
    m.process(np.zeros((1, 200), dtype=np.int8), 200)
    before = m.phase(0)
    m.set_tuning(0, 0, um.duc_step(-300_000, R))
    assert m.phase(0) == before
    assert m.phase(0, m.N + 5) == (before + 5 * um.duc_step(-300_000, R)) & um.MASK32


def spectrum(S, fs):
    z = (S[0] + 1j * S[1]).astype(np.complex128)
    z = z[z.size // 8:]
    sp = np.abs(np.fft.fft(z * np.blackman(z.size))) ** 2
    return np.fft.fftfreq(z.size, 1 / fs), sp


@pytest.mark.parametrize("R", [2, 4, 8])
def test_a_tone_lands_at_its_offset_with_images_60_db_down(R):
    """a tone 30 kHz above a channel's DC, tuned to +f: the peak at f + 30 kHz, everything outside +-300 kHz of it
    (the zero-stuffing images at k x 2.048 MHz) at least 60 dB below, measured on S"""
    f, ft, M = 410_000.0, 30_000.0, 16384
    m = um.DucModel(1, 1, R)
    m.set_tuning(0, 0, um.duc_step(f, R))
    t = np.arange(M)
    x = np.stack([np.round(100 * np.cos(2 * np.pi * ft * t / um.FS_CH)),
                  np.round(100 * np.sin(2 * np.pi * ft * t / um.FS_CH))], axis=1).astype(np.int8)
    _, st = m.process(x.reshape(1, -1), 2 * M, stages=True)
    fr, sp = spectrum(st["S"][0], R * um.FS_CH)
    assert abs(fr[np.argmax(sp)] - (f + ft)) < 2000
    far = np.abs(fr - (f + ft)) > 300_000
    assert 10 * np.log10(sp.max() / sp[far].max()) >= 60.0


def test_a_wbfm_channel_stays_inside_220_khz(oracle):
    """a WBFM channel from count.raw through the oracle's modulator at R = 8: its power beyond +-220 kHz of its centre
    is >= 55 dB below the in-band power (stage B's splatter guard and stage A's image rejection), measured on S"""
    R, f = 8, -1_500_000.0
    pcm = dm.count_raw()[9000:9000 + 2048]
    x = oracle.wbfmmod().process(pcm)
    m = um.DucModel(1, 1, R)
    m.set_tuning(0, 0, um.duc_step(f, R))
    _, st = m.process(x.reshape(1, -1), x.size, stages=True)
    fr, sp = spectrum(st["S"][0], R * um.FS_CH)
    inband = sp[np.abs(fr - f) <= 220_000].sum()
    outband = sp[np.abs(fr - f) > 220_000].sum()
    assert 10 * np.log10(inband / outband) >= 55.0


def test_clip_count_equals_a_direct_count():
    R, W, C = 2, 2, 5
    m = tuned(W, C, R)
    m.set_output_shift(0, 6)
    m.set_output_shift(1, 7)
    want = np.zeros(W, dtype=np.int64)
    for call in range(3):
        out, st = m.process(lcg(C, 1200, call), 1200, stages=True)
        for w in range(W):
            s = int(m.shift[w])
            y = (st["S"][w] + (1 << (s - 1))) >> s
            want[w] += int(((y > 127) | (y < -128)).sum())
            assert (out[w].reshape(-1, 2).T == np.clip(y, -128, 127)).all()
    assert (m.clips == want).all() and want.min() > 0
    m.reset()
    assert not m.clips.any()


# ---- the closed loop on the models
@pytest.fixture(scope="module")
def closed_loop(oracle):
    streams, audio, amps = um.loop_stations(oracle)
    cap, m = um.loop_duc(streams, amps)
    d = dm.DdcModel(1, 2, dm.SEL_R)
    for c, f in enumerate(dm.SEL_OFFSETS):
        d.set_tuning(c, 0, dm.ddc_step(f + 64_000, dm.SEL_R))
        d.set_gain_shift(c, dm.SEL_GAIN_SHIFT[c])
    rx_in = d.process(cap, dm.SEL_BLOCKS * 262144)
    pcm = [dm.oracle_rx_wbfm(oracle, rx_in[c]) for c in range(2)]
    return audio, m, cap, pcm


def test_closed_loop_two_wbfm_stations_400_khz_apart(closed_loop):
    """The DDC selectivity test's stations, built by the DUC instead of float upsampling.  Measured: own audio 0.974 /
    0.990 (weak / strong station), the other station's 0.040 / 0.040 (the excerpts' own floor is 0.047)."""
    audio, m, cap, pcm = closed_loop
    assert m.clips[0] == 0, "the levels fit int8 at the default shift"
    rms = np.sqrt(np.mean(cap.astype(np.float64) ** 2) * 2)
    assert 40 < rms < 120
    for c in range(2):
        own = dm.best_corr(audio[c], pcm[c])
        other = dm.best_corr(audio[1 - c], pcm[c])
        assert own >= 0.85 and other <= 0.05, (c, own, other)
