"""tests/dcs_model.py against the library's own slow loop (hrfd_dcs_debug_slow, the contract of include/hrfd.h sample by sample in
plain C++), the code words against their anchors, the same bytes for every cut of a stream into calls, detection under the
defaults, and the squelch the verdicts drive.  No GPU, and no tolerance anywhere: everything is integer."""
import ctypes as C

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api
from tests import dcs_model as dm

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def distinct_codes(K, first=()):
    """K (code, inverted) pairs no two of which are aliases, `first` in front"""
    out, seen = [], set()
    for code, inv in list(first) + [(c, i) for i in (False, True) for c in range(512)]:
        cw = dm.canonical(dm.word(code, inv))
        if cw not in seen and len(out) < K:
            seen.add(cw)
            out.append((code, inv))
    assert len(out) == K
    return [c for c, _ in out], [i for _, i in out]


def slow(lib, m, pcm_row, n_pcm_row, state, codes, inv, grp):
    """one channel through hrfd_dcs_debug_slow under the model's settings; `state` (uint32 [300]) is replaced"""
    x = np.ascontiguousarray(pcm_row, dtype=np.int16).ravel()
    B, K = x.size // 512, len(codes)
    taps = m.taps.astype(np.int16)
    c16, i8, g8 = np.array(codes, dtype=np.uint16), np.array(inv, dtype=np.uint8), np.array(grp, dtype=np.uint8)
    mh = m.min_hits.astype(np.uint32)
    npc = None if n_pcm_row is None else np.ascontiguousarray(n_pcm_row, dtype=np.uint32)
    hits, best, present = np.zeros((B, K), dtype=np.uint16), np.zeros((B, 4), dtype=np.uint8), np.zeros((B, 4), dtype=np.uint8)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = lib.hrfd_dcs_debug_slow(p(taps), taps.size, p(c16), p(i8), p(g8), K, p(mh), p(x), p(npc), B, p(state),
                                 p(hits) if K else None, p(best), p(present))
    assert rc == 0, lib.hrfd_last_error().decode()
    return hits, best, present


# a. the words
def test_code_words_and_their_anchors(lib):
    assert dm.word(0o023) == 0x763813 == api.dcs_word(0o023)
    same = [c for c in range(512) if dm.canonical(dm.word(c)) == dm.canonical(dm.word(0o023))]
    comp = [c for c in range(512) if dm.canonical(dm.word(c)) == dm.canonical(dm.word(0o023, True))]
    assert same == [0o023, 0o340, 0o766] and comp == [0o047, 0o375, 0o707]
    assert api.dcs_aliases(0o023) == (same, comp)
    assert dm.canonical(dm.word(0o023, True)) == dm.canonical(dm.word(0o047))          # D023I = D047N
    for code in range(512):
        for inv in (False, True):
            w, cw = C.c_uint32(0), C.c_uint32(0)
            assert lib.hrfd_dcs_code_word(code, int(inv), C.byref(w), C.byref(cw)) == 0
            assert w.value == dm.word(code, inv) == api.dcs_word(code, inv)
            assert cw.value == dm.canonical(w.value) == api.dcs_canonical(w.value)
            assert (w.value & 0xFFF) == (0x800 | code if not inv else (0x800 | code) ^ 0xFFF)
            if not inv:
                assert all(dm.polymod(dm.rot23(w.value, r)) == 0 for r in range(23)), oct(code)
    assert lib.hrfd_dcs_code_word(512, 0, C.byref(w), C.byref(cw)) == EINVAL
    assert dm.DELAY[0] == 0 and dm.DELAY[22] == 1309 and dm.DELAY[1] == 59 and dm.DELAY[21] == 1250


def random_taps(rng, T):
    h = rng.integers(-32768, 32768, size=T).astype(np.int64)
    scale = 65535.0 / np.abs(h).sum()
    if scale < 1.0:
        h = np.trunc(h * scale).astype(np.int64)
    return h


def taps_for(T, rng):
    return {1: np.array([16384]), 2: np.array([-20000, 30000]), 255: api.dcs_lowpass_taps()}.get(T, random_taps(rng, T))


# b. the model against the library's slow loop
@pytest.mark.parametrize("with_n_pcm", [False, True])
@pytest.mark.parametrize("K", [0, 1, 128])
@pytest.mark.parametrize("T", [1, 2, 255, 512])
def test_model_equals_the_slow_loop(lib, T, K, with_n_pcm):
    rng = np.random.default_rng(1000 * T + 10 * K + with_n_pcm)
    Cn = 2                                                  # channel 0: random PCM, channel 1: D754 under noise
    codes, inv = distinct_codes(K, [(0o754, False)])
    grp = [int(g) for g in rng.integers(0, 3, size=K)]      # group 3 stays empty
    m = dm.DcsModel(Cn)
    m.set_taps(taps_for(T, rng))
    m.set_codes(codes, inv, grp)
    m.set_min_hits(dm.ALL, 100)
    m.set_min_hits(1, 1)
    state = [np.zeros(dm.STATE_DW, dtype=np.uint32) for _ in range(Cn)]
    t0, some = 0, 0
    for B in (4, 1, 3):                                     # state carried over three calls
        n = 512 * B
        pcm = np.stack([rng.integers(-32768, 32768, size=n), dm.levels(0o754, n, 2000, t0) + dm.white(rng, n, 300.0)])
        pcm = dm.to_pcm(pcm).reshape(Cn, B, 512)
        n_pcm = rng.choice(np.array([0, 1, 511, 512, 513, 0xFFFFFFFF], dtype=np.uint32), size=(Cn, B)) if with_n_pcm else None
        hits, best, present = m.process(pcm, n_pcm)
        for c in range(Cn):
            h, b, p = slow(lib, m, pcm[c], None if n_pcm is None else n_pcm[c], state[c], codes, inv, grp)
            assert (h == hits[c]).all() and (b == best[c]).all() and (p == present[c]).all(), (T, K, B, c)
            assert (state[c] == m.state()[c]).all(), (T, K, B, c)
        assert (best[:, :, 3] == dm.NO_BEST).all() and (present[:, :, 3] == 0).all()
        some += int(hits.sum())
        t0 += n
    if K and T in (1, 255) and not with_n_pcm:
        assert some > 1000                                  # the comparison is not one of zeros


# c. cut anywhere
def test_every_cut_gives_the_same_outputs(lib):
    rng = np.random.default_rng(5)
    B = 12
    codes, inv = distinct_codes(3, [(0o754, False), (0o023, True)])
    grp = [0, 1, 0]
    pcm = dm.to_pcm(np.stack([dm.levels(0o754, 512 * B, 2000) + dm.white(rng, 512 * B, 500.0),
                              dm.levels(0o023, 512 * B, 900, 77, True) + dm.white(rng, 512 * B, 100.0)])).reshape(2, B, 512)
    n_pcm = np.full((2, B), 512, dtype=np.uint32)
    n_pcm[1, 7] = 100

    def run(cuts, through_slow):
        m = dm.DcsModel(2)
        m.set_taps(api.dcs_lowpass_taps())
        m.set_codes(codes, inv, grp)
        state = [np.zeros(dm.STATE_DW, dtype=np.uint32) for _ in range(2)]
        parts, at = [], 0
        for k in cuts:
            if through_slow:
                per = [slow(lib, m, pcm[c, at:at + k], n_pcm[c, at:at + k], state[c], codes, inv, grp) for c in range(2)]
                parts.append([np.stack([per[c][i] for c in range(2)]) for i in range(3)])
            else:
                parts.append(m.process(pcm[:, at:at + k], n_pcm[:, at:at + k]))
            at += k
        return [np.concatenate([p[i] for p in parts], axis=1) for i in range(3)], (np.stack(state) if through_slow else m.state())

    whole, st = run([B], False)
    assert whole[2][0, 4:, 0].all() and whole[2][1, 4:7, 1].all()      # both codes are seen: the cuts below cut something
    for cuts in ([1] * 12, [5, 1, 6], [3, 3, 3, 3]):       # single blocks reach three calls back for their bits
        for through_slow in (False, True):
            got, s = run(cuts, through_slow)
            assert all((a == b).all() for a, b in zip(got, whole)) and (s == st).all(), (cuts, through_slow)


# d. detection with the defaults
def detector(codes, inv=None):
    m = dm.DcsModel(1)
    m.set_taps(api.dcs_lowpass_taps())
    m.set_codes(codes, inv)
    return m


def test_default_taps():
    h = api.dcs_lowpass_taps()
    assert h.dtype == np.int16 and h.size == 255 and (h == h[::-1]).all() and abs(int(h.sum()) - 16384) < 64
    assert int(np.abs(h.astype(np.int64)).sum()) == 27415
    assert api.dcs_lowpass_taps(1).tolist() == [16384]
    for bad in (0, 513):
        with pytest.raises(ValueError):
            api.dcs_lowpass_taps(bad)
    x = api.dcs_levels(0o754, 3000, 2000, 123)
    assert x.dtype == np.int16 and (x == dm.levels(0o754, 3000, 2000, 123)).all() and set(x.tolist()) == {-2000, 2000}
    assert (api.dcs_levels(0o754, 3000, 2000, 123, True) == -x).all()
    # bit 0 goes first: the 23 bits from time 0 on, sampled mid-bit, are the word
    mid = [int(api.dcs_levels(0o023, 1400, 1)[(1250 * k + 625) // 21]) for k in range(23)]
    assert sum((1 if v > 0 else 0) << k for k, v in enumerate(mid)) == 0x763813


@pytest.mark.parametrize("noise_rms", [0.0, 4000.0])
def test_d754_is_found_clean_and_under_white_noise(noise_rms):
    """D754 at amplitude 2000: absent in blocks 0 and 1 (a word and the filter reach 1820 samples back), present with the
    right index in every block from 4 on.  8 blocks: four settled ones.  Clean, a settled block has 503 to 508 hits of 512.
    Under white noise of 4000 rms the seed matters: the signal's 2000 stand against some 1100 rms of noise behind the
    filter, a settled block has 200 hits in the median and falls below the 128 of min_hits in about one block of five
    (54 of 240 blocks over 20 seeds; 31 of 40 runs of 8 blocks kept every block from 4 on present).  The seed here was
    fixed before the first run, and this run holds with 238 to 321 hits; a squelch that must hold through such noise
    needs a lower min_hits or a debounce over blocks, which the bank leaves to its caller."""
    rng = np.random.default_rng(754)
    B = 8
    codes, inv = distinct_codes(5, [(0o023, False), (0o754, False)])
    x = dm.levels(0o754, 512 * B, 2000) + (dm.white(rng, 512 * B, noise_rms) if noise_rms else 0)
    hits, best, present = detector(codes, inv).process(dm.to_pcm(x).reshape(1, B, 512))
    print(f"noise {noise_rms}: hits of D754 per block {hits[0, :, 1].tolist()}, of the others at most {np.delete(hits[0], 1, axis=1).max()}")
    assert present[0, 4:, 0].all() and (best[0, 4:, 0] == 1).all()
    assert not present[0, :2, 0].any()


def test_white_noise_over_many_seeds_the_property_not_a_seed():
    """What holds under white noise of 4000 rms whatever the seed: over 20 seeds x 12 settled blocks the median block has
    more hits than min_hits asks for, and more than the most that noise alone gives any of 128 listed codes in 100 blocks;
    every block's best is the code sent wherever it has a hit at all.  What does not hold, although the issue's table (217
    to 303 hits) suggests it: that every single block stays above 128.  The count of those that fall below is printed."""
    settled = []
    for seed in range(20):
        rng = np.random.default_rng(seed)
        B = 16
        codes, inv = distinct_codes(5, [(0o023, False), (0o754, False)])
        x = dm.levels(0o754, 512 * B, 2000) + dm.white(rng, 512 * B, 4000.0)
        hits, best, present = detector(codes, inv).process(dm.to_pcm(x).reshape(1, B, 512))
        assert (best[0, 4:, 0][hits[0, 4:, 1] > 0] == 1).all() and np.delete(hits[0], 1, axis=1).max() < dm.DEFAULT_MIN_HITS
        settled += hits[0, 4:, 1].tolist()
    codes, inv = distinct_codes(128)
    noise = detector(codes, inv).process(dm.to_pcm(dm.white(np.random.default_rng(4000), 512 * 100, 4000.0)).reshape(1, 100, 512))[0]
    print(f"white noise 4000 rms: median {np.median(settled)} hits, {sum(v < 128 for v in settled)} of {len(settled)} settled blocks "
          f"below 128; noise alone at most {noise.max()}")
    assert np.median(settled) > dm.DEFAULT_MIN_HITS and np.median(settled) > noise.max()


def test_an_inverted_code_is_found_as_inverted_only():
    B = 8
    x = dm.to_pcm(dm.levels(0o754, 512 * B, 2000, inverted=True)).reshape(1, B, 512)
    hits, best, present = detector([0o754], [True]).process(x)
    assert present[0, 4:, 0].all() and (best[0, :, 0] == 0).all() and hits[0, 4:, 0].min() > 400
    hits, best, present = detector([0o754], [False]).process(x)
    assert not present.any() and hits.max() == 0


def test_a_listed_alias_is_refused(lib):
    for codes, inv, names in (([0o023, 0o114, 0o340], [0, 0, 0], ("entries 0 (D023N) and 2 (D340N)", "0x")),
                              ([0o047, 0o023], [0, 1], ("entries 0 (D047N) and 1 (D023I)", "aliases"))):
        c16, i8 = np.array(codes, dtype=np.uint16), np.array(inv, dtype=np.uint8)
        rc = lib.hrfd_dcs_set_codes(None, C.c_void_p(c16.ctypes.data), C.c_void_p(i8.ctypes.data), None, len(codes))
        err = lib.hrfd_last_error().decode()
        assert rc == EINVAL and err.startswith("hrfd_dcs_set_codes") and all(n in err for n in names), err
        with pytest.raises(AssertionError):
            dm.DcsModel(1).set_codes(codes, inv)


def test_noise_alone_and_silence_open_nothing():
    rng = np.random.default_rng(4000)
    B = 100
    codes, inv = distinct_codes(128)
    m = detector(codes, inv)
    hits, best, present = m.process(dm.to_pcm(dm.white(rng, 512 * B, 4000.0)).reshape(1, B, 512))
    print("noise alone: the most hits of any of 128 codes in a block:", hits.max())
    assert not present.any() and hits.max() < 128
    m.reset()
    hits, best, present = m.process(np.zeros((1, 3, 512), dtype=np.int16))
    assert hits.max() == 0 and not present.any() and (best[:, :, 0] == 0).all() and (best[:, :, 1:] == dm.NO_BEST).all()


# e. the squelch
def test_the_verdicts_drive_the_audio_banks_gate():
    from tests.audio_model import AudioModel
    rng = np.random.default_rng(9)
    B = 12
    codes, inv = distinct_codes(3, [(0o023, False), (0o754, False), (0o411, True)])
    n = 512 * B
    half = n // 2
    x = np.stack([dm.levels(0o754, n, 2000), np.concatenate([dm.levels(0o754, half, 2000), dm.levels(0o023, n - half, 2000, half)]),
                  dm.white(rng, n, 3000.0)])
    m = dm.DcsModel(3)
    m.set_taps(api.dcs_lowpass_taps())
    m.set_codes(codes, inv, [1, 1, 1])
    hits, best, present = m.process(dm.to_pcm(x).reshape(3, B, 512))
    a = AudioModel(3)
    a.set_want(1)
    a.set_want(0, 2)
    opened = a.gate(best, present, 512, 1)
    assert (opened == ((present[:, :, 1] == 1) & (best[:, :, 1] == np.array([1, 1, 0])[:, None]))).all()
    assert opened[0, 4:].all() and opened[1, 4:6].all() and not opened[1, 10:].any() and not opened[2].any() and not opened[:, :2].any()
    assert not a.gate(best, present, 512, 0).any()          # nothing is listed in group 0


# f. the closed loop on the models and the CPU oracle: what tests/test_gpu_dcs.py asserts of the same chain on the device
#    passes here first
def test_closed_loop_dcs_over_two_wbfm_stations(oracle):
    from tests import ddc_model as ddm
    from tests import duc_model as um
    from tests import tone_model as tm
    streams, amps = tm.loop_streams(oracle, dm.loop_audio())
    cap, duc = um.loop_duc(streams, amps)
    assert duc.clips[0] == 0
    d = ddm.DdcModel(1, 2, ddm.SEL_R)
    for c, f in enumerate(ddm.SEL_OFFSETS):
        d.set_tuning(c, 0, ddm.ddc_step(f + 64_000, ddm.SEL_R))
        d.set_gain_shift(c, ddm.SEL_GAIN_SHIFT[c])
    rx_in = d.process(cap, ddm.SEL_BLOCKS * 262144)
    pcm = np.stack([ddm.oracle_rx_wbfm(oracle, rx_in[c]) for c in range(2)])
    hits, best, present = dm.loop_model().process(pcm.reshape(2, dm.LOOP_BLOCKS, 512))
    print("hits of each station's own code per block:", hits[0, :, 0].tolist(), hits[1, :, 1].tolist())
    dm.loop_check(hits, best, present)
