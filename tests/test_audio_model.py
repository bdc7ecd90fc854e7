"""The numpy model of the audio bank (tests/audio_model.py) against a sample-by-sample restatement of the contract
(include/hrfd.h) in Python integers, its independence of how a batch is cut into calls, and the high-pass helper's taps
against what a voice filter behind a CTCSS decoder has to do.  No GPU."""
import numpy as np

from hackrfdiags_amd import api
from tests import audio_model as am


def slow(pcm, n_pcm, open_, taps, hist, prev, buses):
    """the contract in Python integers: pcm [C][N], n_pcm / open_ [C][n_blocks] or None, hist [C][T - 1] and prev [C] (both
    replaced), buses [(channels, gains)] -> (z [C][N], mix [M][N], clips [M])"""
    C, N, T = len(pcm), len(pcm[0]), len(taps)
    z = [[0] * N for _ in range(C)]
    for c in range(C):
        x = []
        for j in range(N):
            b, pos = divmod(j, 512)
            lim = 512 if n_pcm is None else min(int(n_pcm[c][b]), 512)
            x.append(int(pcm[c][j]) if pos < lim else 0)
        xx = list(hist[c]) + x
        for j in range(N):
            b, n = divmod(j, 512)
            acc = sum(int(taps[k]) * xx[T - 1 + j - k] for k in range(T))
            assert abs(acc) < (1 << 31) - (1 << 14)
            y = max(-32768, min(32767, (acc + (1 << 13)) >> 14))
            q = 1 if open_ is None or open_[c][b] != 0 else 0
            p = prev[c] if b == 0 else (1 if open_ is None or open_[c][b - 1] != 0 else 0)
            if p == q:
                e = 32768 * q
            elif q:
                e = min(32768, 512 * (n + 1))
            else:
                e = max(0, 32768 - 512 * (n + 1))
            z[c][j] = (y * e + (1 << 14)) >> 15
        hist[c] = xx[len(xx) - (T - 1):] if T > 1 else []
        prev[c] = 1 if open_ is None or open_[c][N // 512 - 1] != 0 else 0
    mix, clips = [], []
    for channels, gains in buses:
        row, n_clips = [], 0
        for j in range(N):
            s = sum(int(g) * z[int(c)][j] for c, g in zip(channels, gains))
            r = (s + (1 << 11)) >> 12
            m = max(-32768, min(32767, r))
            n_clips += m != r
            row.append(m)
        mix.append(row)
        clips.append(n_clips)
    return z, mix, clips


def test_model_against_python_integers():
    C, n_blocks, T = 2, 3, 5
    rng = np.random.default_rng(1)
    taps = [16384, -16384, 12000, -12000, 8767]             # sum |h| = 65535: the filter saturates on full-range input
    buses = [([0, 1, 1], [4096, 32767, 32767]), ([], []), ([1], [-20000])]
    m = am.AudioModel(C, len(buses))
    m.set_taps(taps)
    for i, (ch, g) in enumerate(buses):
        m.set_bus(i, ch, g)
    hist, prev = [[0] * (T - 1) for _ in range(C)], [0] * C
    for call, (n_pcm, open_) in enumerate([(None, None), ([[512, 100, 0], [513, 1, 511]], [[1, 0, 0], [0, 7, 255]]),
                                           (None, [[0, 1, 1], [1, 1, 0]]), ([[0, 0, 2 ** 32 - 1], [2, 300, 512]], None)]):
        pcm = rng.integers(-32768, 32768, size=(C, 512 * n_blocks), dtype=np.int16)
        got = m.process(pcm, n_pcm, open_)
        want = slow(pcm.tolist(), n_pcm, open_, taps, hist, prev, buses)
        for name, g, w in zip(("out", "mix", "clips"), got, want):
            assert (g.reshape(len(w), -1) == np.array(w, dtype=np.int64).reshape(len(w), -1)).all(), (call, name)
        assert m.hist.tolist() == hist and m.prev.tolist() == prev, call
    # the case does reach both saturations: of the filter (the last call is all open, z = y) and of the buses
    assert got[0].max() == 32767 and got[0].min() == -32768 and got[2][0] > 0 and got[2][1] == 0


def test_one_call_of_six_blocks_equals_calls_of_one_two_and_three():
    C = 3
    rng = np.random.default_rng(2)
    pcm = rng.integers(-32768, 32768, size=(C, 6, 512), dtype=np.int16)
    n_pcm = rng.choice(np.array([0, 7, 511, 512, 600], dtype=np.uint32), size=(C, 6))
    open_ = rng.integers(0, 2, size=(C, 6), dtype=np.uint8)
    for taps in ([20000, -9000], api.audio_highpass_taps(511), rng.integers(-127, 128, size=512)):
        whole, parts = am.AudioModel(C, 2), am.AudioModel(C, 2)
        for m in (whole, parts):
            m.set_taps(taps)
            m.set_bus(0, [0, 2], [4096, 4096])
            m.set_bus(1, [1, 1, 0], [30000, 30000, -5])
        out, mix, clips = whole.process(pcm, n_pcm, open_)
        cut = [parts.process(pcm[:, a:b], n_pcm[:, a:b], open_[:, a:b]) for a, b in ((0, 1), (1, 3), (3, 6))]
        assert (np.concatenate([c[0] for c in cut], axis=1) == out).all()
        assert (np.concatenate([c[1] for c in cut], axis=1) == mix).all()
        assert (sum(c[2].astype(np.int64) for c in cut) == clips).all()
        assert (whole.hist == parts.hist).all() and (whole.prev == parts.prev).all()


def test_gate_model_against_a_loop():
    rng = np.random.default_rng(3)
    C, n_blocks = 4, 16
    m = am.AudioModel(C)
    for want in (5, am.ANY_TONE, am.NO_TONE):
        m.set_want(want)
        m.set_want(6, 3)
        for L in (128, 512, 4096):
            F = 512 * n_blocks // L
            best = rng.choice(np.array([5, 6, 255], dtype=np.uint8), size=(C, F, 4))
            present = rng.integers(0, 3, size=(C, F, 4), dtype=np.uint8)
            for group in range(4):
                got = m.gate(best, present, L, group)
                for c in range(C):
                    w = int(m.want[c])
                    for b in range(n_blocks):
                        frames = range(b * 512 // L, (b + 1) * 512 // L) if L <= 512 else [b * 512 // L]
                        hit = any(present[c, f, group] != 0 and (w == am.ANY_TONE or best[c, f, group] == w) for f in frames)
                        assert got[c, b] == (1 if w == am.NO_TONE or hit else 0), (want, L, group, c, b)


def response_db(h, freqs_hz):
    n = np.arange(len(h), dtype=np.float64)
    H = np.array([np.sum(h * np.exp(-2j * np.pi * f / api.TONE_FS * n)) for f in freqs_hz]) / 16384.0
    return 20.0 * np.log10(np.maximum(np.abs(H), 1e-12))


def test_highpass_helper_removes_ctcss_and_keeps_the_voice_band():
    h = api.audio_highpass_taps()
    assert h.dtype == np.int16 and h.size == 511 and (h == h[::-1]).all()
    assert int(np.abs(h.astype(np.int64)).sum()) == 45955      # inside the tap check's 65535
    hd = h.astype(np.float64)
    stop = response_db(hd, api.CTCSS_HZ)
    assert len(api.CTCSS_HZ) == 50 and stop.max() <= -55.0, (stop.max(), api.CTCSS_HZ[int(stop.argmax())])
    assert api.CTCSS_HZ[int(stop.argmax())] == 131.8 and abs(stop.max() + 58.1) < 0.1, stop.max()
    voice = response_db(hd, np.arange(350.0, 3801.0, 10.0))
    assert np.abs(voice).max() <= 0.05, np.abs(voice).max()
