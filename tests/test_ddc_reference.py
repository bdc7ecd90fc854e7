"""The DDC model (tests/ddc_model.py) against two independent statements of the contract in include/hrfd.h, without a
GPU: the integer restatement of tests/ddc_reference.py (bit for bit, over multi-call sequences with every setter), and
the same operation in float64 (within an error budget derived below).  The GPU tests hold the kernel to the model, so a
mistake the model shares with the kernel -- a rotation sign, a decimation phase, a tap order -- is caught here."""
import numpy as np
import pytest

from tests import ddc_model as dm
from tests import ddc_reference as dr


def random_taps(rng, n, limit=65535):
    """n random taps, asymmetric (the default filters are symmetric and would hide a reversed tap order), sum |h|
    close to the limit"""
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    while True:
        h = rng.integers(-32768, 32768, size=n).astype(np.int64)
        s = int(np.abs(h).sum())
        if s > limit:
            h = np.sign(h) * ((np.abs(h) * limit) // s)
        if n == 1 or (h != h[::-1]).any():
            return h


def pair(W, C, R):
    m = dm.DdcModel(W, C, R)
    return m, dr.DdcReference(W, C, R, m.hA, m.hB)


def apply(objs, name, *args):
    for o in objs:
        getattr(o, name)(*args)


# ---- 1. the model equals the integer restatement
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_model_equals_independent_reference(R):
    rng = np.random.default_rng(1000 + R)
    W, C = 3, 4
    m, ref = pair(W, C, R)
    both = (m, ref)
    H = dm.history_len(R)
    for c in range(C):
        apply(both, "set_tuning", c, (c + 1) % W, int(rng.integers(0, 2 ** 32)))
        apply(both, "set_gain_shift", c, 2 * c)
    # call lengths in bytes: 2 (one output), shorter than the history H (in input samples), and longer
    events = [
        (2, None), (2, "retune"), (100, None), (2 * (H // R) - 2, "capture"), (2, "filter_a"), (1000, "filter_b"),
        (6, "gain"), (2 * H, "retune"), (300, "reset"), (2, None), (44, "filter_a_max"), (1500, "filter_b_max"),
        (2, "bypass_a"), (800, "bypass_b"), (600, "restore"), (2, "gain_all"), (400, None),
    ]
    for i, (ob, ev) in enumerate(events):
        c = i % C
        if ev == "retune":
            apply(both, "set_tuning", c, int(m.capture[c]), int(rng.integers(0, 2 ** 32)))
        elif ev == "capture":
            apply(both, "set_tuning", c, (int(m.capture[c]) + 1) % W, int(m.step[c]))
        elif ev == "filter_a":
            apply(both, "set_filter", 0, random_taps(rng, int(rng.integers(1, 65))))
        elif ev == "filter_b":
            apply(both, "set_filter", 1, random_taps(rng, int(rng.integers(1, 257))))
        elif ev == "filter_a_max":
            apply(both, "set_filter", 0, random_taps(rng, 64))
        elif ev == "filter_b_max":
            apply(both, "set_filter", 1, random_taps(rng, 256))
        elif ev == "bypass_a":
            apply(both, "set_filter", 0, [])
        elif ev == "bypass_b":
            apply(both, "set_filter", 1, [])
        elif ev == "restore":
            a, b = dm.default_taps(R)
            apply(both, "set_filter", 0, a)
            apply(both, "set_filter", 1, b)
        elif ev == "gain":
            apply(both, "set_gain_shift", c, int(rng.integers(0, 8)))
        elif ev == "gain_all":
            for cc in range(C):
                apply(both, "set_gain_shift", cc, 7 - cc)
        elif ev == "reset":
            apply(both, "reset")
        scale = (1, 1, 4, 16)[i % 4]                                 # full scale (saturating) and smaller inputs
        cap = (rng.integers(-128, 128, size=(W, R * ob)) // scale).astype(np.int8)
        got, want = m.process(cap, ob), ref.process(cap, ob)
        assert (got == want).all(), f"R={R} call {i} ({ob} bytes, {ev}): {np.argwhere(got != want)[:5]}"
        for cc in range(C):
            assert m.phase(cc) == ref.theta(cc, ref.N), f"phase ch{cc} after call {i}"


def test_reference_sees_a_reversed_tap_order():
    """the comparison above can fail: the model with stage B's taps reversed differs from the reference"""
    rng = np.random.default_rng(7)
    R, W, C = 2, 1, 1
    m, ref = pair(W, C, R)
    h = random_taps(rng, 40)
    m.set_filter(1, h[::-1])
    ref.set_filter(1, h)
    cap = (rng.integers(-128, 128, size=(W, R * 2000)) // 4).astype(np.int8)
    assert (m.process(cap, 2000) != ref.process(cap, 2000)).any()


# ---- 2. the model against the operation in float64
def error_budget(x_max: float, iq_sum_max: float, h_a, h_b, g: int) -> float:
    """|model - float| bound per output component, in output LSB, for inputs that saturate nowhere.

    mixer: theta is rounded to the nearest of 4096 table phases, an error of at most 2 pi 2^19 / 2^32 = pi / 4096 rad;
      it moves the exactly rotated sample 32767 (I + jQ) e^{-j phi} by at most 32767 |x| pi / 4096 in each component.
      The table holds 32767 cos rounded to integers (|delta| <= 1/2 per entry): I c + Q s is off by at most
      (|I| + |Q|) / 2.  The rounded shift (v + 128) >> 8 adds at most 1/2.  So, in y LSB,
        E_y = (32767 |x|max pi / 4096 + (|I| + |Q|)max / 2) / 256 + 1/2
    stage A: the error of every y under a tap reaches a by sum |hA| / 32768; the rounded shift adds 1/2:
        E_a = E_y sum|hA| / 32768 + 1/2        (T_A = 0: E_a = E_y)
    stage B: E_b = E_a sum|hB| / 32768 + 1/2   (T_B = 0: E_b = E_a)
    output: (b + r) >> (7 - g) is b / 2^(7 - g) rounded half up (+1/2 at most) for g < 7 and exact for g = 7:
        E = E_b / 2^(7 - g) + (1/2 if g < 7 else 0)"""
    e = (32767.0 * x_max * np.pi / 4096.0 + iq_sum_max / 2.0) / 256.0 + 0.5
    for h in (h_a, h_b):
        if len(h):
            e = e * float(np.abs(np.asarray(h, dtype=np.int64)).sum()) / 32768.0 + 0.5
    return e / 2.0 ** (7 - g) + (0.5 if g < 7 else 0.0)


@pytest.mark.parametrize("taps", ["default", "random"])
@pytest.mark.parametrize("g", [0, 3])
@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_model_within_float64_error_budget(R, g, taps):
    rng = np.random.default_rng(R * 10 + g + (taps == "random") * 100)
    W, C = 1, 3
    m = dm.DdcModel(W, C, R)
    if taps == "random":
        # short ones: long random filters pass little of any tone, and the check needs a signal well above the budget
        m.set_filter(0, random_taps(rng, int(rng.integers(3, 9))))
        m.set_filter(1, random_taps(rng, int(rng.integers(3, 17))))
        if R == 1:
            m.set_filter(0, [])
    steps = [int(rng.integers(0, 2 ** 32)) for _ in range(C)]
    for c in range(C):
        m.set_tuning(c, 0, steps[c])
        m.set_gain_shift(c, g)
    # one tone in every channel's passband (60 kHz from its centre) over a little noise, small enough that no stage
    # saturates
    amp = {0: 25.0, 3: 3.0}[g]
    calls = (2000, 3000, 2 * 2048)
    n_in = sum(calls) * R // 2
    t = np.arange(n_in, dtype=np.float64)
    z = sum(amp * np.exp(2j * np.pi * (steps[c] / 2.0 ** 32 + (-1) ** c * 60e3 / (R * dm.FS_OUT)) * t + 1j * c)
            for c in range(C))
    x = np.stack([np.round(z.real), np.round(z.imag)], axis=1) + rng.integers(-2, 3, size=(n_in, 2))
    x = x.astype(np.int8)
    outs, accA, accB = [], [], []
    o = 0
    for ob in calls:
        cap = x[o:o + R * ob // 2].reshape(1, -1)
        o += R * ob // 2
        out, st = m.process(cap, ob, stages=True)
        outs.append(out.astype(np.int64).reshape(C, -1, 2))
        for acc, lst in ((st["accA"], accA), (st["accB"], accB)):
            if acc is not None:
                lst.append(acc)
    for lst in (accA, accB):
        if lst:
            acc = np.concatenate([a.reshape(-1) for a in lst])
            assert np.abs((acc + (1 << 14)) >> 15).max() < 32767, "an FIR stage saturated: lower the input"
    got = np.concatenate(outs, axis=1)
    assert np.abs(got).max() < 127, "the output saturated: lower the input"
    xi = x.astype(np.int64)
    n = np.arange(xi.shape[0], dtype=np.int64)
    bound = error_budget(float(np.sqrt((xi ** 2).sum(axis=1)).max()), float(np.abs(xi).sum(axis=1).max()), m.hA, m.hB, g)
    worst = 0.0
    for c in range(C):
        f = dr.float_ddc(xi, (n * steps[c]) & dm.MASK32, m.hA, m.hB, R, g)
        err = max(np.abs(got[c, :, 0] - f.real).max(), np.abs(got[c, :, 1] - f.imag).max())
        worst = max(worst, float(err))
        assert err <= bound, f"ch{c}: |model - float| = {err:.3f} LSB > budget {bound:.3f}"
    assert np.abs(got).max() >= 16, "too small a signal to tell anything"
    print(f"\nR={R} g={g} {taps}: worst |model - float64| {worst:.3f} LSB, budget {bound:.3f} LSB, "
          f"peak |out| {np.abs(got).max()}")


def test_float_budget_sees_a_rotation_sign_error():
    """the budget is tight enough to fail on a mixer that rotates the wrong way"""
    rng = np.random.default_rng(3)
    R, g = 2, 0
    m = dm.DdcModel(1, 1, R)
    step = dm.ddc_step(300_000, R)
    m.set_tuning(0, 0, step)
    x = rng.integers(-40, 41, size=(R * 2000, 2)).astype(np.int8)
    got = m.process(x.reshape(1, -1), 4000).astype(np.int64).reshape(-1, 2)
    xi = x.astype(np.int64)
    n = np.arange(xi.shape[0], dtype=np.int64)
    wrong = dr.float_ddc(xi, (-n * step) & dm.MASK32, m.hA, m.hB, R, g)
    bound = error_budget(float(np.sqrt((xi ** 2).sum(axis=1)).max()), float(np.abs(xi).sum(axis=1).max()), m.hA, m.hB, g)
    assert max(np.abs(got[:, 0] - wrong.real).max(), np.abs(got[:, 1] - wrong.imag).max()) > bound
