"""The transmit key of the DUC bank and the receive key of the DDC bank in the shapes their own suites do not reach, tolerance 0
everywhere.

K. k_duc<R, true>: every filter shape of test_gpu_duc's random-tap test under a key whose rows hold every case of the masking
   (the boundary between the dwords the kernel reads and the dwords it zeroes moves with the tap counts), the filters changed
   between keyed calls; the masked history under the longest look-back; transmit at key block 2^10; key rows more than 4 GiB
   apart; 16 captures x 64 channels.
R. k_ddc<R, true>: the zero store at every row residue modulo 16 under every short-tile length, receive at key blocks that
   straddle rx blocks, key rows and output rows more than 4 GiB apart, 16 x 64, a keyed stream under the largest filters with
   every setter between its calls.

The oracles are the own suites': a second, unkeyed handle with the same settings over the masked input (DUC) or with its
output masked in numpy (DDC), and the numpy models; the helpers of tests/test_gpu_duc_key.py, tests/test_gpu_ddc_key.py and
tests/test_gpu_bank_launch_shapes.py are used as they are.  What decides whether a shape reaches its path is restated in
tests/test_key_launch_shapes_model.py, checked there without a device, and asserted here next to the calls."""
import functools

import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import ddc_model as dm
from tests import duc_model as um
from tests import test_gpu_ddc_key as tr
from tests import test_gpu_duc_key as tk
from tests import test_key_launch_shapes_model as ks
from tests.test_gpu_bank_launch_shapes import big, far_equals_dense, far_rows, torch_dev      # noqa: F401
from tests.test_gpu_ddc import lcg_captures
from tests.test_gpu_duc import branch_taps, pcm_for

pytestmark = pytest.mark.gpu

TILE = ks.TILE
full_scale = tk.full_scale


def same(got, want, what):
    assert got.shape == want.shape and (got == want).all(), f"{what}: differs at {np.argwhere(got != want)[:5].tolist()}"


# ================================================================ K. the keyed DUC
K1_AMPS = (32768, 20000, 32767, 32768, 12345)


def duc_trio(W, C, R, caps, k):
    """a keyed handle, the unkeyed oracle handle and the model under one tuning"""
    keyed, oracle, model = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0), um.DucModel(W, C, R)
    for c in range(C):
        step = um.duc_step((-300_000 + 170_000 * c) * R / 2, R)
        for h in (keyed, oracle):
            h.set_step(c, caps[c], step)
            h.set_amplitude(K1_AMPS[c % 5], c)
        model.set_tuning(c, caps[c], step)
        model.set_amplitude(c, K1_AMPS[c % 5])
    for w in range(W):
        for h in (keyed, oracle):
            h.set_output_shift(6 + 2 * w, w)
        model.set_output_shift(w, 6 + 2 * w)
    keyed.set_key_block(k)
    return keyed, oracle, model


def set_filters(handles, rng, ta, tb, R):
    taps = branch_taps(rng, ta, R), branch_taps(rng, tb, 1)
    for h in handles:
        h.set_filter(0, taps[0])
        h.set_filter(1, taps[1])


def duc_call(torch, dev, trio, x, key, k, R, W):
    """one keyed call (key None: unkeyed) on the three; keyed-off input bytes are 0x7f on the keyed handle alone"""
    keyed, oracle, model = trio
    ib = x.shape[1]
    if key is None:
        xk, d_key, stride, seen = x, None, 0, x
    else:
        assert keyed.n_keys(ib) == key.shape[1]
        xk, seen = tk.masked(x, key, k, 0), tk.masked(x, key, k, 0x7f)
        d_key, stride = tk.padded_key(torch, dev, key)
    r = {"got": tk.run_device(torch, dev, keyed, seen, R, W, d_key, stride), "want": tk.run_device(torch, dev, oracle, xk, R, W),
         "model": model.process(xk, ib)}
    r["clips"] = [(keyed.clips(w), oracle.clips(w), int(model.clips[w])) for w in range(W)]
    r["skips"] = keyed.key_skips()
    return r


def check_duc_call(r, what):
    same(r["got"], r["want"], f"{what}: the oracle handle")
    same(r["got"], r["model"], f"{what}: the model")
    for w, (a, b, m) in enumerate(r["clips"]):
        assert a == b == m, (what, w, a, b, m)


@functools.lru_cache(maxsize=None)
def k1_case(R):
    """one handle pair and one model: a keyed call of three tiles and 77 samples under every tap pair, the filters set between
    the calls"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(700 + R)
    trio = duc_trio(ks.K1_W, ks.K1_C, R, ks.K1_CAPS, ks.K1_K)
    calls = []
    for ta, tb in ks.duc_tap_pairs(R):
        set_filters(trio, rng, ta, tb, R)
        x = full_scale(rng, ks.K1_C, 2 * ks.K1_M)
        calls.append(((ta, tb), duc_call(torch, dev, trio, x, ks.K1_KEY, ks.K1_K, R, ks.K1_W)))
    return calls


@pytest.mark.parametrize("R", ks.RATES)
def test_keyed_duc_under_every_filter_shape(R):
    """K1.  The filters change between keyed calls, so every call but the first also looks back into a masked history that
    a call with another look-back stored"""
    pairs = ks.duc_tap_pairs(R)
    geo = [ks.duc_geometry(ta, tb, R) for ta, tb in pairs]
    assert {g[3] for g in geo} == {0, 1} and min(g[2] for g in geo) == 0 and max(g[2] for g in geo) == ks.duc_geometry(64, 256, R)[2]
    assert any(a[2] < b[2] for a, b in zip(geo, geo[1:])), "a longer look-back than the call that stored the history"
    units = [ks.duc_unit(ks.K1_KEY[c], t, ks.K1_K) for c in range(ks.K1_C) for t in range(4)]
    assert set(units) == {"skip", (True, True), (True, False), (False, True)}
    per_call = tk.rule_skips(ks.K1_KEY, ks.K1_M, ks.K1_K)
    assert per_call == units.count("skip") == 6
    calls = k1_case(R)
    assert [p for p, _ in calls] == pairs
    for i, (p, r) in enumerate(calls):
        check_duc_call(r, f"R={R} taps {p[0]}/{p[1]}")
        assert r["skips"] == (i + 1) * per_call, f"R={R} taps {p}: key_skips"
        # capture 0's tile 3 has idle channels only: silence
        assert not r["got"][0, 2 * R * 3 * TILE:].any()
    assert min(a for a, _, _ in calls[-1][1]["clips"]) > 0 and any(((r["got"] != 127) & (r["got"] != -128) & (r["got"] != 0)).any() for _, r in calls)


def test_unkeyed_call_behind_a_keyed_off_block_under_the_longest_look_back(torch_dev):
    """K2: 64 / 256 taps at R = 1 look back 318 samples, the whole history.  The keyed call stores it masked: 18 samples of its
    first key block and 300 of its last, which is off on three channels"""
    torch, dev = torch_dev
    R = 1
    assert ks.duc_geometry(64, 256, R)[2] == ks.DUC_H == um.H and ks.K2_M - ks.DUC_H == TILE - 18
    rng = np.random.default_rng(720)
    trio = duc_trio(ks.K1_W, ks.K1_C, R, ks.K1_CAPS, ks.K1_K)
    set_filters(trio, rng, 64, 256, R)
    first = duc_call(torch, dev, trio, full_scale(rng, ks.K1_C, 2 * ks.K2_M), ks.K2_KEY, ks.K1_K, R, ks.K1_W)
    check_duc_call(first, "K2, the keyed call")
    behind = duc_call(torch, dev, trio, full_scale(rng, ks.K1_C, 2 * ks.K2_BEHIND), None, ks.K1_K, R, ks.K1_W)
    check_duc_call(behind, "K2, the unkeyed call behind it")
    assert behind["got"].any() and first["skips"] == behind["skips"] == tk.rule_skips(ks.K2_KEY, ks.K2_M, ks.K1_K) == 2


@pytest.mark.parametrize("kind", [api.MOD_WBFM, api.MOD_FM], ids=["wbfm", "fm"])
def test_transmit_keyed_at_the_smallest_key_block(torch_dev, kind):
    """K3: 520 PCM samples are 130 tiles and, at key block 2^10, 130 key bytes of 4 PCM samples each"""
    torch, dev = torch_dev
    R, W, C, n, k = 4, 2, 3, 520, 10
    ma, mb = api.Mod(kind, C, device=0), api.Mod(kind, C, device=0)
    da, db = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0)
    for d in (da, db):
        for c in range(C):
            d.tune(c, c % W, -400_000 + 350_000 * c)
        d.set_key_block(k)
    ib = 512 * n
    assert da.n_keys(ib) == 130 and ib // 2 == 130 * TILE and (1 << k) // 256 == 4
    key = np.zeros((C, 130), dtype=np.uint8)
    key[0] = (np.random.default_rng(730).integers(0, 3, size=130) == 0) * 0x81     # a random key
    key[2, -1] = 1                                             # on in its last byte only; channel 1 is off from the first sample
    assert key[0].any() and not key[0].all() and not key[1].any()
    d_key, stride = tk.padded_key(torch, dev, key)
    mid = torch.zeros((C, ib), dtype=torch.int8, device=dev)
    s = torch.cuda.Stream()
    for call in range(2):                                      # the second call without a key
        kp = d_key.data_ptr() if call == 0 else None
        pcm = torch.from_numpy(pcm_for(kind, C, n, call)).to(dev)
        got = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        want = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        da.transmit(ma, pcm.data_ptr(), n, got.data_ptr(), R * ib, s.cuda_stream, d_key=kp, key_stride=stride)
        mb.process_device(pcm.data_ptr(), n, mid.data_ptr(), s.cuda_stream)
        db.process_device(mid.data_ptr(), ib, ib, want.data_ptr(), R * ib, s.cuda_stream, d_key=kp, key_stride=stride)
        torch.cuda.synchronize()
        same(got.cpu().numpy(), want.cpu().numpy(), f"K3, call {call}")
        # capture 1 has channel 1 alone, which is off from the call's first sample: silence under the key
        assert bool(got[0].any()) and bool(got[1].any()) == (call == 1)
    rule =tk.rule_skips(key, ib // 2, k)
    assert da.key_skips() == db.key_skips() == rule and rule >= 129 + 128
    for w in range(W):
        assert da.clips(w) == db.clips(w)


def test_far_key_rows_duc(torch_dev, big):
    """K4: two channels on two captures, their key rows more than 4 GiB apart.  Row 1's key differs from row 0's, and behind
    row 0 lie random bytes: a stride cut to 32 bits reads one or the other"""
    R, W, C, M, k = 2, 2, 2, 2 * TILE + 77, 10
    key = np.array([[1, 0, 0], [0, 0, 9]], dtype=np.uint8)
    x = full_scale(np.random.default_rng(740), C, 2 * M)

    def handle(keyed):
        d = api.Duc(W, C, R, device=0)
        for c in range(C):
            d.tune(c, c, -300_000 + 500_000 * c)
        if keyed:
            d.set_key_block(k)
        return d

    oracle = handle(False)
    want = tk.run_device(*torch_dev, oracle, tk.masked(x, key, k, 0), R, W)

    def call(far):
        torch, dev = torch_dev
        d = handle(True)
        rows = far_rows(torch_dev, key.shape[1], 71, key, far)
        assert d.n_keys(2 * M) == key.shape[1] == rows.n and (rows.stride > 1 << 32 if far else rows.stride == 3)
        got = tk.run_device(torch, dev, d, tk.masked(x, key, k, 0x7f), R, W, _Ptr(rows.ptr), rows.stride)
        rows.check("the key", unchanged=True)
        return {"captures": got, "clips": np.array([d.clips(0), d.clips(1)]), "skips": np.array(d.key_skips())}

    got = far_equals_dense(torch_dev, call, "Duc")
    same(got["captures"], want, "K4, the far key against the oracle handle")
    assert got["captures"][1].any() and int(got["skips"]) == tk.rule_skips(key, M, k) == 2
    assert got["clips"].tolist() == [oracle.clips(0), oracle.clips(1)]


class _Ptr:
    """a device address where the suites' run_device takes a tensor"""

    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


def test_keyed_duc_16_captures_64_channels(torch_dev):
    """K5: R = 8, 16 x 64, two tiles and 77 samples, 8 of the 64 channels on"""
    torch, dev = torch_dev
    W, C, R, M, k = ks.K5_W, ks.K5_C, ks.K5_R, ks.K5_M, 10
    key, on = ks.k5_key(5)
    assert key.shape == (C, 3) and len(on) == ks.K5_ON and not np.delete(key, on, axis=0).any()
    keyed, oracle = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0)
    for h in (keyed, oracle):
        for c in range(C):
            h.tune(c, c % W, (c - 32) * 200_000.0)
        h.set_output_shift(7)
    keyed.set_key_block(k)
    x = full_scale(np.random.default_rng(750), C, 2 * M)
    d_key, stride = tk.padded_key(torch, dev, key)
    got = tk.run_device(torch, dev, keyed, tk.masked(x, key, k, 0x7f), R, W, d_key, stride)
    want = tk.run_device(torch, dev, oracle, tk.masked(x, key, k, 0), R, W)
    same(got, want, "K5")
    assert keyed.key_skips() == tk.rule_skips(key, M, k) >= 2 * (C - ks.K5_ON)
    assert sorted({int(c) % W for c in on}) == [w for w in range(W) if got[w].any()]
    for w in range(W):
        assert keyed.clips(w) == oracle.clips(w)


# ================================================================ R. the keyed DDC
def ddc_pair(W, C, R, k, with_model=False):
    keyed, oracle = api.Ddc(W, C, R, device=0), api.Ddc(W, C, R, device=0)
    model = dm.DdcModel(W, C, R) if with_model else None
    for c in range(C):
        step = dm.ddc_step((-300_000 + 170_000 * (c % 7)) * R / 2 + 1000.0 * c, R)
        for h in (keyed, oracle):
            h.set_step(c, c % W, step)
            h.set_gain_shift(c % 3, c)
        if model is not None:
            model.set_tuning(c, c % W, step)
            model.set_gain_shift(c, c % 3)
    keyed.set_key_block(k)
    return keyed, oracle, model


def ddc_call(torch_dev, keyed, oracle, cap, R, C, key, k, what, model=None, **layout):
    """one keyed call against the oracle handle's masked rows (and the model's): rows, guards, captures"""
    torch, dev = torch_dev
    ob = cap.shape[1] // R
    assert keyed.n_keys(ob) == key.shape[1]
    d_key, stride = tr.padded_key(torch, dev, key)
    got, guard, got_cap = tr.run_device(torch, dev, keyed, cap, R, C, d_key, stride, **layout)
    plain, want_guard, _ = tr.run_device(torch, dev, oracle, cap, R, C, **layout)
    same(got, tr.masked(plain, key, k), f"{what}: the oracle handle")
    if model is not None:
        same(got, tr.masked(model.process(cap, ob), key, k), f"{what}: the model")
    assert (guard == want_guard).all(), f"{what}: a byte outside the rows at {np.flatnonzero(guard != want_guard)[:5].tolist()}"
    assert (got_cap == cap).all(), f"{what}: the captures changed"
    return got


def test_zero_store_at_every_alignment(torch_dev):
    """R1: 16 rows a whole number of 16 bytes and one apart, so that they start at every residue modulo 16 wherever the
    allocation lies.  Single short tiles of every length with all but one channel keyed off, then the same lengths as the
    second tile behind a tile that is on"""
    R, W, C, k = 2, 2, ks.R1_C, 10
    keyed, oracle, _ = ddc_pair(W, C, R, k)
    per = np.zeros(C, dtype=np.uint64)
    seen = set()
    for i, M in enumerate(ks.R1_M):
        ob, on = 2 * M, ks.r1_on_channel(i)
        layout = dict(base=3, pad=ks.r1_pad(ob))
        assert (ob + layout["pad"]) % 16 == 1 and M < TILE
        reach = [ks.r1_reach(M, first, on) for first in range(16)]
        assert all(len({r for r, _ in x}) == 15 for x in reach)
        assert all(set().union(*(cl for _, cl in x)) <= ks.R1_CLASSES[ob] for x in reach)
        seen |= ks.R1_CLASSES[ob]
        key = np.zeros((C, 1), dtype=np.uint8)
        key[on] = 1 + i
        got = ddc_call(torch_dev, keyed, oracle, lcg_captures(W, R * ob, 900 + i), R, C, key, k, f"R1, one tile of {M}", **layout)
        assert not np.delete(got, on, axis=0).any()
        per = per + api.ddc_count_key_skips(key, ob, k)[0]
        assert tr.meters(keyed, C) == ([int(v) for v in per], int(per.sum())) and per[on] == i
    assert seen == ks.ZERO_CLASSES
    for i, M in enumerate(ks.R1_M):
        ob = 2 * (TILE + M)
        layout = dict(base=3, pad=ks.r1_pad(ob))
        assert (ob + layout["pad"]) % 16 == 1 and (2 * TILE) % 16 == 0      # the second tile starts at its row's residue
        assert all(len(ks.r1_reach(M, first)) == 16 for first in range(16))
        key = np.array([[1 + c, 0] for c in range(C)], dtype=np.uint8)
        got = ddc_call(torch_dev, keyed, oracle, lcg_captures(W, R * ob, 920 + i), R, C, key, k, f"R1, a tile and {M}", **layout)
        assert got[:, :2 * TILE].any(axis=1).all() and not got[:, 2 * TILE:].any()
        per = per + api.ddc_count_key_skips(key, ob, k)[0]
    assert tr.meters(keyed, C) == ([int(v) for v in per], int(per.sum())) and int(per.sum()) == 15 * 10 + 16 * 10


R2_KEYS = {10: np.array([[1, 0, 2, 0, 0, 3], [0, 0x80, 1, 1, 0, 0], [0, 0, 0, 0, 0, 0], [1, 1, 1, 0, 1, 1]], dtype=np.uint8),
           12: np.array([[1, 0], [0, 1], [0, 0], [1, 1]], dtype=np.uint8)}


@pytest.mark.parametrize("k", [10, 12])
@pytest.mark.parametrize("mode", [api.WBFM, api.FM], ids=["wbfm", "fm"])
def test_receive_keyed_with_key_blocks_that_straddle_rx_blocks(torch_dev, mode, k):
    """R2: rx blocks of 1536 samples, key blocks of 1024 or 4096: the law is call-local, whatever the rx bank's blocks are.
    The oracle is the unkeyed DDC, the mask, and the rx bank's device entry block by block (it refuses several blocks of
    fewer than 20480 bytes in one call; receive runs them through the same exact per-block path)"""
    torch, dev = torch_dev
    R, W, C, B, bb = 2, 2, 4, ks.R2_BLOCKS, ks.R2_BLOCK_BYTES
    ob = B * bb
    key = R2_KEYS[k]
    da, db = api.Ddc(W, C, R, device=0), api.Ddc(W, C, R, device=0)
    ra, rb = api.Rx(C, device=0), api.Rx(C, device=0)
    for d, rx in ((da, ra), (db, rb)):
        rx.set_mode(mode)
        for c, f in enumerate((-400_000, 150_000, 0, 320_000)):
            d.tune(c, c % W, f)
            d.set_gain_shift(2, c)
    da.set_key_block(k)
    assert da.n_keys(ob) == key.shape[1] and ob // 2 == 6 * TILE and (bb // 2) % (1 << k) != 0 and (1 << k) % (bb // 2) != 0
    d_key, stride = tr.padded_key(torch, dev, key)
    on = torch.from_numpy(np.repeat(key != 0, 2 << k, axis=1)[:, :ob].copy()).to(dev)
    mid = torch.zeros((C, ob), dtype=torch.int8, device=dev)
    cap_pcm = api.pcm_capacity(bb)
    for call in range(2):                                      # the second call without a key
        keyed = call == 0
        cap = (lcg_captures(W, R * ob, 960 + call).astype(np.int16) // 6).astype(np.int8)
        dcap = torch.from_numpy(cap).to(dev)
        pa, na, ma, aa = (torch.zeros((C, B, cap_pcm), dtype=torch.int16, device=dev), torch.zeros((C, B), dtype=torch.int32, device=dev),
                          torch.zeros((C, B), dtype=torch.int32, device=dev), torch.zeros((C, B), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        da.receive(ra, dcap.data_ptr(), R * ob, bb, B, pa.data_ptr(), na.data_ptr(), ma.data_ptr(), aa.data_ptr(),
                   d_key=d_key.data_ptr() if keyed else None, key_stride=stride)
        db.process_device(dcap.data_ptr(), R * ob, ob, mid.data_ptr(), ob)
        torch.cuda.synchronize()
        if keyed:
            mid = torch.where(on, mid, torch.zeros_like(mid))
            torch.cuda.synchronize()
        # the rx bank's own device entry takes blocks this short one per call: block b from where block b - 1 left the state
        per_block = []
        for b in range(B):
            o = (torch.zeros((C, cap_pcm), dtype=torch.int16, device=dev), torch.zeros(C, dtype=torch.int32, device=dev),
                 torch.zeros(C, dtype=torch.int32, device=dev), torch.zeros(C, dtype=torch.uint8, device=dev))
            rb.process_device(mid.data_ptr() + b * bb, ob, bb, 1, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr())
            torch.cuda.synchronize()
            per_block.append(o)
        pb, nb, mb, ab = (torch.stack([o[j] for o in per_block], dim=1) for j in range(4))
        for name, a, b in (("pcm", pa, pb), ("n_pcm", na, nb), ("magnitude", ma, mb), ("allowed", aa, ab)):
            assert torch.equal(a, b), (mode, k, call, name)
        assert na.any() and ma.any()
    per, total = api.ddc_count_key_skips(key, ob, k)
    assert tr.meters(da, C) == ([int(v) for v in per], total) and total > 0


def test_far_key_rows_and_output_rows_ddc(torch_dev, big):
    """R3: the key rows and the output rows each more than 4 GiB apart.  Channel 1 is keyed off: its far row is written by the
    zero store"""
    R, W, C, M, k = 2, 1, 2, TILE + 77, 10
    ob = 2 * M
    key = np.array([[3, 0], [0, 0]], dtype=np.uint8)
    cap = lcg_captures(W, R * ob, 970)

    def handle(keyed):
        d = api.Ddc(W, C, R, device=0)
        for c in range(C):
            d.tune(c, 0, -300_000 + 500_000 * c)
        if keyed:
            d.set_key_block(k)
        return d

    plain = handle(False).process(cap, ob)

    def call(far):
        torch, dev = torch_dev
        d = handle(True)
        rows, out = far_rows(torch_dev, key.shape[1], 72, key, far), far_rows(torch_dev, ob, 73, None, far)
        assert not far or min(rows.stride, out.stride) > 1 << 32
        dcap = torch.from_numpy(cap).to(dev)
        torch.cuda.synchronize()
        d.process_device(dcap.data_ptr(), R * ob, ob, out.ptr, out.stride, d_key=rows.ptr, key_stride=rows.stride)
        torch.cuda.synchronize()
        rows.check("the key", unchanged=True)
        assert (dcap.cpu().numpy() == cap).all()
        return {"rows": out.check("the rows").view(np.int8), "meters": np.array(tr.meters(d, C)[0])}

    got = far_equals_dense(torch_dev, call, "Ddc")
    same(got["rows"], tr.masked(plain, key, k), "R3, the far rows against the oracle handle")
    assert got["rows"][0, :2 * TILE].any() and not got["rows"][1].any() and got["meters"].tolist() == [1, 2]


def test_keyed_ddc_16_captures_64_channels(torch_dev):
    """R4: R = 8, 16 x 64, two tiles and 77 outputs, 8 of the 64 channels on"""
    W, C, R, M, k = ks.K5_W, ks.K5_C, ks.K5_R, ks.K5_M, 10
    key, on = ks.k5_key(6)
    keyed, oracle, _ = ddc_pair(W, C, R, k)
    got = ddc_call(torch_dev, keyed, oracle, lcg_captures(W, R * 2 * M, 980), R, C, key, k, "R4")
    assert got[on].any(axis=1).all() and not np.delete(got, on, axis=0).any()
    per, total = api.ddc_count_key_skips(key, 2 * M, k)
    assert tr.meters(keyed, C) == ([int(v) for v in per], total) and total >= 3 * (C - ks.K5_ON)
    assert [int(v) for v in per] == [int((key[c] == 0).sum()) for c in range(C)]


@pytest.mark.parametrize("R", [1, 8])
def test_keyed_stream_under_the_largest_filters_with_every_setter(torch_dev, R):
    """R5: 64 / 256 taps, so that the filters look back over the whole history (255 R + 63 samples); between the keyed calls a
    retune, a filter change, a capture switch and a reset, as in test_gpu_ddc's streaming test.  The skip does not depend on
    any of it; the history workgroups and N run under the key"""
    W, C, k = 2, 3, 10
    rng = np.random.default_rng(990 + R)
    keyed, oracle, model = ddc_pair(W, C, R, k, with_model=True)
    handles = (keyed, oracle, model)
    set_filters(handles, rng, 64, 256, 1)
    assert model.hA.size == 64 and model.hB.size == 256 and model.H == 255 * R + 63 == 64 - 1 + R * (256 - 1)
    per = np.zeros(C, dtype=np.uint64)
    for i, M in enumerate([1, 511, 1024, 1025, 2 * TILE + 300, 700, 1200]):
        if i == 2:
            for h in (keyed, oracle):
                h.set_step(1, 1, dm.ddc_step(-777_000, R))     # retune
            model.set_tuning(1, 1, dm.ddc_step(-777_000, R))
        if i == 3:
            set_filters(handles, rng, 64, 256, 1)              # filter change, the longest again
        if i == 4:
            for h in (keyed, oracle):
                h.set_step(0, 1, dm.ddc_step(55_000, R))       # capture switch
            model.set_tuning(0, 1, dm.ddc_step(55_000, R))
        if i == 5:
            for h in handles:
                h.reset()
        nk = keyed.n_keys(2 * M)
        key = (rng.integers(0, 2, size=(C, nk)) == 0).astype(np.uint8) * 5
        if i == 4:
            key[0], key[1], key[2] = (5, 0, 5), (0, 5, 0), (0, 0, 0)
        got = ddc_call(torch_dev, keyed, oracle, lcg_captures(W, R * 2 * M, 1000 + 7 * R + i), R, C, key, k, f"R5, R={R} call {i}", model,
                       base=1 + i, pad=8 + i)
        if i == 4:
            assert got[0].any() and got[1].any() and ((got != 127) & (got != -128) & (got != 0)).any()
        per = per + api.ddc_count_key_skips(key, 2 * M, k)[0]
        for c in range(C):
            assert keyed.phase(c) == oracle.phase(c) == model.phase(c), f"phase of channel {c} behind call {i}"
        if i == 4:
            assert tr.meters(keyed, C) == ([int(v) for v in per], int(per.sum())) and per.sum() > 0
            per[:] = 0                                         # the reset in front of call 5 clears the meters
    assert tr.meters(keyed, C) == ([int(v) for v in per], int(per.sum()))
