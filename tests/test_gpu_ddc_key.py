"""The DDC bank's receive key on the device (hrfd_ddc_*_keyed, include/hrfd.h): a keyed call writes
outk[c][m] = key[c][m >> k] != 0 ? out[c][m] : (0, 0), out being what the unkeyed call writes, and leaves everything else as
the unkeyed call leaves it.  The oracle throughout is a second, unkeyed handle with the same settings over the same
captures, its output masked in numpy (in the law test tests/ddc_model.py's DdcModel as well); output buffers start as 0x5A,
not zeros, so a unit that is not stored shows, and so does a byte stored outside a row.  hrfd_ddc_get_key_skips is held, per
channel and as the sum, to hrfd_ddc_key.h's slow count (hrfd_ddc_count_key_skips)."""
import functools

import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import ddc_model as dm
from tests.test_gpu_ddc import lcg_captures

pytestmark = pytest.mark.gpu

TILE = 1024
FULL = 262144
GUARD = 0x5A


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def masked(out, key, k):
    """out [C, 2 M] with both bytes of every keyed-off sample zero"""
    M = out.shape[1] // 2
    on = np.asarray(key)[:, np.arange(M) >> k] != 0
    return np.where(np.repeat(on, 2, axis=1), out, np.int8(0)).astype(np.int8)


def padded_key(torch, dev, key, pad=3):
    """the key rows n_keys + pad bytes apart with 0xff in the gaps, on the device; the last row ends the buffer"""
    key = np.asarray(key, dtype=np.uint8)
    C, nk = key.shape
    buf = np.full(C * (nk + pad), 0xff, dtype=np.uint8)
    buf.reshape(C, nk + pad)[:, :nk] = key
    return torch.from_numpy(buf[:(C - 1) * (nk + pad) + nk].copy()).to(dev), nk + pad


def run_device(torch, dev, d, cap, R, C, d_key=None, key_stride=0, base=3, pad=13):
    """one call over cap [W, R * ob] into rows ob + pad bytes apart that start `base` bytes into a buffer of guard bytes;
    returns (the rows [C, ob], the whole buffer with the rows set to the guard value, the captures as they are afterwards).
    Behind the last row lie a whole tile's bytes of guard: a zero store that ignored the short last tile's length would land
    in them, where it shows, and not outside the buffer"""
    ob = cap.shape[1] // R
    dcap = torch.from_numpy(np.ascontiguousarray(cap)).to(dev)
    buf = torch.full((base + C * (ob + pad) + 2 * TILE + 16,), GUARD, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    d.process_device(dcap.data_ptr(), R * ob, ob, buf.data_ptr() + base, ob + pad,
                     d_key=None if d_key is None else d_key.data_ptr(), key_stride=key_stride)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    rows = np.stack([host[base + c * (ob + pad):base + c * (ob + pad) + ob] for c in range(C)]).copy()
    for c in range(C):
        host[base + c * (ob + pad):base + c * (ob + pad) + ob] = GUARD
    return rows, host, dcap.cpu().numpy()


def meters(d, C):
    return [d.key_skips(c) for c in range(C)], d.key_skips()


# ---- 1, 2. the law and the meter, all four rates
LAW_W, LAW_C, LAW_K, LAW_M = 2, 5, 10, 5 * TILE + 37
LAW_CAPS = [1, 0, 1, 0, 1]                                     # non-contiguous
LAW_KEY = np.array([[1, 0, 0, 0x80, 0, 2],                     # on and off by turns, the short tile on
                    [0, 0, 0, 0, 0, 0],                        # never
                    [2, 1, 0x80, 1, 2, 1],                     # always
                    [0, 1, 1, 0, 2, 0],                        # off from the call's first sample, the short tile off
                    [0x80, 0, 0, 0, 0, 0]], dtype=np.uint8)
SHORT_KEY = np.array([[1], [0], [2], [0], [0x80]], dtype=np.uint8)     # a single short tile, on and off


def law_handles(R):
    keyed, oracle, model = api.Ddc(LAW_W, LAW_C, R, device=0), api.Ddc(LAW_W, LAW_C, R, device=0), dm.DdcModel(LAW_W, LAW_C, R)
    for c in range(LAW_C):
        step = dm.ddc_step((-300_000 + 170_000 * c) * R / 2, R)
        for h in (keyed, oracle):
            h.set_step(c, LAW_CAPS[c], step)
            h.set_gain_shift(c % 3, c)
        model.set_tuning(c, LAW_CAPS[c], step)
        model.set_gain_shift(c, c % 3)
    keyed.set_key_block(LAW_K)
    return keyed, oracle, model


@functools.lru_cache(maxsize=None)
def law_case(R):
    """on the keyed handle, the oracle handle and the model: a keyed call of five tiles and a remainder, an unkeyed call behind
    it, then keyed calls of 1 and of 1023 samples; the meters after each, and after reset"""
    import torch
    dev = torch.device("cuda:0")
    keyed, oracle, model = law_handles(R)
    assert keyed.n_keys(2 * LAW_M) == LAW_KEY.shape[1] == 6
    r = {"calls": [], "meters": [], "want_meters": []}
    per = np.zeros(LAW_C, dtype=np.uint64)
    plan = [(LAW_M, LAW_KEY), (700, None), (1, SHORT_KEY), (1023, SHORT_KEY)]
    for i, (M, key) in enumerate(plan):
        cap = lcg_captures(LAW_W, R * 2 * M, 100 + 10 * R + i)
        d_key, stride = (None, 0) if key is None else padded_key(torch, dev, key)
        got, got_guard, got_cap = run_device(torch, dev, keyed, cap, R, LAW_C, d_key, stride)
        plain, want_guard, _ = run_device(torch, dev, oracle, cap, R, LAW_C)
        mod = model.process(cap, 2 * M)
        if key is not None:
            assert keyed.n_keys(2 * M) == key.shape[1]
            plain, mod = masked(plain, key, LAW_K), masked(mod, key, LAW_K)
            per = per + api.ddc_count_key_skips(key, 2 * M, LAW_K)[0]
        r["calls"].append({"M": M, "got": got, "want": plain, "model": mod, "guards": (got_guard == want_guard).all(),
                           "captures": (got_cap == cap).all()})
        r["meters"].append(meters(keyed, LAW_C))
        r["want_meters"].append(([int(v) for v in per], int(per.sum())))
    r["phase"] = [(keyed.phase(c), oracle.phase(c)) for c in range(LAW_C)]
    r["oracle_meters"] = meters(oracle, LAW_C)
    keyed.reset()
    r["meters_reset"] = meters(keyed, LAW_C)
    return r


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_keyed_call_is_the_masked_unkeyed_call(R):
    r = law_case(R)
    for i, call in enumerate(r["calls"]):
        got, want = call["got"], call["want"]
        assert (got == want).all(), f"call {i} of {call['M']} samples, oracle handle: {np.argwhere(got != want)[:5]}"
        assert (got == call["model"]).all(), f"call {i}, model: {np.argwhere(got != call['model'])[:5]}"
        assert call["guards"], f"call {i}: a byte outside the rows"
        assert call["captures"], f"call {i}: the captures changed"
    first = r["calls"][0]["got"]
    assert not first[1].any() and first[2].any() and first[0, :2 * TILE].any() and not first[0, 2 * TILE:4 * TILE].any()
    assert ((first == 127) | (first == -128)).any(), "the outputs saturate"
    # the history and N are the unkeyed call's: the unkeyed call behind the keyed one, and everything behind that
    assert r["calls"][1]["got"].any()
    for a, b in r["phase"]:
        assert a == b


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_key_skips_counts_the_skipped_units_per_channel(R):
    r = law_case(R)
    assert r["want_meters"][0] == ([3, 6, 0, 3, 5], 17)           # by hand, per row
    assert r["want_meters"][3] == ([3, 8, 0, 5, 5], 21)           # two single-tile calls more
    for i, (got, want) in enumerate(zip(r["meters"], r["want_meters"])):
        assert got == want, f"behind call {i}"                 # call 1 is unkeyed: the meters stay
    assert r["oracle_meters"] == ([0] * LAW_C, 0)
    assert r["meters_reset"] == ([0] * LAW_C, 0)


def test_the_meter_refuses_a_channel_the_bank_does_not_have():
    d = api.Ddc(1, 3, 1, device=0)
    assert d.key_skips(2) == 0 and d.key_skips(api.ALL) == 0
    for channel in (3, 0xFFFFFFFE):
        with pytest.raises(Exception, match="channel"):
            d.key_skips(channel)
    d.set_key_block(17)
    for k in (9, 18):
        with pytest.raises(Exception, match="key block"):
            d.set_key_block(k)
    # n_keys at the edges of a block, for the smallest and the largest
    for k, want in ((10, [1, 1, 2, 128, 129]), (17, [1, 1, 1, 1, 2])):
        d.set_key_block(k)
        assert [d.n_keys(2 * M) for M in (1, 1024, 1025, 1 << 17, (1 << 17) + 1)] == want
    d.set_key_block(10)
    buf = np.zeros(16, dtype=np.int8)
    with pytest.raises(Exception, match="key_stride 1"):       # under the handle's block, not the largest
        d.process_device(buf, 4096, 4096, buf, 4096, d_key=buf, key_stride=1)


# ---- 3. identities
def test_no_key_all_on_all_off_and_the_host_entry(torch_dev):
    torch, dev = torch_dev
    R, W, C, M, k = 4, 2, 3, 2 * TILE + 77, 10
    hs = [api.Ddc(W, C, R, device=0) for _ in range(6)]
    for h in hs:
        for c in range(C):
            h.tune(c, c % W, -500_000 + 450_000 * c)
        h.set_key_block(k)
    cap = lcg_captures(W, R * 2 * M, 3)
    plain, plain_guard, _ = run_device(torch, dev, hs[0], cap, R, C)
    assert (hs[1].process(cap, 2 * M, key=None) == plain).all(), "no key, the host entry"
    d_on, s_on = padded_key(torch, dev, np.array([[1, 2, 0x80]] * C, dtype=np.uint8), pad=0)
    got, guard, _ = run_device(torch, dev, hs[2], cap, R, C, d_on, s_on)
    assert (got == plain).all() and (guard == plain_guard).all(), "every key on"
    assert meters(hs[2], C) == ([0] * C, 0), "a keyed call with every byte on moves no meter"
    d_off, s_off = padded_key(torch, dev, np.zeros((C, 3), dtype=np.uint8))
    got, guard, got_cap = run_device(torch, dev, hs[3], cap, R, C, d_off, s_off)
    assert not got.any() and (guard == plain_guard).all() and (got_cap == cap).all(), "every key off: rows of zeros"
    assert meters(hs[3], C) == ([3] * C, 3 * C)
    key = np.array([[1, 0, 0], [0, 0, 3], [0, 1, 0]], dtype=np.uint8)
    d_key, stride = padded_key(torch, dev, key)
    dev_entry, _, _ = run_device(torch, dev, hs[4], cap, R, C, d_key, stride)
    host_entry = hs[5].process(cap, 2 * M, key=key)
    assert (dev_entry == masked(plain, key, k)).all() and (host_entry == dev_entry).all(), "the host entry"
    assert meters(hs[4], C) == meters(hs[5], C) == ([2, 2, 2], 6)
    # behind all of it every handle is where the unkeyed one is
    cap2 = lcg_captures(W, R * 600, 4)
    want = hs[0].process(cap2, 600)
    for i in (2, 3, 4, 5):
        assert (hs[i].process(cap2, 600) == want).all(), i


# ---- 4. streams: a stream cut into calls, every call with its own call-local key rows
@pytest.mark.parametrize("R", [1, 8])
def test_streams_cut_into_keyed_calls(torch_dev, R):
    torch, dev = torch_dev
    W, C = 2, 3
    cuts = [1, 511, 1024, 1025, 2 * TILE + 300]
    rng = np.random.default_rng(40 + R)
    keyed, oracle = api.Ddc(W, C, R, device=0), api.Ddc(W, C, R, device=0)
    for h in (keyed, oracle):
        for c in range(C):
            h.tune(c, (c + 1) % W, 120_000.0 * (c - 1) * R)
    keyed.set_key_block(10)
    k, per = 10, np.zeros(C, dtype=np.uint64)
    for i, M in enumerate(cuts):
        if i == 3:
            for h in (keyed, oracle):
                h.tune(1, 1, -90_000.0 * R)                    # a retune between two calls: theta_ref from N on both
        if i == 4:
            keyed.set_key_block(11)
            k = 11
        nk = keyed.n_keys(2 * M)
        assert nk == (M + (1 << k) - 1) >> k
        key = (rng.integers(0, 2, size=(C, nk)) == 0).astype(np.uint8) * 5
        if i == 3:
            key[0], key[1], key[2] = (5, 0), (0, 5), (0, 0)    # two tiles, the second of one sample
        if i == 4:
            key[0], key[1] = (0, 7), (7, 0)                    # two blocks of two tiles; the second holds the remainder
        cap = lcg_captures(W, R * 2 * M, 50 + 7 * R + i)
        d_key, stride = padded_key(torch, dev, key)
        got, guard, _ = run_device(torch, dev, keyed, cap, R, C, d_key, stride, base=1 + i, pad=8 + i)
        plain, want_guard, _ = run_device(torch, dev, oracle, cap, R, C, base=1 + i, pad=8 + i)
        want = masked(plain, key, k)
        assert (got == want).all(), f"call {i} of {M} samples: {np.argwhere(got != want)[:5]}"
        assert (guard == want_guard).all(), f"call {i}: a byte outside the rows"
        per = per + api.ddc_count_key_skips(key, 2 * M, k)[0]
    assert meters(keyed, C) == ([int(v) for v in per], int(per.sum())) and per.sum() > 0
    assert keyed.phase(1) == oracle.phase(1)


# ---- 5. the real granularity: one rx block of 512 PCM samples per key byte
def test_default_key_block(torch_dev):
    torch, dev = torch_dev
    R, W, C, ob = 8, 1, 2, FULL + 2048
    keyed, oracle = api.Ddc(W, C, R, device=0), api.Ddc(W, C, R, device=0)
    for h in (keyed, oracle):
        for c in range(C):
            h.tune(c, 0, -3_000_000.0 + 5_000_000.0 * c)
    key = np.array([[1, 0], [0, 1]], dtype=np.uint8)
    assert keyed.n_keys(ob) == 2 and keyed.n_keys(FULL) == 1 and keyed.n_keys(FULL + 2) == 2
    cap = lcg_captures(W, R * ob, 5)
    d_key, stride = padded_key(torch, dev, key)
    got, _, _ = run_device(torch, dev, keyed, cap, R, C, d_key, stride)
    plain, _, _ = run_device(torch, dev, oracle, cap, R, C)
    want = masked(plain, key, 17)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert got[0, :FULL].any() and not got[0, FULL:].any() and not got[1, :FULL].any() and got[1, FULL:].any()
    assert meters(keyed, C) == ([1, 128], 129)


# ---- 6. receive: the keyed DDC, then the rx bank over every channel
@pytest.mark.parametrize("mode", [api.WBFM, api.FM], ids=["wbfm", "fm"])
def test_receive_keyed_equals_keyed_ddc_then_rx(torch_dev, mode):
    torch, dev = torch_dev
    R, W, C, B = 2, 2, 4, 3
    ob = B * FULL
    da, db = api.Ddc(W, C, R, device=0), api.Ddc(W, C, R, device=0)
    ra, rb = api.Rx(C, device=0), api.Rx(C, device=0)
    for d, rx in ((da, ra), (db, rb)):
        rx.set_mode(mode)
        for c, f in enumerate((-400_000, 150_000, 0, 320_000)):
            d.tune(c, c % W, f)
            d.set_gain_shift(2, c)
    key = np.array([[1, 0, 2], [0, 0x80, 1], [0, 0, 0], [1, 1, 0]], dtype=np.uint8)    # open and close inside the batch
    assert da.n_keys(ob) == B
    d_key, stride = padded_key(torch, dev, key)
    on = torch.from_numpy(np.repeat(key != 0, FULL, axis=1)).to(dev)
    mid = torch.zeros((C, ob), dtype=torch.int8, device=dev)
    for call in range(2):                                      # the second call without a key
        keyed = call == 0
        cap = (lcg_captures(W, R * ob, 60 + call).astype(np.int16) // 6).astype(np.int8)      # a noise floor rx can demodulate
        dcap = torch.from_numpy(cap).to(dev)
        outs = []
        for _ in range(2):
            outs.append((torch.zeros((C, B, 512), dtype=torch.int16, device=dev), torch.zeros((C, B), dtype=torch.int32, device=dev),
                         torch.zeros((C, B), dtype=torch.int32, device=dev), torch.zeros((C, B), dtype=torch.uint8, device=dev)))
        torch.cuda.synchronize()
        (pa, na, ma, aa), (pb, nb, mb, ab) = outs
        da.receive(ra, dcap.data_ptr(), R * ob, FULL, B, pa.data_ptr(), na.data_ptr(), ma.data_ptr(), aa.data_ptr(),
                   d_key=d_key.data_ptr() if keyed else None, key_stride=stride)
        db.process_device(dcap.data_ptr(), R * ob, ob, mid.data_ptr(), ob)
        torch.cuda.synchronize()
        if keyed:
            mid = torch.where(on, mid, torch.zeros_like(mid))
            torch.cuda.synchronize()
        rb.process_device(mid.data_ptr(), ob, FULL, B, pb.data_ptr(), nb.data_ptr(), mb.data_ptr(), ab.data_ptr())
        torch.cuda.synchronize()
        for name, a, b in (("pcm", pa, pb), ("n_pcm", na, nb), ("magnitude", ma, mb), ("allowed", aa, ab)):
            assert torch.equal(a, b), (mode, call, name)
        assert pa.any() and na.any()
    assert meters(da, C) == ([128, 128, 384, 128], 768)


# ---- 7. listening only where someone transmits, end to end
E2E_LOG2N, E2E_HALF_BAND = 10, 4                               # 8 kHz bins at R = 4; a band is 9 bins = 72 kHz around the carrier


def e2e_bands(offsets, R):
    N = 1 << E2E_LOG2N
    return [(int(round(f / (R * dm.FS_OUT / N))) - E2E_HALF_BAND) % N for f in offsets]


@functools.lru_cache(maxsize=None)
def e2e_threshold(R, offsets):
    """the band threshold from the models alone: tests/duc_model.py over a silent FM carrier on channel 0 at the test's
    amplitude with channel 1 keyed off, tests/spec_model.py over its capture with one band per channel.  The carrier is
    (62, 0): the FM modulator writes 16000 cos / sin as int16 (include/hrfd.h, the modulators), 62 as int8.  The active band
    holds the carrier, the idle one what channel 0 leaves 400 kHz away (the DUC's stop band and the capture's rounding):
    932 192 against 8.9 per frame, a gap of 50.2 dB.  The threshold lies halfway in dB: 2 886 per frame."""
    from tests import duc_model as um
    from tests import spec_model as sm
    M, N = 8192, 1 << E2E_LOG2N
    duc = um.DucModel(1, 2, R)
    for c, f in enumerate(offsets):
        duc.set_tuning(c, 0, um.duc_step(f, R))
        duc.set_amplitude(c, 32768 // 5)
    x = np.zeros((2, 2 * M), dtype=np.int8)
    x[0, 0::2] = 62
    spec = sm.SpecModel(1, R, E2E_LOG2N)
    for b, first in enumerate(e2e_bands(offsets, R)):
        spec.set_band(b, 0, first, 2 * E2E_HALF_BAND + 1, 0)
    n_frames = R * M // N
    _, bp, _ = spec.process(duc.process(x, 2 * M), n_frames)
    active, idle = int(bp[0]) / n_frames, max(int(bp[1]) / n_frames, 1.0)
    gap_db = 10 * np.log10(active / idle)
    return int(round((active * idle) ** 0.5)), gap_db, active, idle


def test_listening_only_where_someone_transmits_end_to_end(torch_dev):
    """AfskGen -> TxKey -> Mod (FM) -> Duc.transmit(d_key=) -> Spectrum, one band per channel, block by block -> RxKey ->
    Ddc.receive(d_key=) -> Rx (FM) -> Afsk -> Hdlc: test_gpu_duc_key's push-to-talk loop with the receiver keyed by what the
    spectrum bank hears.  Channel 0 sends one frame in the middle of 16 blocks, channel 1 never talks.  The spectrum's
    verdicts are the transmitter's key block for block, the frame returns on channel 0 with its CRC good, channel 1's DDC
    rows are exactly zero and every one of its tiles is skipped."""
    from tests import afsk_model as am
    torch, dev = torch_dev
    R, B, C = dm.SEL_R, dm.SEL_BLOCKS, 2
    offsets = (-200_000.0, 200_000.0)
    thr, gap_db, active, idle = e2e_threshold(R, offsets)
    print(f"model band power per frame: active {active:.0f}, idle {idle:.1f}, gap {gap_db:.1f} dB, threshold {thr}")
    assert gap_db >= 20.0, "the bands are too close: widen the spacing"
    payloads = am.random_payloads(np.random.default_rng(7), 1)
    gen = api.AfskGen(C, device=0)
    gen.send(0, payloads, start=5 * 512 + 100)
    d_audio = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    d_active = torch.zeros((C, B), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(None, 0, B, d_audio.data_ptr(), d_active=d_active.data_ptr())
    torch.cuda.synchronize()
    d_txkey = api.TxKey(C, hold=1)(d_active, None)
    txkey = d_txkey.cpu().numpy()
    first, last = int(np.flatnonzero(txkey[0])[0]), int(np.flatnonzero(txkey[0])[-1])
    assert first == 5 and last < B - 2 and not txkey[1].any()

    mod, duc = api.Mod(api.MOD_FM, C, device=0), api.Duc(1, C, R, device=0)
    for c, f in enumerate(offsets):
        duc.tune(c, 0, f)
        duc.set_amplitude(32768 // 5, c)
    dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    duc.transmit(mod, d_audio.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL, d_key=d_txkey.data_ptr(), key_stride=B)
    torch.cuda.synchronize()

    # the survey: one call per block of 64 ms, 512 frames of 1024 samples
    spec = api.Spectrum(1, R, E2E_LOG2N, device=0)
    for b, first_bin in enumerate(e2e_bands(offsets, R)):
        spec.set_band(b, 0, first_bin, 2 * E2E_HALF_BAND + 1, thr)
    n_frames = R * FULL // (2 << E2E_LOG2N)
    d_power = torch.zeros((1, 1 << E2E_LOG2N), dtype=torch.int64, device=dev)
    d_bp = torch.zeros((B, C), dtype=torch.int64, device=dev)
    d_present = torch.zeros((B, C), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for b in range(B):
        spec.process_device(dcap.data_ptr() + b * R * FULL, R * B * FULL, n_frames, d_power.data_ptr(),
                            d_bp[b].data_ptr(), d_present[b].data_ptr())
    torch.cuda.synchronize()
    present, bp = d_present.cpu().numpy(), d_bp.cpu().numpy() / n_frames
    print("band power per frame, channel 0:", [int(v) for v in bp[:, 0]], "channel 1:", [int(v) for v in bp[:, 1]])
    # block last + 1 holds the tail the DUC's filters leave behind the key (318 channel samples of 131 072): neither of the
    # model's two powers, so its verdict is the spectrum's to give; every other block is decided by the threshold
    settled = np.arange(B) != last + 1
    assert (present[settled, 0] == txkey[0][settled]).all(), "the spectrum hears channel 0 exactly where it is keyed"
    assert not present[:, 1].any()
    # what it hears stands where the model puts it: within 3 dB of the model's carrier (the message spreads it inside the band)
    on = txkey[0] != 0
    assert (bp[on, 0] >= active / 2).all() and (bp[on, 0] <= active * 2).all()

    d_rxkey = api.RxKey(C, [0, 1], hold=1)(d_present)
    rxkey = d_rxkey.cpu().numpy()
    want_rx = [int(any(present[j, 0] for j in range(max(0, b - 1), b + 1))) for b in range(B)]
    assert rxkey[0].tolist() == want_rx and want_rx[first:last + 2] == [1] * (last + 2 - first) and not rxkey[1].any()
    n_on = int(rxkey[0].sum())

    ddc, rx = api.Ddc(1, C, R, device=0), api.Rx(C, device=0)
    rx.set_mode(api.FM)
    for c, f in enumerate(offsets):
        ddc.tune(c, 0, f)
        ddc.set_gain_shift(dm.SEL_GAIN_SHIFT[0], c)
    dec, hdlc = api.Afsk(C, device=0), api.Hdlc(C, device=0)
    d_pcm = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    d_n = torch.zeros((C, B), dtype=torch.int32, device=dev)
    n_bits = dec.max_bits(B)
    d_bits = torch.zeros((C, n_bits), dtype=torch.uint8, device=dev)
    d_count = torch.zeros(C, dtype=torch.int32, device=dev)
    out_bytes = hdlc.max_out(n_bits)
    d_rec = torch.zeros((C, out_bytes), dtype=torch.uint8, device=dev)
    d_frames, d_bad, d_dropped = (torch.zeros(C, dtype=torch.int32, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr(), d_key=d_rxkey.data_ptr(),
                key_stride=B)
    dec.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_bits.data_ptr(), n_bits, d_count.data_ptr())
    torch.cuda.synchronize()
    hdlc.process_device(d_bits.data_ptr(), n_bits, d_count.data_ptr(), n_bits, d_rec.data_ptr(), out_bytes, out_bytes,
                        d_frames.data_ptr(), d_bad.data_ptr(), d_dropped.data_ptr())
    torch.cuda.synchronize()
    frames = d_frames.cpu().numpy()
    got = [p for _, p, _ in api.Hdlc.parse(d_rec[0].cpu().numpy(), frames[0])]
    assert got == [bytes(p) for p in payloads], f"channel 0: {len(got)} good frames of 1"
    assert frames[1] == 0
    tiles = FULL // 2 // TILE
    assert meters(ddc, C) == ([tiles * (B - n_on), tiles * B], tiles * (2 * B - n_on)), "the idle channel's skips are its tiles"

    # the DDC's rows themselves, from a second handle under the same key: exactly zero wherever the key is off
    d2 = api.Ddc(1, C, R, device=0)
    for c, f in enumerate(offsets):
        d2.tune(c, 0, f)
        d2.set_gain_shift(dm.SEL_GAIN_SHIFT[0], c)
    band = torch.full((C, B * FULL), GUARD, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    d2.process_device(dcap.data_ptr(), R * B * FULL, B * FULL, band.data_ptr(), B * FULL, d_key=d_rxkey.data_ptr(), key_stride=B)
    torch.cuda.synchronize()
    rows = band.cpu().numpy().reshape(C, B, FULL)
    assert not rows[1].any(), "the idle channel's DDC rows"
    for b in range(B):
        assert bool(rows[0, b].any()) == bool(rxkey[0, b]), f"channel 0, block {b}"
    assert d2.key_skips(1) == tiles * B
