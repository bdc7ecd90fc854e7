"""The DUC bank's transmit key on the device (hrfd_duc_*_keyed, include/hrfd.h): a keyed call leaves behind exactly what the
unkeyed call leaves behind for the masked input xk[c][m] = key[c][m >> k] != 0 ? x[c][m] : 0.  The oracle throughout is a
second, unkeyed handle with the same settings that is given xk (in the first test the numpy model of tests/duc_model.py as
well); keyed-off input bytes are 0x7f, not zeros, so a kernel that reads them shows.  hrfd_duc_get_key_skips is held to the
work contract's rule, restated here from the key rows."""
import functools

import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import duc_model as um
from tests.test_gpu_duc import pcm_for

pytestmark = pytest.mark.gpu

TILE = 1024


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def full_scale(rng, C, n_bytes):
    """random int8 over the whole range with a run of full scale, so that the sums clip"""
    x = rng.integers(-128, 128, size=(C, n_bytes), dtype=np.int8)
    x[:, n_bytes // 3:n_bytes // 3 + min(400, n_bytes // 4)] = 127
    return x


def masked(x, key, k, fill):
    """x [C, 2 M] with every keyed-off sample's two bytes replaced by `fill`"""
    M = x.shape[1] // 2
    on = np.asarray(key)[:, np.arange(M) >> k] != 0
    return np.where(np.repeat(on, 2, axis=1), x, np.int8(fill)).astype(np.int8)


def rule_skips(key, M, k):
    """the work contract: unit (c, t) is skipped iff t >= 1 and the key is off in the block of tile t and of tile t - 1"""
    n = 0
    for row in np.asarray(key):
        for t in range(1, (M + TILE - 1) // TILE):
            n += int(row[(TILE * t) >> k] == 0 and row[(TILE * (t - 1)) >> k] == 0)
    return n


def padded_key(torch, dev, key, pad=3):
    """the key rows n_keys + pad bytes apart with 0xff in the gaps, on the device; the last row ends the buffer"""
    key = np.asarray(key, dtype=np.uint8)
    C, nk = key.shape
    buf = np.full(C * (nk + pad), 0xff, dtype=np.uint8)
    buf.reshape(C, nk + pad)[:, :nk] = key
    return torch.from_numpy(buf[:(C - 1) * (nk + pad) + nk].copy()).to(dev), nk + pad


def run_device(torch, dev, d, x, R, W, d_key=None, key_stride=0):
    ib = x.shape[1]
    din = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    d.process_device(din.data_ptr(), ib, ib, out.data_ptr(), R * ib, d_key=None if d_key is None else d_key.data_ptr(),
                     key_stride=key_stride)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1, 2. the law and the meter, all four rates
LAW_W, LAW_C, LAW_K, LAW_M = 2, 5, 10, 5 * TILE + 600
LAW_CAPS = [1, 0, 1, 0, 1]                                     # non-contiguous
LAW_KEY = np.array([[1, 0, 0, 0x80, 0, 0],                     # on -> off, off - off, off -> on
                    [0, 0, 0, 0, 0, 0],                        # never
                    [2, 1, 255, 1, 7, 1],                      # always
                    [1, 1, 0, 0, 9, 1],                        # with channel 1: capture 0 is idle in tiles 2 and 3
                    [0, 1, 0, 0, 0, 1]], dtype=np.uint8)       # the muted channel


def law_handles(R):
    keyed, oracle, model = api.Duc(LAW_W, LAW_C, R, device=0), api.Duc(LAW_W, LAW_C, R, device=0), um.DucModel(LAW_W, LAW_C, R)
    for c in range(LAW_C):
        step = um.duc_step((-300_000 + 170_000 * c) * R / 2, R)
        for h in (keyed, oracle):
            h.set_step(c, LAW_CAPS[c], step)
        model.set_tuning(c, LAW_CAPS[c], step)
    for h in (keyed, oracle):
        h.set_amplitude(0, 4)
    model.set_amplitude(4, 0)
    keyed.set_key_block(LAW_K)
    return keyed, oracle, model


@functools.lru_cache(maxsize=None)
def law_case(R):
    """one keyed call and an unkeyed call behind it on the keyed handle, the oracle handle and the model"""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(100 + R)
    keyed, oracle, model = law_handles(R)
    assert keyed.n_keys(2 * LAW_M) == LAW_KEY.shape[1] == 6
    x = full_scale(rng, LAW_C, 2 * LAW_M)
    xk = masked(x, LAW_KEY, LAW_K, 0)
    d_key, stride = padded_key(torch, dev, LAW_KEY)
    r = {"got": run_device(torch, dev, keyed, masked(x, LAW_KEY, LAW_K, 0x7f), R, LAW_W, d_key, stride),
         "want": run_device(torch, dev, oracle, xk, R, LAW_W), "model": model.process(xk, 2 * LAW_M)}
    r["clips"] = [(keyed.clips(w), oracle.clips(w), int(model.clips[w])) for w in range(LAW_W)]
    r["skips"] = keyed.key_skips()
    x2 = full_scale(rng, LAW_C, 1400)
    r["got2"], r["want2"] = run_device(torch, dev, keyed, x2, R, LAW_W), run_device(torch, dev, oracle, x2, R, LAW_W)
    r["model2"] = model.process(x2, 1400)
    r["skips2"] = keyed.key_skips()
    keyed.reset()
    r["skips_reset"] = keyed.key_skips()
    return r


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_keyed_call_is_the_unkeyed_call_over_the_masked_input(R):
    r = law_case(R)
    assert (r["got"] == r["want"]).all(), f"captures: {np.argwhere(r['got'] != r['want'])[:5]}"
    assert (r["got"] == r["model"]).all(), f"model: {np.argwhere(r['got'] != r['model'])[:5]}"
    for w, (a, b, m) in enumerate(r["clips"]):
        assert a == b == m, (w, a, b, m)
    assert r["clips"][1][0] > 0, "the outputs clip"
    # the stored history is the masked one: an unkeyed call behind it
    assert (r["got2"] == r["want2"]).all(), f"the call behind: {np.argwhere(r['got2'] != r['want2'])[:5]}"
    assert (r["got2"] == r["model2"]).all()


@pytest.mark.parametrize("R", [1, 2, 4, 8])
def test_key_skips_counts_the_skipped_units(R):
    r = law_case(R)
    want = rule_skips(LAW_KEY, LAW_M, LAW_K)
    assert want == 2 + 5 + 0 + 1 + 2                           # by hand, per row
    assert r["skips"] == want and r["skips2"] == want, "an unkeyed call skips nothing"
    assert r["skips_reset"] == 0


# ---- 3. identities
def test_all_on_no_key_and_the_host_entry(torch_dev):
    torch, dev = torch_dev
    R, W, C, M, k = 4, 2, 3, 2 * TILE + 77, 10
    rng = np.random.default_rng(3)
    hs = [api.Duc(W, C, R, device=0) for _ in range(5)]
    for h in hs:
        for c in range(C):
            h.tune(c, c % W, -500_000 + 450_000 * c)
        h.set_key_block(k)
    x = full_scale(rng, C, 2 * M)
    plain = run_device(torch, dev, hs[0], x, R, W)
    d_on, s_on = padded_key(torch, dev, np.full((C, 3), 1, dtype=np.uint8), pad=0)
    assert (run_device(torch, dev, hs[1], x, R, W, d_on, s_on) == plain).all(), "every key on"
    assert hs[1].key_skips() == 0
    assert (hs[2].process(x, 2 * M, key=None) == plain).all(), "no key"
    key = np.array([[1, 0, 0], [0, 0, 3], [0, 1, 0]], dtype=np.uint8)
    d_key, stride = padded_key(torch, dev, key)
    dev_entry = run_device(torch, dev, hs[3], masked(x, key, k, 0x7f), R, W, d_key, stride)
    host_entry = hs[4].process(masked(x, key, k, 0x7f), 2 * M, key=key)
    assert (host_entry == dev_entry).all(), "the host entry"
    assert (dev_entry != plain).any()
    assert hs[3].key_skips() == hs[4].key_skips() == rule_skips(key, M, k) == 2
    for w in range(W):
        assert hs[3].clips(w) == hs[4].clips(w)


# ---- 4. streams: a stream cut into calls, every call with its own call-local key rows
@pytest.mark.parametrize("R", [1, 8])
def test_streams_cut_into_keyed_calls(torch_dev, R):
    torch, dev = torch_dev
    W, C, total = 2, 3, 3 * TILE + 10
    rng = np.random.default_rng(40 + R)
    keyed, oracle = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0)
    for h in (keyed, oracle):
        for c in range(C):
            h.tune(c, (c + 1) % W, 120_000.0 * (c - 1) * R)
    keyed.set_key_block(10)
    x = full_scale(rng, C, 2 * total)
    cuts = [1, 511, 1024, 1025]
    cuts.append(total - sum(cuts))
    at, k, skips = 0, 10, 0
    for i, M in enumerate(cuts):
        if i == 4:
            keyed.set_key_block(11)                            # keeps the history
            k = 11
        nk = keyed.n_keys(2 * M)
        assert nk == (M + (1 << k) - 1) >> k
        key = (rng.integers(0, 3, size=(C, nk)) == 0).astype(np.uint8) * 5
        if i == 2:
            key[0, :] = 0                                      # idle from the call's first sample: tile 0 is still computed
        if i == 3:
            key[0], key[1] = (5, 0), (0, 0)                    # two tiles: one behind an on block (computed), one skipped
        part = x[:, 2 * at:2 * (at + M)]
        d_key, stride = padded_key(torch, dev, key)
        got = run_device(torch, dev, keyed, masked(part, key, k, 0x7f), R, W, d_key, stride)
        want = run_device(torch, dev, oracle, masked(part, key, k, 0), R, W)
        assert (got == want).all(), f"call {i} of {M} samples: {np.argwhere(got != want)[:5]}"
        skips += rule_skips(key, M, k)
        at += M
    assert keyed.key_skips() == skips
    for w in range(W):
        assert keyed.clips(w) == oracle.clips(w)
    assert keyed.phase(1) == oracle.phase(1)


# ---- 5. the real granularity: one block of 512 PCM samples per key byte
def test_default_key_block(torch_dev):
    torch, dev = torch_dev
    R, W, C, ib = 8, 1, 2, 262144 + 2048
    rng = np.random.default_rng(5)
    keyed, oracle = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0)
    for h in (keyed, oracle):
        for c in range(C):
            h.tune(c, 0, -3_000_000.0 + 5_000_000.0 * c)
    key = np.array([[1, 0], [0, 1]], dtype=np.uint8)
    assert keyed.n_keys(ib) == 2 and keyed.n_keys(262144) == 1 and keyed.n_keys(262146) == 2
    x = full_scale(rng, C, ib)
    d_key, stride = padded_key(torch, dev, key)
    got = run_device(torch, dev, keyed, masked(x, key, 17, 0x7f), R, W, d_key, stride)
    want = run_device(torch, dev, oracle, masked(x, key, 17, 0), R, W)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert keyed.key_skips() == rule_skips(key, ib // 2, 17) == 127
    assert keyed.clips(0) == oracle.clips(0)


# ---- 6. transmit: the modulator runs over every channel, the DUC over those that are keyed on
@pytest.mark.parametrize("kind", [api.MOD_WBFM, api.MOD_FM], ids=["wbfm", "fm"])
def test_transmit_keyed_equals_mod_then_keyed_duc(torch_dev, kind):
    torch, dev = torch_dev
    R, W, C, n = 4, 2, 3, 512 + 8
    ma, mb = api.Mod(kind, C, device=0), api.Mod(kind, C, device=0)
    da, db = api.Duc(W, C, R, device=0), api.Duc(W, C, R, device=0)
    for d in (da, db):
        for c in range(C):
            d.tune(c, c % W, -400_000 + 350_000 * c)
    ib = 512 * n
    assert da.n_keys(ib) == 2
    d_key, stride = padded_key(torch, dev, np.array([[1, 0], [0, 1], [0, 0]], dtype=np.uint8))
    mid = torch.zeros((C, ib), dtype=torch.int8, device=dev)
    s = torch.cuda.Stream()
    for call in range(2):                                      # the second call without a key
        key = d_key.data_ptr() if call == 0 else None
        pcm = torch.from_numpy(pcm_for(kind, C, n, call)).to(dev)
        got = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        want = torch.zeros((W, R * ib), dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        da.transmit(ma, pcm.data_ptr(), n, got.data_ptr(), R * ib, s.cuda_stream, d_key=key, key_stride=stride)
        mb.process_device(pcm.data_ptr(), n, mid.data_ptr(), s.cuda_stream)
        db.process_device(mid.data_ptr(), ib, ib, want.data_ptr(), R * ib, s.cuda_stream, d_key=key, key_stride=stride)
        torch.cuda.synchronize()
        assert (got.cpu().numpy() == want.cpu().numpy()).all(), (kind, call)
        assert got.any()
    # 130 tiles, 128 in the first block: [1, 0] skips the last tile, [0, 1] tiles 1..127, [0, 0] all but tile 0
    assert da.key_skips() == db.key_skips() == 1 + 127 + 129


# ---- 7. push-to-talk, end to end
def test_push_to_talk_end_to_end(torch_dev):
    """AfskGen -> TxKey -> Mod (FM) -> Duc.transmit(d_key=) -> Ddc.receive -> Rx (FM) -> Afsk -> Hdlc, test_gpu_afskgen's RF
    loop with two FM channels on one capture whose PCM is silent but for one frame on channel 0 in the middle of 16 blocks.
    Under the key (hold = 1) the frame returns with its CRC good, the capture is exactly zero wherever both channels are off
    in a block and in the one in front of it, and channel 1, which never talks, adds nothing at all.  Without the key both
    carriers stand in the capture throughout."""
    from tests import afsk_model as am
    from tests import ddc_model as dm
    torch, dev = torch_dev
    R, B, FULL, C = dm.SEL_R, dm.SEL_BLOCKS, 262144, 2
    offsets = (-200_000.0, 200_000.0)
    payloads = am.random_payloads(np.random.default_rng(7), 1)
    gen = api.AfskGen(C, device=0)
    gen.send(0, payloads, start=5 * 512 + 100)
    assert gen.pending(0)[1] < 12 * 512
    d_audio = torch.zeros((C, B, 512), dtype=torch.int16, device=dev)
    d_active = torch.zeros((C, B), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gen.process_device(None, 0, B, d_audio.data_ptr(), d_active=d_active.data_ptr())
    torch.cuda.synchronize()
    d_key = api.TxKey(C, hold=1)(d_active, None)
    active, key = d_active.cpu().numpy(), d_key.cpu().numpy()
    first, last = int(np.flatnonzero(active[0])[0]), int(np.flatnonzero(active[0])[-1])
    assert first == 5 and 9 <= last <= 11 and not active[1].any()
    assert key[0].tolist() == [int(first <= b <= last + 1) for b in range(B)] and not key[1].any()

    def chain(d_key):
        mod = api.Mod(api.MOD_FM, C, device=0)
        duc = api.Duc(1, C, R, device=0)
        for c, f in enumerate(offsets):
            duc.tune(c, 0, f)
            duc.set_amplitude(32768 // 5, c)
        dcap = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
        torch.cuda.synchronize()
        duc.transmit(mod, d_audio.data_ptr(), B * 512, dcap.data_ptr(), R * B * FULL,
                     d_key=None if d_key is None else d_key.data_ptr(), key_stride=B)
        torch.cuda.synchronize()
        return duc, dcap

    duc, dcap = chain(d_key)
    # an idle block skips its 128 tiles, but for the first tile behind a block that talks and the stream's first tile
    n_on = int(key[0].sum())
    assert duc.key_skips() == rule_skips(key, B * FULL // 2, 17) == 128 * (B - n_on) - 2 + 128 * B - 1
    _, dcap_open = chain(None)
    cap = dcap.cpu().numpy().reshape(B, R * FULL)
    cap_open = dcap_open.cpu().numpy().reshape(B, R * FULL)
    idle = [b for b in range(B) if not key[:, b].any() and (b == 0 or not key[:, b - 1].any())]
    assert idle == [b for b in range(B) if b < first or b > last + 2]
    for b in idle:
        assert not cap[b, 2 * 320 * R:].any(), f"block {b} under the key"
        assert np.abs(cap_open[b, 2 * 320 * R:].astype(np.int32)).max() >= 20, f"block {b} without the key: the carriers"
    # channel 1 never talks: the capture is the one of a bank in which it is muted
    mod = api.Mod(api.MOD_FM, C, device=0)
    muted = api.Duc(1, C, R, device=0)
    for c, f in enumerate(offsets):
        muted.tune(c, 0, f)
        muted.set_amplitude(32768 // 5 if c == 0 else 0, c)
    dcap_muted = torch.zeros((1, R * B * FULL), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    muted.transmit(mod, d_audio.data_ptr(), B * 512, dcap_muted.data_ptr(), R * B * FULL, d_key=d_key.data_ptr(), key_stride=B)
    torch.cuda.synchronize()
    assert (dcap_muted.cpu().numpy().reshape(B, -1) == cap).all(), "channel 1 adds nothing under its key"

    # the receiver: the frame returns, and channel 1's band is silent
    ddc = api.Ddc(1, C, R, device=0)
    rx = api.Rx(C, device=0)
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
    ddc.receive(rx, dcap.data_ptr(), R * B * FULL, FULL, B, d_pcm.data_ptr(), d_n.data_ptr())
    dec.process_device(d_pcm.data_ptr(), 1024 * B, d_n.data_ptr(), B, d_bits.data_ptr(), n_bits, d_count.data_ptr())
    torch.cuda.synchronize()
    hdlc.process_device(d_bits.data_ptr(), n_bits, d_count.data_ptr(), n_bits, d_rec.data_ptr(), out_bytes, out_bytes,
                        d_frames.data_ptr(), d_bad.data_ptr(), d_dropped.data_ptr())
    torch.cuda.synchronize()
    frames = d_frames.cpu().numpy()
    got = [p for _, p, _ in api.Hdlc.parse(d_rec[0].cpu().numpy(), frames[0])]
    assert got == [bytes(p) for p in payloads], f"channel 0: {len(got)} good frames of 1"
    # channel 1's band, straight out of the DDC.  Without the key its carrier stands there, as strong as channel 0's in its
    # own band (the same amplitude; channel 0's is spread by its message, so within a factor of two).  Under the key what
    # is left is channel 0's splatter, 60 dB down behind the DDC's filters, and the capture's rounding (a twelfth of an
    # LSB^2 over 8.2 MHz, 5 % of it in band, against a carrier of several LSB): more than 30 dB below the carrier
    band = torch.zeros((C, B * FULL), dtype=torch.int8, device=dev)
    power = []
    for source in (dcap, dcap_open):
        d2 = api.Ddc(1, C, R, device=0)
        for c, f in enumerate(offsets):
            d2.set_step(c, 0, api.ddc_step(f, R))
        torch.cuda.synchronize()
        d2.process_device(source.data_ptr(), R * B * FULL, B * FULL, band.data_ptr(), B * FULL)
        torch.cuda.synchronize()
        power.append([float((band[c].to(torch.float32) ** 2).mean().item()) for c in range(C)])
    print(f"channel 1's band: mean power {power[0][1]:.5f} under the key, {power[1][1]:.3f} without; channel 0's {power[1][0]:.3f}")
    assert power[1][1] >= power[1][0] / 2 > 0 and power[0][1] <= power[1][1] / 1000

    # the tail: behind the message's last PCM sample the modulator's interpolator still moves the carrier's frequency, and
    # the DUC's filters look back 318 samples more.  The carrier's phase step per channel sample, averaged over windows of 256
    # samples (the sum telescopes to the phase at the window's two ends: two roundings of 1 / 127 rad over 256 samples, about
    # 2e-5 rad), against the idle carrier's in the stream's last block; the message's own peak is 2 pi 8000 / 32768 x
    # 3500 Hz / 2.048 MHz = 2.6e-3 rad.  A window counts as the message's while it differs by more than 2e-4 rad
    mod = api.Mod(api.MOD_FM, C, device=0)
    mid = torch.zeros((C, B * FULL), dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    mod.process_device(d_audio.data_ptr(), B * 512, mid.data_ptr())
    torch.cuda.synchronize()
    iq = mid[0].cpu().numpy().astype(np.float64).reshape(-1, 2)
    z = iq[:, 0] + 1j * iq[:, 1]
    turn = (z[1:] * np.conj(z[:-1]))[:(len(z) - 1) // 256 * 256].reshape(-1, 256).sum(axis=1)
    idle_turn = turn[-512:].sum()
    moving = np.flatnonzero(np.abs(np.angle(turn * np.conj(idle_turn))) > 2e-4)
    pcm0 = d_audio[0].cpu().numpy().ravel()
    end_pcm = int(np.flatnonzero(pcm0)[-1]) + 1
    end_rf = 256 * (int(moving[-1]) + 1) + 318
    tail, past_block = end_rf - 256 * end_pcm, end_rf - (last + 1) * (FULL // 2)
    print(f"the message's tail: the capture needs {tail} channel samples ({tail / 2048:.3f} ms) behind its last PCM sample; "
          f"here that is {past_block} samples behind the end of its last active block")
    assert tail <= FULL // 2 and past_block <= FULL // 2, "one block of hold covers a message that ends with its block"
