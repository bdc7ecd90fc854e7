"""The handles own their device buffers (DevBuf, hackrfdiags_amd/csrc/hrfd_buf.h): a receive handle driven through the
growth of every buffer it has, every output against the CPU oracle, then destroyed and created again; the same create, use,
destroy, create for the modulators and the Nco at their smallest sizes."""
import numpy as np
import pytest

from hackrfdiags_amd import api, synth
from tests.reflib import AM, FM, WBFM, LSB, USB, NONE

pytestmark = pytest.mark.gpu
BB = 32768                                                  # 2048 samples at 256 kS/s, 64 PCM samples
MODES = [WBFM, AM, FM, LSB, USB, NONE, WBFM, FM]


def _check(orcs, xs, off, nb, n, got, pending=0, rows_cleared=True):
    pcm, n_pcm, mag, allowed, dump = got
    for c, o in enumerate(orcs):
        held = pending
        for b in range(nb):
            wp, wm, wa, wd = o.process(xs[c, off + b * n:off + (b + 1) * n])
            assert n_pcm[c, b] == len(wp) and mag[c, b] == wm and bool(allowed[c, b]) == wa, (off, c, b)
            assert (pcm[c, b, :len(wp)] == wp).all(), (off, c, b)
            assert not rows_cleared or (pcm[c, b, len(wp):] == 0).all(), (off, c, b)
            if dump is not None:
                cnt = 2 * ((held + n // 2) // 8)
                held = (held + n // 2) % 8
                assert cnt == len(wd) and (dump[c, b, :cnt] == wd).all(), (off, c, b)


def test_receive_handle_through_every_buffers_growth_and_a_second_handle(oracle):
    import torch
    C = len(MODES)
    total = 8 * BB + 1000
    xs = np.stack([synth.make_input("fmtone" if c % 3 else "amtone", 900 + c, (total + synth.BLOCK_BYTES - 1) // synth.BLOCK_BYTES)[:total]
                   for c in range(C)])

    def handle():
        rx, orcs = api.Rx(C), []
        for c, m in enumerate(MODES):
            rx.set_mode(m, c)
            orcs.append(oracle.rx())
            orcs[-1].set_mode(m)
        return rx, orcs

    rx, orcs = handle()
    # the host entry with the 256 kS/s dump: staging, per-unit scratch, SSB rails for 2 blocks
    first = rx.process_block(xs[:, :2 * BB].reshape(C, 2, BB), 2, want_iq256=True)
    _check(orcs, xs, 0, 2, BB, first)
    # 4 blocks: all of them regrow
    _check(orcs, xs, 2 * BB, 4, BB, rx.process_block(xs[:, 2 * BB:6 * BB].reshape(C, 4, BB), 4, want_iq256=True))
    # the device entry, the launch bracketed with events and the stamp buffer attached
    rx.debug_enable_timing(2)
    rx.debug_stamps(64)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(xs[:, 6 * BB:8 * BB].copy()).to(dev)
    out = torch.zeros((C, 2, BB // 512), dtype=torch.int16, device=dev)
    npcm = torch.zeros((C, 2), dtype=torch.int32, device=dev)
    mag = torch.zeros((C, 2), dtype=torch.int32, device=dev)
    alw = torch.zeros((C, 2), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rx.process_device(x.data_ptr(), 2 * BB, BB, 2, out.data_ptr(), d_n_pcm=npcm.data_ptr(), d_magnitude=mag.data_ptr(),
                      d_allowed=alw.data_ptr())
    assert rx.sync() == 0, rx.failed_channels()
    _check(orcs, xs, 6 * BB, 2, BB, (out.cpu().numpy(), npcm.cpu().numpy(), mag.cpu().numpy(), alw.cpu().numpy(), None))
    assert rx.debug_kernel_ms(0) > 0.0
    assert rx.debug_stamps(64, read=True).shape == (64, 48)
    rx.debug_stamps(0)                                       # the stamp buffer is given back, and once more with the handle
    rx.debug_stamps(8)
    # 1000 bytes: off the 512-byte grid, the general-length state is built
    _check(orcs, xs, 8 * BB, 1, 1000, rx.process_block(xs[:, 8 * BB:].reshape(C, 1, 1000), 1, want_iq256=True))
    assert rx.debug_ragged() == (True, 1)
    rx.close()
    # a second handle starts where the first one started
    rx2, _ = handle()
    again = rx2.process_block(xs[:, :2 * BB].reshape(C, 2, BB), 2, want_iq256=True)
    for a, b in zip(first, again):
        assert (a == b).all()
    assert rx2.debug_ragged() == (False, 0)
    rx2.close()


@pytest.mark.parametrize("kind, name", [(api.MOD_SSB, "ssbmod"), (api.MOD_WBFM, "wbfmmod")])
def test_modulator_handle_created_used_destroyed_and_created_again(oracle, kind, name):
    pcm = synth.lcg_pcm(5, 3).reshape(1, 3)
    outs = []
    for _ in range(2):
        m = api.Mod(kind, 1)
        o = oracle.ssbmod(True) if name == "ssbmod" else oracle.wbfmmod()
        got = [m.process(pcm[:, :1]), m.process(pcm[:, 1:3])]          # one sample, then the buffers grow (flat: one channel)
        assert got[0].shape == (512,) and got[1].shape == (1024,)
        assert (got[0] == o.process(pcm[0, :1])).all() and (got[1] == o.process(pcm[0, 1:3])).all()
        outs.append(np.concatenate(got))
        m.close()
    assert (outs[0] == outs[1]).all()


def test_nco_handle_created_used_destroyed_and_created_again(oracle):
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    outs = []
    for _ in range(2):
        g, o = api.Nco(256000.0, 75000.0, 1), oracle.nco(256000.0, 75000.0)
        for count in (1, 2):                                # one sample, then the outputs grow
            (i, q), (wi, wq) = g.run(count, fast=True), o.run(count, True)
            assert (bits(i) == bits(wi)).all() and (bits(q) == bits(wq)).all()
            outs.append((bits(i).copy(), bits(q).copy()))
        g.close()
    assert all((a == b).all() for x, y in zip(outs[:2], outs[2:]) for a, b in zip(x, y))
