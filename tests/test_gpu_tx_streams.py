"""The modulator handle on the banks' host core: calls on different streams with no host wait between
them, scratch that grows and setters that upload under a pending launch, hrfd_duc_transmit mixed with
hrfd_mod_process_device, and the refusal of calls whose 32-bit arithmetic would wrap.  Every result byte for byte against
the same calls on a second handle, on one stream with a host wait behind each call -- and against the CPU oracle for
the kinds that have one."""
import numpy as np
import pytest

from hackrfdiags_amd import api, synth
from tests import tx_slices_model as M

pytestmark = pytest.mark.gpu
C9 = 9                                                      # a partial group of eight
ORACLE = {api.MOD_SSB: "ssbmod", api.MOD_AM: "ammod", api.MOD_FM: "fmmod", api.MOD_WBFM: "wbfmmod"}


@pytest.fixture(scope="module")
def gpu():
    import torch
    if api.device_count() < 1:
        pytest.fail("no GPU visible: the HIP path cannot run (and there is no CPU fallback)")
    return torch, torch.device("cuda:0"), torch.cuda.Stream()


def pcm_calls(lengths, seed, C=C9):
    return [np.stack([synth.lcg_pcm(seed + 31 * i + c, n) for c in range(C)]) for i, n in enumerate(lengths)]


def run(gpu, kind, xs, streams, prepare=None, between=None, wait=False, C=C9):
    """the calls xs[i] on streams[i] (None: the handle's own) of one new handle; between(m, i) runs in front of call i.
    wait: a host wait behind every call (the reference); otherwise none until all calls are out.  Returns (handle, outputs)."""
    torch, dev, _ = gpu
    m = api.Mod(kind, C, device=0)
    if prepare:
        prepare(m)
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    d_out = [torch.zeros((C, 512 * x.shape[1]), dtype=torch.int8, device=dev) for x in xs]
    torch.cuda.synchronize()
    for i, x in enumerate(xs):
        if between:
            between(m, i)
        m.process_device(d_in[i].data_ptr(), x.shape[1], d_out[i].data_ptr(), streams[i])
        if wait:
            m.sync()
    torch.cuda.synchronize()
    m.sync()
    return m, [o.cpu().numpy() for o in d_out]


def same(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g == w).all(), (what, i, np.argwhere(g != w)[:3])


@pytest.mark.parametrize("kind,n,sliced", [(api.MOD_SSB, 512, None), (api.MOD_AM, 512, None), (api.MOD_SIG_PM, 512, None),
                                           (api.MOD_FM, 4096, None), (api.MOD_FM, 3968, None),
                                           (api.MOD_WBFM, 1664, 2), (api.MOD_WBFM, 1536, None)],
                         ids=["ssb", "am", "sig_pm", "fm_sliced", "fm_whole", "wbfm_sliced", "wbfm_whole"])
def test_stream_hand_over(gpu, oracle, kind, n, sliced):
    """three calls, the handle's stream / a caller's / the handle's, no host wait between them: the pipelines, the phase
    accumulators and the scratch are handed from launch to launch on the device"""
    side = gpu[2].cuda_stream
    xs = pcm_calls([n] * 3, 400 + kind)
    prepare = (lambda m: m.debug_set_sliced(sliced)) if sliced is not None else None
    _, got = run(gpu, kind, xs, [None, side, None], prepare)
    _, want = run(gpu, kind, xs, [None] * 3, prepare, wait=True)
    same(got, want, "hand-over")
    if kind in ORACLE:
        for c in (0, C9 - 1):
            o = getattr(oracle, ORACLE[kind])(True) if kind == api.MOD_SSB else getattr(oracle, ORACLE[kind])()
            for i, x in enumerate(xs):
                ref = np.concatenate([o.process(x[c, s:s + 512]) for s in range(0, n, 512)]) if kind == api.MOD_SSB else o.process(x[c])
                assert (got[i][c] == ref).all(), (i, c)


@pytest.mark.parametrize("kind", [api.MOD_AM, api.MOD_FM, api.MOD_WBFM], ids=["am", "fm", "wbfm"])
def test_scratch_grows_under_a_pending_launch(gpu, kind):
    """512 samples on a caller's stream, then 2048 on the handle's with no wait: the rails, phases or cells the first
    launch may still read are freed and allocated anew only when it is through"""
    xs = pcm_calls([512, 2048], 500 + kind)
    _, got = run(gpu, kind, xs, [gpu[2].cuda_stream, None])
    _, want = run(gpu, kind, xs, [None, None], wait=True)
    same(got, want, "growth")


@pytest.mark.parametrize("kind", [api.MOD_SSB, api.MOD_AM, api.MOD_FM, api.MOD_WBFM], ids=["ssb", "am", "fm", "wbfm"])
def test_setter_between_calls_on_two_streams(gpu, kind):
    """a setter and a channel's reset between two calls on different streams: the upload waits for the first launch, the
    first call's output is that of a handle nobody touched, the second call's differs from it and is the reference's"""
    def between(m, i):
        if i == 1:
            if kind == api.MOD_SSB:
                m.set_sideband(False, channel=2)
            else:
                m.set_param({api.MOD_AM: 0.3, api.MOD_FM: 1500.0, api.MOD_WBFM: 30000.0}[kind], channel=2)
            m.reset(channel=5)
    xs = pcm_calls([512, 512], 600 + kind)
    _, got = run(gpu, kind, xs, [gpu[2].cuda_stream, None], between=between)
    _, want = run(gpu, kind, xs, [None, None], between=between, wait=True)
    _, untouched = run(gpu, kind, xs, [None, None], wait=True)
    same(got, want, "setter")
    assert (got[0] == untouched[0]).all()
    for c in range(C9):
        assert (got[1][c] == untouched[1][c]).all() == (c not in (2, 5)), c


@pytest.mark.parametrize("kind", [api.MOD_SSB, api.MOD_FM, api.MOD_WBFM], ids=["ssb", "fm", "wbfm"])
def test_transmit_then_process_device_on_the_handles_own_streams(gpu, kind):
    """Duc.transmit runs the modulator on the DUC's stream; Mod.process_device(stream=None) behind it runs on the
    modulator's own, with no wait: the second call continues the first one's state"""
    torch, dev, _ = gpu
    R, W, n, ib = 4, 2, 512, 512 * 512
    xs = pcm_calls([n, n], 700 + kind)
    d_in = [torch.from_numpy(x).to(dev) for x in xs]
    cap = [torch.zeros((W, R * ib), dtype=torch.int8, device=dev) for _ in range(2)]
    out = [torch.zeros((C9, ib), dtype=torch.int8, device=dev) for _ in range(3)]
    mods, ducs = [api.Mod(kind, C9, device=0) for _ in range(2)], [api.Duc(W, C9, R, device=0) for _ in range(2)]
    for d in ducs:
        for c in range(C9):
            d.tune(c, c % W, -400_000 + 90_000 * c)
    torch.cuda.synchronize()
    ducs[0].transmit(mods[0], d_in[0].data_ptr(), n, cap[0].data_ptr(), R * ib)
    mods[0].process_device(d_in[1].data_ptr(), n, out[0].data_ptr())
    torch.cuda.synchronize()
    mods[1].process_device(d_in[0].data_ptr(), n, out[1].data_ptr())
    mods[1].sync()
    ducs[1].process_device(out[1].data_ptr(), ib, ib, cap[1].data_ptr(), R * ib)
    torch.cuda.synchronize()
    mods[1].process_device(d_in[1].data_ptr(), n, out[2].data_ptr())
    mods[1].sync()
    assert (cap[0].cpu().numpy() == cap[1].cpu().numpy()).all()
    assert (out[0].cpu().numpy() == out[2].cpu().numpy()).all()


@pytest.mark.parametrize("kind", [api.MOD_SSB, api.MOD_AM, api.MOD_FM, api.MOD_WBFM, api.MOD_SIG_PM],
                         ids=["ssb", "am", "fm", "wbfm", "sig_pm"])
def test_a_call_above_the_bound_is_refused_and_changes_nothing(gpu, kind):
    """one sample above tx_check_call's bound for this bank: HRFD_EINVAL with the numbers in its text, from both entries,
    nothing launched (the buffers are one byte long), and the calls around it are those of a handle that never saw it"""
    torch, dev, _ = gpu
    n_bad = M.max_n(kind, C9) + 1
    byte = torch.zeros(1, dtype=torch.int8, device=dev)
    host = np.zeros(1, dtype=np.int16)

    def between(m, i):
        if i == 1:
            assert m.L.hrfd_mod_process_device(m.h, byte.data_ptr(), n_bad, byte.data_ptr(), None) == -1
            assert str(n_bad) in m.L.hrfd_last_error().decode() and str(C9) in m.L.hrfd_last_error().decode()
            assert m.L.hrfd_mod_process(m.h, host.ctypes.data, n_bad, host.ctypes.data, None) == -1
            assert m.L.hrfd_last_error().decode().startswith("hrfd_mod_process: ")
    xs = pcm_calls([512, 512], 800 + kind)
    _, got = run(gpu, kind, xs, [None, None], between=between)
    _, want = run(gpu, kind, xs, [None, None], wait=True)
    same(got, want, "refusal")
    assert int(byte.cpu()[0]) == 0
