"""The DDC and DUC banks refuse bad arguments on a live handle (the counterpart of test_arguments_are_refused in
tests/test_gpu_spec_edges.py), and a refused call leaves the sample counter and the history alone: the valid call behind
the refusals equals the model's, which saw none of them."""
import numpy as np
import pytest

from hackrfdiags_amd import api
from tests import ddc_model as dm
from tests import duc_model as um
from tests.test_gpu_ddc import lcg_captures
from tests.test_gpu_duc import lcg_channels

pytestmark = pytest.mark.gpu
W, C, R, NB = 2, 3, 2, 2048


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda:0")


def bad_calls(call, narrow_row, wide_row):
    """process_device(narrow side first?) is the caller's: call(n_bytes, narrow_stride, wide_stride, in_offset)"""
    for n_bytes in (3, 0, (1 << 25) + 2):
        with pytest.raises(api.HrfdError):
            call(n_bytes, 1 << 26, 1 << 27, 0)
    for narrow, wide, off in ((narrow_row - 2, wide_row, 0), (narrow_row, wide_row - 2, 0), (narrow_row, wide_row, 1)):
        with pytest.raises(api.HrfdError):
            call(NB, narrow, wide, off)


def test_ddc_arguments_are_refused(torch_dev):
    torch, dev = torch_dev
    d, m = api.Ddc(W, C, R, device=0), dm.DdcModel(W, C, R)
    for c in range(C):
        d.set_step(c, c % W, dm.ddc_step(90_000 * (c + 1), R))
        m.set_tuning(c, c % W, dm.ddc_step(90_000 * (c + 1), R))
    cap = lcg_captures(W, R * NB, 5)
    assert (d.process(cap, NB) == m.process(cap, NB)).all()
    din = torch.zeros((W, R * NB + 16), dtype=torch.int8, device=dev)
    dout = torch.zeros((C, NB), dtype=torch.int8, device=dev)
    for args in ((C, 0, 1), (0, W, 1)):
        with pytest.raises(api.HrfdError):
            d.set_step(*args)
    bad_calls(lambda n, narrow, wide, off: d.process_device(din.data_ptr() + off, wide, n, dout.data_ptr(), narrow), NB, R * NB)
    with pytest.raises(api.HrfdError):
        d.process_device(din.data_ptr(), R * NB + 1, NB, dout.data_ptr(), NB)          # an odd capture stride
    with pytest.raises(api.HrfdError):
        d.process(np.zeros((W, 0), dtype=np.int8), 0)
    rx = api.Rx(C - 1, device=0)
    pcm = torch.zeros((C, 4), dtype=torch.int16, device=dev)
    n_pcm = torch.zeros((C, 1), dtype=torch.int32, device=dev)
    with pytest.raises(api.HrfdError):
        d.receive(rx, din.data_ptr(), R * NB, NB, 1, pcm.data_ptr(), n_pcm.data_ptr())
    cap = lcg_captures(W, R * NB, 6)
    assert (d.process(cap, NB) == m.process(cap, NB)).all()
    assert all(d.phase(c) == m.phase(c) for c in range(C))


def test_duc_arguments_are_refused(torch_dev):
    torch, dev = torch_dev
    d, m = api.Duc(W, C, R, device=0), um.DucModel(W, C, R)
    for c in range(C):
        d.set_step(c, c % W, um.duc_step(90_000 * (c + 1), R))
        m.set_tuning(c, c % W, um.duc_step(90_000 * (c + 1), R))
    ch = lcg_channels(C, NB // R, 5)
    assert (d.process(ch, NB // R) == m.process(ch, NB // R)).all()
    din = torch.zeros((C, NB + 16), dtype=torch.int8, device=dev)
    dout = torch.zeros((W, R * NB), dtype=torch.int8, device=dev)
    for args in ((C, 0, 1), (0, W, 1)):
        with pytest.raises(api.HrfdError):
            d.set_step(*args)
    bad_calls(lambda n, narrow, wide, off: d.process_device(din.data_ptr() + off, narrow, n, dout.data_ptr(), wide), NB, R * NB)
    with pytest.raises(api.HrfdError):
        d.process_device(din.data_ptr(), NB + 1, NB, dout.data_ptr(), R * NB)          # an odd channel stride
    with pytest.raises(api.HrfdError):
        d.process(np.zeros((C, 0), dtype=np.int8), 0)
    mod = api.Mod(api.MOD_WBFM, C + 1, device=0)
    pcm = torch.zeros((C + 1, 4), dtype=torch.int16, device=dev)
    with pytest.raises(api.HrfdError):
        d.transmit(mod, pcm.data_ptr(), 4, dout.data_ptr(), R * NB)
    ch = lcg_channels(C, NB // R, 6)                                                   # 2048 output bytes per capture
    assert (d.process(ch, NB // R) == m.process(ch, NB // R)).all()
    assert all(d.phase(c) == m.phase(c) for c in range(C))
