"""CPU-side checks of the DUC bank's transmit key (hrfd_duc_set_key_block, hrfd_duc_n_keys, hrfd_duc_get_key_skips and the
*_keyed calls): every argument error comes back as HRFD_EINVAL before any device is touched, with a NULL handle where the
argument alone decides, so these hold on a machine without a GPU; api.Duc exposes the calls; api.TxKey on CPU tensors equals
a plain loop."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from hackrfdiags_amd import _lib, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "hackrfdiags_amd", "csrc")])
    return _lib.load()


def err(L):
    return L.hrfd_last_error().decode(errors="replace")


def test_key_symbols_are_exported(L):
    for name in ("set_key_block", "n_keys", "get_key_skips", "process_keyed", "process_device_keyed", "transmit_keyed"):
        assert hasattr(L, "hrfd_duc_" + name), name


@pytest.mark.parametrize("k", [0, 9, 18, 0xFFFFFFFF])
def test_set_key_block_refuses_bad_blocks_without_a_handle(L, k):
    assert L.hrfd_duc_set_key_block(None, k) == EINVAL and "key block" in err(L) and "2^10..2^17" in err(L)


@pytest.mark.parametrize("k", [10, 17])
def test_set_key_block_needs_a_handle(L, k):
    assert L.hrfd_duc_set_key_block(None, k) == EINVAL and "handle" in err(L)


def test_getters_refuse_a_null_result_and_a_null_handle(L):
    n32, n64 = C.c_uint32(7), C.c_uint64(7)
    assert L.hrfd_duc_n_keys(None, 4096, None) == EINVAL and "NULL result" in err(L)
    assert L.hrfd_duc_n_keys(None, 4096, C.byref(n32)) == EINVAL and "handle" in err(L) and n32.value == 7
    assert L.hrfd_duc_get_key_skips(None, None) == EINVAL and "NULL result" in err(L)
    assert L.hrfd_duc_get_key_skips(None, C.byref(n64)) == EINVAL and "handle" in err(L) and n64.value == 7


def test_keyed_calls_refuse_a_short_key_stride_without_a_handle(L):
    buf = np.zeros(64, dtype=np.int8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    # 2^17 + 1 channel samples are two keys under the largest key block, which asks the least
    ib = 2 * ((1 << 17) + 1)
    assert L.hrfd_duc_process_device_keyed(None, ptr, ib, ib, ptr, 1, ptr, 8 * ib, None) == EINVAL
    assert "key_stride 1" in err(L) and "n_keys = 2" in err(L)
    assert L.hrfd_duc_process_device_keyed(None, ptr, ib, ib, ptr, 0, ptr, 8 * ib, None) == EINVAL and "key_stride 0" in err(L)
    assert L.hrfd_duc_transmit_keyed(None, ptr, ptr, 513, ptr, 1, ptr, 1 << 30, None) == EINVAL and "key_stride 1" in err(L)
    assert L.hrfd_duc_transmit_keyed(None, ptr, ptr, 512, ptr, 1, ptr, 1 << 30, None) == EINVAL and "NULL" in err(L)
    # a stride that suffices, or no key at all: only the handle is missing
    assert L.hrfd_duc_process_device_keyed(None, ptr, ib, ib, ptr, 2, ptr, 8 * ib, None) == EINVAL and "NULL" in err(L)
    assert L.hrfd_duc_process_device_keyed(None, ptr, ib, ib, None, 0, ptr, 8 * ib, None) == EINVAL and "NULL" in err(L)
    assert L.hrfd_duc_process_keyed(None, ptr, 4, ptr, ptr) == EINVAL and "NULL" in err(L)
    assert L.hrfd_duc_transmit_keyed(None, None, ptr, 1, ptr, 1, ptr, 1 << 20, None) == EINVAL
    assert L.hrfd_duc_transmit_keyed(None, ptr, ptr, 0, ptr, 1, ptr, 1 << 20, None) == EINVAL and "n_per_channel" in err(L)
    assert "hrfd_duc_transmit_keyed" in err(L)


def test_header_declares_the_key_block():
    text = open(os.path.join(ROOT, "include", "hrfd.h")).read()
    for name in ("hrfd_duc_set_key_block", "hrfd_duc_n_keys", "hrfd_duc_get_key_skips", "hrfd_duc_process_keyed",
                 "hrfd_duc_process_device_keyed", "hrfd_duc_transmit_keyed", "xk[c][m] = key[c][m >> k] != 0 ? x[c][m] : 0",
                 "+-220 kHz"):
        assert name in text, name


def test_duc_exposes_the_key():
    for name in ("set_key_block", "n_keys", "key_skips"):
        assert callable(getattr(api.Duc, name)), name
    # trailing keywords: the positional calls of before keep their meaning
    assert list(inspect.signature(api.Duc.process).parameters) == ["self", "channels", "in_bytes", "key"]
    assert list(inspect.signature(api.Duc.process_device).parameters)[-3:] == ["stream", "d_key", "key_stride"]
    assert list(inspect.signature(api.Duc.transmit).parameters)[-3:] == ["stream", "d_key", "key_stride"]
    for fn, name in ((api.Duc.process, "key"), (api.Duc.process_device, "d_key"), (api.Duc.transmit, "d_key")):
        assert inspect.signature(fn).parameters[name].default is None


def txkey_loop(inputs, C_, hold):
    """key[c][b] = 1 iff any input is on in stream blocks b - hold .. b; blocks in front of the stream are off"""
    n = next(a.shape[1] for a in inputs if a is not None)
    on = np.zeros((C_, n), dtype=bool)
    for a in inputs:
        if a is not None:
            on |= a != 0
    key = np.zeros((C_, n), dtype=np.uint8)
    for c in range(C_):
        for b in range(n):
            key[c, b] = int(any(on[c, j] for j in range(max(0, b - hold), b + 1)))
    return key


@pytest.mark.parametrize("hold", [0, 1, 3])
@pytest.mark.parametrize("cut", [1, 2, 5])
def test_txkey_equals_a_plain_loop(hold, cut):
    import torch
    rng = np.random.default_rng(10 * hold + cut)
    C_, n = 4, 40
    tone = (rng.integers(0, 6, size=(C_, n)) == 0).astype(np.uint8)
    afsk = ((rng.integers(0, 9, size=(C_, n)) == 0) * 200).astype(np.uint8)
    tone[2] = 0
    afsk[2] = 0
    afsk[2, 7] = 1                                             # one block on: exactly hold + 1 keys
    ptt = np.zeros((C_, n), dtype=np.uint8)
    ptt[1, 20:23] = 1
    want = txkey_loop([tone, None, afsk, ptt], C_, hold)
    assert want[2].sum() == hold + 1 and want[2, 7] == 1
    tk = api.TxKey(C_, hold=hold)
    got = []
    for at in range(0, n, cut):
        part = [None if a is None else torch.from_numpy(a[:, at:at + cut].copy()) for a in (tone, None, afsk, ptt)]
        k = tk(*part)
        assert k.dtype == torch.uint8 and tuple(k.shape) == (C_, cut) and k.is_contiguous()
        got.append(k.numpy())
    assert (np.concatenate(got, axis=1) == want).all()
    assert set(np.unique(want)) <= {0, 1}


def test_txkey_refuses_nothing_to_key():
    with pytest.raises(ValueError):
        api.TxKey(2)(None, None)
    with pytest.raises(ValueError):
        api.TxKey(0)
    with pytest.raises(ValueError):
        api.TxKey(2, hold=-1)
