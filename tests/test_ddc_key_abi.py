"""CPU-side checks of the DDC bank's receive key (hrfd_ddc_set_key_block, hrfd_ddc_n_keys, hrfd_ddc_get_key_skips,
hrfd_ddc_count_key_skips and the *_keyed calls): every argument error comes back as HRFD_EINVAL before any device is touched,
with a NULL handle where the argument alone decides, so these hold on a machine without a GPU; api.Ddc exposes the calls.
n_keys needs a handle, so its arithmetic is held here through the host-only count (its stride check is n_keys) and in
tests/cpp/san_ddc_key.cc; tests/test_gpu_ddc_key.py asks the handle.  The meter's channel (< C or ALL) needs a handle's C
as well: without one only the NULL result and the NULL handle are refused here, the range check itself
(ddc_key_check_channel) is held in tests/cpp/san_ddc_key.cc and, on a handle, in tests/test_gpu_ddc_key.py."""
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
    for name in ("set_key_block", "n_keys", "get_key_skips", "count_key_skips", "process_keyed", "process_device_keyed",
                 "receive_keyed"):
        assert hasattr(L, "hrfd_ddc_" + name), name
        assert getattr(L, "hrfd_ddc_" + name).argtypes is not None, name


@pytest.mark.parametrize("k", [0, 9, 18, 0xFFFFFFFF])
def test_set_key_block_refuses_bad_blocks_without_a_handle(L, k):
    assert L.hrfd_ddc_set_key_block(None, k) == EINVAL and "key block" in err(L) and "2^10..2^17" in err(L)


@pytest.mark.parametrize("k", [10, 17])
def test_set_key_block_needs_a_handle(L, k):
    assert L.hrfd_ddc_set_key_block(None, k) == EINVAL and "handle" in err(L)


def test_getters_refuse_a_null_result_and_a_null_handle(L):
    n32, n64 = C.c_uint32(7), C.c_uint64(7)
    assert L.hrfd_ddc_n_keys(None, 4096, None) == EINVAL and "NULL result" in err(L)
    assert L.hrfd_ddc_n_keys(None, 4096, C.byref(n32)) == EINVAL and "handle" in err(L) and n32.value == 7
    for channel in (0, api.ALL):
        assert L.hrfd_ddc_get_key_skips(None, channel, None) == EINVAL and "NULL result" in err(L)
        assert L.hrfd_ddc_get_key_skips(None, channel, C.byref(n64)) == EINVAL and "handle" in err(L) and n64.value == 7


# M output samples -> n_keys at k = 10 and at k = 17
N_KEYS = [(1, 1, 1), (1024, 1, 1), (1025, 2, 1), (1 << 17, 128, 1), ((1 << 17) + 1, 129, 2)]


@pytest.mark.parametrize("M,n10,n17", N_KEYS)
def test_n_keys_is_the_stride_a_call_needs(L, M, n10, n17):
    """a key_stride of n_keys is taken, one below it is refused with n_keys in the text: by the host-only count under both
    key blocks, and by the keyed device entry without a handle (which checks against the largest block, 2^17)"""
    for k, nk in ((10, n10), (17, n17)):
        assert nk == -(-M // (1 << k))
        key = np.ones((2, nk), dtype=np.uint8)
        per, total = np.zeros(2, dtype=np.uint64), C.c_uint64(7)
        p_per = per.ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.hrfd_ddc_count_key_skips(key.ctypes.data, nk, 2, 2 * M, k, p_per, C.byref(total)) == 0, err(L)
        assert total.value == 0 and not per.any()
        assert L.hrfd_ddc_count_key_skips(key.ctypes.data, nk - 1, 2, 2 * M, k, p_per, C.byref(total)) == EINVAL
        assert f"key_stride {nk - 1}" in err(L) and f"n_keys = {nk}" in err(L)
    buf = np.zeros(64, dtype=np.int8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.hrfd_ddc_process_device_keyed(None, ptr, 8 * 2 * M, 2 * M, ptr, n17 - 1, ptr, 2 * M, None) == EINVAL
    assert f"key_stride {n17 - 1}" in err(L) and f"n_keys = {n17}" in err(L)
    assert L.hrfd_ddc_process_device_keyed(None, ptr, 8 * 2 * M, 2 * M, ptr, n17, ptr, 2 * M, None) == EINVAL
    assert "NULL" in err(L) and "key_stride" not in err(L)


def test_count_key_skips_counts_and_refuses(L):
    key = np.array([[0, 1, 0, 0x80, 0, 0], [0, 0, 0, 0, 0, 0], [1, 2, 3, 4, 5, 6]], dtype=np.uint8)
    per, total = api.ddc_count_key_skips(key, 2 * (5 * 1024 + 37), 10)
    assert per.tolist() == [4, 6, 0] and total == 10
    per, total = api.ddc_count_key_skips(key[:, :3], 2 * (5 * 1024 + 37), 11)      # two tiles per byte
    assert per.tolist() == [4, 6, 0] and total == 10
    n = C.c_uint64(0)
    k8 = np.zeros(8, dtype=np.uint8)
    for k in (9, 18):
        assert L.hrfd_ddc_count_key_skips(k8.ctypes.data, 8, 1, 2048, k, None, C.byref(n)) == EINVAL and "key block" in err(L)
    assert L.hrfd_ddc_count_key_skips(k8.ctypes.data, 8, 1, 2048, 10, None, None) == EINVAL and "NULL result" in err(L)
    assert L.hrfd_ddc_count_key_skips(None, 8, 1, 2048, 10, None, C.byref(n)) == EINVAL
    assert L.hrfd_ddc_count_key_skips(k8.ctypes.data, 8, 0, 2048, 10, None, C.byref(n)) == EINVAL
    assert L.hrfd_ddc_count_key_skips(k8.ctypes.data, 8, 1, 2048, 10, None, C.byref(n)) == 0 and n.value == 1   # per_channel NULL


def test_keyed_calls_refuse_a_short_key_stride_without_a_handle(L):
    buf = np.zeros(64, dtype=np.int8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    n = C.c_uint32(0)
    # 2^17 + 1 output samples are two keys under the largest key block, which asks the least
    ob = 2 * ((1 << 17) + 1)
    assert L.hrfd_ddc_process_device_keyed(None, ptr, 8 * ob, ob, ptr, 1, ptr, ob, None) == EINVAL
    assert "key_stride 1" in err(L) and "n_keys = 2" in err(L) and "hrfd_ddc_process_device_keyed" in err(L)
    assert L.hrfd_ddc_process_device_keyed(None, ptr, 8 * ob, ob, ptr, 0, ptr, ob, None) == EINVAL and "key_stride 0" in err(L)
    # receive: 3 blocks of 262144 bytes are 3 keys
    args = (ptr, 1 << 30, 262144, 3)
    assert L.hrfd_ddc_receive_keyed(None, ptr, *args, ptr, 2, 0, ptr, ptr, None, None, C.byref(n)) == EINVAL
    assert "key_stride 2" in err(L) and "n_keys = 3" in err(L) and "hrfd_ddc_receive_keyed" in err(L)
    # a stride that suffices, or no key at all: only the handle is missing
    assert L.hrfd_ddc_receive_keyed(None, ptr, *args, ptr, 3, 0, ptr, ptr, None, None, C.byref(n)) == EINVAL and "NULL" in err(L)
    assert L.hrfd_ddc_receive_keyed(None, ptr, *args, None, 0, 0, ptr, ptr, None, None, C.byref(n)) == EINVAL and "NULL" in err(L)
    assert L.hrfd_ddc_process_device_keyed(None, ptr, 8 * ob, ob, ptr, 2, ptr, ob, None) == EINVAL and "NULL" in err(L)
    assert L.hrfd_ddc_process_device_keyed(None, ptr, 8 * ob, ob, None, 0, ptr, ob, None) == EINVAL and "NULL" in err(L)
    assert L.hrfd_ddc_process_keyed(None, ptr, 4, ptr, ptr) == EINVAL and "NULL" in err(L)
    # the unkeyed entries keep their names in their refusals
    assert L.hrfd_ddc_receive(None, None, *args, 0, ptr, ptr, None, None, C.byref(n)) == EINVAL
    assert err(L).startswith("hrfd_ddc_receive:")
    assert L.hrfd_ddc_receive_keyed(None, ptr, ptr, 1 << 30, 3, 1, ptr, 1, 0, ptr, ptr, None, None, C.byref(n)) == EINVAL
    assert "block_bytes" in err(L)


def test_header_declares_the_key_block():
    text = open(os.path.join(ROOT, "include", "hrfd.h")).read()
    for name in ("hrfd_ddc_set_key_block", "hrfd_ddc_n_keys", "hrfd_ddc_get_key_skips", "hrfd_ddc_count_key_skips",
                 "hrfd_ddc_process_keyed", "hrfd_ddc_process_device_keyed", "hrfd_ddc_receive_keyed",
                 "outk[c][m] = key[c][m >> k] != 0 ? out[c][m] : (0, 0)", "key[c][(1024 t) >> k] == 0"):
        assert name in text, name


def test_ddc_exposes_the_key():
    for name in ("set_key_block", "n_keys", "key_skips"):
        assert callable(getattr(api.Ddc, name)), name
    assert inspect.signature(api.Ddc.key_skips).parameters["channel"].default == api.ALL
    # trailing keywords: the positional calls of before keep their meaning
    assert list(inspect.signature(api.Ddc.process).parameters) == ["self", "captures", "out_bytes", "key"]
    assert list(inspect.signature(api.Ddc.process_device).parameters)[-3:] == ["stream", "d_key", "key_stride"]
    assert list(inspect.signature(api.Ddc.receive).parameters)[-4:] == ["d_magnitude", "d_allowed", "d_key", "key_stride"]
    for fn, name in ((api.Ddc.process, "key"), (api.Ddc.process_device, "d_key"), (api.Ddc.receive, "d_key")):
        assert inspect.signature(fn).parameters[name].default is None
    assert callable(api.RxKey) and callable(api.ddc_count_key_skips)
