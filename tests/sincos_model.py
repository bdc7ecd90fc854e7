"""sinf / cosf on the CPU, through the project's own checker (oracle/hrfd_oracle.c: orc_sincosf_eval / _digest):

    MODEL0, MODEL1   glibc 2.35's algorithm restated without / with fma() (oracle/sincosf_model.h)
    LIBM             this host's sinf / cosf

numpy's float32 sin / cos are NOT libm's (they differ from it on about one float in eight), so nothing here goes
through numpy for a sine.  A chunk is 2^20 consecutive float bit patterns (chunk k: k << 20 ...); its digest is the
wrapping 64-bit sum of a mix of (pattern, bits(sin), bits(cos)), the same mix the device computes
(hrfd_debug_sincosf_digest).  ctypes releases the GIL during a call, so the chunk ranges are spread over threads."""
from __future__ import annotations

import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import reflib

MODEL0, MODEL1, LIBM = 0, 1, 2
CHUNK = 1 << 20
# |x| < 120: bit patterns 0 .. 0x42F00000 - 1, and the same with the sign bit
TOP = 0x42F00000
POS = (0, TOP >> 20)                   # (first chunk, chunks): 0..1070
NEG = (2048, TOP >> 20)                # 2048..3118
RANGES = {"pos": POS, "neg": NEG}
assert TOP % CHUNK == 0 and np.array([TOP], dtype=np.uint32).view(np.float32)[0] == 120.0

_f32p = C.POINTER(C.c_float)
_u64p = C.POINTER(C.c_uint64)


@functools.lru_cache(maxsize=None)
def _lib():
    reflib.build_oracle()
    L = C.CDLL(reflib.ORACLE_SO)
    L.orc_sincosf_eval.argtypes = [C.c_int, _f32p, C.c_size_t, _f32p, _f32p]
    L.orc_sincosf_digest.argtypes = [C.c_int, C.c_uint32, C.c_uint32, _u64p]
    return L


def workers() -> int:
    return min(16, len(os.sched_getaffinity(0)))


def from_bits(u) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(u, dtype=np.uint32)).view(np.float32)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def eval(source: int, x):
    """(sin, cos) of every float of x as float32 arrays"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    sn, cs = np.empty_like(x), np.empty_like(x)
    rc = _lib().orc_sincosf_eval(source, x.ctypes.data_as(_f32p), x.size, sn.ctypes.data_as(_f32p), cs.ctypes.data_as(_f32p))
    assert rc == 0, (source, rc)
    return sn, cs


def digest(source: int, first_chunk: int, n_chunks: int, piece: int = 4) -> np.ndarray:
    """uint64 [n_chunks]: the digests of chunks first_chunk .. first_chunk + n_chunks - 1"""
    out = np.zeros(n_chunks, dtype=np.uint64)
    L = _lib()

    def run(lo):
        n = min(piece, n_chunks - lo)
        rc = L.orc_sincosf_digest(source, first_chunk + lo, n, out[lo:lo + n].ctypes.data_as(_u64p))
        assert rc == 0, (source, first_chunk + lo, n, rc)

    with ThreadPoolExecutor(workers()) as pool:
        list(pool.map(run, range(0, n_chunks, piece)))
    return out


@functools.lru_cache(maxsize=None)
def range_digest(source: int, sign: str) -> np.ndarray:
    """the digests of every chunk of |x| < 120 with that sign ("pos" / "neg"); computed once per process, read-only"""
    d = digest(source, *RANGES[sign])
    d.setflags(write=False)
    return d


def chunk_patterns(chunk: int) -> np.ndarray:
    return (np.uint32(chunk) << np.uint32(20)) + np.arange(CHUNK, dtype=np.uint32)


# The floats with |x| < 120 on which glibc's algorithm gives another result with fused multiply-adds than without:
# 12 for sinf, 22 for cosf, all with |x| > 17.  tests/test_sincos_model.py derives this list anew from the two models (by
# digest, then by value) and requires it to be exactly this; tests/test_gpu_sincos.py uses it to show that the device's
# `variant` argument is live.  (sinf is odd and cosf even in both variants, so the patterns come in sign pairs.)
FMA_DIFFERS_SIN = (
    0x4255B0A9, 0x42A35C07, 0x42A35D44, 0x42A97360, 0x42CF5854, 0x42E87A55,
    0xC255B0A9, 0xC2A35C07, 0xC2A35D44, 0xC2A97360, 0xC2CF5854, 0xC2E87A55,
)
FMA_DIFFERS_COS = (
    0x418A3ADB, 0x418A3ADC, 0x418A3ADD, 0x418A3ADE, 0x41BC76D9, 0x4202EB4B, 0x42687A55, 0x4280CE28, 0x42870E40, 0x42C55FAA,
    0x42D8D23E,
    0xC18A3ADB, 0xC18A3ADC, 0xC18A3ADD, 0xC18A3ADE, 0xC1BC76D9, 0xC202EB4B, 0xC2687A55, 0xC280CE28, 0xC2870E40, 0xC2C55FAA,
    0xC2D8D23E,
)
