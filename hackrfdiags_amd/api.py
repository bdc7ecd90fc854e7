"""Python mirror of the C ABI (include/hrfd.h) -- thin ctypes plumbing used by
the tests and bench.py.  Names follow the reference: an Rx is C channels of
IqDataProcessor + demodulators; process_block == acceptIqData."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import HrfdError, check  # noqa: F401

NONE, AM, FM, WBFM, LSB, USB = range(6)
ALL = 0xFFFFFFFF
BLOCK_BYTES = 262144


def pcm_capacity(block_bytes: int) -> int:
    """row length of the PCM output for a block length: ceil(block_bytes / 512) (hrfd_rx_pcm_capacity)"""
    return (int(block_bytes) + 511) // 512


def iq256_capacity(block_bytes: int) -> int:
    """row length in bytes of the 256 kS/s dump for a block length: 2 * ceil(block_bytes / 16) (hrfd_rx_iq256_capacity)"""
    return 2 * ((int(block_bytes) // 2 + 7) // 8)


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data)
    return C.c_void_p(int(a))          # raw device pointer (e.g. torch tensor .data_ptr())


class Rx:
    """n_channels receive chains (hrfd_rx_*)."""

    def __init__(self, n_channels: int, device: int = -1):
        self.L = _lib.load()
        self.n = int(n_channels)
        h = C.c_void_p()
        check(self.L.hrfd_rx_create(self.n, device, C.byref(h)), "hrfd_rx_create")
        self.h = h
        self.gain_db = 0
        self._transports = []          # Ingest objects over this handle: destroyed before it (they use it when they go)

    def close(self):
        for t in list(getattr(self, "_transports", ())):
            t.close()
        if getattr(self, "h", None):
            self.L.hrfd_rx_destroy(self.h)
            self.h = None

    __del__ = close

    def set_mode(self, mode, channel=ALL):
        check(self.L.hrfd_rx_set_mode(self.h, channel, mode), "hrfd_rx_set_mode")

    def set_gain(self, mode, gain, channel=ALL):
        check(self.L.hrfd_rx_set_gain(self.h, channel, mode, C.c_float(gain)), "hrfd_rx_set_gain")

    def set_threshold(self, threshold, channel=ALL):
        check(self.L.hrfd_rx_set_threshold(self.h, channel, threshold), "hrfd_rx_set_threshold")

    def reset_demod(self, mode, channel=ALL):
        check(self.L.hrfd_rx_reset_demod(self.h, channel, mode), "hrfd_rx_reset_demod")

    def process_block(self, iq: np.ndarray, n_blocks: int = 1, want_iq256: bool = False):
        """iq: int8 [C, n_blocks, block_bytes] (or flat).  Host buffers in, host arrays out:
        (pcm [C,B,npcm], n_pcm [C,B], magnitude [C,B], allowed [C,B], iq256 [C,B,bb/8] | None)"""
        iq = np.ascontiguousarray(iq, dtype=np.int8).reshape(self.n, n_blocks, -1)
        bb = iq.shape[2]
        npcm = pcm_capacity(bb)                            # rows: what a call of any even length can complete at most
        pcm = np.zeros((self.n, n_blocks, npcm), dtype=np.int16)
        n_pcm = np.zeros((self.n, n_blocks), dtype=np.uint32)
        mag = np.zeros((self.n, n_blocks), dtype=np.uint32)
        allowed = np.zeros((self.n, n_blocks), dtype=np.uint8)
        iq256 = np.zeros((self.n, n_blocks, iq256_capacity(bb)), dtype=np.int8) if want_iq256 else None
        check(self.L.hrfd_rx_process_block(self.h, _ptr(iq), bb, n_blocks, self.gain_db, _ptr(pcm),
                                           _ptr(n_pcm), _ptr(mag), _ptr(allowed), _ptr(iq256)),
              "hrfd_rx_process_block")
        return pcm, n_pcm, mag, allowed, iq256

    def reduce_sample_rate(self, iq: np.ndarray) -> np.ndarray:
        """IqDataProcessor::reduceSampleRate for one block of every channel: iq int8 [C, block_bytes] -> the 256 kS/s
        stream int8 [C, block_bytes / 8] (with the Fs/4 rotation); only the decimator pipelines advance"""
        iq = np.ascontiguousarray(iq, dtype=np.int8).reshape(self.n, -1)
        out = np.zeros((self.n, iq256_capacity(iq.shape[1])), dtype=np.int8)
        check(self.L.hrfd_rx_reduce_sample_rate(self.h, _ptr(iq), iq.shape[1], _ptr(out)), "hrfd_rx_reduce_sample_rate")
        return out

    def process_device(self, d_iq, channel_stride, block_bytes, n_blocks, d_pcm, d_n_pcm=None,
                       d_magnitude=None, d_allowed=None, d_iq256=None, stream=None):
        """All pointers are device addresses (ints); asynchronous."""
        check(self.L.hrfd_rx_process_device(self.h, _ptr(d_iq), channel_stride, block_bytes, n_blocks,
                                            self.gain_db, _ptr(d_pcm), _ptr(d_n_pcm), _ptr(d_magnitude),
                                            _ptr(d_allowed), _ptr(d_iq256), _ptr(stream)),
              "hrfd_rx_process_device")

    def pending_samples(self) -> int:
        """IQ samples the front end holds back after the calls so far (0..7): the next call of bb bytes completes
        (pending + bb // 2) // 8 samples at 256 kS/s (IqDataProcessor::reduceSampleRate's count)"""
        v = C.c_uint32(0)
        check(self.L.hrfd_rx_pending_samples(self.h, C.byref(v)), "hrfd_rx_pending_samples")
        return int(v.value)

    def sync(self) -> int:
        """waits for the last process_device; returns the number of channels that did not commit"""
        v = C.c_uint32(0)
        check(self.L.hrfd_rx_sync(self.h, C.byref(v)), "hrfd_rx_sync")
        return int(v.value)

    def failed_channels(self) -> np.ndarray:
        """uint8 [n_channels]: != 0 where the channel did not commit in the launch sync() last waited for"""
        out = np.zeros(self.n, dtype=np.uint8)
        check(self.L.hrfd_rx_failed_channels(self.h, out.ctypes.data, self.n), "hrfd_rx_failed_channels")
        return out

    # test hooks
    def debug_set_atan(self, mode: int):
        """-1 automatic, 0 force the atan2 table gather, 1 require the arithmetic atan2 kernel."""
        check(self.L.hrfd_rx_debug_set_atan(self.h, int(mode)), "hrfd_rx_debug_set_atan")

    def debug_atan_eval(self, tab: bool = False):
        """The arithmetic atan2 of the WBFM kernels over all (q, i): float32 [256][256]; tab: the
        first-octant-table variant of k_rx_wbfm_flow instead of the polynomial one."""
        out = np.zeros((256, 256), dtype=np.float32)
        fn = (self.L.hrfd_rx_debug_atan_eval_quad if tab == "quad" else
              self.L.hrfd_rx_debug_atan_eval_tab if tab else self.L.hrfd_rx_debug_atan_eval)
        check(fn(self.h, out.ctypes.data_as(C.POINTER(C.c_float))), "hrfd_rx_debug_atan_eval")
        return out

    def debug_ragged(self):
        """(the handle left the 512-byte grid, launches that ran on the general-length kernel k_rx_ragged)"""
        off, n = C.c_int32(0), C.c_ulonglong(0)
        check(self.L.hrfd_rx_debug_ragged(self.h, C.byref(off), C.byref(n)), "hrfd_rx_debug_ragged")
        return bool(off.value), int(n.value)

    def debug_mag_skipped(self) -> int:
        """launches so far that ran on the WBFM flow kernel's instantiation without the squelch magnitude (no magnitude
        buffer passed and no gate of the bank could close)"""
        n = C.c_ulonglong(0)
        fn = self.L.hrfd_rx_debug_mag_skipped
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
        check(fn(self.h, C.byref(n)), "hrfd_rx_debug_mag_skipped")
        return int(n.value)

    def debug_set_run_len(self, blocks: int):
        """consecutive blocks of a channel per WBFM workgroup (0 = automatic)"""
        check(self.L.hrfd_rx_debug_set_run_len(self.h, int(blocks)), "hrfd_rx_debug_set_run_len")

    def debug_set_warm(self, warm: int):
        check(self.L.hrfd_rx_debug_set_warm(self.h, warm), "hrfd_rx_debug_set_warm")

    def debug_enable_timing(self, slots=1):
        """HIP events around the demodulator kernels of every launch (slot = launch % slots)."""
        check(self.L.hrfd_rx_debug_enable_timing(self.h, int(slots)), "hrfd_rx_debug_enable_timing")

    def debug_timing_every(self, n: int):
        """bracket only every n-th launch with events (the others run back to back, as in a host that does not measure)"""
        check(self.L.hrfd_rx_debug_timing_every(self.h, int(n)), "hrfd_rx_debug_timing_every")

    def debug_kernel_ms(self, slot=0) -> float:
        ms = C.c_float(0)
        check(self.L.hrfd_rx_debug_kernel_ms(self.h, int(slot), C.byref(ms)), "hrfd_rx_debug_kernel_ms")
        return float(ms.value)

    def debug_stamps(self, groups: int, read: bool = False):
        """groups > 0, read=False: allocate stamp storage; read=True: fetch [groups, 48] uint64 (kDbgSlots)."""
        if not read:
            check(self.L.hrfd_rx_debug_stamps(self.h, groups, None), "hrfd_rx_debug_stamps")
            return None
        out = np.zeros((groups, 48), dtype=np.uint64)
        check(self.L.hrfd_rx_debug_stamps(self.h, groups, _ptr(out)), "hrfd_rx_debug_stamps")
        return out

    def debug_set_stream(self, kernel):
        """test hook: WBFM batches on 0 / False = the block kernel k_rx_wbfm, anything else = k_rx_wbfm_flow where it
        applies (the default)"""
        check(self.L.hrfd_rx_debug_set_stream(self.h, int(kernel)), "hrfd_rx_debug_set_stream")

    def debug_set_fir_flow(self, mode: int):
        """test hook: AM / SSB / FM batches on the flow kernel's FIR modes: -1 automatic, 0 never, 1 always, 2 always and one
        launch per kind (a bank of several kinds does not take k_rx_flow_bank)"""
        check(self.L.hrfd_rx_debug_set_fir_flow(self.h, int(mode)), "hrfd_rx_debug_set_fir_flow")

    def debug_set_gated(self, on: bool):
        """test hook: False = no gated second pass on the device (closed gates in a batch go back to the host's replay)"""
        check(self.L.hrfd_rx_debug_set_gated(self.h, int(bool(on))), "hrfd_rx_debug_set_gated")

    def debug_expire(self, where: int):
        """test hook: workgroup 0 of the next k_rx_wbfm_flow launch treats its wait `where` (1..6) as expired"""
        check(self.L.hrfd_rx_debug_expire(self.h, int(where)), "hrfd_rx_debug_expire")

    def debug_set_stagger(self, units: int):
        check(self.L.hrfd_rx_debug_set_stagger(self.h, units), "hrfd_rx_debug_set_stagger")

    def debug_counters(self):
        """[repairs, gate_viol, spec_viol, committed, total_repairs, total_uncommitted_launches,
        total_launches, host_replays] -- the first four describe the last launch."""
        out = (C.c_uint32 * 8)()
        check(self.L.hrfd_rx_debug_counters(self.h, out), "hrfd_rx_debug_counters")
        return list(out)


class SingleChannelRx:
    """One channel with the call shape the golden checks use (mirrors one
    IqDataProcessor::acceptIqData call per process())."""

    def __init__(self, device: int = -1):
        self.rx = Rx(1, device)

    @property
    def gain_db(self):
        return self.rx.gain_db

    @gain_db.setter
    def gain_db(self, v):
        self.rx.gain_db = int(v)

    def set_mode(self, mode):
        self.rx.set_mode(mode)

    def set_gain(self, mode, gain):
        self.rx.set_gain(mode, gain)

    def set_threshold(self, t):
        self.rx.set_threshold(t)

    def process(self, iq):
        pending = self.rx.pending_samples()
        pcm, n_pcm, mag, allowed, iq256 = self.rx.process_block(iq, 1, want_iq256=True)
        n = int(n_pcm[0, 0])
        n256 = 2 * ((pending + np.asarray(iq).size // 2) // 8)    # decimatedByteCount of this call
        return pcm[0, 0, :n].copy(), int(mag[0, 0]), bool(allowed[0, 0]), iq256[0, 0, :n256]


class Demod:
    """n_channels instances of one demodulator class on 256 kS/s mixed IQ
    (hrfd_demod_*; mirrors X::acceptIqData / setDemodulatorGain / resetDemodulator)."""

    def __init__(self, mode: int, n_channels: int = 1, device: int = -1):
        self.L = _lib.load()
        self.n = int(n_channels)
        h = C.c_void_p()
        check(self.L.hrfd_demod_create(mode, self.n, device, C.byref(h)), "hrfd_demod_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.hrfd_demod_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self, channel=ALL):
        check(self.L.hrfd_demod_reset(self.h, channel), "hrfd_demod_reset")

    def set_gain(self, gain, channel=ALL):
        check(self.L.hrfd_demod_set_gain(self.h, channel, C.c_float(gain)), "hrfd_demod_set_gain")

    def set_sideband(self, lsb, channel=ALL):
        check(self.L.hrfd_demod_set_sideband(self.h, channel, int(bool(lsb))), "hrfd_demod_set_sideband")

    def process(self, iq256):
        """iq256: int8 [C, bytes] (or flat for C == 1) -> pcm int16 [C, bytes/64]"""
        iq256 = np.ascontiguousarray(iq256, dtype=np.int8).reshape(self.n, -1)
        nb = iq256.shape[1]
        pcm = np.zeros((self.n, (nb + 63) // 64), dtype=np.int16)
        n_pcm = np.zeros(self.n, dtype=np.uint32)
        check(self.L.hrfd_demod_process(self.h, _ptr(iq256), nb, _ptr(pcm), _ptr(n_pcm)), "hrfd_demod_process")
        assert (n_pcm == n_pcm[0]).all()                   # the channels of a handle have seen the same lengths
        pcm = pcm[:, :int(n_pcm[0])]
        return pcm if self.n > 1 else pcm[0]


MOD_SSB, MOD_INTERP, MOD_AM, MOD_FM, MOD_WBFM = 1, 2, 3, 4, 5
MOD_SIG_AM, MOD_SIG_DSB, MOD_SIG_PM, MOD_SIG_FM = 6, 7, 8, 9   # signals/{am,dsb,pm,fm}.cc | interpolateSignal


class Ingest:
    """Pinned-memory, double-buffered block transport in front of an Rx (hrfd_ingest_*)."""

    def __init__(self, rx: "Rx", block_bytes: int, n_blocks: int, n_slots: int = 2):
        self.L = _lib.load()
        self.rx = rx
        self.block_bytes, self.n_blocks, self.C = int(block_bytes), int(n_blocks), rx.n
        h = C.c_void_p()
        check(self.L.hrfd_ingest_create(rx.h, self.block_bytes, self.n_blocks, int(n_slots), C.byref(h)),
              "hrfd_ingest_create")
        self.h = h
        rx._transports.append(self)    # whichever of the two goes first, the transport is destroyed before the handle

    def close(self):
        if getattr(self, "h", None):
            self.L.hrfd_ingest_destroy(self.h)
            self.h = None
            if self in self.rx._transports:
                self.rx._transports.remove(self)

    __del__ = close

    def acquire(self) -> np.ndarray:
        """the next free slot's pinned input buffer as int8 [C, n_blocks, block_bytes] (a view)"""
        p = C.c_void_p()
        check(self.L.hrfd_ingest_acquire(self.h, C.byref(p)), "hrfd_ingest_acquire")
        n = self.C * self.n_blocks * self.block_bytes
        buf = (C.c_int8 * n).from_address(p.value)
        return np.frombuffer(buf, dtype=np.int8).reshape(self.C, self.n_blocks, self.block_bytes)

    def submit(self, gain_db: int = 0):
        check(self.L.hrfd_ingest_submit(self.h, int(gain_db)), "hrfd_ingest_submit")

    def collect(self):
        """(pcm [C, B, bytes/512], n_pcm [C, B], magnitude [C, B], allowed [C, B]) -- copies"""
        ps = [C.c_void_p() for _ in range(4)]
        check(self.L.hrfd_ingest_collect(self.h, *[C.byref(p) for p in ps]), "hrfd_ingest_collect")
        units = self.C * self.n_blocks
        npcm = pcm_capacity(self.block_bytes)

        def view(p, ctype, dtype, count):
            return np.frombuffer((ctype * count).from_address(p.value), dtype=dtype).copy()

        pcm = view(ps[0], C.c_int16, np.int16, units * npcm).reshape(self.C, self.n_blocks, npcm)
        n_pcm = view(ps[1], C.c_uint32, np.uint32, units).reshape(self.C, self.n_blocks)
        mag = view(ps[2], C.c_uint32, np.uint32, units).reshape(self.C, self.n_blocks)
        allowed = view(ps[3], C.c_uint8, np.uint8, units).reshape(self.C, self.n_blocks)
        return pcm, n_pcm, mag, allowed

    def replayed(self) -> int:
        n = C.c_uint64(0)
        check(self.L.hrfd_ingest_replayed(self.h, C.byref(n)), "hrfd_ingest_replayed")
        return int(n.value)


def fanout_channel_range(n_channels: int, n_shards: int, shard: int):
    """(first, count) of a shard: hrfd_fanout_channel_range (pure arithmetic, needs no GPU)"""
    L = _lib.load()
    first, count = C.c_uint32(0), C.c_uint32(0)
    check(L.hrfd_fanout_channel_range(int(n_channels), int(n_shards), int(shard), C.byref(first), C.byref(count)),
          "hrfd_fanout_channel_range")
    return int(first.value), int(count.value)


class Fanout:
    """One process, several devices: n_channels receive chains sharded over `devices` (hrfd_fanout_*)."""

    def __init__(self, n_channels: int, devices):
        self.L = _lib.load()
        self.n = int(n_channels)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        check(self.L.hrfd_fanout_create(self.n, devs, len(devices), C.byref(h)), "hrfd_fanout_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.hrfd_fanout_destroy(self.h)
            self.h = None

    __del__ = close

    def set_mode(self, mode, channel=ALL):
        check(self.L.hrfd_fanout_set_mode(self.h, channel, mode), "hrfd_fanout_set_mode")

    def set_gain(self, mode, gain, channel=ALL):
        check(self.L.hrfd_fanout_set_gain(self.h, channel, mode, C.c_float(gain)), "hrfd_fanout_set_gain")

    def set_threshold(self, threshold, channel=ALL):
        check(self.L.hrfd_fanout_set_threshold(self.h, channel, threshold), "hrfd_fanout_set_threshold")

    def scatter(self, src_device: int, d_iq_all, block_bytes: int, n_blocks: int, src_stream=None):
        check(self.L.hrfd_fanout_scatter(self.h, int(src_device), _ptr(d_iq_all), int(block_bytes), int(n_blocks),
                                         _ptr(src_stream)), "hrfd_fanout_scatter")

    def shards(self) -> int:
        n = C.c_uint32(0)
        check(self.L.hrfd_fanout_shards(self.h, C.byref(n)), "hrfd_fanout_shards")
        return int(n.value)

    def input(self, shard: int, block_bytes: int, n_blocks: int):
        """instead of scatter, for a host that feeds every device itself: (device address of the shard's input buffer
        [count][n_blocks][block_bytes], first channel, count).  Size every shard's buffer with the same block_bytes and
        n_blocks before filling any: a call that grows the buffers moves them"""
        p, first, count = C.c_void_p(), C.c_uint32(0), C.c_uint32(0)
        check(self.L.hrfd_fanout_input(self.h, int(shard), int(block_bytes), int(n_blocks), C.byref(p), C.byref(first),
                                       C.byref(count)), "hrfd_fanout_input")
        return int(p.value), int(first.value), int(count.value)

    def process(self, gain_db: int = 0):
        check(self.L.hrfd_fanout_process(self.h, int(gain_db)), "hrfd_fanout_process")

    def collect(self, dst_device: int, d_pcm_all, d_n_pcm_all=None) -> int:
        """waits, repairs, gathers; returns the number of channels that were replayed on the exact path"""
        n = C.c_uint32(0)
        check(self.L.hrfd_fanout_collect(self.h, int(dst_device), _ptr(d_pcm_all), _ptr(d_n_pcm_all), C.byref(n)),
              "hrfd_fanout_collect")
        return int(n.value)


class Mod:
    """n_channels SSB modulators / interpolateSignal cascades (hrfd_mod_*)."""

    def __init__(self, kind: int, n_channels: int = 1, device: int = -1):
        self.L = _lib.load()
        self.n = int(n_channels)
        self.kind = kind
        h = C.c_void_p()
        check(self.L.hrfd_mod_create(kind, self.n, device, C.byref(h)), "hrfd_mod_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.hrfd_mod_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self, channel=ALL):
        check(self.L.hrfd_mod_reset(self.h, channel), "hrfd_mod_reset")

    def set_sideband(self, lsb, channel=ALL):
        check(self.L.hrfd_mod_set_sideband(self.h, channel, int(bool(lsb))), "hrfd_mod_set_sideband")

    def set_modulation_index(self, index, channel=ALL):
        check(self.L.hrfd_mod_set_modulation_index(self.h, channel, float(index)), "hrfd_mod_set_modulation_index")

    def set_deviation(self, deviation_hz, channel=ALL):
        check(self.L.hrfd_mod_set_deviation(self.h, channel, float(deviation_hz)), "hrfd_mod_set_deviation")

    def set_param(self, value, channel=ALL):
        """the kind's parameter: AM modulation index / FM, WBFM deviation (mirrors tests.reflib._Mod)"""
        (self.set_modulation_index if self.kind == MOD_AM else self.set_deviation)(value, channel)

    def process(self, pcm):
        """SSB / AM / FM: int16 [C, n]; INTERP: int16 [C, 2n] IQ pairs -> int8 [C, 512 n]"""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n = pcm.shape[1] // (2 if self.kind == MOD_INTERP else 1)
        out = np.zeros((self.n, 512 * n), dtype=np.int8)
        ob = C.c_uint32(0)
        check(self.L.hrfd_mod_process(self.h, _ptr(pcm), n, _ptr(out), C.byref(ob)), "hrfd_mod_process")
        assert ob.value == 512 * n
        return out if self.n > 1 else out[0]

    def debug_set_sliced(self, mode: int):
        """test hook (WBFM): 0 = the call's passes one after the other, 1 = time slices when the phase recurrence's
        stream has CUs of its own (the default), 2 = always"""
        check(self.L.hrfd_mod_debug_set_sliced(self.h, int(mode)), "hrfd_mod_debug_set_sliced")

    def debug_set_scan(self, kind: int):
        """test hook (FM, WBFM): 1 = the phase recurrence on round 2's k_phase_scan<64> (0: k_phase_rows, the default)"""
        check(self.L.hrfd_mod_debug_set_scan(self.h, int(kind)), "hrfd_mod_debug_set_scan")

    def debug_set_tail(self, kind: int):
        """test hook (WBFM): 0 = the lookup pass and the x8 cascade as two kernels (rounds 2-5), 1 = k_wb_tail (the default)"""
        check(self.L.hrfd_mod_debug_set_tail(self.h, int(kind)), "hrfd_mod_debug_set_tail")

    def process_device(self, d_pcm, n, d_out, stream=None):
        check(self.L.hrfd_mod_process_device(self.h, _ptr(d_pcm), n, _ptr(d_out), _ptr(stream)),
              "hrfd_mod_process_device")

    def sync(self):
        check(self.L.hrfd_mod_sync(self.h), "hrfd_mod_sync")


class Play:
    """hrfd_play_*: DataProvider's cyclic .iq playback, one read position per channel, image in HBM."""

    def __init__(self, n_channels: int = 1, device: int = -1):
        self.L = _lib.load()
        self.h = C.c_void_p()
        self.C = n_channels
        check(self.L.hrfd_play_create(n_channels, device, C.byref(self.h)), "hrfd_play_create")

    def close(self):
        if self.h:
            self.L.hrfd_play_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def load_file(self, path: str):
        check(self.L.hrfd_play_load_file(self.h, path.encode()), "hrfd_play_load_file")

    def load(self, data: np.ndarray):
        data = np.ascontiguousarray(data, dtype=np.int8)
        check(self.L.hrfd_play_load(self.h, _ptr(data), data.size), "hrfd_play_load")

    def set_position(self, index: int, channel=ALL):
        check(self.L.hrfd_play_set_position(self.h, channel, index), "hrfd_play_set_position")

    def position(self, channel: int) -> int:
        v = C.c_uint32()
        check(self.L.hrfd_play_get_position(self.h, channel, C.byref(v)), "hrfd_play_get_position")
        return v.value

    def get(self, nbytes: int) -> np.ndarray:
        out = np.zeros((self.C, nbytes), dtype=np.int8)
        check(self.L.hrfd_play_get(self.h, _ptr(out), nbytes), "hrfd_play_get")
        return out

    def get_device(self, d_out, channel_stride: int, nbytes: int, stream=None):
        check(self.L.hrfd_play_get_device(self.h, d_out, channel_stride, nbytes, stream), "hrfd_play_get_device")


class Nco:
    """n_channels oscillators (hrfd_nco_*; Nco::run / Nco::runFast)."""

    def __init__(self, sample_rate: float, frequency: float, n_channels: int = 1, device: int = -1):
        self.L = _lib.load()
        self.n = int(n_channels)
        h = C.c_void_p()
        check(self.L.hrfd_nco_create(self.n, C.c_float(sample_rate), C.c_float(frequency), device, C.byref(h)),
              "hrfd_nco_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.hrfd_nco_destroy(self.h)
            self.h = None

    __del__ = close

    def set_frequency(self, f, channel=ALL):
        check(self.L.hrfd_nco_set_frequency(self.h, channel, C.c_float(f)), "hrfd_nco_set_frequency")

    def reset(self, channel=ALL):
        check(self.L.hrfd_nco_reset(self.h, channel), "hrfd_nco_reset")

    def run(self, count: int, fast: bool = False):
        i = np.zeros((self.n, count), dtype=np.float32)
        q = np.zeros((self.n, count), dtype=np.float32)
        check(self.L.hrfd_nco_run(self.h, int(fast), count, _ptr(i), _ptr(q)), "hrfd_nco_run")
        return (i, q) if self.n > 1 else (i[0], q[0])


DDC_FS_OUT = 2_048_000
DDC_STATION_SHIFT_HZ = 64_000      # the station sits 64 kHz below the channel's centre, as the reference tunes (Radio.cc:1191)


def ddc_step(offset_hz: float, decimation: int) -> int:
    """the DDC's phase step for a tone at offset_hz from the capture's centre: round(f / (R * 2.048e6) * 2^32) mod 2^32"""
    return int(round(float(offset_hz) / (int(decimation) * DDC_FS_OUT) * 2.0 ** 32)) & 0xFFFFFFFF


class _Bank:
    """What Ddc, Duc, Spectrum, Conditioner and Tones share: the handle of hrfd_<_prefix>_create and its release."""
    _prefix = ""

    def _create(self, *args):
        self.L = _lib.load()
        h = C.c_void_p()
        check(self._fn("create")(*args, C.byref(h)), f"hrfd_{self._prefix}_create")
        self.h = h

    def _fn(self, name):
        return getattr(self.L, f"hrfd_{self._prefix}_{name}")

    def _call(self, name, *args):
        check(self._fn(name)(self.h, *args), f"hrfd_{self._prefix}_{name}")

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    __del__ = close


class _PcmBank(_Bank):
    """What Tones, Audio and Resampler share beyond _Bank: their hot kernels go out through the chunked launch."""

    def debug_set_max_wgs(self, n: int):
        """test hook (needs HRFD_DEBUG_HOOKS=1): at most n workgroups per launch, 1..2^22 (the default), so that a small call
        is cut into launches the way one of more than 2^22 workgroups is"""
        self._call("debug_set_max_wgs", int(n))


class _TunedBank(_Bank):
    """The calls of Ddc and Duc that differ in the prefix only."""

    def reset(self):
        self._call("reset")

    def set_step(self, channel: int, capture: int, step: int):
        self._call("set_tuning", int(channel), int(capture), int(step) & 0xFFFFFFFF)

    def _set_filter(self, stage: int, taps):
        t = np.ascontiguousarray(taps, dtype=np.int16)
        self._call("set_filter", int(stage), t.ctypes.data_as(C.POINTER(C.c_int16)), t.size)

    def phase(self, channel: int) -> int:
        v = C.c_uint32(0)
        self._call("get_phase", int(channel), C.byref(v))
        return int(v.value)


class Ddc(_TunedBank):
    """A bank of digital down-converters (hrfd_ddc_*): n_captures wideband int8 IQ captures at decimation x 2.048 MS/s
    in, n_channels int8 IQ streams at 2.048 MS/s out, the input Rx takes."""

    _prefix = "ddc"

    def __init__(self, n_captures: int, n_channels: int, decimation: int, device: int = -1):
        self.W, self.n, self.R = int(n_captures), int(n_channels), int(decimation)
        self._create(self.W, self.n, self.R, device)

    def tune(self, channel: int, capture: int, station_offset_hz: float):
        """put the station at station_offset_hz from the capture's centre where Rx expects it (64 kHz below the
        channel's centre)"""
        f = float(station_offset_hz) + DDC_STATION_SHIFT_HZ
        if abs(f) > self.R * DDC_FS_OUT / 2:
            raise ValueError(f"station offset {station_offset_hz} Hz + 64 kHz is outside the capture's "
                             f"+-{self.R * DDC_FS_OUT // 2} Hz")
        self.set_step(channel, capture, ddc_step(f, self.R))

    def set_gain_shift(self, g: int, channel=ALL):
        check(self.L.hrfd_ddc_set_gain_shift(self.h, channel, int(g)), "hrfd_ddc_set_gain_shift")

    def set_filter(self, stage: int, taps):
        """stage 0 = A (decimating), 1 = B (channel); empty taps = bypass"""
        self._set_filter(stage, taps)

    def set_key_block(self, log2_samples: int):
        """the receive key's block: 2^log2_samples output samples per key byte, 10..17 (default 17: one rx block of 512 PCM
        samples); from the next call on"""
        self._call("set_key_block", int(log2_samples))

    def n_keys(self, out_bytes: int) -> int:
        """key bytes per channel of a call of out_bytes: ceil(out_bytes / 2 / 2^key block)"""
        v = C.c_uint32(0)
        self._call("n_keys", int(out_bytes), C.byref(v))
        return int(v.value)

    def key_skips(self, channel=ALL) -> int:
        """units (channel, tile of 1024 outputs) the keyed calls skipped since create / reset, of one channel or of the
        whole bank (ALL); waits for the last call"""
        v = C.c_uint64(0)
        self._call("get_key_skips", int(channel), C.byref(v))
        return int(v.value)

    def process(self, captures: np.ndarray, out_bytes: int, key=None) -> np.ndarray:
        """captures int8 [n_captures, decimation * out_bytes] -> int8 [n_channels, out_bytes]; blocking.  key: uint8
        [n_channels, n_keys(out_bytes)], a channel is received where its byte is non-zero and is zeros elsewhere (None:
        every channel is received)"""
        cap = np.ascontiguousarray(captures, dtype=np.int8).reshape(self.W, self.R * int(out_bytes))
        out = np.zeros((self.n, int(out_bytes)), dtype=np.int8)
        if key is None:
            check(self.L.hrfd_ddc_process(self.h, _ptr(cap), int(out_bytes), _ptr(out)), "hrfd_ddc_process")
            return out
        k = np.ascontiguousarray(key, dtype=np.uint8).reshape(self.n, self.n_keys(out_bytes))
        self._call("process_keyed", _ptr(cap), int(out_bytes), _ptr(k), _ptr(out))
        return out

    def process_device(self, d_captures, capture_stride: int, out_bytes: int, d_out, out_stride: int, stream=None,
                       d_key=None, key_stride: int = 0):
        """device pointers (ints); asynchronous on stream (None = the handle's own).  d_key: the key rows, key_stride >=
        n_keys(out_bytes) bytes apart (None: every channel is received)"""
        if d_key is None:
            check(self.L.hrfd_ddc_process_device(self.h, _ptr(d_captures), int(capture_stride), int(out_bytes),
                                                 _ptr(d_out), int(out_stride), _ptr(stream)), "hrfd_ddc_process_device")
            return
        self._call("process_device_keyed", _ptr(d_captures), int(capture_stride), int(out_bytes), _ptr(d_key), int(key_stride),
                   _ptr(d_out), int(out_stride), _ptr(stream))

    def receive(self, rx: "Rx", d_captures, capture_stride: int, block_bytes: int, n_blocks: int, d_pcm, d_n_pcm,
                d_magnitude=None, d_allowed=None, d_key=None, key_stride: int = 0) -> int:
        """the DDC, then rx's bank over its output (device pointers); returns the channels replayed exactly.  d_key as in
        process_device: the DDC runs where a channel is keyed on, rx's bank over every channel"""
        n = C.c_uint32(0)
        if d_key is None:
            check(self.L.hrfd_ddc_receive(self.h, rx.h, _ptr(d_captures), int(capture_stride), int(block_bytes),
                                          int(n_blocks), rx.gain_db, _ptr(d_pcm), _ptr(d_n_pcm), _ptr(d_magnitude),
                                          _ptr(d_allowed), C.byref(n)), "hrfd_ddc_receive")
            return int(n.value)
        self._call("receive_keyed", rx.h, _ptr(d_captures), int(capture_stride), int(block_bytes), int(n_blocks), _ptr(d_key),
                   int(key_stride), rx.gain_db, _ptr(d_pcm), _ptr(d_n_pcm), _ptr(d_magnitude), _ptr(d_allowed), C.byref(n))
        return int(n.value)


def ddc_count_key_skips(key, out_bytes: int, log2_samples: int):
    """what one keyed call of out_bytes adds to Ddc.key_skips under key block 2^log2_samples, counted on the host unit by
    unit (hrfd_ddc_count_key_skips): key uint8 [n_channels, n_keys] -> (per channel uint64 [n_channels], their sum)"""
    k = np.ascontiguousarray(key, dtype=np.uint8)
    per, total = np.zeros(k.shape[0], dtype=np.uint64), C.c_uint64(0)
    check(_lib.load().hrfd_ddc_count_key_skips(_ptr(k), k.shape[1], k.shape[0], int(out_bytes), int(log2_samples),
                                               per.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total)),
          "hrfd_ddc_count_key_skips")
    return per, int(total.value)


class RxKey:
    """The receivers' key from the spectrum bank's verdicts: key[c][b] is 1 iff channel c's band was present in one of the
    stream blocks b - hold .. b, or the channel has no band (band_of_channel[c] < 0: always on).  A block is 64 ms: one rx
    block, Ddc's default key block, one Spectrum call per block.  `present` is Spectrum's uint8 verdict per band, a torch
    tensor [n_blocks, K] ([K]: one block); any non-zero byte counts.  Blocks in front of the first call are off.  hold keeps
    a channel open behind its band's last present block: the DDC's filters delay a transmission's tail past the block in
    which the spectrum last sees it ("Listening only where someone transmits").  The carry between calls is
    a [n_channels] tensor on the input's device, so no call waits for the device."""

    _NEVER = -(1 << 40)

    def __init__(self, n_channels: int, band_of_channel, hold: int = 1):
        band = np.asarray(band_of_channel, dtype=np.int64).reshape(-1)
        if int(n_channels) < 1 or int(hold) < 0 or band.size != int(n_channels):
            raise ValueError(f"RxKey: n_channels {n_channels} >= 1, hold {hold} >= 0 and one band per channel (got {band.size})")
        self.n, self.hold = int(n_channels), int(hold)
        self._band = band
        self._on_dev = None                                # (band index clamped to 0, always-on mask) on the input's device
        self._last = None                                  # [n]: the last present block, counted from the next call's first (< 0)

    def reset(self):
        self._last = None

    def __call__(self, present):
        """present: uint8 [n_blocks, K] or [K] -> uint8 [n_channels, n_blocks]"""
        import torch
        p = present.reshape(1, -1) if present.dim() == 1 else present
        n, K = int(p.shape[0]), int(p.shape[1])
        if int(self._band.max()) >= K:
            raise ValueError(f"RxKey: band {int(self._band.max())} of a channel is not below the spectrum's {K} bands")
        if n == 0:
            return torch.zeros((self.n, 0), dtype=torch.uint8, device=p.device)
        if self._on_dev is None or self._on_dev[0].device != p.device:
            band = torch.from_numpy(self._band).to(p.device)
            self._on_dev = (torch.clamp(band, min=0), band < 0)
        if self._last is None or self._last.device != p.device:
            self._last = torch.full((self.n,), self._NEVER, dtype=torch.int64, device=p.device)
        index, always = self._on_dev
        on = (p.index_select(1, index) != 0).t() | always[:, None]     # [n_channels, n_blocks]
        at = torch.arange(n, dtype=torch.int64, device=p.device)
        # the last present block at or in front of every block, call-local (the carry's are negative)
        here = torch.where(on, at, torch.full_like(at, self._NEVER))
        last = torch.maximum(torch.cummax(here, dim=1).values, self._last[:, None])
        self._last = torch.clamp(last[:, -1] - n, min=self._NEVER)
        return ((at - last) <= self.hold).to(torch.uint8).contiguous()


def duc_step(offset_hz: float, interpolation: int) -> int:
    """the DUC's phase step that puts a channel's DC at offset_hz from the capture's centre (the same formula as
    ddc_step): round(f / (R * 2.048e6) * 2^32) mod 2^32"""
    return ddc_step(offset_hz, interpolation)


class Duc(_TunedBank):
    """A bank of digital up-converters (hrfd_duc_*): n_channels int8 IQ streams at 2.048 MS/s (what Mod writes) in,
    n_captures wideband int8 IQ captures at interpolation x 2.048 MS/s out, each the sum of the channels tuned to it."""

    _prefix = "duc"

    def __init__(self, n_captures: int, n_channels: int, interpolation: int, device: int = -1):
        self.W, self.n, self.R = int(n_captures), int(n_channels), int(interpolation)
        self._create(self.W, self.n, self.R, device)

    def tune(self, channel: int, capture: int, offset_hz: float):
        """put the channel's DC (the station, as the modulators write it) at offset_hz from the capture's centre"""
        if abs(float(offset_hz)) > self.R * DDC_FS_OUT / 2:
            raise ValueError(f"offset {offset_hz} Hz is outside the capture's +-{self.R * DDC_FS_OUT // 2} Hz")
        self.set_step(channel, capture, duc_step(offset_hz, self.R))

    def set_amplitude(self, amplitude: int, channel=ALL):
        """A = 0..32768 (32768: unity, 0: muted)"""
        check(self.L.hrfd_duc_set_amplitude(self.h, channel, int(amplitude)), "hrfd_duc_set_amplitude")

    def set_output_shift(self, s: int, capture=ALL):
        check(self.L.hrfd_duc_set_output_shift(self.h, capture, int(s)), "hrfd_duc_set_output_shift")

    def set_filter(self, stage: int, taps):
        """stage 0 = A (interpolating), 1 = B (channel); empty taps = bypass"""
        self._set_filter(stage, taps)

    def clips(self, capture: int) -> int:
        """output samples (I and Q apart) of the capture that saturated since create / reset; waits for the last call"""
        v = C.c_uint64(0)
        check(self.L.hrfd_duc_get_clips(self.h, int(capture), C.byref(v)), "hrfd_duc_get_clips")
        return int(v.value)

    def set_key_block(self, log2_samples: int):
        """the transmit key's block: 2^log2_samples channel samples per key byte, 10..17 (default 17: one block of 512 PCM
        samples); from the next call on"""
        self._call("set_key_block", int(log2_samples))

    def n_keys(self, in_bytes: int) -> int:
        """key bytes per channel of a call of in_bytes: ceil(in_bytes / 2 / 2^key block)"""
        v = C.c_uint32(0)
        self._call("n_keys", int(in_bytes), C.byref(v))
        return int(v.value)

    def key_skips(self) -> int:
        """units (channel, tile of 1024 channel samples) the keyed calls skipped since create / reset; waits for the last
        call"""
        v = C.c_uint64(0)
        self._call("get_key_skips", C.byref(v))
        return int(v.value)

    def process(self, channels: np.ndarray, in_bytes: int, key=None) -> np.ndarray:
        """channels int8 [n_channels, in_bytes] -> int8 [n_captures, interpolation * in_bytes]; blocking.  key: uint8
        [n_channels, n_keys(in_bytes)], a channel sends where its byte is non-zero (None: every channel sends)"""
        x = np.ascontiguousarray(channels, dtype=np.int8).reshape(self.n, int(in_bytes))
        out = np.zeros((self.W, self.R * int(in_bytes)), dtype=np.int8)
        if key is None:
            check(self.L.hrfd_duc_process(self.h, _ptr(x), int(in_bytes), _ptr(out)), "hrfd_duc_process")
            return out
        k = np.ascontiguousarray(key, dtype=np.uint8).reshape(self.n, self.n_keys(in_bytes))
        self._call("process_keyed", _ptr(x), int(in_bytes), _ptr(k), _ptr(out))
        return out

    def process_device(self, d_channels, channel_stride: int, in_bytes: int, d_captures, capture_stride: int,
                       stream=None, d_key=None, key_stride: int = 0):
        """device pointers (ints); asynchronous on stream (None = the handle's own).  d_key: the key rows, key_stride >=
        n_keys(in_bytes) bytes apart (None: every channel sends)"""
        if d_key is None:
            check(self.L.hrfd_duc_process_device(self.h, _ptr(d_channels), int(channel_stride), int(in_bytes),
                                                 _ptr(d_captures), int(capture_stride), _ptr(stream)),
                  "hrfd_duc_process_device")
            return
        self._call("process_device_keyed", _ptr(d_channels), int(channel_stride), int(in_bytes), _ptr(d_key), int(key_stride),
                   _ptr(d_captures), int(capture_stride), _ptr(stream))

    def transmit(self, mod: "Mod", d_pcm, n_per_channel: int, d_captures, capture_stride: int, stream=None, d_key=None,
                 key_stride: int = 0):
        """mod's bank over d_pcm, then the DUC over its output (device pointers); asynchronous on stream.  d_key as in
        process_device: the modulator runs over every channel, the DUC over those that are keyed on"""
        if d_key is None:
            check(self.L.hrfd_duc_transmit(self.h, mod.h, _ptr(d_pcm), int(n_per_channel), _ptr(d_captures),
                                           int(capture_stride), _ptr(stream)), "hrfd_duc_transmit")
            return
        self._call("transmit_keyed", mod.h, _ptr(d_pcm), int(n_per_channel), _ptr(d_key), int(key_stride), _ptr(d_captures),
                   int(capture_stride), _ptr(stream))


class TxKey:
    """The transmitters' key from what asks a channel to send: key[c][b] is 1 iff any input is on in one of the stream
    blocks b - hold .. b of channel c (a block is 64 ms: 512 PCM samples, Duc's default key block).  The inputs are the
    `active` arrays of ToneGen and AfskGen and a caller's push-to-talk array, torch uint8 tensors [n_channels, n_blocks] on
    one device, any of them None.  Blocks in front of the first call are off.  hold keeps a channel keyed behind its last
    on block: the modulator's interpolator and the DUC's channel filter delay a message's tail past the block in which its
    `active` byte ends ("Keying the transmitters").  The carry between calls is a [n_channels] tensor on
    the inputs' device, so no call waits for the device."""

    _NEVER = -(1 << 40)

    def __init__(self, n_channels: int, hold: int = 1):
        if int(n_channels) < 1 or int(hold) < 0:
            raise ValueError(f"TxKey: n_channels {n_channels} >= 1 and hold {hold} >= 0")
        self.n, self.hold = int(n_channels), int(hold)
        self._last = None                                  # [n]: the last on block, counted from the next call's first (< 0)

    def reset(self):
        self._last = None

    def __call__(self, *inputs):
        """inputs: uint8 [n_channels, n_blocks] tensors or None (at least one tensor) -> uint8 [n_channels, n_blocks]"""
        import torch
        on = None
        for a in inputs:
            if a is not None:
                b = a.reshape(self.n, -1) != 0
                on = b if on is None else on | b
        if on is None:
            raise ValueError("TxKey: at least one input must be a tensor")
        n = on.shape[1]
        if n == 0:
            return torch.zeros((self.n, 0), dtype=torch.uint8, device=on.device)
        if self._last is None or self._last.device != on.device:
            self._last = torch.full((self.n,), self._NEVER, dtype=torch.int64, device=on.device)
        at = torch.arange(n, dtype=torch.int64, device=on.device)
        # the last on block at or in front of every block, call-local (the carry's are negative)
        here = torch.where(on, at, torch.full_like(at, self._NEVER))
        last = torch.maximum(torch.cummax(here, dim=1).values, self._last[:, None])
        self._last = torch.clamp(last[:, -1] - n, min=self._NEVER)
        return ((at - last) <= self.hold).to(torch.uint8).contiguous()

SPEC_MAX_FRAMES = 65536
SPEC_MAX_THRESHOLD = 1 << 44
# Full scale of the spectrum bank, from the model (tests/spec_model.py): a tone of amplitude 127 on a bin centre under the
# default window.  The window scales it by w / 256 (mean of the Hann table: 32767 / 2), the transform divides by N, so the
# bin holds |X| = 127 * (32767 / 2) / 256 = 8127.8 and p = |X|^2 per frame, whatever N is.  0 dBFS is that power in one bin.
SPEC_FULL_SCALE_POWER = (127.0 * 32767.0 / 512.0) ** 2


def spec_bin_hz(decimation: int, log2_n: int) -> float:
    """width of one bin: R * 2 048 000 / N Hz"""
    return int(decimation) * DDC_FS_OUT / float(1 << int(log2_n))


def spec_offsets_hz(decimation: int, log2_n: int) -> np.ndarray:
    """offset from the capture's centre of every natural-order bin (k >= N / 2 are the negative offsets)"""
    n = 1 << int(log2_n)
    k = np.arange(n)
    return np.where(k < n // 2, k, k - n) * spec_bin_hz(decimation, log2_n)


def spec_dbfs(power, n_frames: int, floor_db: float = -200.0) -> np.ndarray:
    """for display: 10 log10(power per frame / SPEC_FULL_SCALE_POWER), empty bins at floor_db"""
    p = np.asarray(power, dtype=np.float64) / (float(n_frames) * SPEC_FULL_SCALE_POWER)
    return np.where(p > 0, 10 * np.log10(np.maximum(p, 1e-300)), floor_db).clip(min=floor_db)


def spec_threshold(dbfs: float, n_bins: int = 1) -> int:
    """spec_dbfs's inverse for set_band: the power per frame of n_bins bins that each stand at dbfs"""
    t = int(round(SPEC_FULL_SCALE_POWER * 10.0 ** (float(dbfs) / 10.0) * int(n_bins)))
    return min(max(t, 0), SPEC_MAX_THRESHOLD)


def find_stations(power, n_frames: int, decimation: int, log2_n: int, bandwidth_hz: float, raster_hz: float,
                  min_db_over_floor: float, floor_percentile: float = 25.0):
    """[(capture, offset_hz, band_power)] of the stations in power [W, N] (Spectrum.process): the sums of every window of
    bandwidth_hz (exact integers, circular over the bins), the floor of a capture = the floor_percentile of those sums,
    candidates = windows at least min_db_over_floor above it that are the largest within one bandwidth on either side
    (the earlier bin wins a tie), centres snapped to the raster.  Sorted by capture, then offset."""
    P = np.asarray(power, dtype=np.uint64)
    n = 1 << int(log2_n)
    P = P.reshape(-1, n)
    bin_hz = spec_bin_hz(decimation, log2_n)
    nb = min(n, max(1, int(round(float(bandwidth_hz) / bin_hz))))
    ratio = 10.0 ** (float(min_db_over_floor) / 10.0)
    found = []
    for w in range(P.shape[0]):
        row = [int(v) for v in P[w]]
        cum = [0]
        for v in row + row[:nb]:
            cum.append(cum[-1] + v)
        sums = [cum[i + nb] - cum[i] for i in range(n)]             # window starting at bin i
        floor = float(np.percentile(np.asarray(sums, dtype=np.float64), floor_percentile))
        order = sorted(range(n), key=lambda i: (-sums[i], i))
        taken = []
        for i in order:
            if not float(sums[i]) >= ratio * max(floor, 1.0):        # the one float comparison
                break
            if all(min((i - j) % n, (j - i) % n) >= nb for j in taken):
                taken.append(i)
        for i in taken:
            centre = (i + (nb - 1) / 2.0) % n
            off = (centre if centre < n / 2 else centre - n) * bin_hz
            found.append((w, float(round(off / float(raster_hz)) * float(raster_hz)), sums[i]))
    found.sort(key=lambda t: (t[0], t[1]))
    return found


def tune_from_scan(ddc: "Ddc", stations, first_channel: int = 0):
    """Ddc.tune(channel, capture, offset_hz) for every station of find_stations, channels counted from first_channel
    (tune adds the 64 kHz of Radio.cc:1191); returns {channel: (capture, offset_hz)}"""
    chan_map = {}
    for i, (capture, offset_hz, _) in enumerate(stations):
        ddc.tune(first_channel + i, capture, offset_hz)
        chan_map[first_channel + i] = (capture, offset_hz)
    return chan_map


class Spectrum(_Bank):
    """A bank of windowed integer FFTs (hrfd_spec_*): n_captures wideband int8 IQ captures at decimation x 2.048 MS/s in,
    the power of every bin of a 2^log2_n point transform summed over a call's frames out, and the verdicts of the bands."""

    _prefix = "spec"

    def __init__(self, n_captures: int, decimation: int, log2_n: int, device: int = -1):
        self.W, self.R, self.log2_n, self.N = int(n_captures), int(decimation), int(log2_n), 1 << int(log2_n)
        self._create(self.W, self.R, self.log2_n, device)

    def set_window(self, w=None):
        """N int16 values; None restores the default (Hann)"""
        if w is None:
            check(self.L.hrfd_spec_set_window(self.h, None), "hrfd_spec_set_window")
            return
        t = np.ascontiguousarray(w, dtype=np.int16)
        if t.size != self.N:
            raise ValueError(f"the window needs {self.N} entries, got {t.size}")
        check(self.L.hrfd_spec_set_window(self.h, t.ctypes.data_as(C.POINTER(C.c_int16))), "hrfd_spec_set_window")

    def set_band(self, band: int, capture: int, first_bin: int, n_bins: int, threshold: int):
        """band == n_bands appends; bins modulo N; threshold in power units per frame (spec_threshold)"""
        check(self.L.hrfd_spec_set_band(self.h, int(band), int(capture), int(first_bin), int(n_bins), int(threshold)),
              "hrfd_spec_set_band")

    def clear_bands(self):
        check(self.L.hrfd_spec_clear_bands(self.h), "hrfd_spec_clear_bands")

    @property
    def n_bands(self) -> int:
        v = C.c_uint32(0)
        check(self.L.hrfd_spec_n_bands(self.h, C.byref(v)), "hrfd_spec_n_bands")
        return int(v.value)

    def process(self, captures: np.ndarray, n_frames: int):
        """captures int8 [n_captures, 2 N n_frames] -> (power uint64 [n_captures, N], band_power uint64 [K],
        present uint8 [K]); blocking"""
        cap = np.ascontiguousarray(captures, dtype=np.int8).reshape(self.W, 2 * self.N * int(n_frames))
        k = self.n_bands
        power = np.zeros((self.W, self.N), dtype=np.uint64)
        bp, pr = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint8)
        check(self.L.hrfd_spec_process(self.h, _ptr(cap), int(n_frames), _ptr(power), _ptr(bp) if k else None,
                                       _ptr(pr) if k else None), "hrfd_spec_process")
        return power, bp, pr

    def process_device(self, d_captures, capture_stride: int, n_frames: int, d_power, d_band_power=None, d_present=None,
                       stream=None):
        """device pointers (ints); asynchronous on stream (None = the handle's own)"""
        check(self.L.hrfd_spec_process_device(self.h, _ptr(d_captures), int(capture_stride), int(n_frames), _ptr(d_power),
                                              _ptr(d_band_power), _ptr(d_present), _ptr(stream)),
              "hrfd_spec_process_device")


CAL_IDENTITY = (16384, 0, 0, 16384)
CAL_DEGENERATE = 1


def cal_sum(moments_list) -> np.ndarray:
    """the word-wise sum (modulo 2^64) of the moments of several calls: int64 [..., 8] each, all of one shape"""
    total = None
    for m in moments_list:
        u = np.ascontiguousarray(m, dtype=np.int64).view(np.uint64)
        total = u.copy() if total is None else total + u
    if total is None:
        raise ValueError("cal_sum needs at least one set of moments")
    return total.view(np.int64)


def cal_solve(moments):
    """hrfd_cal_solve over one capture's moments (int64 [8]): (dc int32 [2] in Q8, m int16 [4] in Q14, solved); solved is
    False where the moments are degenerate and m is the identity.  Host only: needs no device."""
    L = _lib.load()
    mom = np.ascontiguousarray(moments, dtype=np.int64)
    if mom.shape != (8,):
        raise ValueError(f"cal_solve takes one capture's 8 moments, got shape {mom.shape}")
    dc, m = np.zeros(2, dtype=np.int32), np.zeros(4, dtype=np.int16)
    rc = L.hrfd_cal_solve(mom.ctypes.data_as(C.POINTER(C.c_int64)), dc.ctypes.data_as(C.POINTER(C.c_int32)),
                          m.ctypes.data_as(C.POINTER(C.c_int16)))
    if rc not in (0, CAL_DEGENERATE):
        check(rc, "hrfd_cal_solve")
    return dc, m, rc == 0


class Conditioner(_Bank):
    """A bank of capture conditioners (hrfd_cal_*): n_captures int8 IQ captures in, the same captures with one Q8 offset
    taken off and one 2 x 2 Q14 matrix applied per capture out, and / or the moments of the raw input (cal_solve)."""

    _prefix = "cal"

    def __init__(self, n_captures: int, device: int = -1):
        self.W = int(n_captures)
        self._create(self.W, device)

    def set_correction(self, dc=None, m=None, capture=ALL):
        """dc: 2 values in Q8, None = (0, 0); m: (m_ii, m_iq, m_qi, m_qq) in Q14, None = the identity"""
        d = None if dc is None else np.ascontiguousarray(dc, dtype=np.int32).reshape(2)
        t = None if m is None else np.ascontiguousarray(m, dtype=np.int16).reshape(4)
        self._call("set_correction", int(capture),
                   None if d is None else d.ctypes.data_as(C.POINTER(C.c_int32)),
                   None if t is None else t.ctypes.data_as(C.POINTER(C.c_int16)))

    def correction(self, capture: int):
        """(dc int32 [2], m int16 [4]) of one capture"""
        dc, m = np.zeros(2, dtype=np.int32), np.zeros(4, dtype=np.int16)
        self._call("get_correction", int(capture), dc.ctypes.data_as(C.POINTER(C.c_int32)),
                   m.ctypes.data_as(C.POINTER(C.c_int16)))
        return dc, m

    def process(self, captures: np.ndarray, want_out: bool = True, want_moments: bool = True):
        """captures int8 [n_captures, n_bytes] -> (out int8 [n_captures, n_bytes] or None, moments int64 [n_captures, 8]
        or None); blocking"""
        cap = np.ascontiguousarray(captures, dtype=np.int8).reshape(self.W, -1)
        out = np.zeros_like(cap) if want_out else None
        mom = np.zeros((self.W, 8), dtype=np.int64) if want_moments else None
        self._call("process", _ptr(cap), cap.shape[1], _ptr(out), _ptr(mom))
        return out, mom

    def process_device(self, d_in, in_stride: int, n_bytes: int, d_out, out_stride: int, d_moments=None, stream=None):
        """device pointers (ints), d_out or d_moments may be None; asynchronous on stream (None = the handle's own)"""
        self._call("process_device", _ptr(d_in), int(in_stride), int(n_bytes), _ptr(d_out), int(out_stride),
                   _ptr(d_moments), _ptr(stream))

    def debug_set_workgroups(self, n: int):
        """test hook (HRFD_DEBUG_HOOKS=1): the workgroups a launch aims for, 2048 by default; 1 gives every capture one"""
        self._call("debug_set_workgroups", int(n))


TONE_FS = 8000
TONE_GROUPS = 4
TONE_MAX_TONES = 128
TONE_MAX_RATIO = 1 << 20
TONE_NO_BEST = 255
# the 50 CTCSS sub-tones (TIA-603 and the common extensions)
CTCSS_HZ = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
            123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
            183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)
DTMF_LOW_HZ = (697.0, 770.0, 852.0, 941.0)
DTMF_HIGH_HZ = (1209.0, 1336.0, 1477.0, 1633.0)
DTMF_KEYS = ("123A", "456B", "789C", "*0#D")


def tone_step(f_hz: float) -> int:
    """the tone bank's phase step for a tone at f_hz in 8 kS/s audio: round(f / 8000 * 2^32) mod 2^32"""
    return int(round(float(f_hz) / TONE_FS * 2.0 ** 32)) & 0xFFFFFFFF


def tone_default_window(frame_len: int) -> np.ndarray:
    """the bank's default window: round(32767 * 0.5 * (1 - cos(2 pi n / L)))"""
    n = np.arange(int(frame_len), dtype=np.float64)
    return np.floor(32767.0 * 0.5 * (1.0 - np.cos(2.0 * np.pi * n / int(frame_len))) + 0.5).astype(np.int16)


def tone_gain(window) -> float:
    """P / E of a pure tone on a tone's frequency under the window: S1^2 / (2 S2), S1 = sum w / 32768, S2 = sum (w / 32768)^2"""
    w = np.asarray(window, dtype=np.float64) / 32768.0
    return float(w.sum() ** 2 / (2.0 * (w * w).sum()))


def tone_threshold(window, fraction: float) -> int:
    """set_threshold's ratio_q8 for "the tone holds at least this fraction of the frame's energy" under the window"""
    return min(max(int(round(256.0 * float(fraction) * tone_gain(window))), 0), TONE_MAX_RATIO)


def tone_fraction(power, energy, window) -> np.ndarray:
    """the fraction of each frame's energy a tone holds: power [..., K] / (energy [...] x tone_gain), 0 for an empty frame"""
    p = np.asarray(power, dtype=np.float64)
    e = np.asarray(energy, dtype=np.float64)[..., None] * tone_gain(window)
    return np.where(e > 0, p / np.maximum(e, 1e-300), 0.0)


def dtmf_digit(low_best: int, high_best: int) -> str:
    """the key of a row (index into DTMF_LOW_HZ) and a column (index into DTMF_HIGH_HZ)"""
    return DTMF_KEYS[int(low_best)][int(high_best)]


class Tones(_PcmBank):
    """A bank of tone detectors (hrfd_tone_*): the PCM of n_channels channels as Rx / Ddc.receive write it in, per frame of
    frame_len samples the power at every tone of one shared list, the frame's energy and a verdict per tone group out."""

    _prefix = "tone"

    def __init__(self, n_channels: int, frame_len: int, device: int = -1):
        self.n, self.frame_len = int(n_channels), int(frame_len)
        self._create(self.n, self.frame_len, device)
        self.window = tone_default_window(self.frame_len)

    def set_tones(self, freqs_hz=None, groups=None, steps=None):
        """the whole list: frequencies in Hz (tone_step) or raw steps; groups 0..3 per tone, None = all 0"""
        if (freqs_hz is None) == (steps is None):
            raise ValueError("set_tones takes either freqs_hz or steps")
        s = np.ascontiguousarray([tone_step(f) for f in freqs_hz] if steps is None else
                                 [int(v) & 0xFFFFFFFF for v in steps], dtype=np.uint32)
        g = None if groups is None else np.ascontiguousarray(groups, dtype=np.uint8)
        if g is not None and g.size != s.size:
            raise ValueError(f"{s.size} tones but {g.size} groups")
        self._call("set_tones", s.ctypes.data_as(C.POINTER(C.c_uint32)),
                   None if g is None else g.ctypes.data_as(C.POINTER(C.c_uint8)), s.size)

    @property
    def n_tones(self) -> int:
        v = C.c_uint32(0)
        self._call("n_tones", C.byref(v))
        return int(v.value)

    def set_window(self, w=None):
        """frame_len int16 values in -32767..32767; None restores the default (Hann)"""
        if w is None:
            self._call("set_window", None)
            self.window = tone_default_window(self.frame_len)
            return
        t = np.ascontiguousarray(w, dtype=np.int16)
        if t.size != self.frame_len:
            raise ValueError(f"the window needs {self.frame_len} entries, got {t.size}")
        self._call("set_window", t.ctypes.data_as(C.POINTER(C.c_int16)))
        self.window = t.copy()

    def set_threshold(self, group=ALL, fraction=None, ratio_q8=None, min_energy=None):
        """present needs P_best >= (E ratio_q8) >> 8 and E >= min_energy: ratio_q8 directly, or the fraction of the frame's
        energy under the window set last (tone_threshold); defaults 16 L and 256 L"""
        if fraction is not None and ratio_q8 is not None:
            raise ValueError("set_threshold takes either fraction or ratio_q8")
        r = tone_threshold(self.window, fraction) if fraction is not None else \
            16 * self.frame_len if ratio_q8 is None else int(ratio_q8)
        e = 256 * self.frame_len if min_energy is None else int(min_energy)
        self._call("set_threshold", int(group), r, e)

    def _frames(self, n_blocks: int) -> int:
        return 512 * int(n_blocks) // self.frame_len

    def process(self, pcm: np.ndarray, n_pcm=None):
        """pcm int16 [n_channels, n_blocks, 512], n_pcm uint32 [n_channels, n_blocks] or None -> (power uint64 [C, F, K],
        energy uint64 [C, F], valid uint32 [C, F], best uint8 [C, F, 4], present uint8 [C, F, 4]); blocking"""
        x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n_blocks = x.shape[1] // 512
        if x.shape[1] != 512 * n_blocks:
            raise ValueError(f"a channel's PCM must be whole blocks of 512 samples, got {x.shape[1]} samples")
        npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32).reshape(self.n, n_blocks)
        F, K = self._frames(n_blocks), self.n_tones
        power = np.zeros((self.n, F, K), dtype=np.uint64)
        energy = np.zeros((self.n, F), dtype=np.uint64)
        valid = np.zeros((self.n, F), dtype=np.uint32)
        best = np.zeros((self.n, F, TONE_GROUPS), dtype=np.uint8)
        present = np.zeros((self.n, F, TONE_GROUPS), dtype=np.uint8)
        self._call("process", _ptr(x), _ptr(npc), n_blocks, _ptr(power), _ptr(energy), _ptr(valid), _ptr(best), _ptr(present))
        return power, energy, valid, best, present

    def process_device(self, d_pcm, channel_stride: int, d_n_pcm, n_blocks: int, d_power=None, d_energy=None, d_valid=None,
                       d_best=None, d_present=None, stream=None):
        """device pointers (ints), d_n_pcm and any output may be None (not every output); asynchronous on stream (None = the
        handle's own)"""
        self._call("process_device", _ptr(d_pcm), int(channel_stride), _ptr(d_n_pcm), int(n_blocks), _ptr(d_power),
                   _ptr(d_energy), _ptr(d_valid), _ptr(d_best), _ptr(d_present), _ptr(stream))


AUDIO_MAX_BUSES = 64
AUDIO_MAX_TAPS = 512
AUDIO_MAX_LIST = 4096
AUDIO_ANY_TONE = 254
AUDIO_NO_TONE = 255
AUDIO_UNITY_GAIN = 4096            # a bus gain of 1.0 (Q12)


def audio_highpass_taps(T: int = 511, cutoff_hz: float = 300.0) -> np.ndarray:
    """T odd int16 taps in Q14 for Audio.set_taps that take the sub-audible tones out of the voice band: a sinc low-pass at
    cutoff_hz under np.blackman, normalised to unity at DC, subtracted from a unit impulse at the centre (spectral
    inversion), round(h * 16384).  A design aid on the host, not part of the bank's exact contract."""
    T = int(T)
    if T < 3 or T > AUDIO_MAX_TAPS or T % 2 == 0:
        raise ValueError(f"spectral inversion needs an odd tap count in 3..{AUDIO_MAX_TAPS - 1}, got {T}")
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2
    low = np.sinc(2.0 * float(cutoff_hz) / TONE_FS * n) * np.blackman(T)
    low /= low.sum()
    h = -low
    h[(T - 1) // 2] += 1.0
    return np.floor(h * 16384.0 + 0.5).astype(np.int16)


class Audio(_PcmBank):
    """The audio bank (hrfd_audio_*): the PCM of n_channels channels as Rx / Ddc.receive write it in; every channel's audio
    behind one voice filter and a click-free per-block gate, and n_buses monitor mixes of it out.  gate / gate_device turn
    the verdicts of Tones into the gate (tone squelch)."""

    _prefix = "audio"

    def __init__(self, n_channels: int, n_buses: int = 1, device: int = -1):
        self.n, self.m = int(n_channels), int(n_buses)
        self._create(self.n, self.m, device)

    def set_taps(self, taps):
        """1..512 int16 taps in Q14 with sum |h| <= 65535, one list for every channel; zeroes every channel's history and
        gate"""
        t = np.ascontiguousarray(taps, dtype=np.int16).ravel()
        self._call("set_taps", t.ctypes.data_as(C.POINTER(C.c_int16)), t.size)

    def set_bus(self, bus: int, channels=(), gains=()):
        """the whole list of one bus: channels and their gains, int16 in Q12 (AUDIO_UNITY_GAIN = 1.0), -32767..32767; empty
        lists clear the bus"""
        ch = np.ascontiguousarray(channels, dtype=np.uint32).ravel()
        g = np.ascontiguousarray(gains).ravel()
        if g.size and (g.min() < -32768 or g.max() > 32767):
            raise ValueError("a bus gain must fit int16")
        g = g.astype(np.int16)
        if g.size != ch.size:
            raise ValueError(f"{ch.size} channels but {g.size} gains")
        self._call("set_bus", int(bus), ch.ctypes.data_as(C.POINTER(C.c_uint32)), g.ctypes.data_as(C.POINTER(C.c_int16)), ch.size)

    def set_want(self, want: int, channel: int = ALL):
        """the tone that opens a channel's squelch: an index into the Tones list, AUDIO_ANY_TONE, or AUDIO_NO_TONE (always
        open, the default)"""
        self._call("set_want", int(channel), int(want))

    def reset(self, channel: int = ALL):
        """zero the filter history and the gate of one channel, or of all"""
        self._call("reset", int(channel))

    def gate(self, best, present, frame_len: int, group: int) -> np.ndarray:
        """best, present uint8 [n_channels, F, 4] as Tones.process returns them -> open uint8 [n_channels, n_blocks];
        blocking"""
        b = np.ascontiguousarray(best, dtype=np.uint8).reshape(self.n, -1, TONE_GROUPS)
        p = np.ascontiguousarray(present, dtype=np.uint8).reshape(self.n, -1, TONE_GROUPS)
        if b.shape != p.shape:
            raise ValueError(f"best {b.shape} and present {p.shape} differ")
        n_blocks, rest = divmod(b.shape[1] * int(frame_len), 512)
        if rest:
            raise ValueError(f"{b.shape[1]} frames of {frame_len} samples are no whole number of blocks")
        out = np.zeros((self.n, n_blocks), dtype=np.uint8)
        self._call("gate", _ptr(b), _ptr(p), int(frame_len), int(group), n_blocks, _ptr(out))
        return out

    def gate_device(self, d_best, d_present, frame_len: int, group: int, n_blocks: int, d_open, stream=None):
        """device pointers (ints); asynchronous on stream (None = the handle's own)"""
        self._call("gate_device", _ptr(d_best), _ptr(d_present), int(frame_len), int(group), int(n_blocks), _ptr(d_open),
                   _ptr(stream))

    def process(self, pcm: np.ndarray, n_pcm=None, open=None, want_out: bool = True, want_mix: bool = True):
        """pcm int16 [n_channels, n_blocks, 512], n_pcm uint32 and open uint8 [n_channels, n_blocks] or None -> (out int16
        [n_channels, n_blocks, 512] or None, mix int16 [n_buses, n_blocks, 512] or None, clips uint32 [n_buses] or None);
        blocking"""
        x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n_blocks = x.shape[1] // 512
        if x.shape[1] != 512 * n_blocks:
            raise ValueError(f"a channel's PCM must be whole blocks of 512 samples, got {x.shape[1]} samples")
        npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32).reshape(self.n, n_blocks)
        op = None if open is None else np.ascontiguousarray(open, dtype=np.uint8).reshape(self.n, n_blocks)
        out = np.zeros((self.n, n_blocks, 512), dtype=np.int16) if want_out else None
        mix = np.zeros((self.m, n_blocks, 512), dtype=np.int16) if want_mix else None
        clips = np.zeros(self.m, dtype=np.uint32) if want_mix else None
        self._call("process", _ptr(x), _ptr(npc), _ptr(op), n_blocks, _ptr(out), _ptr(mix), _ptr(clips))
        return out, mix, clips

    def process_device(self, d_pcm, channel_stride: int, d_n_pcm, d_open, n_blocks: int, d_out=None, out_stride: int = 0,
                       d_mix=None, d_clips=None, stream=None):
        """device pointers (ints); d_n_pcm, d_open and any output may be None (not both d_out and d_mix); out_stride 0 =
        dense rows; asynchronous on stream (None = the handle's own)"""
        self._call("process_device", _ptr(d_pcm), int(channel_stride), _ptr(d_n_pcm), _ptr(d_open), int(n_blocks), _ptr(d_out),
                   int(out_stride) if out_stride else 1024 * int(n_blocks), _ptr(d_mix), _ptr(d_clips), _ptr(stream))


RESAMP_MAX_RATIO = 512
RESAMP_MAX_TAPS = 16384
RESAMP_MAX_BRANCH = 512
RESAMP_MAX_IN = 524288


def resample_taps(up: int, down: int, taps_per_branch: int, atten_db: float = None) -> np.ndarray:
    """int16 taps in Q14 for Resampler(…, up, down).set_taps: a Kaiser-windowed sinc at the prototype rate (up times the
    input rate), cut off at half the lower of the two rates, DC gain `up`, round(h * 16384), of odd length T = up *
    taps_per_branch (less one where that is even).  With 8 kS/s as the lower rate the transition band runs from 3.4 to
    4.6 kHz: atten_db, the Kaiser window's stop-band attenuation, defaults to what the length gives over that band,
    between 60 and 80 dB (more says nothing behind the rounding to Q14).  A design aid on the host, not part of the bank's
    exact contract."""
    L, M, K = int(up), int(down), int(taps_per_branch)
    if not (1 <= L <= RESAMP_MAX_RATIO and 1 <= M <= RESAMP_MAX_RATIO and 1 <= K <= RESAMP_MAX_BRANCH):
        raise ValueError(f"up, down and taps_per_branch must be 1..512, got {L}, {M}, {K}")
    T = L * K - (1 - (L * K) % 2)
    if T < 3 or T > RESAMP_MAX_TAPS:
        raise ValueError(f"{L} x {K} taps give a length of {T}: need 3..{RESAMP_MAX_TAPS}")
    low = max(L, M)                                        # the prototype rate in units of the lower rate
    width = 2.0 * np.pi * (4600.0 - 3400.0) / TONE_FS / low        # the transition band in radians per prototype sample
    if atten_db is None:
        atten_db = min(80.0, max(60.0, 8.0 + 2.285 * width * (T - 1)))
    a = float(atten_db)
    beta = 0.1102 * (a - 8.7) if a > 50.0 else (0.5842 * (a - 21.0) ** 0.4 + 0.07886 * (a - 21.0) if a > 21.0 else 0.0)
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2
    h = np.sinc(n / low) * np.kaiser(T, beta)
    h *= L / h.sum()
    return np.floor(h * 16384.0 + 0.5).astype(np.int16)


class Resampler(_PcmBank):
    """The resampler bank (hrfd_resamp_*): the PCM of n_channels channels at up / down times its rate, the same rational
    polyphase filter for every channel: 8 kS/s to a sound card's 48 kS/s with (6, 1), a microphone's 48 kS/s to the
    modulators' 8 kS/s with (1, 6), 44.1 kS/s with (441, 80) and (80, 441).  Exact in integers and independent of how a stream
    is cut into calls; a handle other than (1, 1) needs set_taps before its first call (resample_taps designs them)."""

    _prefix = "resamp"

    def __init__(self, n_channels: int, up: int, down: int, device: int = -1):
        self.n, self.up, self.down = int(n_channels), int(up), int(down)
        self._create(self.n, self.up, self.down, device)

    def set_taps(self, taps):
        """1..16384 int16 taps in Q14 at up times the input rate, at most 512 per branch and sum |h| <= 65535 over every
        branch; zeroes every channel's history and the handle's phase"""
        t = np.ascontiguousarray(taps, dtype=np.int16).ravel()
        self._call("set_taps", t.ctypes.data_as(C.POINTER(C.c_int16)), t.size)

    def reset(self, channel: int = ALL):
        """zero the history of one channel, or the histories of all and the handle's phase"""
        self._call("reset", int(channel))

    def out_count(self, n_in: int) -> int:
        """the outputs per channel the next call gives if it takes n_in samples"""
        v = C.c_uint32(0)
        self._call("out_count", int(n_in), C.byref(v))
        return int(v.value)

    def process(self, pcm: np.ndarray, n_pcm=None) -> np.ndarray:
        """pcm int16 [n_channels, n_in], n_pcm uint32 [n_channels, n_in / 512] or None -> out int16 [n_channels, n_out];
        blocking"""
        x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n_in = x.shape[1]
        npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32).reshape(self.n, -1)
        if npc is not None and npc.shape[1] * 512 != n_in:
            raise ValueError(f"n_pcm needs whole blocks of 512 samples and one entry per block, got {n_in} samples, {npc.shape[1]} entries")
        cap = max(1, self.out_count(n_in))                 # (a call may give no output; an empty array has no address to pass)
        out = np.zeros((self.n, cap), dtype=np.int16)
        v = C.c_uint32(0)
        self._call("process", _ptr(x), _ptr(npc), n_in, _ptr(out), cap, C.byref(v))
        return np.ascontiguousarray(out[:, :v.value])

    def process_device(self, d_pcm, channel_stride: int, d_n_pcm, n_in: int, d_out, out_stride: int, out_capacity: int,
                       stream=None) -> int:
        """device pointers (ints); d_n_pcm may be None; rows of d_out take out_capacity samples and lie out_stride bytes
        apart (0 = dense at out_capacity); asynchronous on stream (None = the handle's own).  Returns n_out, the samples
        written per row"""
        v = C.c_uint32(0)
        self._call("process_device", _ptr(d_pcm), int(channel_stride), _ptr(d_n_pcm), int(n_in), _ptr(d_out),
                   int(out_stride) if out_stride else 2 * int(out_capacity), int(out_capacity), C.byref(v), _ptr(stream))
        return int(v.value)


LEVEL_FRAME = 64
LEVEL_MAX_WEIGHTS = 64
LEVEL_MAX_BLOCKS = 1024
LEVEL_UNITY = 32768                # w[0], and the largest weight
LEVEL_FRAME_MS = 1000.0 * LEVEL_FRAME / TONE_FS


def level_weights(hang_ms: float, release_ms: float, W: int = LEVEL_MAX_WEIGHTS) -> np.ndarray:
    """W uint16 release weights in Q15 for Leveler.set_weights, one per frame of 8 ms: entry k weighs the peak of the frame
    that lies 8 k ms back.  32768 while 8 k <= hang_ms, then 32768 exp(-(8 k - hang_ms) / release_ms), rounded; w[0] is
    32768 whatever the arguments say.  A design aid on the host, not part of the bank's exact contract."""
    W = int(W)
    if W < 1 or W > LEVEL_MAX_WEIGHTS:
        raise ValueError(f"W must be 1..{LEVEL_MAX_WEIGHTS}, got {W}")
    if not (hang_ms >= 0.0 and release_ms > 0.0):
        raise ValueError(f"need hang_ms >= 0 and release_ms > 0, got {hang_ms}, {release_ms}")
    t = np.maximum(np.arange(W, dtype=np.float64) * LEVEL_FRAME_MS - float(hang_ms), 0.0)
    w = np.floor(LEVEL_UNITY * np.exp(-t / float(release_ms)) + 0.5).astype(np.uint16)
    w[0] = LEVEL_UNITY
    return w


class Leveler(_Bank):
    """The level bank (hrfd_level_*): the PCM of n_channels channels as Rx / Ddc.receive write it in, the same audio at an even
    loudness out: a per-channel automatic gain control with a peak detector per frame of 64 samples, a table of release
    weights (hang, then decay) and a gain that attacks at the frame boundary and releases in a ramp.  Exact in integers,
    |out| <= target always, independent of how a stream is cut into calls.  (Its kernel is one launch of one workgroup per
    channel, so unlike Tones, Audio and Resampler it has no chunked launch and no debug_set_max_wgs.)"""

    _prefix = "level"

    def __init__(self, n_channels: int, device: int = -1):
        self.n = int(n_channels)
        self._create(self.n, device)

    def set_weights(self, w):
        """1..64 uint16 release weights in Q15, w[0] = 32768 and none above it, one table for every channel
        (level_weights designs one); keeps the peaks"""
        a = np.ascontiguousarray(w).ravel()
        if a.size and (a.min() < 0 or a.max() > 65535):
            raise ValueError("a weight must fit uint16")
        a = a.astype(np.uint16)
        self._call("set_weights", a.ctypes.data_as(C.POINTER(C.c_uint16)), a.size)

    def set(self, target: int, floor: int, channel: int = ALL):
        """the level the loudest sample of a frame is brought to (0..32767) and the envelope below which the gain stops
        rising (16..32768: the largest gain is target / floor), of one channel or of all; keeps the peaks"""
        self._call("set", int(channel), int(target), int(floor))

    def set_bypass(self, on: bool, channel: int = ALL):
        """pass one channel, or all, through unchanged; gain and peak are still reported"""
        self._call("set_bypass", int(channel), 1 if on else 0)

    def reset(self, channel: int = ALL):
        """zero the peaks of one channel, or of all"""
        self._call("reset", int(channel))

    def process(self, pcm: np.ndarray, n_pcm=None, want_out: bool = True, want_gain: bool = True, want_peak: bool = True):
        """pcm int16 [n_channels, n_blocks, 512], n_pcm uint32 [n_channels, n_blocks] or None -> (out int16 [n_channels,
        n_blocks, 512] or None, gain uint32 [n_channels, 8 n_blocks] or None, peak uint16 [n_channels, 8 n_blocks] or None);
        blocking"""
        x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n_blocks = x.shape[1] // 512
        if x.shape[1] != 512 * n_blocks:
            raise ValueError(f"a channel's PCM must be whole blocks of 512 samples, got {x.shape[1]} samples")
        npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32).reshape(self.n, n_blocks)
        out = np.zeros((self.n, n_blocks, 512), dtype=np.int16) if want_out else None
        gain = np.zeros((self.n, 8 * n_blocks), dtype=np.uint32) if want_gain else None
        peak = np.zeros((self.n, 8 * n_blocks), dtype=np.uint16) if want_peak else None
        self._call("process", _ptr(x), _ptr(npc), n_blocks, _ptr(out), _ptr(gain), _ptr(peak))
        return out, gain, peak

    def process_device(self, d_pcm, channel_stride: int, d_n_pcm, n_blocks: int, d_out=None, out_stride: int = 0, d_gain=None,
                       d_peak=None, stream=None):
        """device pointers (ints); d_n_pcm and any output may be None (not all three outputs); out_stride 0 = the input's
        stride where d_out is d_pcm (in place), dense rows otherwise; asynchronous on stream (None = the handle's own)"""
        if not out_stride:
            in_place = d_out is not None and _ptr(d_out).value == _ptr(d_pcm).value
            out_stride = int(channel_stride) if in_place else 1024 * int(n_blocks)
        self._call("process_device", _ptr(d_pcm), int(channel_stride), _ptr(d_n_pcm), int(n_blocks), _ptr(d_out), int(out_stride),
                   _ptr(d_gain), _ptr(d_peak), _ptr(stream))


DCS_MAX_TAPS = 512
DCS_MAX_CODES = 128
DCS_MAX_BLOCKS = 1024
DCS_NO_BEST = 255                  # best of a group without entries
DCS_WORD_BITS = 23
DCS_GENERATOR = 0xC75              # the (23,12) Golay code's g, bit i = x^i
DCS_BIT_NUM, DCS_BIT_DEN = 1250, 21        # samples per bit: 8000 / 134.4


def dcs_word(code: int, inverted: bool = False) -> int:
    """the 23-bit word of a DCS code (three octal digits, 0..0o777): (p << 12) | 0x800 | code with p the remainder of
    (0x800 | code) x^11 modulo DCS_GENERATOR; the complement in 23 bits where inverted.  dcs_word(0o023) == 0x763813"""
    code = int(code)
    if not 0 <= code <= 0o777:
        raise ValueError(f"a DCS code has three octal digits (0..0o777), got {code}")
    data = 0x800 | code
    p = data << 11
    for i in range(22, 10, -1):
        if p >> i & 1:
            p ^= DCS_GENERATOR << (i - 11)
    w = p << 12 | data
    return w ^ 0x7FFFFF if inverted else w


def dcs_canonical(word: int) -> int:
    """the least of the 23 rotations of a word: what the bank compares, since every sample phase sees a rotation"""
    w = int(word) & 0x7FFFFF
    return min(((w >> r) | (w << (23 - r))) & 0x7FFFFF for r in range(23))


def dcs_aliases(code: int):
    """(same, inverse): the codes a receiver cannot tell from `code`, itself among them, and the codes whose inverted form
    it cannot tell from it.  dcs_aliases(0o023) == ([0o023, 0o340, 0o766], [0o047, 0o375, 0o707]).  A list for Dcs.set_codes
    may hold one of the six only"""
    c = dcs_canonical(dcs_word(code))
    return ([k for k in range(512) if dcs_canonical(dcs_word(k)) == c],
            [k for k in range(512) if dcs_canonical(dcs_word(k, True)) == c])


def dcs_lowpass_taps(T: int = 255, cutoff_hz: float = 300.0) -> np.ndarray:
    """T int16 taps in Q14 for Dcs.set_taps that keep the sub-audible band and take the voice out: a sinc low-pass at
    cutoff_hz under np.blackman, normalised to unity at DC, round(h * 16384).  A design aid on the host like
    audio_highpass_taps, not part of the bank's exact contract."""
    T = int(T)
    if T < 1 or T > DCS_MAX_TAPS:
        raise ValueError(f"T must be 1..{DCS_MAX_TAPS}, got {T}")
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2
    low = np.sinc(2.0 * float(cutoff_hz) / TONE_FS * n) * (np.blackman(T) if T > 2 else np.ones(T))
    low /= low.sum()
    return np.floor(low * 16384.0 + 0.5).astype(np.int16)


def dcs_levels(code: int, n: int, amplitude: int, t0: int = 0, inverted: bool = False) -> np.ndarray:
    """n int16 samples of a DCS code as it is sent, from stream time t0 on: +amplitude where bit floor(21 t / 1250) mod 23
    of the word is 1, -amplitude where it is 0 (bit 0 goes first, 134.4 bit/s).  The host restatement of the DcsGen bank's law
    under its default tap: what DcsGen writes for the code, generate only, at the stream times t0 .. t0 + n - 1 (21 t must fit
    int64 here).  DcsGen is the transmit side; this is for tests and for a host that has no device at hand."""
    a = int(amplitude)
    if not 0 <= a <= 32767:
        raise ValueError(f"amplitude must be 0..32767, got {a}")
    w = dcs_word(code, inverted)
    t = np.arange(int(t0), int(t0) + int(n), dtype=np.int64)
    bit = (w >> ((t * DCS_BIT_DEN // DCS_BIT_NUM) % DCS_WORD_BITS)) & 1
    return np.where(bit == 1, a, -a).astype(np.int16)


class Dcs(_Bank):
    """The DCS bank (hrfd_dcs_*): the PCM of n_channels channels as Rx / Ddc.receive write it in; per block, how many samples
    end a 23-bit word of each listed code (hits) and the tone bank's kind of verdict over them (best, present), which
    Audio.gate / Audio.gate_device take unchanged at frame_len = 512.  No clock recovery: a word is 23 slicer bits on a
    fixed grid behind a sample.  Exact in integers, independent of how a stream is cut into calls.  (One launch of one
    workgroup per channel, like Leveler: no chunked launch and no debug_set_max_wgs.)"""

    _prefix = "dcs"

    def __init__(self, n_channels: int, device: int = -1):
        self.n = int(n_channels)
        self._create(self.n, device)

    def set_taps(self, taps):
        """1..512 int16 taps in Q14 with sum |h| <= 65535, one list for every channel (dcs_lowpass_taps designs one); zeroes
        every channel's state"""
        t = np.ascontiguousarray(taps, dtype=np.int16).ravel()
        self._call("set_taps", _ptr(t), t.size)

    def set_codes(self, codes, inverted=None, groups=None):
        """the whole list, 0..128 entries: codes 0..0o777, inverted (bools) and groups (0..3) per entry or None; two aliases in
        one list are refused.  Keeps the channels' state"""
        c = np.ascontiguousarray(codes).ravel()
        if c.size and (c.min() < 0 or c.max() > 65535):
            raise ValueError("a code must fit uint16")
        c = c.astype(np.uint16)
        inv = None if inverted is None else np.ascontiguousarray(inverted).ravel().astype(bool).astype(np.uint8)
        grp = None if groups is None else np.ascontiguousarray(groups).ravel()
        if grp is not None:
            if grp.size and (grp.min() < 0 or grp.max() > 255):
                raise ValueError("a group must fit uint8")
            grp = grp.astype(np.uint8)
        for name, a in (("inverted", inv), ("groups", grp)):
            if a is not None and a.size != c.size:
                raise ValueError(f"{c.size} codes but {a.size} {name}")
        self._call("set_codes", _ptr(c), _ptr(inv), _ptr(grp), c.size)

    def n_codes(self) -> int:
        v = C.c_uint32(0)
        self._call("n_codes", C.byref(v))
        return int(v.value)

    def set_min_hits(self, group: int = ALL, n: int = 128):
        """the samples of a block of 512 that must match a group's best entry for it to be present, 1..512, of one group
        or of all"""
        self._call("set_min_hits", int(group), int(n))

    def reset(self, channel: int = ALL):
        """zero the state of one channel, or of all"""
        self._call("reset", int(channel))

    def process(self, pcm: np.ndarray, n_pcm=None):
        """pcm int16 [n_channels, n_blocks, 512], n_pcm uint32 [n_channels, n_blocks] or None -> (hits uint16 [n_channels,
        n_blocks, K], best uint8 [n_channels, n_blocks, 4], present uint8 [n_channels, n_blocks, 4]); blocking"""
        x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n_blocks = x.shape[1] // 512
        if x.shape[1] != 512 * n_blocks:
            raise ValueError(f"a channel's PCM must be whole blocks of 512 samples, got {x.shape[1]} samples")
        npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32).reshape(self.n, n_blocks)
        hits = np.zeros((self.n, n_blocks, self.n_codes()), dtype=np.uint16)
        best = np.zeros((self.n, n_blocks, TONE_GROUPS), dtype=np.uint8)
        present = np.zeros((self.n, n_blocks, TONE_GROUPS), dtype=np.uint8)
        self._call("process", _ptr(x), _ptr(npc), n_blocks, _ptr(hits) if hits.size else None, _ptr(best), _ptr(present))
        return hits, best, present

    def process_device(self, d_pcm, channel_stride: int, d_n_pcm, n_blocks: int, d_hits=None, d_best=None, d_present=None,
                       stream=None):
        """device pointers (ints); d_n_pcm and any output may be None (not all three outputs); d_hits takes uint16
        [n_channels, n_blocks, K], d_best and d_present uint8 [n_channels, n_blocks, 4], all dense; asynchronous on stream
        (None = the handle's own)"""
        self._call("process_device", _ptr(d_pcm), int(channel_stride), _ptr(d_n_pcm), int(n_blocks), _ptr(d_hits), _ptr(d_best),
                   _ptr(d_present), _ptr(stream))


TONEGEN_TRACKS = 2
TONEGEN_MAX_SEGMENTS = 32
TONEGEN_MAX_BLOCKS = 1024
TONEGEN_FOREVER = 0xFFFFFFFF
TONEGEN_APPEND = 0xFFFFFFFFFFFFFFFF
TONEGEN_RAMP = 64


def tonegen_samples(ms: float) -> int:
    """milliseconds at 8 kS/s in samples, rounded"""
    return int(round(float(ms) * TONE_FS / 1000.0))


def tonegen_segment(length: int, hz_a: float = 0.0, amp_a: int = 0, hz_b: float = 0.0, amp_b: int = 0, gap: int = 0):
    """one segment for ToneGen.queue: (gap, length, step_a, step_b, amp_a, amp_b) with the steps of tone_step"""
    return (int(gap), int(length), tone_step(hz_a), tone_step(hz_b), int(amp_a), int(amp_b))


def tonegen_dtmf(key: str):
    """(row Hz, column Hz) of a DTMF key"""
    for r, row in enumerate(DTMF_KEYS):
        if key in row and len(key) == 1:
            return DTMF_LOW_HZ[r], DTMF_HIGH_HZ[row.index(key)]
    raise ValueError(f"{key!r} is no DTMF key (one of {''.join(DTMF_KEYS)})")


def _tonegen_segs(segs) -> np.ndarray:
    try:
        rows = [[int(v) for v in s] for s in segs]
    except TypeError:
        raise ValueError("segments are sequences of six integers (gap, length, step_a, step_b, amp_a, amp_b)")
    if any(len(r) != 6 for r in rows) or any(v < 0 or v > 0xFFFFFFFF for r in rows for v in r):
        raise ValueError("a segment is six values that fit uint32: gap, length, step_a, step_b, amp_a, amp_b")
    return np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 6)


class _GenBank(_Bank):
    """What ToneGen, AfskGen and DcsGen share beyond _Bank: the clock, the clip counters and the process calls of a generator on
    transmit PCM.  _max_blocks is the bank's limit on the blocks of a call."""
    _max_blocks = 0

    def reset(self):
        """empty every queue, time = 0, clips = 0"""
        self._call("reset")

    def time(self) -> int:
        """the stream time of the next call's first sample"""
        v = C.c_uint64(0)
        self._call("time", C.byref(v))
        return int(v.value)

    def clips(self, channel: int) -> int:
        """samples of the channel the saturation changed, since create or reset; blocking"""
        v = C.c_uint64(0)
        self._call("get_clips", int(channel), C.byref(v))
        return int(v.value)

    def process(self, pcm, n_blocks: int = None, want_active: bool = False):
        """pcm int16 [n_channels, n_blocks, 512], or None with n_blocks (generate only) -> out int16 [n_channels, n_blocks,
        512], or (out, active uint8 [n_channels, n_blocks]) with want_active; blocking"""
        x = None
        if pcm is not None:
            x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
            if x.shape[1] % 512 != 0 or (n_blocks is not None and x.shape[1] != 512 * int(n_blocks)):
                raise ValueError(f"a channel's PCM must be whole blocks of 512 samples, got {x.shape[1]} samples")
            n_blocks = x.shape[1] // 512
        elif n_blocks is None:
            raise ValueError("generate only needs n_blocks")
        n_blocks = int(n_blocks)
        if n_blocks < 0 or n_blocks > 0xFFFFFFFF:
            raise ValueError(f"n_blocks {n_blocks}")
        out = np.zeros((self.n, min(n_blocks, self._max_blocks), 512), dtype=np.int16)
        active = np.zeros((self.n, min(n_blocks, self._max_blocks)), dtype=np.uint8) if want_active else None
        self._call("process", _ptr(x), n_blocks, _ptr(out), _ptr(active))
        return (out, active) if want_active else out

    def process_device(self, d_pcm, channel_stride: int, n_blocks: int, d_out, out_stride: int = 0, d_active=None, stream=None):
        """device pointers (ints); d_pcm None = generate only, d_active may be None; out_stride 0 = the input's stride where
        d_out is d_pcm (in place), dense rows otherwise; asynchronous on stream (None = the handle's own)"""
        if not out_stride:
            in_place = d_pcm is not None and d_out is not None and _ptr(d_out).value == _ptr(d_pcm).value
            out_stride = int(channel_stride) if in_place else 1024 * int(n_blocks)
        self._call("process_device", _ptr(d_pcm), int(channel_stride), int(n_blocks), _ptr(d_out), int(out_stride), _ptr(d_active),
                   _ptr(stream))


class ToneGen(_GenBank):
    """The tone generator bank (hrfd_tonegen_*): signalling on the PCM of n_channels transmit channels, the mirror of Tones.
    Segments of one or two sines with a ramp of 8 ms at either end are queued on two tracks per channel at absolute stream
    times and added, saturating, to the rows Mod and Duc.transmit read: DTMF digits, CTCSS sub-tones, tone bursts, paging
    sequences.  Exact in integers on the detector's phase grid, and independent of how a stream is cut into calls.  (Its
    kernel is one launch of at most 2^22 workgroups, so it has no chunked launch and no debug_set_max_wgs.)"""

    _prefix = "tonegen"
    _max_blocks = TONEGEN_MAX_BLOCKS

    def __init__(self, n_channels: int, device: int = -1):
        self.n = int(n_channels)
        self._create(self.n, device)

    def queue(self, channel: int, track: int, segs, start: int = TONEGEN_APPEND):
        """1..32 segments (gap, length, step_a, step_b, amp_a, amp_b; tonegen_segment makes one) on one track of one channel
        or of all (ALL): the first begins at start + its gap, each next one its gap behind the end of the one before; start
        TONEGEN_APPEND = max(time, the end of the track's last segment).  Refused whole if anything is out of order."""
        a = _tonegen_segs(segs)
        self._call("queue", int(channel), int(track), _ptr(a), a.shape[0], int(start))

    def cut(self, channel: int = ALL, track: int = 0):
        """ramp the segment in progress down over the next 64 samples and drop those not yet begun"""
        self._call("cut", int(channel), int(track))

    def set_time(self, N: int):
        """move the clock only; the queues stay"""
        self._call("set_time", int(N))

    def pending(self, channel: int, track: int = 0):
        """(segments of the track that have not ended, the end of the last of them: the time itself where there is none,
        2^64 - 1 behind a FOREVER segment)"""
        n, end = C.c_uint32(0), C.c_uint64(0)
        self._call("pending", int(channel), int(track), C.byref(n), C.byref(end))
        return int(n.value), int(end.value)

    # ---- what the segments are for
    def dial(self, channel: int, keys: str, on_ms: float = 96, off_ms: float = 32, amplitude: int = 8000, track: int = 0,
             start: int = TONEGEN_APPEND):
        """DTMF: every key of `keys` (at most 32 with what the track still holds) for on_ms behind a pause of off_ms, row
        and column at the same amplitude"""
        on, off = tonegen_samples(on_ms), tonegen_samples(off_ms)
        segs = []
        for key in keys:
            lo, hi = tonegen_dtmf(key)
            segs.append(tonegen_segment(on, lo, amplitude, hi, amplitude, gap=off))
        self.queue(channel, track, segs, start)

    def ctcss(self, channel: int, hz: float, amplitude: int = 1000, track: int = 1, start: int = TONEGEN_APPEND):
        """a sub-tone without an end (cut(channel, track) ramps it down)"""
        self.queue(channel, track, [tonegen_segment(TONEGEN_FOREVER, hz, amplitude)], start)

    def burst(self, channel: int, hz: float = 1750.0, ms: float = 500, amplitude: int = 8000, track: int = 0,
              start: int = TONEGEN_APPEND):
        """one tone for ms milliseconds: the 1750 Hz burst that opens a repeater"""
        self.queue(channel, track, [tonegen_segment(tonegen_samples(ms), hz, amplitude)], start)

    def tones(self, channel: int, hz_list, ms_each: float, amplitude: int = 8000, track: int = 0, gap_ms: float = 0,
              start: int = TONEGEN_APPEND):
        """sequential tones for paging and selcall, ms_each each, gap_ms of silence between; the caller brings the table"""
        n, gap = tonegen_samples(ms_each), tonegen_samples(gap_ms)
        segs = [tonegen_segment(n, hz, amplitude, gap=gap if i else 0) for i, hz in enumerate(hz_list)]
        self.queue(channel, track, segs, start)


DCSGEN_MAX_SEGMENTS = 8
DCSGEN_MAX_BLOCKS = 1024
DCSGEN_MAX_TAPS = 512
DCSGEN_FOREVER = 0xFFFFFFFF
DCSGEN_APPEND = 0xFFFFFFFFFFFFFFFF
DCSGEN_DEFAULT_TAIL = 1440         # 180 ms of turn-off code
DCSGEN_PERIOD = 28750              # samples after which both grids repeat: 23 words of 1250 samples, 483 bit times


def dcsgen_segment(length: int, code: int = None, inverted: bool = False, amplitude: int = 2000, tail: int = DCSGEN_DEFAULT_TAIL,
                   gap: int = 0, word: int = None):
    """one segment for DcsGen.queue: (gap, length, tail, word, amp), the word that of a code (dcs_word) or any 23 bits
    given as `word`"""
    if (code is None) == (word is None):
        raise ValueError("a segment needs exactly one of code and word")
    return (int(gap), int(length), int(tail), dcs_word(code, inverted) if word is None else int(word), int(amplitude))


def _dcsgen_segs(segs) -> np.ndarray:
    try:
        rows = [[int(v) for v in s] for s in segs]
    except TypeError:
        raise ValueError("segments are sequences of five integers (gap, length, tail, word, amp)")
    if any(len(r) != 5 for r in rows) or any(v < 0 or v > 0xFFFFFFFF for r in rows for v in r):
        raise ValueError("a segment is five values that fit uint32: gap, length, tail, word, amp")
    return np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 5)


class DcsGen(_GenBank):
    """The DCS generator bank (hrfd_dcsgen_*): digital coded squelch on the PCM of n_channels transmit channels, the mirror of
    Dcs.  Segments of a 23-bit word sent cyclically at 134.4 bit/s, each with a tail of the 134.4 Hz turn-off code, are
    queued per channel at absolute stream times, shaped by one FIR for the bank and added, saturating, to the rows Mod and
    Duc.transmit read.  The bit grid is a function of the stream time alone, so a code queued again goes on in phase, and the
    output does not depend on how a stream is cut into calls.  Exact in integers.  (Its kernel is one launch of at most 2^22
    workgroups, so it has no chunked launch and no debug_set_max_wgs.)"""

    _prefix = "dcsgen"
    _max_blocks = DCSGEN_MAX_BLOCKS

    def __init__(self, n_channels: int, device: int = -1):
        self.n = int(n_channels)
        self._create(self.n, device)

    def set_taps(self, taps):
        """1..512 int16 taps in Q14 with sum |h| <= 65535, one shaping filter for every channel (dcs_lowpass_taps designs
        one that keeps the code's edges out of the voice band); from the next call on, the queue and the clock stay"""
        t = np.asarray(taps).ravel()
        if t.size and (t.min() < -32768 or t.max() > 32767):
            raise ValueError("a tap must fit int16")
        t = np.ascontiguousarray(t, dtype=np.int16)
        self._call("set_taps", _ptr(t), t.size)

    def queue(self, channel: int, segs, start: int = DCSGEN_APPEND):
        """1..8 segments (gap, length, tail, word, amp; dcsgen_segment makes one) on one channel or on all (ALL): the first
        begins at start + its gap, each next one its gap behind the end of the one before, tail included; start
        DCSGEN_APPEND = max(time, the end of the channel's last segment).  Refused whole if anything is out of order."""
        a = _dcsgen_segs(segs)
        self._call("queue", int(channel), _ptr(a), a.shape[0], int(start))

    def send(self, channel: int, code: int, inverted: bool = False, amplitude: int = 2000, length: int = DCSGEN_FOREVER,
             tail: int = DCSGEN_DEFAULT_TAIL, start: int = DCSGEN_APPEND):
        """one code, without an end unless length says so: cut(channel) ends it with its turn-off tail"""
        self.queue(channel, [dcsgen_segment(length, code, inverted, amplitude, tail)], start)

    def cut(self, channel: int = ALL, with_tail: bool = True):
        """unkey: the code in progress ends now and its turn-off tail follows (with_tail) or nothing does; a tail in
        progress runs out (with_tail) or ends now; segments not yet begun are dropped"""
        self._call("cut", int(channel), 1 if with_tail else 0)

    def set_time(self, N: int):
        """move the clock only; the queues stay"""
        self._call("set_time", int(N))

    def pending(self, channel: int):
        """(segments of the channel that have not ended, the end of the last of them: the time itself where there is none,
        2^64 - 1 behind a FOREVER segment).  A segment has ended 511 samples behind its end: the shaping filter's reach"""
        n, end = C.c_uint32(0), C.c_uint64(0)
        self._call("pending", int(channel), C.byref(n), C.byref(end))
        return int(n.value), int(end.value)


AFSK_MAX_WINDOW = 32
AFSK_MAX_BLOCKS = 1024
AFSK_BIT = 1                       # of a byte of bits: the value
AFSK_CARRIER = 2                   # of a byte of bits: the carrier flag


def afsk_step(hz: float) -> int:
    """a tone's or a baud rate's phase step at 8 kS/s: round(f / 8000 * 2^32), not reduced (4000 gives 2^31)"""
    return int(round(float(hz) / TONE_FS * 2.0 ** 32))


def afsk_max_bits(baud_step: int, loop_shift: int, n_blocks: int) -> int:
    """the most bits a call of n_blocks gives: ((512 n_blocks (baud_step + (2^31 >> A))) >> 32) + 1"""
    return ((512 * int(n_blocks) * (int(baud_step) + ((1 << 31) >> int(loop_shift)))) >> 32) + 1


def crc16_x25(data) -> int:
    """CRC-16/X.25 (the frame check sequence of HDLC and AX.25): reflected 0x1021, start 0xFFFF, inverted"""
    crc = 0xFFFF
    for byte in bytes(data):
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc ^ 0xFFFF


def hdlc_frames(bits, min_payload: int = 1):
    """the payloads of the HDLC frames in one channel's bit stream (Afsk's bits: only bit 0 of a byte counts), host only:
    frames lie between 0x7E flags, a zero behind five ones is a stuffed one and is dropped, seven ones abort, bytes come
    LSB first, and the last two are the CRC-16/X.25 of the rest, low byte first.  Returns the payloads (bytes, without the
    check sequence) of the frames whose check sequence is good, in order.  Pass the streams of successive calls joined: a
    frame may span calls."""
    frames, cur, ones = [], None, 0
    for v in (np.asarray(bits, dtype=np.uint8).ravel() & 1).tolist():
        if v:
            ones += 1
            if cur is not None:
                cur.append(1)
            if ones >= 7:
                cur = None
            continue
        if ones == 6:                                      # a flag: its 0 and six 1s are the last seven bits taken
            if cur is not None and len(cur) >= 7 + 8 * (int(min_payload) + 2) and (len(cur) - 7) % 8 == 0:
                data = np.packbits(np.array(cur[:-7], dtype=np.uint8), bitorder="little").tobytes()
                if crc16_x25(data[:-2]) == data[-2] | (data[-1] << 8):
                    frames.append(data[:-2])
            cur = []
        elif ones != 5 and cur is not None:                # (behind five ones: a stuffed zero)
            cur.append(0)
        ones = 0
    return frames


class Afsk(_Bank):
    """The AFSK bank (hrfd_afsk_*): the PCM of n_channels channels as Rx / Ddc.receive write it in, the packet data on them
    out: per channel the bits a recovered clock samples off a mark / space discriminator (Bell 202 by default), each with a
    carrier flag, and optionally the discriminator's decision for every sample.  One modem for all channels.  Exact in
    integers, independent of how a stream is cut into calls.  hdlc_frames turns a channel's bits into frames.  (Its kernel is
    one launch of one workgroup per channel, so like Leveler it has no chunked launch and no debug_set_max_wgs.)"""

    _prefix = "afsk"

    def __init__(self, n_channels: int, mark_hz: float = 1200, space_hz: float = 2200, baud: float = 1200, window: int = 8,
                 loop_shift: int = 2, nrzi: bool = True, device: int = 0):
        self.n = int(n_channels)
        self._create(self.n, device)
        self.set_modem(mark_hz, space_hz, baud, window, loop_shift, nrzi)

    def set_modem(self, mark_hz: float = 1200, space_hz: float = 2200, baud: float = 1200, window: int = 8, loop_shift: int = 2,
                  nrzi: bool = True, steps=None):
        """the modem of every channel (steps = (mark_step, space_step, baud_step) overrides the three rates); resets every
        channel"""
        m, s, b = (int(v) for v in steps) if steps is not None else (afsk_step(mark_hz), afsk_step(space_hz), afsk_step(baud))
        for name, v in (("mark_step", m), ("space_step", s), ("baud_step", b), ("window", window), ("loop_shift", loop_shift)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must fit uint32, got {v}")
        self._call("set_modem", m, s, b, int(window), int(loop_shift), 1 if nrzi else 0)
        self.baud_step, self.loop_shift = b, int(loop_shift)

    def set_carrier(self, min_power: int):
        """the carrier flag is set where P_mark + P_space > min_power (0..2^64-1; 0 unless set)"""
        self._call("set_carrier", int(min_power))

    def reset(self, channel: int = ALL):
        """zero the state of one channel, or of all"""
        self._call("reset", int(channel))

    def max_bits(self, n_blocks: int) -> int:
        """the most bits a call of n_blocks gives a channel: the least length of a row of bits"""
        v = C.c_uint32(0)
        self._call("max_bits", int(n_blocks), C.byref(v))
        return int(v.value)

    def process(self, pcm: np.ndarray, n_pcm=None, want_bits: bool = True, want_hard: bool = False):
        """pcm int16 [n_channels, n_blocks, 512], n_pcm uint32 [n_channels, n_blocks] or None -> (bits: a list of n_channels
        uint8 arrays, one byte per bit: AFSK_BIT | AFSK_CARRIER; or None, hard uint8 [n_channels, n_blocks, 64] or None);
        blocking"""
        x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(self.n, -1)
        n_blocks = x.shape[1] // 512
        if x.shape[1] != 512 * n_blocks:
            raise ValueError(f"a channel's PCM must be whole blocks of 512 samples, got {x.shape[1]} samples")
        npc = None if n_pcm is None else np.ascontiguousarray(n_pcm, dtype=np.uint32).reshape(self.n, n_blocks)
        rows = np.zeros((self.n, self.max_bits(n_blocks)), dtype=np.uint8) if want_bits else None
        n_bits = np.zeros(self.n, dtype=np.uint32) if want_bits else None
        hard = np.zeros((self.n, n_blocks, 64), dtype=np.uint8) if want_hard else None
        self._call("process", _ptr(x), _ptr(npc), n_blocks, _ptr(rows), _ptr(n_bits), _ptr(hard))
        bits = [rows[c, :n_bits[c]].copy() for c in range(self.n)] if want_bits else None
        return bits, hard

    def process_device(self, d_pcm, channel_stride: int, d_n_pcm, n_blocks: int, d_bits=None, bits_stride: int = 0, d_n_bits=None,
                       d_hard=None, stream=None):
        """device pointers (ints); d_n_pcm, d_hard, or d_bits with d_n_bits may be None (not all outputs); bits_stride 0 =
        rows of max_bits(n_blocks) bytes; asynchronous on stream (None = the handle's own)"""
        if not bits_stride and d_bits is not None:
            bits_stride = self.max_bits(n_blocks)
        self._call("process_device", _ptr(d_pcm), int(channel_stride), _ptr(d_n_pcm), int(n_blocks), _ptr(d_bits), int(bits_stride),
                   _ptr(d_n_bits), _ptr(d_hard), _ptr(stream))


HDLC_MAX_BITS = 1 << 20
HDLC_MAX_PAYLOAD = 1021


def hdlc_max_out(max_bits: int, min_payload: int = 1, max_payload: int = 512) -> int:
    """a row of records that never drops: 11 F + min(F P, P + max_bits / 8) rounded up to 4, F = 1 + (max_bits - 1) / (8 (m + 3))"""
    F = 1 + (int(max_bits) - 1) // (8 * (int(min_payload) + 3))
    P = int(max_payload)
    return (11 * F + min(F * P, P + int(max_bits) // 8) + 3) & ~3


class Hdlc(_Bank):
    """The HDLC bank (hrfd_hdlc_*): the rows of bits Afsk.process_device writes in, read where they lie on the device, the
    packet frames in them out: per channel a row of records (end_bit, n_payload, fcs, payload) of the frames whose
    CRC-16/X.25 is good, and the counts of records, bad frames and dropped records.  The state (a partial frame, the run of
    ones) lives on the device: a stream may be cut into calls anywhere.  With require_carrier off the payloads are those of
    hdlc_frames over the joined stream that have at most max_payload bytes.  (One launch of one workgroup per channel, so
    like Afsk it has no chunked launch and no debug_set_max_wgs.)"""

    _prefix = "hdlc"

    def __init__(self, n_channels: int, min_payload: int = 1, max_payload: int = 512, require_carrier: bool = False, device: int = 0):
        self.n = int(n_channels)
        self._create(self.n, device)
        if (int(min_payload), int(max_payload)) != (1, 512):
            self.set_limits(min_payload, max_payload)
        if require_carrier:
            self.set_require_carrier(True)

    def set_limits(self, min_payload: int = 1, max_payload: int = 512):
        """payloads of min_payload..max_payload bytes (1..1021); resets every channel"""
        for name, v in (("min_payload", min_payload), ("max_payload", max_payload)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must fit uint32, got {v}")
        self._call("set_limits", int(min_payload), int(max_payload))

    def set_require_carrier(self, on: bool):
        """on: a bit without the carrier flag ends the frame it lies in"""
        self._call("set_require_carrier", 1 if on else 0)

    def reset(self, channel: int = ALL):
        """forget the partial frame of one channel, or of all"""
        self._call("reset", int(channel))

    def max_out(self, max_bits: int) -> int:
        """the bytes of a row of records that never drops for a call of max_bits bits under the handle's limits"""
        v = C.c_uint32(0)
        self._call("max_out", int(max_bits), C.byref(v))
        return int(v.value)

    @staticmethod
    def parse(row, n_frames: int):
        """the first n_frames records of a row of records (uint8) -> [(end_bit, payload bytes, fcs)]"""
        row = np.ascontiguousarray(row, dtype=np.uint8).ravel()
        frames, at = [], 0
        for _ in range(int(n_frames)):
            end_bit, n, fcs = (int(v) for v in np.frombuffer(row[at:at + 8].tobytes(), dtype="<u4,<u2,<u2")[0])
            frames.append((end_bit, row[at + 8:at + 8 + n].tobytes(), fcs))
            at += 8 + ((n + 3) & ~3)
        return frames

    def process(self, bits_list, out_bytes: int = None, want_counts: bool = False):
        """bits_list: per channel a uint8 array of bits as Afsk.process gives them (any lengths) -> per channel
        [(end_bit, payload)] of the good frames that close in this call; with want_counts also (n_frames, n_bad, dropped),
        uint32 [n_channels] each.  out_bytes: the row of records, max_out of the longest row unless given; blocking"""
        if len(bits_list) != self.n:
            raise ValueError(f"need the bits of {self.n} channels, got {len(bits_list)}")
        rows = [np.ascontiguousarray(b, dtype=np.uint8).ravel() for b in bits_list]
        max_bits = max(1, max(len(r) for r in rows))
        dense = np.zeros((self.n, max_bits), dtype=np.uint8)
        for c, r in enumerate(rows):
            dense[c, :len(r)] = r
        n_bits = np.array([len(r) for r in rows], dtype=np.uint32)
        out_bytes = self.max_out(max_bits) if out_bytes is None else int(out_bytes)
        out = np.zeros((self.n, out_bytes), dtype=np.uint8)
        n_frames, n_bad, dropped = (np.zeros(self.n, dtype=np.uint32) for _ in range(3))
        self._call("process", _ptr(dense), _ptr(n_bits), max_bits, _ptr(out), out_bytes, _ptr(n_frames), _ptr(n_bad), _ptr(dropped))
        frames = [[(e, p) for e, p, _ in self.parse(out[c], n_frames[c])] for c in range(self.n)]
        return (frames, (n_frames, n_bad, dropped)) if want_counts else frames

    def process_device(self, d_bits, bits_stride: int, d_n_bits, max_bits: int, d_out, out_stride: int, out_bytes: int, d_n_frames,
                       d_n_bad, d_dropped, stream=None):
        """device pointers (ints): the rows of bits and counts of Afsk.process_device, max_bits the most a row holds; rows of
        records out_stride apart of out_bytes each; d_n_bad may be None; asynchronous on stream (None = the handle's own)"""
        self._call("process_device", _ptr(d_bits), int(bits_stride), _ptr(d_n_bits), int(max_bits), _ptr(d_out), int(out_stride),
                   int(out_bytes), _ptr(d_n_frames), _ptr(d_n_bad), _ptr(d_dropped), _ptr(stream))


AFSKGEN_MAX_MESSAGES = 4
AFSKGEN_MAX_BITS = 8192
AFSKGEN_MAX_BLOCKS = 1024
AFSKGEN_NRZI = 1
AFSKGEN_APPEND = 0xFFFFFFFFFFFFFFFF
AFSKGEN_RAMP = 64


def hdlc_encode(payloads, n_lead_flags: int = 12, n_between: int = 2, n_tail_flags: int = 3) -> np.ndarray:
    """the bit stream of HDLC frames for AfskGen.queue, one uint8 of 0 / 1 per bit, host only: n_lead_flags 0x7E flags, then
    per frame the payload and its CRC-16/X.25, low byte first, every byte LSB first, a zero stuffed behind five ones, with
    n_between flags between frames and n_tail_flags behind the last.  The inverse of hdlc_frames.  The first and the last 64
    samples of a message are ramped, about ten bits at 1200 baud: that is what the lead and tail flags are for, so keep at
    least a dozen in front and two behind."""
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    payloads = [bytes(p) for p in payloads]
    out = flag * int(n_lead_flags)
    for i, p in enumerate(payloads):
        crc = crc16_x25(p)
        ones = 0
        for byte in p + bytes([crc & 255, crc >> 8]):
            for k in range(8):
                b = (byte >> k) & 1
                out.append(b)
                ones = ones + 1 if b else 0
                if ones == 5:
                    out.append(0)
                    ones = 0
        out += flag * int(n_between if i + 1 < len(payloads) else n_tail_flags)
    return np.array(out, dtype=np.uint8)


HDLCGEN_MAX_BITS = 1 << 20
HDLCGEN_MAX_FLAGS = 255


def hdlc_records(payloads) -> np.ndarray:
    """payloads -> one row of the HDLC bank's records (uint8): uint32 end_bit = 0, uint16 n_payload, uint16 fcs = 0, the
    payload, zeros up to a multiple of 4.  The framer ignores end_bit and fcs"""
    out = bytearray()
    for p in payloads:
        p = bytes(p)
        if not 1 <= len(p) <= HDLC_MAX_PAYLOAD:
            raise ValueError(f"a payload has 1..{HDLC_MAX_PAYLOAD} bytes, got {len(p)}")
        out += (0).to_bytes(4, "little") + len(p).to_bytes(2, "little") + b"\0\0" + p + b"\0" * (-len(p) & 3)
    return np.frombuffer(bytes(out), dtype=np.uint8).copy()


def hdlcgen_max_bits(n_frames: int, payload_bytes: int, n_lead_flags: int = 12, n_between: int = 2, n_tail_flags: int = 3) -> int:
    """a row of bits that never drops n_frames frames of payload_bytes together: D + D // 5 with D = 8 (payload_bytes +
    2 n_frames), and the lead + (n_frames - 1) between + tail flags"""
    D = 8 * (int(payload_bytes) + 2 * int(n_frames))
    return D + D // 5 + 8 * (int(n_lead_flags) + (int(n_frames) - 1) * int(n_between) + int(n_tail_flags))


def hdlc_encode_c(payloads, n_lead_flags: int = 12, n_between: int = 2, n_tail_flags: int = 3, max_bits: int = None,
                  want_counts: bool = False):
    """hdlc_encode through the library's host entry hrfd_hdlc_encode (no GPU): the same bits, from the C text that restates
    the framer bank's law for one row.  max_bits: the row's room, the bound of the payloads unless given; frames that do
    not fit are dropped under the bank's rule.  With want_counts also (n_sent, dropped)"""
    payloads = [bytes(p) for p in payloads]
    row = hdlc_records(payloads)
    if row.size == 0:
        row = np.zeros(4, dtype=np.uint8)
    if max_bits is None:
        max_bits = hdlcgen_max_bits(len(payloads), sum(len(p) for p in payloads), n_lead_flags, n_between, n_tail_flags) if payloads else 1
    for name, v in (("n_lead_flags", n_lead_flags), ("n_between", n_between), ("n_tail_flags", n_tail_flags), ("max_bits", max_bits)):
        if not 0 <= int(v) <= 0xFFFFFFFF:
            raise ValueError(f"{name} must fit uint32, got {v}")
    bits = np.zeros(min(int(max_bits), HDLCGEN_MAX_BITS), dtype=np.uint8)
    n_bits, n_sent, dropped = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().hrfd_hdlc_encode(_ptr(row), row.size, len(payloads), int(n_lead_flags), int(n_between), int(n_tail_flags),
                                       _ptr(bits), int(max_bits), C.byref(n_bits), C.byref(n_sent), C.byref(dropped)),
          "hrfd_hdlc_encode")
    out = bits[:n_bits.value].copy()
    return (out, (int(n_sent.value), int(dropped.value))) if want_counts else out


class HdlcGen(_Bank):
    """The HDLC framer bank (hrfd_hdlcgen_*): rows of frame records in, read where they lie on the device (Hdlc's own rows
    among them), the bits that say them out: per channel a row of one byte per bit, flags, the CRC-16/X.25 check sequence and
    bit stuffing included, as AfskGen.queue takes it and Hdlc reads it; for the same flag counts hdlc_encode bit for bit.
    A frame that does not fit a row's max_bits is dropped with every frame behind it and counted.  The bank keeps nothing
    between calls.  (One launch of one workgroup per channel, so like Hdlc it has no chunked launch and no
    debug_set_max_wgs.)"""

    _prefix = "hdlcgen"

    def __init__(self, n_channels: int, n_lead_flags: int = 12, n_between: int = 2, n_tail_flags: int = 3, device: int = 0):
        self.n = int(n_channels)
        self._create(self.n, device)
        if (int(n_lead_flags), int(n_between), int(n_tail_flags)) != (12, 2, 3):
            self.set_flags(n_lead_flags, n_between, n_tail_flags)

    def set_flags(self, n_lead_flags: int = 12, n_between: int = 2, n_tail_flags: int = 3):
        """flags in front of the first frame (0..255), between two frames and behind the last (1..255 each)"""
        for name, v in (("n_lead_flags", n_lead_flags), ("n_between", n_between), ("n_tail_flags", n_tail_flags)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must fit uint32, got {v}")
        self._call("set_flags", int(n_lead_flags), int(n_between), int(n_tail_flags))

    def max_bits(self, n_frames: int, payload_bytes: int) -> int:
        """a row of bits that never drops n_frames frames of payload_bytes together under the handle's flag counts"""
        v = C.c_uint32(0)
        self._call("max_bits", int(n_frames), int(payload_bytes), C.byref(v))
        return int(v.value)

    def pack(self, payloads_per_channel):
        """per channel a list of payloads -> (rows uint8 [n_channels, in_bytes] of records, n_frames uint32 [n_channels])"""
        if len(payloads_per_channel) != self.n:
            raise ValueError(f"need the payloads of {self.n} channels, got {len(payloads_per_channel)}")
        recs = [hdlc_records(p) for p in payloads_per_channel]
        rows = np.zeros((self.n, max(4, max(r.size for r in recs))), dtype=np.uint8)
        for c, r in enumerate(recs):
            rows[c, :r.size] = r
        return rows, np.array([len(p) for p in payloads_per_channel], dtype=np.uint32)

    def process(self, payloads_per_channel, max_bits: int = None, want_counts: bool = False):
        """per channel a list of payloads -> per channel the bits (uint8, 0 / 1) of one message that says them; with
        want_counts also (n_sent, dropped), uint32 [n_channels] each.  max_bits: a row's room, the bound of the longest
        channel unless given; blocking"""
        rows, n_frames = self.pack(payloads_per_channel)
        if max_bits is None:
            max_bits = max([1] + [self.max_bits(len(p), sum(len(bytes(q)) for q in p)) for p in payloads_per_channel if len(p)])
        bits, (n_bits, n_sent, dropped) = self.process_rows(rows, n_frames, int(max_bits))
        out = [bits[c, :n_bits[c]].copy() for c in range(self.n)]
        return (out, (n_sent, dropped)) if want_counts else out

    def process_rows(self, rows: np.ndarray, n_frames, max_bits: int):
        """rows uint8 [n_channels, in_bytes] of records (pack's, or Hdlc's), n_frames uint32 [n_channels] -> (bits uint8
        [n_channels, max_bits], (n_bits, n_sent, dropped)); blocking"""
        rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(self.n, -1)
        nf = np.ascontiguousarray(n_frames, dtype=np.uint32).reshape(self.n)
        bits = np.zeros((self.n, int(max_bits)), dtype=np.uint8)
        n_bits, n_sent, dropped = (np.zeros(self.n, dtype=np.uint32) for _ in range(3))
        self._call("process", _ptr(rows), rows.shape[1], _ptr(nf), _ptr(bits), int(max_bits), _ptr(n_bits), _ptr(n_sent), _ptr(dropped))
        return bits, (n_bits, n_sent, dropped)

    def process_device(self, d_in, in_stride: int, in_bytes: int, d_n_frames, d_bits, bits_stride: int, max_bits: int, d_n_bits,
                       d_n_sent=None, d_dropped=None, stream=None):
        """device pointers (ints): rows of records in_stride apart of in_bytes each and their counts (Hdlc.process_device's
        d_out and d_n_frames as they are); rows of bits bits_stride apart of max_bits each, and the counts; d_n_sent and
        d_dropped may be None; asynchronous on stream (None = the handle's own)"""
        self._call("process_device", _ptr(d_in), int(in_stride), int(in_bytes), _ptr(d_n_frames), _ptr(d_bits), int(bits_stride),
                   int(max_bits), _ptr(d_n_bits), _ptr(d_n_sent), _ptr(d_dropped), _ptr(stream))


def ax25_address(call: str, ssid: int = 0, last: bool = False) -> bytes:
    """the seven bytes of an AX.25 address field: the call sign in capitals, filled up to six with spaces, every character
    shifted left by one, then the SSID byte 0x60 | ssid << 1, with bit 0 set on the last address of the header"""
    call = str(call).upper()
    if not 1 <= len(call) <= 6 or not all(c.isascii() and c.isalnum() for c in call):
        raise ValueError(f"a call sign has 1..6 letters and digits, got {call!r}")
    if not 0 <= int(ssid) <= 15:
        raise ValueError(f"ssid must be 0..15, got {ssid}")
    return bytes(ord(c) << 1 for c in call.ljust(6)) + bytes([0x60 | (int(ssid) << 1) | (1 if last else 0)])


def _ax25_station(s):
    """a station as 'CALL', 'CALL-SSID' or (call, ssid) -> (call, ssid)"""
    if isinstance(s, str):
        call, _, ssid = s.partition("-")
        return call, int(ssid) if ssid else 0
    return str(s[0]), int(s[1])


def ax25_ui_frame(dest, src, info, path=(), pid: int = 0xF0) -> bytes:
    """the payload of an AX.25 UI frame (what APRS sends), without flags and check sequence, ready for HdlcGen or
    hdlc_encode: destination, source and up to eight digipeaters ("CALL-SSID" or (call, ssid)), control 0x03, the PID
    (0xF0: no layer 3) and the information field"""
    path = list(path)
    if len(path) > 8:
        raise ValueError(f"at most 8 digipeaters, got {len(path)}")
    if not 0 <= int(pid) <= 255:
        raise ValueError(f"pid must be 0..255, got {pid}")
    stations = [_ax25_station(s) for s in [dest, src] + path]
    head = b"".join(ax25_address(c, s, last=(i + 1 == len(stations))) for i, (c, s) in enumerate(stations))
    frame = head + bytes([0x03, int(pid)]) + bytes(info)
    if len(frame) > HDLC_MAX_PAYLOAD:
        raise ValueError(f"the frame has {len(frame)} bytes, more than {HDLC_MAX_PAYLOAD}")
    return frame


def ax25_parse(payload):
    """the inverse of ax25_ui_frame: {"dest": (call, ssid), "src": (call, ssid), "path": [(call, ssid), ..], "control", "pid",
    "info"}; ValueError for what is no UI frame (a header that does not end, control other than 0x03)"""
    p = bytes(payload)
    stations, at = [], 0
    while True:
        if at + 7 > len(p) or len(stations) == 10:
            raise ValueError("the address field does not end")
        a = p[at:at + 7]
        if any(v & 1 for v in a[:6]):
            raise ValueError("a call sign byte with its low bit set")
        stations.append(("".join(chr(v >> 1) for v in a[:6]).rstrip(), (a[6] >> 1) & 15))
        at += 7
        if a[6] & 1:
            break
    if len(stations) < 2 or at + 2 > len(p):
        raise ValueError("no destination and source, or no control and PID behind them")
    if p[at] != 0x03:
        raise ValueError(f"control 0x{p[at]:02X} is no UI frame")
    return {"dest": stations[0], "src": stations[1], "path": stations[2:], "control": p[at], "pid": p[at + 1], "info": p[at + 2:]}


class AfskGen(_GenBank):
    """The AFSK generator bank (hrfd_afskgen_*): packet data on the PCM of n_channels transmit channels, the mirror of Afsk.
    Messages of up to 8192 bits, each with a modem of its own (Bell 202 by default), are queued per channel at absolute
    stream times, at most four that have not ended, and added, saturating, to the rows Mod and Duc.transmit read, as
    continuous-phase AFSK with a ramp of 8 ms at either end.  Exact in integers on the tone generator's phase grid, and
    independent of how a stream is cut into calls; it composes with ToneGen by running one behind the other, in place.
    (Its kernel is one launch of one workgroup per channel, so like Leveler and Afsk it has no chunked launch and no
    debug_set_max_wgs.)"""

    _prefix = "afskgen"
    _max_blocks = AFSKGEN_MAX_BLOCKS

    def __init__(self, n_channels: int, device: int = 0):
        self.n = int(n_channels)
        self._create(self.n, device)

    def queue(self, channel: int, bits, mark_hz: float = 1200, space_hz: float = 2200, baud: float = 1200, amplitude: int = 8000,
              nrzi: bool = True, start: int = AFSKGEN_APPEND, gap: int = 0, steps=None):
        """one message of 1..8192 bits (one value per bit, only bit 0 counts: a row of Afsk's bits can be queued as it is) on
        one channel or on all (ALL); it begins at start + gap, start AFSKGEN_APPEND = max(time, the end of the channel's last
        message).  steps = (mark_step, space_step, baud_step) overrides the three rates.  Refused whole if anything is out
        of order."""
        b = np.ascontiguousarray(np.asarray(bits).ravel() & 1, dtype=np.uint8)
        m, s, r = (int(v) for v in steps) if steps is not None else (afsk_step(mark_hz), afsk_step(space_hz), afsk_step(baud))
        msg = [int(gap), int(b.size), m, s, r, int(amplitude), AFSKGEN_NRZI if nrzi else 0, 0]
        if any(v < 0 or v > 0xFFFFFFFF for v in msg):
            raise ValueError(f"gap, the bit count, the steps and the amplitude must fit uint32, got {msg[:6]}")
        if not 0 <= int(start) <= AFSKGEN_APPEND:
            raise ValueError(f"start {start}")
        a = np.array(msg, dtype=np.uint32)
        self._call("queue", int(channel), _ptr(a), _ptr(b), int(start))

    def send(self, channel: int, payloads, **modem):
        """queue(channel, hdlc_encode(payloads), ...): one message of HDLC frames with the default flag counts"""
        self.queue(channel, hdlc_encode(payloads), **modem)

    def send_all(self, framer, payloads_per_channel, **modem):
        """the whole bank's packets at once: one framer call (an HdlcGen of as many channels) frames every channel's
        payloads on the device, then one queue per channel that has a frame.  Refused before anything is queued if a
        channel's message passes 8192 bits"""
        if framer.n != self.n:
            raise ValueError(f"the framer has {framer.n} channels, the generator {self.n}")
        messages, (_, dropped) = framer.process(payloads_per_channel, want_counts=True)
        for c, m in enumerate(messages):
            if m.size > AFSKGEN_MAX_BITS or dropped[c]:
                raise ValueError(f"channel {c}: a message of {m.size} bits ({int(dropped[c])} frames dropped); a message has at most "
                                 f"{AFSKGEN_MAX_BITS} bits")
        for c, m in enumerate(messages):
            if m.size:
                self.queue(c, m, **modem)

    def cut(self, channel: int = ALL):
        """ramp the message in progress down over the next 64 samples and drop those not yet begun"""
        self._call("cut", int(channel))

    def set_time(self, N: int):
        """move the clock; refused while a channel holds a message that has not ended"""
        self._call("set_time", int(N))

    def pending(self, channel: int):
        """(messages of the channel that have not ended, the end of the last of them: the time itself where there is none)"""
        n, end = C.c_uint32(0), C.c_uint64(0)
        self._call("pending", int(channel), C.byref(n), C.byref(end))
        return int(n.value), int(end.value)


class Engine:
    """Factory with the interface tests/goldencheck.py expects."""

    def ssbmod(self, lsb=True):
        m = Mod(MOD_SSB, 1)
        m.set_sideband(lsb)
        return m

    def interp(self):
        return Mod(MOD_INTERP, 1)

    def ammod(self):
        return Mod(MOD_AM, 1)

    def fmmod(self):
        return Mod(MOD_FM, 1)

    def wbfmmod(self):
        return Mod(MOD_WBFM, 1)

    def rx(self):
        return SingleChannelRx()

    def demod(self, mode):
        return Demod(mode, 1)


def q15_table(name: str) -> np.ndarray:
    """a constant table of the library (hrfd_q15_table): the count first, then the whole table"""
    L = _lib.load()
    n = L.hrfd_q15_table(name.encode(), None, 0)
    buf = np.zeros(n, dtype=np.int16)
    if n:
        L.hrfd_q15_table(name.encode(), buf.ctypes.data_as(C.POINTER(C.c_int16)), n)
    return buf


def atan2_table() -> np.ndarray:
    L = _lib.load()
    out = np.zeros((256, 256), dtype=np.float32)
    check(L.hrfd_atan2_table(out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def dbfs_table() -> np.ndarray:
    L = _lib.load()
    out = np.zeros(257, dtype=np.int32)
    check(L.hrfd_dbfs_table(out.ctypes.data_as(C.POINTER(C.c_int32))))
    return out


def debug_sincosf_eval(variant: int, form: int, x):
    """(sin, cos) of every float of x by the device's restatement of glibc's sinf / cosf (hrfd_debug_sincosf_eval):
    variant 0 / 1 without / with fused multiply-adds, form 0 the pair function, 1 the one-sided ones."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    sn, cs = np.empty_like(x), np.empty_like(x)
    f32p = C.POINTER(C.c_float)
    check(_lib.load().hrfd_debug_sincosf_eval(int(variant), int(form), x.ctypes.data_as(f32p), x.size,
                                              sn.ctypes.data_as(f32p), cs.ctypes.data_as(f32p)), "hrfd_debug_sincosf_eval")
    return sn, cs


def debug_sincosf_digest(variant: int, form: int, first_chunk: int, n_chunks: int, timed: bool = False):
    """uint64 [n_chunks]: the device's digests of chunks of 2^20 float bit patterns (hrfd_debug_sincosf_digest);
    timed: (digests, the kernel's milliseconds)"""
    out = np.zeros(max(int(n_chunks), 0), dtype=np.uint64)
    ms = C.c_float(0.0)
    check(_lib.load().hrfd_debug_sincosf_digest(int(variant), int(form), int(first_chunk), int(n_chunks),
                                                out.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(ms) if timed else None),
          "hrfd_debug_sincosf_digest")
    return (out, float(ms.value)) if timed else out


def device_count() -> int:
    return int(_lib.load().hrfd_device_count())
