"""Locate / load libhrfd.so (the C ABI of include/hrfd.h) with ctypes.

There is deliberately no fallback: if the shared library is missing the import
raises, and if there is no GPU every create call returns HRFD_ENODEV.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# HRFD_LIB selects another build of the same library (tools/gpu_ab.py compares tuning variants)
LIB_PATH = os.environ.get("HRFD_LIB") or os.path.join(PKG_DIR, "lib", "libhrfd.so")

_i16p = C.POINTER(C.c_int16)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p

_lib = None
_runtime = None        # the HIP runtime CDLL the library was bound to


def _load_hip_runtime():
    """libhrfd.so carries no DT_NEEDED entry for the HIP runtime: a process must
    hold exactly ONE HIP/HSA runtime.  When PyTorch is importable we bind to the
    runtime it ships (so torch tensors, streams and RCCL share the device context
    with our kernels); otherwise to the system ROCm runtime.  Set
    HRFD_HIP_RUNTIME=/path/libamdhip64.so to force a choice."""
    global _runtime
    if _runtime is not None:
        return _runtime
    cands = []
    forced = os.environ.get("HRFD_HIP_RUNTIME")
    if forced:
        cands.append(forced)
    elif os.environ.get("HRFD_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401  (loads its bundled runtime)
            tl = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
            if os.path.exists(tl):
                cands.append(tl)
        except Exception:
            pass
    cands += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so"]
    last = None
    for c in cands:
        try:
            _runtime = C.CDLL(c, mode=C.RTLD_GLOBAL)
            return _runtime
        except OSError as e:      # try the next candidate
            last = e
    raise HrfdError(f"no HIP runtime could be loaded ({last}); libhrfd.so needs libamdhip64")


class HrfdError(RuntimeError):
    pass


def load() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HrfdError(f"{LIB_PATH} not found: build it with "
                        "`python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _load_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.hrfd_last_error.restype = C.c_char_p
    L.hrfd_version.restype = C.c_int
    L.hrfd_device_count.restype = C.c_int
    L.hrfd_rx_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
    L.hrfd_rx_destroy.argtypes = [_vp]
    L.hrfd_rx_set_mode.argtypes = [_vp, C.c_uint32, C.c_int]
    L.hrfd_rx_set_gain.argtypes = [_vp, C.c_uint32, C.c_int, C.c_float]
    L.hrfd_rx_set_threshold.argtypes = [_vp, C.c_uint32, C.c_int32]
    L.hrfd_rx_reset_demod.argtypes = [_vp, C.c_uint32, C.c_int]
    L.hrfd_rx_process_block.argtypes = [_vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32,
                                        _vp, _vp, _vp, _vp, _vp]
    L.hrfd_rx_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                         _vp, _vp, _vp, _vp, _vp, _vp]
    L.hrfd_rx_sync.argtypes = [_vp, _u32p]
    for name in ("hrfd_rx_pcm_capacity", "hrfd_rx_iq256_capacity", "hrfd_demod_pcm_capacity"):
        getattr(L, name).argtypes = [C.c_uint32]
        getattr(L, name).restype = C.c_uint32
    L.hrfd_rx_pending_samples.argtypes = [_vp, _u32p]
    L.hrfd_rx_debug_ragged.argtypes = [_vp, _i32p, C.POINTER(C.c_ulonglong)]
    L.hrfd_rx_reduce_sample_rate.argtypes = [_vp, _vp, C.c_uint32, _vp]
    L.hrfd_rx_failed_channels.argtypes = [_vp, C.c_void_p, C.c_uint32]
    L.hrfd_rx_debug_set_warm.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_set_atan.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_atan_eval.argtypes = [_vp, _f32p]
    L.hrfd_rx_debug_atan_eval_tab.argtypes = [_vp, _f32p]
    for name, args in (("hrfd_rx_debug_atan_eval_quad", [_vp, _f32p]), ("hrfd_debug_atan2_quadrant", [_u32p, _i32p])):
        if hasattr(L, name):                               # (round-5 hooks: an older build named by HRFD_LIB, as tools/flow_ab.sh compares, has none)
            getattr(L, name).argtypes = args
    L.hrfd_rx_debug_counters.argtypes = [_vp, _u32p]
    L.hrfd_rx_debug_set_stagger.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_expire.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_set_gated.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_set_fir_flow.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_set_stream.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_set_run_len.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_stamps.argtypes = [_vp, C.c_uint32, _vp]
    L.hrfd_rx_debug_enable_timing.argtypes = [_vp, C.c_int]
    L.hrfd_rx_debug_kernel_ms.argtypes = [_vp, C.c_int, _f32p]
    L.hrfd_rx_debug_timing_every.argtypes = [_vp, C.c_int]
    L.hrfd_debug_membw.argtypes = [C.c_int, _vp, C.c_size_t, _vp, _vp]
    L.hrfd_demod_create.argtypes = [C.c_int, C.c_uint32, C.c_int, C.POINTER(_vp)]
    L.hrfd_demod_destroy.argtypes = [_vp]
    L.hrfd_demod_reset.argtypes = [_vp, C.c_uint32]
    L.hrfd_demod_set_gain.argtypes = [_vp, C.c_uint32, C.c_float]
    L.hrfd_demod_set_sideband.argtypes = [_vp, C.c_uint32, C.c_int]
    L.hrfd_demod_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
    L.hrfd_ingest_create.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]
    L.hrfd_ingest_destroy.argtypes = [_vp]
    L.hrfd_ingest_acquire.argtypes = [_vp, C.POINTER(_vp)]
    L.hrfd_ingest_submit.argtypes = [_vp, C.c_uint32]
    L.hrfd_ingest_collect.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]
    L.hrfd_ingest_replayed.argtypes = [_vp, C.POINTER(C.c_uint64)]
    L.hrfd_fanout_channel_range.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p]
    L.hrfd_fanout_create.argtypes = [C.c_uint32, C.POINTER(C.c_int), C.c_uint32, C.POINTER(_vp)]
    L.hrfd_fanout_destroy.argtypes = [_vp]
    L.hrfd_fanout_shards.argtypes = [_vp, _u32p]
    L.hrfd_fanout_set_mode.argtypes = [_vp, C.c_uint32, C.c_int]
    L.hrfd_fanout_set_gain.argtypes = [_vp, C.c_uint32, C.c_int, C.c_float]
    L.hrfd_fanout_set_threshold.argtypes = [_vp, C.c_uint32, C.c_int32]
    L.hrfd_fanout_scatter.argtypes = [_vp, C.c_int, _vp, C.c_uint32, C.c_uint32, _vp]
    L.hrfd_fanout_input.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp), _u32p, _u32p]
    L.hrfd_fanout_process.argtypes = [_vp, C.c_uint32]
    L.hrfd_fanout_collect.argtypes = [_vp, C.c_int, _vp, _vp, _u32p]
    L.hrfd_txring_create.argtypes = [C.c_uint32, C.POINTER(_vp)]
    L.hrfd_txring_destroy.argtypes = [_vp]
    L.hrfd_txring_set_running.argtypes = [_vp, C.c_uint32, C.c_int]
    L.hrfd_txring_write.argtypes = [_vp, C.c_uint32, _vp]
    L.hrfd_txring_read_batch.argtypes = [_vp, _vp]
    L.hrfd_txring_stats.argtypes = [_vp, C.c_uint32, _u32p]
    L.hrfd_mod_create.argtypes = [C.c_int, C.c_uint32, C.c_int, C.POINTER(_vp)]
    L.hrfd_mod_destroy.argtypes = [_vp]
    L.hrfd_mod_reset.argtypes = [_vp, C.c_uint32]
    L.hrfd_mod_set_sideband.argtypes = [_vp, C.c_uint32, C.c_int]
    L.hrfd_mod_set_modulation_index.argtypes = [_vp, C.c_uint32, C.c_float]
    L.hrfd_mod_set_deviation.argtypes = [_vp, C.c_uint32, C.c_float]
    L.hrfd_mod_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _u32p]
    L.hrfd_mod_process_device.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
    L.hrfd_mod_sync.argtypes = [_vp]
    if hasattr(L, "hrfd_libm_variant"):
        L.hrfd_libm_variant.argtypes = []
        L.hrfd_libm_variant.restype = C.c_int
    L.hrfd_mod_debug_set_sliced.argtypes = [_vp, C.c_int]
    L.hrfd_mod_debug_set_scan.argtypes = [_vp, C.c_int]
    if hasattr(L, "hrfd_mod_debug_set_tail"):              # (round 6; an older build named by HRFD_LIB has none)
        L.hrfd_mod_debug_set_tail.argtypes = [_vp, C.c_int]
    L.hrfd_play_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
    L.hrfd_play_destroy.argtypes = [_vp]
    L.hrfd_play_load_file.argtypes = [_vp, C.c_char_p]
    L.hrfd_play_load.argtypes = [_vp, _vp, C.c_uint32]
    L.hrfd_play_set_position.argtypes = [_vp, C.c_uint32, C.c_uint32]
    L.hrfd_play_get_position.argtypes = [_vp, C.c_uint32, _u32p]
    L.hrfd_play_get_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp]
    L.hrfd_play_get.argtypes = [_vp, _vp, C.c_uint32]
    if hasattr(L, "hrfd_debug_sincosf_eval"):              # (an older build named by HRFD_LIB has none)
        L.hrfd_debug_sincosf_eval.argtypes = [C.c_int, C.c_int, _f32p, C.c_size_t, _f32p, _f32p]
        L.hrfd_debug_sincosf_digest.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), _f32p]
    L.hrfd_nco_create.argtypes = [C.c_uint32, C.c_float, C.c_float, C.c_int, C.POINTER(_vp)]
    L.hrfd_nco_destroy.argtypes = [_vp]
    L.hrfd_nco_set_frequency.argtypes = [_vp, C.c_uint32, C.c_float]
    L.hrfd_nco_reset.argtypes = [_vp, C.c_uint32]
    L.hrfd_nco_run.argtypes = [_vp, C.c_int, C.c_uint32, _vp, _vp]
    L.hrfd_ddc_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]
    L.hrfd_ddc_destroy.argtypes = [_vp]
    L.hrfd_ddc_reset.argtypes = [_vp]
    L.hrfd_ddc_set_tuning.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.hrfd_ddc_set_gain_shift.argtypes = [_vp, C.c_uint32, C.c_uint32]
    L.hrfd_ddc_set_filter.argtypes = [_vp, C.c_int, _i16p, C.c_uint32]
    L.hrfd_ddc_get_phase.argtypes = [_vp, C.c_uint32, _u32p]
    L.hrfd_ddc_process.argtypes = [_vp, _vp, C.c_uint32, _vp]
    L.hrfd_ddc_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp]
    L.hrfd_ddc_receive.argtypes = [_vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp,
                                   _u32p]
    if hasattr(L, "hrfd_ddc_set_key_block"):               # (an older build named by HRFD_LIB has no receive key)
        _u64p_key = C.POINTER(C.c_uint64)
        L.hrfd_ddc_set_key_block.argtypes = [_vp, C.c_uint32]
        L.hrfd_ddc_n_keys.argtypes = [_vp, C.c_uint32, _u32p]
        L.hrfd_ddc_get_key_skips.argtypes = [_vp, C.c_uint32, _u64p_key]
        L.hrfd_ddc_count_key_skips.argtypes = [_vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _u64p_key, _u64p_key]
        L.hrfd_ddc_process_keyed.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
        L.hrfd_ddc_process_device_keyed.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, _vp]
        L.hrfd_ddc_receive_keyed.argtypes = [_vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.c_uint32,
                                             _vp, _vp, _vp, _vp, _u32p]
    if hasattr(L, "hrfd_duc_create"):                      # (an older build named by HRFD_LIB has no DUC bank)
        L.hrfd_duc_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_duc_destroy.argtypes = [_vp]
        L.hrfd_duc_reset.argtypes = [_vp]
        L.hrfd_duc_set_tuning.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hrfd_duc_set_amplitude.argtypes = [_vp, C.c_uint32, C.c_uint32]
        L.hrfd_duc_set_output_shift.argtypes = [_vp, C.c_uint32, C.c_uint32]
        L.hrfd_duc_set_filter.argtypes = [_vp, C.c_int, _i16p, C.c_uint32]
        L.hrfd_duc_get_phase.argtypes = [_vp, C.c_uint32, _u32p]
        L.hrfd_duc_get_clips.argtypes = [_vp, C.c_uint32, C.POINTER(C.c_uint64)]
        L.hrfd_duc_process.argtypes = [_vp, _vp, C.c_uint32, _vp]
        L.hrfd_duc_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp]
        L.hrfd_duc_transmit.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp]
    if hasattr(L, "hrfd_duc_set_key_block"):               # (an older build named by HRFD_LIB has no transmit key)
        L.hrfd_duc_set_key_block.argtypes = [_vp, C.c_uint32]
        L.hrfd_duc_n_keys.argtypes = [_vp, C.c_uint32, _u32p]
        L.hrfd_duc_get_key_skips.argtypes = [_vp, C.POINTER(C.c_uint64)]
        L.hrfd_duc_process_keyed.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
        L.hrfd_duc_process_device_keyed.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, _vp]
        L.hrfd_duc_transmit_keyed.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, C.c_uint64, _vp]
    if hasattr(L, "hrfd_spec_create"):                     # (an older build named by HRFD_LIB has no spectrum bank)
        _u64p = C.POINTER(C.c_uint64)
        L.hrfd_spec_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_spec_destroy.argtypes = [_vp]
        L.hrfd_spec_set_window.argtypes = [_vp, _i16p]
        L.hrfd_spec_set_band.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
        L.hrfd_spec_clear_bands.argtypes = [_vp]
        L.hrfd_spec_n_bands.argtypes = [_vp, _u32p]
        L.hrfd_spec_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_spec_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp]
    if hasattr(L, "hrfd_cal_create"):                      # (an older build named by HRFD_LIB has no conditioner bank)
        _i64p = C.POINTER(C.c_int64)
        L.hrfd_cal_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_cal_destroy.argtypes = [_vp]
        L.hrfd_cal_set_correction.argtypes = [_vp, C.c_uint32, _i32p, _i16p]
        L.hrfd_cal_get_correction.argtypes = [_vp, C.c_uint32, _i32p, _i16p]
        L.hrfd_cal_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
        L.hrfd_cal_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, _vp]
        L.hrfd_cal_solve.argtypes = [_i64p, _i32p, _i16p]
        L.hrfd_cal_debug_set_workgroups.argtypes = [_vp, C.c_int]
    if hasattr(L, "hrfd_tone_create"):                     # (an older build named by HRFD_LIB has no tone bank)
        _u8p = C.POINTER(C.c_uint8)
        L.hrfd_tone_create.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_tone_destroy.argtypes = [_vp]
        L.hrfd_tone_set_tones.argtypes = [_vp, _u32p, _u8p, C.c_uint32]
        L.hrfd_tone_n_tones.argtypes = [_vp, _u32p]
        L.hrfd_tone_set_window.argtypes = [_vp, _i16p]
        L.hrfd_tone_set_threshold.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint64]
        L.hrfd_tone_process.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]
        L.hrfd_tone_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]
        if hasattr(L, "hrfd_tone_debug_set_max_wgs"):     # (an older build named by HRFD_LIB has none)
            L.hrfd_tone_debug_set_max_wgs.argtypes = [_vp, C.c_uint32]
    if hasattr(L, "hrfd_audio_create"):                    # (an older build named by HRFD_LIB has no audio bank)
        L.hrfd_audio_create.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_audio_destroy.argtypes = [_vp]
        L.hrfd_audio_set_taps.argtypes = [_vp, _i16p, C.c_uint32]
        L.hrfd_audio_set_bus.argtypes = [_vp, C.c_uint32, _u32p, _i16p, C.c_uint32]
        L.hrfd_audio_set_want.argtypes = [_vp, C.c_uint32, C.c_uint32]
        L.hrfd_audio_reset.argtypes = [_vp, C.c_uint32]
        L.hrfd_audio_gate.argtypes = [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp]
        L.hrfd_audio_gate_device.argtypes = [_vp, _vp, _vp, C.c_uint32, C.c_uint32, C.c_uint32, _vp, _vp]
        L.hrfd_audio_process.argtypes = [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_audio_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, _vp]
        if hasattr(L, "hrfd_audio_debug_set_max_wgs"):     # (an older build named by HRFD_LIB has none)
            L.hrfd_audio_debug_set_max_wgs.argtypes = [_vp, C.c_uint32]
    if hasattr(L, "hrfd_resamp_create"):                   # (an older build named by HRFD_LIB has no resampler bank)
        L.hrfd_resamp_create.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_resamp_destroy.argtypes = [_vp]
        L.hrfd_resamp_set_taps.argtypes = [_vp, _i16p, C.c_uint32]
        L.hrfd_resamp_reset.argtypes = [_vp, C.c_uint32]
        L.hrfd_resamp_out_count.argtypes = [_vp, C.c_uint32, _u32p]
        L.hrfd_resamp_process.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _u32p]
        L.hrfd_resamp_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, _u32p, _vp]
        if hasattr(L, "hrfd_resamp_debug_set_max_wgs"):     # (an older build named by HRFD_LIB has none)
            L.hrfd_resamp_debug_set_max_wgs.argtypes = [_vp, C.c_uint32]
    if hasattr(L, "hrfd_level_create"):                    # (an older build named by HRFD_LIB has no level bank)
        L.hrfd_level_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_level_destroy.argtypes = [_vp]
        L.hrfd_level_set_weights.argtypes = [_vp, C.POINTER(C.c_uint16), C.c_uint32]
        L.hrfd_level_set.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hrfd_level_set_bypass.argtypes = [_vp, C.c_uint32, C.c_int]
        L.hrfd_level_reset.argtypes = [_vp, C.c_uint32]
        L.hrfd_level_process.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_level_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, _vp]
    if hasattr(L, "hrfd_dcs_create"):                      # (an older build named by HRFD_LIB has no DCS bank)
        L.hrfd_dcs_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_dcs_destroy.argtypes = [_vp]
        L.hrfd_dcs_set_taps.argtypes = [_vp, _vp, C.c_uint32]
        L.hrfd_dcs_set_codes.argtypes = [_vp, _vp, _vp, _vp, C.c_uint32]
        L.hrfd_dcs_n_codes.argtypes = [_vp, _u32p]
        L.hrfd_dcs_set_min_hits.argtypes = [_vp, C.c_uint32, C.c_uint32]
        L.hrfd_dcs_reset.argtypes = [_vp, C.c_uint32]
        L.hrfd_dcs_process.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_dcs_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp, _vp]
        L.hrfd_dcs_code_word.argtypes = [C.c_uint32, C.c_int, _u32p, _u32p]
        L.hrfd_dcs_debug_slow.argtypes = [_vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp]
    if hasattr(L, "hrfd_tonegen_create"):                  # (an older build named by HRFD_LIB has no tone generator bank)
        _u64p = C.POINTER(C.c_uint64)
        L.hrfd_tonegen_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_tonegen_destroy.argtypes = [_vp]
        L.hrfd_tonegen_queue.argtypes = [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint32, C.c_uint64]
        L.hrfd_tonegen_cut.argtypes = [_vp, C.c_uint32, C.c_uint32]
        L.hrfd_tonegen_reset.argtypes = [_vp]
        L.hrfd_tonegen_set_time.argtypes = [_vp, C.c_uint64]
        L.hrfd_tonegen_time.argtypes = [_vp, _u64p]
        L.hrfd_tonegen_pending.argtypes = [_vp, C.c_uint32, C.c_uint32, _u32p, _u64p]
        L.hrfd_tonegen_get_clips.argtypes = [_vp, C.c_uint32, _u64p]
        L.hrfd_tonegen_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
        L.hrfd_tonegen_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, _vp]
    if hasattr(L, "hrfd_dcsgen_create"):                   # (an older build named by HRFD_LIB has no DCS generator bank)
        _u64p = C.POINTER(C.c_uint64)
        L.hrfd_dcsgen_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_dcsgen_destroy.argtypes = [_vp]
        L.hrfd_dcsgen_set_taps.argtypes = [_vp, _vp, C.c_uint32]
        L.hrfd_dcsgen_queue.argtypes = [_vp, C.c_uint32, _vp, C.c_uint32, C.c_uint64]
        L.hrfd_dcsgen_cut.argtypes = [_vp, C.c_uint32, C.c_int]
        L.hrfd_dcsgen_reset.argtypes = [_vp]
        L.hrfd_dcsgen_set_time.argtypes = [_vp, C.c_uint64]
        L.hrfd_dcsgen_time.argtypes = [_vp, _u64p]
        L.hrfd_dcsgen_pending.argtypes = [_vp, C.c_uint32, _u32p, _u64p]
        L.hrfd_dcsgen_get_clips.argtypes = [_vp, C.c_uint32, _u64p]
        L.hrfd_dcsgen_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
        L.hrfd_dcsgen_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, _vp]
        L.hrfd_dcsgen_debug_slow.argtypes = [_vp, C.c_uint32, _vp, C.c_uint32, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _u64p]
        L.hrfd_dcsgen_debug_edit.argtypes = [_vp, _u32p, C.c_uint64, C.c_int, _vp, C.c_uint32, C.c_uint64]
    if hasattr(L, "hrfd_afsk_create"):                     # (an older build named by HRFD_LIB has no AFSK bank)
        L.hrfd_afsk_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_afsk_destroy.argtypes = [_vp]
        L.hrfd_afsk_set_modem.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.hrfd_afsk_set_carrier.argtypes = [_vp, C.c_uint64]
        L.hrfd_afsk_reset.argtypes = [_vp, C.c_uint32]
        L.hrfd_afsk_max_bits.argtypes = [_vp, C.c_uint32, _u32p]
        L.hrfd_afsk_process.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_afsk_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint64, _vp, _vp, _vp]
        L.hrfd_afsk_debug_taps.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _i16p]
        L.hrfd_afsk_debug_slow.argtypes = [_u32p, C.c_uint64, _vp, _vp, C.c_uint32, _u32p, _vp, _vp, _vp]
    if hasattr(L, "hrfd_afskgen_create"):                  # (an older build named by HRFD_LIB has no AFSK generator bank)
        L.hrfd_afskgen_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_afskgen_destroy.argtypes = [_vp]
        L.hrfd_afskgen_queue.argtypes = [_vp, C.c_uint32, _vp, _vp, C.c_uint64]
        L.hrfd_afskgen_cut.argtypes = [_vp, C.c_uint32]
        L.hrfd_afskgen_reset.argtypes = [_vp]
        L.hrfd_afskgen_set_time.argtypes = [_vp, C.c_uint64]
        L.hrfd_afskgen_time.argtypes = [_vp, _u64p]
        L.hrfd_afskgen_pending.argtypes = [_vp, C.c_uint32, _u32p, _u64p]
        L.hrfd_afskgen_get_clips.argtypes = [_vp, C.c_uint32, _u64p]
        L.hrfd_afskgen_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp]
        L.hrfd_afskgen_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, C.c_uint64, _vp, _vp]
        L.hrfd_afskgen_debug_levels.argtypes = [_vp, C.c_uint32, C.c_int, _vp]
        L.hrfd_afskgen_debug_length.argtypes = [C.c_uint32, C.c_uint32, _u64p]
        L.hrfd_afskgen_debug_slow.argtypes = [_vp, _vp, _vp, _vp, C.c_uint32, C.c_uint64, _vp, C.c_uint32, _vp, _vp, _u64p]
    if hasattr(L, "hrfd_hdlc_create"):                     # (an older build named by HRFD_LIB has no HDLC bank)
        L.hrfd_hdlc_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_hdlc_destroy.argtypes = [_vp]
        L.hrfd_hdlc_set_limits.argtypes = [_vp, C.c_uint32, C.c_uint32]
        L.hrfd_hdlc_set_require_carrier.argtypes = [_vp, C.c_int]
        L.hrfd_hdlc_reset.argtypes = [_vp, C.c_uint32]
        L.hrfd_hdlc_max_out.argtypes = [_vp, C.c_uint32, _u32p]
        L.hrfd_hdlc_process.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_hdlc_process_device.argtypes = [_vp, _vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp]
        L.hrfd_hdlc_debug_slow.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _vp]
        L.hrfd_hdlc_debug_max_out.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, _u32p]
    if hasattr(L, "hrfd_hdlcgen_create"):                  # (an older build named by HRFD_LIB has no HDLC framer bank)
        L.hrfd_hdlcgen_create.argtypes = [C.c_uint32, C.c_int, C.POINTER(_vp)]
        L.hrfd_hdlcgen_destroy.argtypes = [_vp]
        L.hrfd_hdlcgen_set_flags.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32]
        L.hrfd_hdlcgen_max_bits.argtypes = [_vp, C.c_uint32, C.c_uint64, _u32p]
        L.hrfd_hdlcgen_process.argtypes = [_vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp, _vp]
        L.hrfd_hdlcgen_process_device.argtypes = [_vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, C.c_uint64, C.c_uint32, _vp, _vp, _vp, _vp]
        L.hrfd_hdlc_encode.argtypes = [_vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _vp, C.c_uint32, _vp, _vp, _vp]
    L.hrfd_q15_table.argtypes = [C.c_char_p, _i16p, C.c_int]
    L.hrfd_atan2_table.argtypes = [_f32p]
    L.hrfd_dbfs_table.argtypes = [_i32p]
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().hrfd_last_error().decode(errors="replace")
        raise HrfdError(f"{what} failed ({rc}): {msg}")
