/* include/hrfd_debug.h -- the hrfd_*_debug_* entry points of libhrfd.so: NOT part of the drop-in boundary
 * (include/hrfd.h is; nothing here stands in for an interface of the reference).  They exist for the repository's
 * own tests, tools and bench.py.  Two kinds:
 *
 *   read-only introspection / measurement -- always available
 *   behaviour-changing test hooks         -- INERT unless the process was started with HRFD_DEBUG_HOOKS=1 in its
 *                                            environment (read once, at the first such call): without it they return
 *                                            HRFD_ESTATE and change nothing.  tests/conftest.py sets it; a host
 *                                            application never does, so nothing can switch the shipped library onto its
 *                                            forced-failure and fallback paths at run time.
 */
#ifndef HRFD_DEBUG_H
#define HRFD_DEBUG_H

#include "hrfd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ read-only introspection / measurement */
/* {launches, ..., [4] tiles repaired in place, [5] launches with uncommitted channels, [6] launches} of the handle */
int hrfd_rx_debug_counters(hrfd_rx *h, uint32_t *out8);
/* bracket the demodulator kernels of every launch with HIP events on the launch stream (`slots` pairs, round robin);
 * after a sync hrfd_rx_debug_kernel_ms(slot) is that launch's time: bench.py's roofline.achieved */
int hrfd_rx_debug_enable_timing(hrfd_rx *h, int slots);
int hrfd_rx_debug_kernel_ms(hrfd_rx *h, int slot, float *ms);
/* bracket only every n-th launch (an event record costs ~3 us of queue time: bracketing every launch of a back-to-back
 * sequence puts a gap between kernels that a host which does not measure never sees) */
int hrfd_rx_debug_timing_every(hrfd_rx *h, int n);
/* the device's atan2 (arithmetic form / first-octant-table form) for all 65536 (q, i): must equal hrfd_atan2_table() */
int hrfd_rx_debug_atan_eval(hrfd_rx *h, float *out65536);
int hrfd_rx_debug_atan_eval_tab(hrfd_rx *h, float *out65536);
int hrfd_rx_debug_atan_eval_quad(hrfd_rx *h, float *out65536);   /* first-quadrant table (the re-split WBFM flow kernel) */
/* host only: that table as hrfd_rx_create builds it (16644 words) and the verdict of its proof against hrfd_atan2_table() */
int hrfd_debug_atan2_quadrant(uint32_t *out16644, int *ok);
/* per-workgroup cycle stamps of k_rx_wbfm (probe builds); the cross-block check values of the latest launch */
int hrfd_rx_debug_stamps(hrfd_rx *h, uint32_t cap_groups, unsigned long long *host_out);
int hrfd_rx_debug_chk(hrfd_rx *h, float *pub, float *spec, uint32_t n);
/* *offgrid: the handle was given a block that is not a whole number of PCM samples (512 bytes; inner API 64) and keeps
 * its state in RagState since; *launches: launches so far that ran on k_rx_ragged (hrfd_rx_ragged.hip) */
int hrfd_rx_debug_ragged(hrfd_rx *h, int *offgrid, unsigned long long *launches);
/* *launches: launches so far that ran on the WBFM flow kernel's instantiation without the squelch magnitude (no magnitude
 * buffer was passed and no gate of the bank could close: hrfd.h at `magnitude`) */
int hrfd_rx_debug_mag_skipped(hrfd_rx *h, unsigned long long *launches);

/* the device's restatement of glibc's sinf / cosf (hrfd_tx_kernels.hip: glibc_sincosf*), evaluated on the current
 * device; host pointers.  variant 0 / 1: without / with fused multiply-adds -- selects the template, not what the host's
 * libm was probed to be (hrfd_libm_variant()); form 0: the pair function every product caller uses, 1: the one-sided
 * sinf and cosf called separately.
 *   eval  : sn[i], cs[i] = sin, cos of x[i], n in 1 .. 2^28.
 *   digest: a chunk is 2^20 consecutive float bit patterns u (chunk k: u >> 20 == k); out[k] = the wrapping 64-bit sum
 *           over chunk first_chunk + k of mix(u, bits(sin), bits(cos)), mix(u, s, c) = splitmix64's finaliser of
 *           ((s << 32) | c) + u * 0x9E3779B97F4A7C15 -- the same sum oracle/hrfd_oracle.c makes of the host's libm and of
 *           the restatement in C (orc_sincosf_digest).  The restated range |x| < 120 is chunks 0 .. 1070 and
 *           2048 .. 3118; chunk ranges that leave 0 .. 4095 are refused (HRFD_EINVAL).  *kernel_ms (may be NULL): the
 *           kernel's time.  tests/test_gpu_sincos.py: every float of the range, both variants, both forms. */
int hrfd_debug_sincosf_eval(int variant, int form, const float *x, size_t n, float *sn, float *cs);
int hrfd_debug_sincosf_digest(int variant, int form, uint32_t first_chunk, uint32_t n_chunks, uint64_t *out, float *kernel_ms);

/* two plain stream kernels -- kind 0 reads `bytes` of d_buf (d_sink: one dword that is never written, may be NULL),
 * kind 1 overwrites them; bytes a multiple of 256 KiB; asynchronous on `stream`.  bench.py times them in the same run
 * as the measured denominators beside the 8 TB/s spec peak (`measured_stream_read_GBps` / `_write_GBps`). */
int hrfd_debug_membw(int kind, void *d_buf, size_t bytes, void *d_sink, void *stream);

/* the AFSK bank's laws as the host states them (hrfd_afsk.h), no device needed; host pointers.
 *   taps: out128 = [4][32] int16: the mark tone's cosine and sine taps, then the space tone's, zero from `window` on.
 *   slow: the contract's loop over ONE channel.  modem6 = {mark_step, space_step, baud_step, window, loop_shift, nrzi};
 *         pcm [n_blocks][512], n_pcm [n_blocks] or NULL; state18: the channel's 18 dwords (16 of sample pairs, phi, then
 *         h[n-1] in bit 0 and last in bit 1), zero for a fresh channel, read and replaced; bits (at least
 *         hrfd_afsk_max_bits bytes) with n_bits (one count), and hard [n_blocks][64], as hrfd_afsk_process takes them.
 * tests/test_afsk_model.py holds tests/afsk_model.py against both. */
int hrfd_afsk_debug_taps(uint32_t mark_step, uint32_t space_step, uint32_t window, int16_t *out128);
int hrfd_afsk_debug_slow(const uint32_t *modem6, uint64_t min_power, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks,
                         uint32_t *state18, uint8_t *bits, uint32_t *n_bits, uint8_t *hard);

/* the AFSK generator bank's laws as the host states them (hrfd_afskgen.h), no device needed; host pointers.
 *   levels: bits [n_bits] (1..8192, bit 0 of every byte) -> words [(n_bits + 31) / 32]: bit i & 31 of word i >> 5 = l[i].
 *   length: L of n_bits (any above 0: the law, not the queue's limit) at baud_step, or the refusal of L >= 2^31.
 *   slow:   the contract's loop over ONE channel and one call.  msgs [n_msgs] (at most 4) with their bits one behind the
 *           other in `bits`; message j begins at starts[j] + msgs[j].gap and ends at its E, or at ends[j] where ends is
 *           given and ends[j] lies in front of E (a cut message).  N: the stream time of the call's first sample; pcm
 *           [n_blocks][512] or NULL; out [n_blocks][512] (may be pcm), active [n_blocks] or NULL, *clips (may be NULL) as
 *           hrfd_afskgen_process gives them.  Overlapping messages are refused.
 * tests/test_afskgen_model.py holds tests/afskgen_model.py against all three. */
int hrfd_afskgen_debug_levels(const uint8_t *bits, uint32_t n_bits, int nrzi, uint32_t *words);
int hrfd_afskgen_debug_length(uint32_t n_bits, uint32_t baud_step, uint64_t *length);
int hrfd_afskgen_debug_slow(const hrfd_afskgen_message *msgs, const uint8_t *bits, const uint64_t *starts, const uint64_t *ends,
                            uint32_t n_msgs, uint64_t N, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active,
                            uint64_t *clips);

/* the HDLC bank's law as the host states it (hrfd_hdlc.h), no device needed; host pointers.
 *   slow:    the contract's loop over ONE channel and one call.  limits3 = {min_payload, max_payload, require_carrier}; bits
 *            [n_bits] (0..2^20; may be NULL for 0); state260: the channel's 260 dwords (ones, in_frame, n, 0, the partial
 *            frame), zero for a fresh channel, read and replaced; out [out_bytes] and counts3 = {n_frames, n_bad, dropped} as
 *            hrfd_hdlc_process gives them for the channel.
 *   max_out: hrfd_hdlc_max_out for limits given by value.
 * tests/test_hdlc_model.py holds tests/hdlc_model.py against both. */
int hrfd_hdlc_debug_slow(const uint32_t *limits3, const uint8_t *bits, uint32_t n_bits, uint32_t *state260, uint8_t *out,
                         uint32_t out_bytes, uint32_t *counts3);
int hrfd_hdlc_debug_max_out(uint32_t max_bits, uint32_t min_payload, uint32_t max_payload, uint32_t *out_bytes);

/* the DCS bank's law as the host states it (hrfd_dcs.h), no device needed; host pointers.
 *   slow: the contract's loop over ONE channel and one call.  taps [n_taps]; codes, inverted, groups [n_codes] as
 *         hrfd_dcs_set_codes takes them (an alias is refused alike); min_hits4: one per group; pcm [n_blocks][512], n_pcm
 *         [n_blocks] or NULL; state300: the channel's 300 dwords (256 of sample pairs, the oldest first; 41 of slicer bits, the
 *         oldest in bit 0 of the first; 3 of zeros), zero for a fresh channel, read and replaced; hits [n_blocks][n_codes],
 *         best and present [n_blocks][4] as hrfd_dcs_process gives them for the channel, each or NULL but not all.
 * tests/test_dcs_model.py holds tests/dcs_model.py against it. */
int hrfd_dcs_debug_slow(const int16_t *taps, uint32_t n_taps, const uint16_t *codes, const uint8_t *inverted, const uint8_t *groups,
                        uint32_t n_codes, const uint32_t *min_hits4, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks,
                        uint32_t *state300, uint16_t *hits, uint8_t *best, uint8_t *present);

/* the DCS generator bank's law and queue rules as the host states them (hrfd_dcsgen.h), no device needed; host pointers.  A
 * queue is one channel's, at most 8 rows of six uint64 {S, S + L, E, word, amp, tail} in order of their starts, UINT64_MAX for
 * the S + L and E of a FOREVER segment.
 *   slow: the contract's loop over ONE channel and one call.  taps [n_taps]; N: the stream time of the call's first sample;
 *         pcm [n_blocks][512] or NULL; out [n_blocks][512] (may be pcm), active [n_blocks] or NULL, *clips (may be NULL) as
 *         hrfd_dcsgen_process gives them.
 *   edit: one edit at the clock N, the queue read and replaced (room for 8 rows): op 0 = hrfd_dcsgen_queue of segs [n] at
 *         start = arg, with its refusals; 1 = hrfd_dcsgen_cut with with_tail = arg; 2 = what a call does first: the segments
 *         that have ended leave.
 * tests/test_dcsgen_model.py holds tests/dcsgen_model.py against both. */
int hrfd_dcsgen_debug_slow(const int16_t *taps, uint32_t n_taps, const uint64_t *queue6, uint32_t n_queue, uint64_t N,
                           const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active, uint64_t *clips);
int hrfd_dcsgen_debug_edit(uint64_t *queue6, uint32_t *n_queue, uint64_t N, int op, const hrfd_dcsgen_segment *segs, uint32_t n,
                           uint64_t arg);

/* ------------------------------------------------------------------ behaviour-changing hooks (HRFD_DEBUG_HOOKS=1) */
int hrfd_rx_debug_set_atan(hrfd_rx *h, int mode);        /* -1 automatic, 0 table gather, 1 arithmetic */
int hrfd_rx_debug_set_warm(hrfd_rx *h, int warm);        /* shrink the de-emphasis warm-up, seeds off: forces repairs */
int hrfd_rx_debug_set_run_len(hrfd_rx *h, int blocks);   /* blocks per k_rx_wbfm workgroup */
int hrfd_rx_debug_set_stream(hrfd_rx *h, int on);        /* 0: WBFM batches on the block kernel */
int hrfd_rx_debug_expire(hrfd_rx *h, int where);         /* expire a bounded wait / hold a wave up, once */
int hrfd_rx_debug_set_fir_flow(hrfd_rx *h, int mode);    /* FIR modes: -1 automatic, 0 block kernels, 1 flow, 2 per kind */
int hrfd_rx_debug_set_gated(hrfd_rx *h, int on);         /* 0: no gated pass on the device (host replay instead) */
int hrfd_rx_debug_set_stagger(hrfd_rx *h, int units);
int hrfd_mod_debug_set_sliced(hrfd_mod *h, int on);      /* WBFM modulator: 0 unsliced, 1 automatic, 2 always sliced */
int hrfd_mod_debug_set_scan(hrfd_mod *h, int kind);      /* FM / WBFM modulators: the phase recurrence on 0 = k_phase_rows8 / k_phase_rows, 1 = k_phase_scan<64>, 2 = k_phase_rows */
int hrfd_mod_debug_set_tail(hrfd_mod *h, int kind);      /* WBFM modulator: 0 = k_wb_rails + k_mod<WB_TAIL> (rounds 2-5), 1 = k_wb_tail (one pass) */
int hrfd_cal_debug_set_workgroups(hrfd_cal *c, int wgs); /* conditioner: workgroups a launch aims for, 1 .. 65536 (2048 unless set); 1 = one per capture */
/* tone, audio and resampler banks: the workgroups of one launch of k_tone / k_audio_fir / k_resamp, 1 .. 2^22 (2^22 unless
 * set).  A call that needs more is cut into several launches, so a small n runs a small call the way a call of more than
 * 2^22 workgroups runs (tests/test_gpu_chunked_launch.py) */
int hrfd_tone_debug_set_max_wgs(hrfd_tone *t, uint32_t n);
int hrfd_audio_debug_set_max_wgs(hrfd_audio *a, uint32_t n);
int hrfd_resamp_debug_set_max_wgs(hrfd_resamp *r, uint32_t n);

#ifdef __cplusplus
}
#endif

#endif /* HRFD_DEBUG_H */
