// hackrfdiags_amd/csrc/hrfd_pcm.h -- the PCM contract of the banks behind the receive chain (hrfd_tone, hrfd_audio,
// hrfd_resamp, hrfd_level, hrfd_afsk, and hrfd_hdlc behind that) and in front of the transmit chain (hrfd_tonegen, hrfd_afskgen), in one place: rows of int16 at an even address, an even stride apart, in blocks of 512 samples of
// which an optional n_pcm says how many count; the rounding of a FIR over them; the argument checks the banks share; and,
// for the kernels, the access to 8 consecutive samples of a row (pcm_load8, pcm_store8).
// Plain C++ like hrfd_bank.h (tests/cpp/san_pcm.cc compiles it on the CPU); the includer declares
// `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_bank.h"

#define HRFD_PCM_HD HRFD_BANK_HD

namespace hrfd {

constexpr uint32_t kPcmBlock = 512;        // PCM samples per block row

// samples a block gives: min(n_pcm, 512), every block whole when there is no n_pcm.  n_pcm_row: the channel's row or NULL
HRFD_PCM_HD uint32_t pcm_block_limit(const uint32_t *n_pcm_row, uint32_t block)
{
  if (n_pcm_row == nullptr)
  {
    return kPcmBlock;
  }
  const uint32_t v = n_pcm_row[block];
  return v < kPcmBlock ? v : kPcmBlock;
}

HRFD_PCM_HD int32_t pcm_sat16(int64_t v) { return (int32_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

// y = sat16((acc + 2^13) >> 14).  Taps with sum |h| <= 65535 (bank_tap_sums_ok) and |x| <= 32768 give |acc| <= 65535 *
// 32768 = 2^31 - 2^15 < 2^31 - 2^14, so acc + 2^13 stays inside int32 as every partial sum does
HRFD_PCM_HD int32_t pcm_fir_round(int32_t acc) { return pcm_sat16((int64_t)((acc + (1 << 13)) >> 14)); }

#if defined(__HIPCC__)
// 8 consecutive samples of a row, the 16 bytes one lane of k_level, k_afsk, k_tonegen and k_afskgen loads and stores: rows at
// any even address and stride take one path through a vector type of alignment 2
typedef uint32_t pcm_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t pcm_u4_any __attribute__((ext_vector_type(4), aligned(2)));
__device__ __forceinline__ pcm_u4 pcm_load8(const int16_t *src) { return *(const pcm_u4_any *)src; }
__device__ __forceinline__ void pcm_store8(int16_t *dst, pcm_u4 v) { *(pcm_u4_any *)dst = v; }
#endif

// ---- the shared checks, each under `who`, the public function's name
inline int pcm_check_channels(const char *who, uint32_t n_channels, const void *out)
{
  if (out == nullptr || n_channels == 0 || n_channels > 65536)
  {
    return fail(HRFD_EINVAL, "%s: need 1..65536 channels and a result pointer (got %u)", who, n_channels);
  }
  return HRFD_OK;
}

inline int pcm_check_channel(const char *who, uint32_t channel, uint32_t n_channels)
{
  if (channel >= n_channels && channel != HRFD_ALL_CHANNELS)
  {
    return fail(HRFD_EINVAL, "%s: channel %u (0..%u or HRFD_ALL_CHANNELS)", who, channel, n_channels - 1);
  }
  return HRFD_OK;
}

// the tone bank's frame length, which the audio bank's gate is told
inline int pcm_check_frame_len(const char *who, uint32_t L)
{
  if (L < 128 || L > 8192 || (L & (L - 1)) != 0)
  {
    return fail(HRFD_EINVAL, "%s: frame_len must be a power of two, 128..8192 (got %u)", who, L);
  }
  return HRFD_OK;
}

// L has passed pcm_check_frame_len
inline int pcm_check_frames(const char *who, uint32_t n_blocks, uint32_t L)
{
  if ((kPcmBlock * n_blocks) % L != 0)
  {
    return fail(HRFD_EINVAL, "%s: %u blocks of 512 samples are no whole number of frames of %u", who, n_blocks, L);
  }
  return HRFD_OK;
}

// rows `stride` bytes apart, each row_bytes long; `name` is the parameter's, `note` what the text adds behind the bound
inline int pcm_check_stride(const char *who, const char *name, uint64_t stride, uint64_t row_bytes, const char *note = "")
{
  if ((stride & 1u) != 0 || stride < row_bytes)
  {
    return fail(HRFD_EINVAL, "%s: %s %llu must be even and >= %llu%s", who, name, (unsigned long long)stride,
                (unsigned long long)row_bytes, note);
  }
  return HRFD_OK;
}

// align: 2 (PCM), 4 (n_pcm and other dword arrays) or 8; NULL is aligned
inline bool pcm_aligned(const void *p, uintptr_t align) { return ((uintptr_t)p & (align - 1)) == 0; }

// n_channels input rows of in_row bytes, in_stride apart, against as many output rows: ranges that touch are fine.  `why`
// is the bank's reason
inline int pcm_check_no_overlap(const char *who, const void *in, uint64_t in_stride, uint64_t in_row, const void *out,
                                uint64_t out_stride, uint64_t out_row, uint32_t n_channels, const char *why)
{
  const uint64_t a0 = (uint64_t)(uintptr_t)in, a1 = a0 + (n_channels - 1) * in_stride + in_row;
  const uint64_t b0 = (uint64_t)(uintptr_t)out, b1 = b0 + (n_channels - 1) * out_stride + out_row;
  if (a0 < b1 && b0 < a1)
  {
    return fail(HRFD_EINVAL, "%s: out overlaps the input (%s)", who, why);
  }
  return HRFD_OK;
}

} // namespace hrfd
