// hackrfdiags_amd/csrc/hrfd_gen.h -- what the generator banks in front of the transmit chain (hrfd_tonegen, hrfd_afskgen and,
// for the limits, the output and the checks, hrfd_dcsgen) share and no HIP is needed for: the limits of a call and of the
// stream time, the law of one sample (sine index, mix, ramp, output with its saturation), and the checks of a stream time,
// of a process call and of a getter's channel.  hrfd_bank.hip holds the host part the handles embed (GenCore).  Plain C++
// like hrfd_pcm.h (tests/cpp/san_tonegen.cc, san_afskgen.cc and san_dcsgen.cc compile it on the CPU); the includer declares
// `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_pcm.h"

namespace hrfd {

constexpr uint32_t kGenBlock = kPcmBlock;
constexpr uint32_t kGenMaxBlocks = 1024;   // of one call
constexpr uint32_t kGenMaxAmp = 32767;
constexpr uint32_t kGenRamp = 64;          // samples of the ramp at either end of a segment or message
constexpr uint64_t kGenAppend = ~0ull;     // the start that means: behind what is queued
constexpr uint64_t kGenMaxTime = 1ull << 63;       // every stream time a generator computes with stays below this

// ---- 1. phase and sine: theta = step k mod 2^32 (the low 32 bits of k), i = ((theta + 2^19) >> 20) & 4095 is the tone
// bank's cosine index, and the sine is COS[(i - 1024) & 4095]: k = 0 gives COS[3072] = 0, a zero crossing
HRFD_PCM_HD uint32_t gen_cos_index(uint32_t theta) { return ((theta + (1u << 19)) >> 20) & 4095u; }
HRFD_PCM_HD uint32_t gen_sin_index(uint32_t theta) { return (gen_cos_index(theta) - 1024u) & 4095u; }

// ---- 2. mix: v = (amp_a S_a + amp_b S_b + 2^14) >> 15, the shift arithmetic.  |S| <= 32767 and amp <= 32767:
// 2 * 32767^2 + 2^14 < 2^31
HRFD_PCM_HD int32_t gen_mix(uint32_t amp_a, int32_t S_a, uint32_t amp_b, int32_t S_b)
{
  return ((int32_t)amp_a * S_a + (int32_t)amp_b * S_b + (1 << 14)) >> 15;
}

// ---- 3. ramp: e = min(k + 1, end - n, 64) and g = (v e + 32) >> 6: e = 64 gives g = v.  up = k + 1 and down = end - n,
// each already clamped to 1..64 or more by the caller (|v| <= 65534: v e < 2^23)
HRFD_PCM_HD int32_t gen_ramp(int32_t v, uint32_t up, uint32_t down)
{
  uint32_t e = up < down ? up : down;
  e = e < kGenRamp ? e : kGenRamp;
  return (v * (int32_t)e + 32) >> 6;
}

// ---- 4. output: y = sat16(x + g), g the sum of what sounds; |g| <= 2 * 65534.  *clipped: the saturation changed the value
HRFD_PCM_HD int32_t gen_output(int32_t x, int32_t g, bool *clipped)
{
  const int32_t sum = x + g, y = pcm_sat16(sum);
  *clipped = y != sum;
  return y;
}

// ---- the checks, each under `who`, the public function's name
inline int gen_check_time(const char *who, uint64_t N)
{
  if (N >= kGenMaxTime)
  {
    return fail(HRFD_EINVAL, "%s: stream time %llu (below 2^63)", who, (unsigned long long)N);
  }
  return HRFD_OK;
}

// the channel of a getter (get_clips, pending) against the handle's count.  In front of it, and of the handle, the getter
// refuses a channel of 65536 and more and a missing result pointer under a text of its own
inline int gen_check_one_channel(const char *who, uint32_t channel, uint32_t n_channels)
{
  if (channel >= n_channels)
  {
    return fail(HRFD_EINVAL, "%s: channel %u (0..%u)", who, channel, n_channels - 1);
  }
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle; n_channels: the handle's, or 1 where there is none
// yet (the ranges that must not overlap grow with it).  The dense host entry has no strides.  pcm may be NULL: generate only
inline int gen_check_call(const char *who, const void *pcm, uint64_t in_stride, bool device_entry, uint32_t n_blocks,
                          const void *out, uint64_t out_stride, uint32_t n_channels)
{
  if (n_blocks == 0 || n_blocks > kGenMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kGenMaxBlocks, n_blocks);
  }
  if (out == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument (out)", who);
  }
  const uint64_t row = 2ull * kGenBlock * n_blocks;
  if (device_entry)
  {
    if (pcm != nullptr)
    {
      BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", in_stride, row));
    }
    BANK_TRY(pcm_check_stride(who, "out_stride_bytes", out_stride, row));
  }
  if (!pcm_aligned(pcm, 2) || !pcm_aligned(out, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM and out must sit at even addresses", who);
  }
  const uint64_t si = device_entry ? in_stride : row, so = device_entry ? out_stride : row;
  if (pcm != nullptr && !(out == pcm && si == so))
  {
    return pcm_check_no_overlap(who, pcm, si, row, out, so, row, n_channels,
                                "in place means out at the input's own address and stride, where every sample is read by the "
                                "lane that overwrites it; anywhere else a workgroup would overwrite what another still reads");
  }
  return HRFD_OK;
}

} // namespace hrfd
