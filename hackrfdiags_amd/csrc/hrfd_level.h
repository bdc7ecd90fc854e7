// hackrfdiags_amd/csrc/hrfd_level.h -- what the level bank (hrfd_level_*) needs no HIP for: the limits, the five laws (frame
// peak, envelope, gain, sample gain, output), the argument checks, and a slow loop over one channel that restates the
// contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_audio.h (tests/cpp/san_level.cc compiles it on the CPU;
// hrfd_level.hip includes it for the host side and the kernel); the includer declares `int fail(int code, const char *fmt,
// ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_pcm.h"

#define HRFD_LEVEL_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kLevelBlock = kPcmBlock;
constexpr uint32_t kLevelFrame = 64;           // samples of one frame: one peak, one gain
constexpr uint32_t kLevelFramesPerBlock = kLevelBlock / kLevelFrame;      // 8
constexpr uint32_t kLevelMaxWeights = 64;      // W
constexpr uint32_t kLevelHist = 64;            // peaks kept per channel, whatever W is
constexpr uint32_t kLevelMaxBlocks = 1024;
constexpr uint32_t kLevelUnity = 32768;        // w[0], and the largest weight
constexpr uint32_t kLevelMaxTarget = 32767;
constexpr uint32_t kLevelMinFloor = 16;
constexpr uint32_t kLevelMaxFloor = 32768;
constexpr uint32_t kLevelDefaultTarget = 8192;
constexpr uint32_t kLevelDefaultFloor = 64;
constexpr uint32_t kLevelDefaultHang = 8;      // frames the default table holds at unity
static_assert(kLevelHist >= kLevelMaxWeights, "g[f-1] of a call's first frame reads the peaks of frames f-1 .. f-W");

// one channel's settings as the kernel reads them (8 bytes): the target below, the bypass flag in bit 16; the floor
struct LevelSetting
{
  uint32_t word;
  uint32_t floor;
};
HRFD_LEVEL_HD uint32_t level_pack_word(uint32_t target, bool bypass) { return target | (bypass ? 1u << 16 : 0u); }
HRFD_LEVEL_HD uint32_t level_word_target(uint32_t word) { return word & 0xffffu; }
HRFD_LEVEL_HD bool level_word_bypass(uint32_t word) { return (word >> 16) != 0; }

// ---- 1. peak: p[f] = max |x| over the frame, 0..32768.  |-32768| = 32768 does not fit an int16: the absolute value is
// taken in 32 bits
HRFD_LEVEL_HD uint32_t level_abs(int32_t x) { return (uint32_t)(x < 0 ? -x : x); }

// ---- 2. envelope: E[f] = max(floor, max_k ((p[f-k] w[k] + 2^14) >> 15)), k = 0..W-1.  p, w <= 32768: the product is at
// most 2^30.  w[0] = 32768 gives (p[f] 2^15 + 2^14) >> 15 = p[f], so E[f] >= p[f]
HRFD_LEVEL_HD uint32_t level_weighted(uint32_t p, uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (__umul24(p, w) + (1u << 14)) >> 15;              // both factors fit 24 bits, the product 32
#else
  return (p * w + (1u << 14)) >> 15;
#endif
}

// p_at_f points at p[f] in an array that holds p[f - W + 1 .. f]
HRFD_LEVEL_HD uint32_t level_envelope(const uint16_t *p_at_f, const uint16_t *w, uint32_t W, uint32_t floor)
{
  uint32_t e = floor;
  for (uint32_t k = 0; k < W; k++)
  {
    const uint32_t v = level_weighted(p_at_f[-(int32_t)k], w[k]);
    e = v > e ? v : e;
  }
  return e;
}

// ---- 3. gain: g[f] = (target << 12) / E[f], unsigned floor division, Q12.  target <= 32767 and E >= floor >= 16:
// g <= (32767 << 12) / 16 = 8388352 < 2^23
HRFD_LEVEL_HD uint32_t level_gain(uint32_t target, uint32_t E) { return (target << 12) / E; }

// ---- 4. sample gain of sample n = 0..63 of a frame with gain g behind a frame with gain g_prev: attack at the frame
// boundary, release ramped over the frame.  g_prev <= gs <= g on the ramp ((g - g_prev) (n + 1) < 2^23 x 64 = 2^29), gs = g
// otherwise: gs <= g always
HRFD_LEVEL_HD uint32_t level_sample_gain(uint32_t g_prev, uint32_t g, uint32_t n)
{
  return g <= g_prev ? g : g_prev + (((g - g_prev) * (n + 1)) >> 6);
}

// ---- 5. output: y = (x gs + 2^11) >> 12, the shift arithmetic.
// Proof of |y| <= target, for every x of frame f:
//   |x| <= p[f]                      rule 1
//   p[f] <= E[f]                     rule 2 with w[0] = 32768
//   gs <= g[f]                       rule 4
//   g[f] E[f] <= target << 12        rule 3, a floor division
// so |x gs| <= p[f] g[f] <= E[f] g[f] <= target << 12 < 2^27: the product fits an int32, and both factors fit 24 bits
// (|x| <= 2^15, gs < 2^23), so a 24-bit multiply gives it whole.  Then
//   y <= ((target << 12) + 2^11) >> 12 = target         (2^11 < 2^12)
//   y >= (-(target << 12) + 2^11) >> 12 = -target       (the floor of -target + 1/2)
// No saturation, no clip counter, nothing to tune; target <= 32767 keeps y an int16
HRFD_LEVEL_HD int32_t level_output(int32_t x, uint32_t gs)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (__mul24(x, (int32_t)gs) + (1 << 11)) >> 12;
#else
  return (x * (int32_t)gs + (1 << 11)) >> 12;
#endif
}

// the table of a new handle: 8 frames (64 ms) at unity, then linear to the end of the 64 frames (512 ms)
inline void level_default_weights(uint16_t *w)
{
  for (uint32_t k = 0; k < kLevelMaxWeights; k++)
  {
    w[k] = (uint16_t)(k < kLevelDefaultHang ? kLevelUnity
                                             : (kLevelUnity * (kLevelMaxWeights - k)) / (kLevelMaxWeights - kLevelDefaultHang));
  }
}

// ---- one channel, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512]; n_pcm_row: its [n_blocks] or NULL; w: W weights; hist: the last 64 peaks in time
// order (hist[63] is the newest), read and replaced; out [n_blocks][512], gain and peak [8 n_blocks], each or NULL.  out may
// be pcm_row itself
inline void level_channel_slow(const int16_t *pcm_row, const uint32_t *n_pcm_row, uint32_t n_blocks, const uint16_t *w, uint32_t W,
                               uint32_t target, uint32_t floor, bool bypass, uint16_t *hist, int16_t *out, uint32_t *gain,
                               uint16_t *peak)
{
  uint16_t p[kLevelHist + 1];                  // the 64 frames before, then the frame at hand
  for (uint32_t i = 0; i < kLevelHist; i++)
  {
    p[i] = hist[i];
  }
  // g of the frame in front of the call, from the 64 peaks in front of the call under this call's settings
  uint32_t g_prev = level_gain(target, level_envelope(p + kLevelHist - 1, w, W, floor));
  for (uint32_t f = 0; f < kLevelFramesPerBlock * n_blocks; f++)
  {
    const uint32_t b = f / kLevelFramesPerBlock, lim = pcm_block_limit(n_pcm_row, b);
    int32_t x[kLevelFrame];
    uint32_t pf = 0;
    for (uint32_t n = 0; n < kLevelFrame; n++)
    {
      const uint32_t pos = (f % kLevelFramesPerBlock) * kLevelFrame + n;
      x[n] = pos < lim ? pcm_row[(size_t)f * kLevelFrame + n] : 0;
      const uint32_t a = level_abs(x[n]);
      pf = a > pf ? a : pf;
    }
    // the window slides by one frame: p[0 .. 63] the frames before, p[64] this one
    p[kLevelHist] = (uint16_t)pf;
    const uint32_t g = level_gain(target, level_envelope(p + kLevelHist, w, W, floor));
    if (gain != nullptr)
    {
      gain[f] = g;
    }
    if (peak != nullptr)
    {
      peak[f] = (uint16_t)pf;
    }
    if (out != nullptr)
    {
      for (uint32_t n = 0; n < kLevelFrame; n++)
      {
        out[(size_t)f * kLevelFrame + n] = (int16_t)(bypass ? x[n] : level_output(x[n], level_sample_gain(g_prev, g, n)));
      }
    }
    g_prev = g;
    for (uint32_t i = 0; i < kLevelHist; i++)
    {
      p[i] = p[i + 1];
    }
  }
  for (uint32_t i = 0; i < kLevelHist; i++)
  {
    hist[i] = p[i];
  }
}

// ---- the checks, each under `who`, the public function's name
inline int level_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

// W = 1..64, w[0] = 32768 (E >= p rests on it), every w[k] <= 32768
inline int level_check_weights(const char *who, const uint16_t *w, uint32_t n)
{
  if (n == 0 || n > kLevelMaxWeights || w == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u weights and their array (got %u)", who, kLevelMaxWeights, n);
  }
  if (w[0] != kLevelUnity)
  {
    return fail(HRFD_EINVAL, "%s: w[0] must be 32768 (got %u): the envelope of a frame is never below its own peak", who, w[0]);
  }
  for (uint32_t k = 1; k < n; k++)
  {
    if (w[k] > kLevelUnity)
    {
      return fail(HRFD_EINVAL, "%s: w[%u] = %u is above 32768", who, k, w[k]);
    }
  }
  return HRFD_OK;
}

// n_channels: the handle's, or the largest any handle has where there is none yet
inline int level_check_set(const char *who, uint32_t channel, uint32_t target, uint32_t floor, uint32_t n_channels)
{
  if (target > kLevelMaxTarget)
  {
    return fail(HRFD_EINVAL, "%s: target %u (0..%u)", who, target, kLevelMaxTarget);
  }
  if (floor < kLevelMinFloor || floor > kLevelMaxFloor)
  {
    return fail(HRFD_EINVAL, "%s: floor %u (%u..%u)", who, floor, kLevelMinFloor, kLevelMaxFloor);
  }
  return pcm_check_channel(who, channel, n_channels);
}

// what a process call's sizes and addresses decide without a handle; n_channels: the handle's, or 1 where there is none
// yet (the ranges that must not overlap grow with it).  The dense host entry has no strides.
inline int level_check_call(const char *who, const void *pcm, uint64_t in_stride, bool device_entry, const void *n_pcm,
                            uint32_t n_blocks, const void *out, uint64_t out_stride, const void *gain, const void *peak,
                            uint32_t n_channels)
{
  if (n_blocks == 0 || n_blocks > kLevelMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kLevelMaxBlocks, n_blocks);
  }
  if (out == nullptr && gain == nullptr && peak == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: no output asked for (out, gain and peak are all NULL)", who);
  }
  const uint64_t row = 2ull * kLevelBlock * n_blocks;
  if (device_entry)
  {
    BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", in_stride, row));
    if (out != nullptr)
    {
      BANK_TRY(pcm_check_stride(who, "out_stride_bytes", out_stride, row));
    }
  }
  if (!pcm_aligned(pcm, 2) || !pcm_aligned(out, 2) || !pcm_aligned(peak, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM, out and peak must sit at even addresses", who);
  }
  if (!pcm_aligned(n_pcm, 4) || !pcm_aligned(gain, 4))
  {
    return fail(HRFD_EINVAL, "%s: n_pcm and gain must be 4-byte aligned", who);
  }
  if (pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  const uint64_t si = device_entry ? in_stride : row, so = device_entry ? out_stride : row;
  if (out != nullptr && !(out == pcm && si == so))
  {
    return pcm_check_no_overlap(who, pcm, si, row, out, so, row, n_channels,
                                "in place means out at the input's own address and stride, where every sample is read by the "
                                "lane that overwrites it; anywhere else a workgroup would overwrite what another still reads");
  }
  return HRFD_OK;
}

} // namespace hrfd
