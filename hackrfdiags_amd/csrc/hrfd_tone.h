// hackrfdiags_amd/csrc/hrfd_tone.h -- what the tone bank (hrfd_tone_*) needs no HIP for: the argument checks, the per-sample
// law (window product, phase to table index), the rounding of the sums, the frame's valid count, the group verdict, and a
// slow loop over one frame that restates the contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_bank.h
// (tests/cpp/san_tone.cc compiles it on the CPU; hrfd_tone.hip includes it for the host side and the kernels); the
// includer declares `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_pcm.h"

#define HRFD_TONE_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kToneBlock = kPcmBlock;
constexpr uint32_t kToneGroups = 4;
constexpr uint32_t kToneMaxTones = 128;
constexpr uint32_t kToneNoBest = 255;

// ---- the per-sample law
// u = (x w + 2^14) >> 15: |w| <= 32767, so |u| <= 32767
HRFD_TONE_HD int32_t tone_window(int32_t x, int32_t w) { return (x * w + (1 << 14)) >> 15; }

// the DDC's mixer index of a phase; the sine sits a quarter turn behind the cosine in the same table
HRFD_TONE_HD uint32_t tone_cos_index(uint32_t theta) { return ((theta + (1u << 19)) >> 20) & 4095u; }
HRFD_TONE_HD uint32_t tone_sin_index(uint32_t cos_index) { return (cos_index - 1024u) & 4095u; }

// I' = (I + 2^14) >> 15 (arithmetic), |I| < 2^43 so |I'| <= 2^28; P = I'^2 + Q'^2 < 2^57
HRFD_TONE_HD int64_t tone_round15(int64_t v) { return (v + (1 << 14)) >> 15; }
HRFD_TONE_HD uint64_t tone_power(int64_t I, int64_t Q)
{
  const int64_t i = tone_round15(I), q = tone_round15(Q);
  return (uint64_t)(i * i) + (uint64_t)(q * q);
}

// valid[c][f]: the samples of frame f (L samples from sample f L of the channel) below their block's limit.
// n_pcm_row: the channel's [n_blocks] or NULL
HRFD_TONE_HD uint32_t tone_frame_valid(const uint32_t *n_pcm_row, uint32_t frame, uint32_t L)
{
  if (L >= kToneBlock)
  {
    uint32_t v = 0;
    const uint32_t per = L / kToneBlock;
    for (uint32_t b = 0; b < per; b++)
    {
      v += pcm_block_limit(n_pcm_row, frame * per + b);
    }
    return v;
  }
  const uint32_t per = kToneBlock / L, pos = (frame % per) * L, lim = pcm_block_limit(n_pcm_row, frame / per);
  return lim <= pos ? 0u : (lim - pos < L ? lim - pos : L);
}

// ---- the verdict: E < 2^43 and T <= 2^20, so E T stays inside uint64
HRFD_TONE_HD bool tone_present(uint32_t valid, uint32_t L, uint64_t E, uint64_t E_min, uint64_t P_best, uint32_t T)
{
  return valid == L && E >= E_min && P_best >= ((E * (uint64_t)T) >> 8);
}

// the lowest index among group g's tones with the largest power, kToneNoBest for a group without tones
HRFD_TONE_HD uint32_t tone_best(const uint64_t *P, const uint8_t *groups, uint32_t K, uint32_t g)
{
  uint32_t best = kToneNoBest;
  uint64_t top = 0;
  for (uint32_t k = 0; k < K; k++)
  {
    if (groups[k] == g && (best == kToneNoBest || P[k] > top))
    {
      best = k;
      top = P[k];
    }
  }
  return best;
}

// ---- the settings of one handle the verdict needs
struct ToneThresholds
{
  uint64_t min_energy[kToneGroups];
  uint32_t ratio_q8[kToneGroups];
};

// ---- one frame, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512]; cos_table: the 4096 entries of DDC_COS; power [K] and best / present [4] may
// be NULL
inline void tone_frame_slow(const int16_t *pcm_row, const uint32_t *n_pcm_row, uint32_t frame, uint32_t L, const int16_t *window,
                            const uint32_t *steps, const uint8_t *groups, uint32_t K, const ToneThresholds &th,
                            const int16_t *cos_table, uint64_t *power, uint64_t *energy, uint32_t *valid, uint8_t *best,
                            uint8_t *present)
{
  uint64_t P[kToneMaxTones];
  uint64_t E = 0;
  for (uint32_t k = 0; k < K; k++)
  {
    int64_t I = 0, Q = 0;
    for (uint32_t n = 0; n < L; n++)
    {
      const uint32_t j = frame * L + n, b = j / kToneBlock, pos = j % kToneBlock;
      const int32_t x = pos < pcm_block_limit(n_pcm_row, b) ? pcm_row[j] : 0;
      const int32_t u = tone_window(x, window[n]);
      const uint32_t i = tone_cos_index(steps[k] * n);
      I += (int64_t)u * cos_table[i];
      Q += (int64_t)u * cos_table[tone_sin_index(i)];
      if (k == 0)
      {
        E += (uint64_t)((int64_t)u * u);
      }
    }
    P[k] = tone_power(I, Q);
    if (power != nullptr)
    {
      power[k] = P[k];
    }
  }
  const uint32_t v = tone_frame_valid(n_pcm_row, frame, L);
  if (energy != nullptr)
  {
    *energy = E;
  }
  if (valid != nullptr)
  {
    *valid = v;
  }
  for (uint32_t g = 0; g < kToneGroups; g++)
  {
    const uint32_t bi = tone_best(P, groups, K, g);
    if (best != nullptr)
    {
      best[g] = (uint8_t)bi;
    }
    if (present != nullptr)
    {
      present[g] = bi != kToneNoBest && tone_present(v, L, E, th.min_energy[g], P[bi], th.ratio_q8[g]) ? 1 : 0;
    }
  }
}

// ---- the checks, each under `who`, the public function's name
inline int tone_check_create(const char *who, uint32_t n_channels, uint32_t frame_len, const void *out)
{
  BANK_TRY(pcm_check_channels(who, n_channels, out));
  return pcm_check_frame_len(who, frame_len);
}

inline int tone_check_tones(const char *who, const uint32_t *steps, const uint8_t *groups, uint32_t K)
{
  if (K == 0 || K > kToneMaxTones || steps == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u tones and their steps (got %u)", who, kToneMaxTones, K);
  }
  for (uint32_t k = 0; groups != nullptr && k < K; k++)
  {
    if (groups[k] >= kToneGroups)
    {
      return fail(HRFD_EINVAL, "%s: tone %u has group %u (0..%u)", who, k, (unsigned)groups[k], kToneGroups - 1);
    }
  }
  return HRFD_OK;
}

inline int tone_check_window(const char *who, const int16_t *w, uint32_t L)
{
  for (uint32_t n = 0; w != nullptr && n < L; n++)
  {
    if (w[n] == -32768)
    {
      return fail(HRFD_EINVAL, "%s: window entry %u is -32768 (-32767..32767: |u| must stay below 2^15)", who, n);
    }
  }
  return HRFD_OK;
}

inline int tone_check_threshold(const char *who, uint32_t group, uint32_t ratio_q8, uint64_t min_energy)
{
  if (group >= kToneGroups && group != HRFD_ALL_CHANNELS)
  {
    return fail(HRFD_EINVAL, "%s: group %u (0..%u or HRFD_ALL_CHANNELS)", who, group, kToneGroups - 1);
  }
  if (ratio_q8 > HRFD_TONE_MAX_RATIO)
  {
    return fail(HRFD_EINVAL, "%s: ratio_q8 %u > 2^20 (E x ratio could leave 64 bits)", who, ratio_q8);
  }
  if (min_energy > HRFD_TONE_MAX_ENERGY)
  {
    return fail(HRFD_EINVAL, "%s: min_energy %llu > 2^43 (no frame reaches it)", who, (unsigned long long)min_energy);
  }
  return HRFD_OK;
}

// what a call's sizes and addresses decide without a handle (the dense host entry has no stride)
inline int tone_check_call(const char *who, const void *pcm, uint64_t channel_stride, bool device_entry, uint32_t n_blocks,
                           const void *power, const void *energy, const void *valid, const void *best, const void *present)
{
  if (n_blocks == 0 || n_blocks > HRFD_TONE_MAX_BLOCKS)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, HRFD_TONE_MAX_BLOCKS, n_blocks);
  }
  if (power == nullptr && energy == nullptr && valid == nullptr && best == nullptr && present == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: no output asked for", who);
  }
  if (device_entry)
  {
    BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", channel_stride, 2ull * kToneBlock * n_blocks));
  }
  if (!pcm_aligned(pcm, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM must sit at an even address", who);
  }
  if (!pcm_aligned(power, 8) || !pcm_aligned(energy, 8) || !pcm_aligned(valid, 4))
  {
    return fail(HRFD_EINVAL, "%s: power and energy must be 8-byte aligned, valid 4-byte aligned", who);
  }
  if (pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return HRFD_OK;
}

// what the handle's frame length and tone count decide
inline int tone_check_frames(const char *who, uint32_t L, uint32_t n_blocks, uint32_t n_tones)
{
  BANK_TRY(pcm_check_frames(who, n_blocks, L));
  if (n_tones == 0)
  {
    return fail(HRFD_EINVAL, "%s: no tones set (hrfd_tone_set_tones comes first)", who);
  }
  return HRFD_OK;
}

} // namespace hrfd
