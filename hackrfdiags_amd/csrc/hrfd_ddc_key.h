// hackrfdiags_amd/csrc/hrfd_ddc_key.h -- what the DDC bank's receive key needs no HIP for: the key block's limits, the number
// of key bytes of a call, the block of a sample, the rule by which k_ddc skips a unit, a slow per-channel count of the skipped
// units of a call from its key rows, and the argument checks.  Plain C++ like hrfd_duc_key.h (tests/cpp/san_ddc_key.cc
// compiles it on the CPU; hrfd_ddc.hip includes it for the host side and the kernel); the includer declares
// `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
//
// The law (include/hrfd.h, DDC block): key byte j of a channel's row covers the call-local output samples
// [j 2^k, (j + 1) 2^k); a keyed call writes outk[c][m] = key[c][m >> k] != 0 ? out[c][m] : (0, 0), out being what the unkeyed
// call writes, and leaves everything else as the unkeyed call leaves it.  The DDC carries nothing per channel through time
// (the history is the capture's, the phase a function of the sample counter), so unlike the DUC's key this one has no tile
// that is always computed and masks no history.
#pragma once
#include <stdint.h>

#include "hrfd_bank.h"

namespace hrfd {

constexpr uint32_t kDdcKeyMinLog2 = 10;                // a key block is a whole number of k_ddc's tiles of 1024 outputs
constexpr uint32_t kDdcKeyMaxLog2 = 17;                // 131072 output samples = one rx block = 512 PCM samples
constexpr uint32_t kDdcKeyDefaultLog2 = 17;
constexpr uint32_t kDdcKeyTile = 1024;                 // k_ddc's tile (kBankTile) in output samples
static_assert((1u << kDdcKeyMinLog2) % kDdcKeyTile == 0, "a tile lies in one key block");

// ---- 1. sizes and indices
// key bytes per channel of a call of M output samples: ceil(M / 2^k)
HRFD_BANK_HD uint32_t ddc_key_n(uint32_t M, uint32_t k) { return (uint32_t)(((uint64_t)M + (1ull << k) - 1ull) >> k); }
// the key byte that covers call-local output sample m, 0 <= m < M
HRFD_BANK_HD uint32_t ddc_key_block_of(uint32_t m, uint32_t k) { return m >> k; }
HRFD_BANK_HD uint32_t ddc_key_tiles(uint32_t M) { return (M + kDdcKeyTile - 1u) / kDdcKeyTile; }

// ---- 2. the work contract: unit (channel, tile t) is skipped iff the key is off in the block of the tile's first output.
// t < ddc_key_tiles(M)
HRFD_BANK_HD bool ddc_key_skip(const uint8_t *row, uint32_t t, uint32_t k)
{
  return row[ddc_key_block_of(kDdcKeyTile * t, k)] == 0;
}

// the units a call of M outputs skips, counted unit by unit from its key rows (key_stride bytes apart), per channel into
// per_channel[n_channels] (may be NULL); returns their sum: what hrfd_ddc_get_key_skips grows by
inline uint64_t ddc_key_count_skips(const uint8_t *key, uint64_t key_stride, uint32_t n_channels, uint32_t M, uint32_t k,
                                    uint64_t *per_channel)
{
  uint64_t sum = 0;
  for (uint32_t c = 0; c < n_channels; c++)
  {
    uint64_t n = 0;
    for (uint32_t t = 0; t < ddc_key_tiles(M); t++)
    {
      n += ddc_key_skip(key + (uint64_t)c * key_stride, t, k) ? 1u : 0u;
    }
    if (per_channel != nullptr)
    {
      per_channel[c] = n;
    }
    sum += n;
  }
  return sum;
}

// ---- the checks, each under `who`, the public function's name
inline int ddc_key_check_block(const char *who, uint32_t log2_samples)
{
  if (log2_samples < kDdcKeyMinLog2 || log2_samples > kDdcKeyMaxLog2)
  {
    return fail(HRFD_EINVAL, "%s: the key block must be 2^%u..2^%u output samples (got log2 = %u)", who, kDdcKeyMinLog2,
                kDdcKeyMaxLog2, log2_samples);
  }
  return HRFD_OK;
}

inline int ddc_key_check_result(const char *who, const void *result)
{
  return result != nullptr ? HRFD_OK : fail(HRFD_EINVAL, "%s: NULL result", who);
}

// the meter's channel: one of the bank's, or HRFD_ALL_CHANNELS (the sum)
inline int ddc_key_check_channel(const char *who, uint32_t channel, uint32_t n_channels)
{
  if (channel >= n_channels && channel != HRFD_ALL_CHANNELS)
  {
    return fail(HRFD_EINVAL, "%s: channel %u is neither below %u nor HRFD_ALL_CHANNELS", who, channel, n_channels);
  }
  return HRFD_OK;
}

// a call's key rows: none (the unkeyed call), or rows of at least n_keys bytes.  Without a handle k is the largest block,
// which asks the least
inline int ddc_key_check_stride(const char *who, const void *key, uint64_t key_stride, uint32_t out_bytes, uint32_t k)
{
  if (key != nullptr && key_stride < ddc_key_n(out_bytes / 2u, k))
  {
    return fail(HRFD_EINVAL, "%s: key_stride %llu is below n_keys = %u (out_bytes %u, key block 2^%u)", who,
                (unsigned long long)key_stride, ddc_key_n(out_bytes / 2u, k), out_bytes, k);
  }
  return HRFD_OK;
}

} // namespace hrfd
