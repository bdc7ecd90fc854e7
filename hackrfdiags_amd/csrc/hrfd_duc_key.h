// hackrfdiags_amd/csrc/hrfd_duc_key.h -- what the DUC bank's transmit key needs no HIP for: the key block's limits, the number
// of key bytes of a call, the block of a sample, the mask of a sample, the rule by which k_duc skips a unit, a slow count of
// the skipped units of a call from its key rows, and the argument checks.  Plain C++ like hrfd_hdlc.h
// (tests/cpp/san_duc_key.cc compiles it on the CPU; hrfd_duc.hip includes it for the host side and the kernel); the includer
// declares `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
//
// The law (include/hrfd.h, DUC block): key byte j of a channel's row covers the call-local channel samples
// [j 2^k, (j + 1) 2^k); a keyed call is the unkeyed call over xk[c][m] = key[c][m >> k] != 0 ? x[c][m] : 0.
#pragma once
#include <stdint.h>

#include "hrfd_bank.h"

namespace hrfd {

constexpr uint32_t kDucKeyMinLog2 = 10;                // a key block is a whole number of k_duc's tiles of 1024 samples
constexpr uint32_t kDucKeyMaxLog2 = 17;                // 131072 channel samples = one block of 512 PCM samples
constexpr uint32_t kDucKeyDefaultLog2 = 17;
constexpr uint32_t kDucKeyTile = 1024;                 // k_duc's tile (kBankTile) in channel samples
static_assert((1u << kDucKeyMinLog2) % kDucKeyTile == 0, "a tile lies in one key block");

// ---- 1. sizes and indices
// key bytes per channel of a call of M channel samples: ceil(M / 2^k)
HRFD_BANK_HD uint32_t duc_key_n(uint32_t M, uint32_t k) { return (uint32_t)(((uint64_t)M + (1ull << k) - 1ull) >> k); }
// the key byte that covers call-local sample m, 0 <= m < M
HRFD_BANK_HD uint32_t duc_key_block_of(uint32_t m, uint32_t k) { return m >> k; }
HRFD_BANK_HD uint32_t duc_key_tiles(uint32_t M) { return (M + kDucKeyTile - 1u) / kDucKeyTile; }

// ---- 2. the mask: is call-local sample j read from where it lies?  Samples in front of the call (the history holds xk
// already) and beyond it (zeros) are no business of the key: the row is indexed for 0 <= j < M only
HRFD_BANK_HD bool duc_key_on(const uint8_t *row, int64_t j, uint32_t M, uint32_t k)
{
  return j < 0 || j >= (int64_t)M || row[duc_key_block_of((uint32_t)j, k)] != 0;
}

// ---- 3. the work contract: unit (channel, tile t) is skipped iff t >= 1 and the key is off in the block of the tile and
// in the block of the tile in front of it (where the tile's look-back of at most 320 samples lies).  Tile 0 looks back into
// the history, whose content the call does not know: it is always computed.  t < duc_key_tiles(M)
HRFD_BANK_HD bool duc_key_skip(const uint8_t *row, uint32_t t, uint32_t k)
{
  return t >= 1u && row[duc_key_block_of(kDucKeyTile * t, k)] == 0 && row[duc_key_block_of(kDucKeyTile * (t - 1u), k)] == 0;
}

// the units a call of M samples skips, counted unit by unit from its key rows (key_stride bytes apart): what
// hrfd_duc_get_key_skips grows by.  A channel's amplitude and capture do not matter: the key is tested first
inline uint64_t duc_key_count_skips(const uint8_t *key, uint64_t key_stride, uint32_t n_channels, uint32_t M, uint32_t k)
{
  uint64_t n = 0;
  for (uint32_t c = 0; c < n_channels; c++)
  {
    for (uint32_t t = 0; t < duc_key_tiles(M); t++)
    {
      n += duc_key_skip(key + (uint64_t)c * key_stride, t, k) ? 1u : 0u;
    }
  }
  return n;
}

// ---- the checks, each under `who`, the public function's name
inline int duc_key_check_block(const char *who, uint32_t log2_samples)
{
  if (log2_samples < kDucKeyMinLog2 || log2_samples > kDucKeyMaxLog2)
  {
    return fail(HRFD_EINVAL, "%s: the key block must be 2^%u..2^%u channel samples (got log2 = %u)", who, kDucKeyMinLog2,
                kDucKeyMaxLog2, log2_samples);
  }
  return HRFD_OK;
}

inline int duc_key_check_result(const char *who, const void *result)
{
  return result != nullptr ? HRFD_OK : fail(HRFD_EINVAL, "%s: NULL result", who);
}

// a call's key rows: none (the unkeyed call), or rows of at least n_keys bytes.  Without a handle k is the largest block,
// which asks the least
inline int duc_key_check_stride(const char *who, const void *key, uint64_t key_stride, uint32_t in_bytes, uint32_t k)
{
  if (key != nullptr && key_stride < duc_key_n(in_bytes / 2u, k))
  {
    return fail(HRFD_EINVAL, "%s: key_stride %llu is below n_keys = %u (in_bytes %u, key block 2^%u)", who,
                (unsigned long long)key_stride, duc_key_n(in_bytes / 2u, k), in_bytes, k);
  }
  return HRFD_OK;
}

} // namespace hrfd
