// hackrfdiags_amd/csrc/hrfd_dcs.h -- what the DCS bank (hrfd_dcs_*) needs no HIP for: the limits, the laws (the grid of the 23
// bits behind a sample, the canonical word under rotation, the Golay code words), the layout of a channel's state, the
// argument checks, and a slow loop over one channel that restates the contract of include/hrfd.h sample by sample.  Plain
// C++ like hrfd_level.h (tests/cpp/san_dcs.cc compiles it on the CPU; hrfd_dcs.hip includes it for the host side and the
// kernel); the includer declares `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include <vector>

#include "hrfd_pcm.h"

#define HRFD_DCS_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kDcsBlock = kPcmBlock;
constexpr uint32_t kDcsMaxTaps = 512;
constexpr uint32_t kDcsMaxCodes = 128;         // K
constexpr uint32_t kDcsMaxBlocks = 1024;
constexpr uint32_t kDcsGroups = 4;
constexpr uint32_t kDcsNoBest = 255;           // best of a group without entries: the tone bank's
constexpr uint32_t kDcsWordBits = 23;
constexpr uint32_t kDcsWordMask = (1u << kDcsWordBits) - 1;
constexpr uint32_t kDcsGenerator = 0xC75;      // g of the (23,12) Golay code, bit i = x^i
constexpr uint32_t kDcsDefaultMinHits = 128;
constexpr uint32_t kDcsNoEntry = 0xffffffffu;  // no canonical word (they have 23 bits): pads the sorted list

// ---- 3. the grid: bit k of a word, counted from the newest, lies D[k] = floor(1250 k / 21) samples back (8000 / 134.4 =
// 1250 / 21 samples a bit): D[0] = 0, D[22] = 1309
HRFD_DCS_HD uint32_t dcs_delay(uint32_t k) { return (1250u * k) / 21u; }
constexpr uint32_t kDcsReach = (1250u * 22u) / 21u;                  // 1309: the oldest slicer bit a sample's word reads

// ---- 9. a channel's state, kDcsStateDw dwords: the last 512 inputs as the filter saw them as 256 packed pairs, the oldest
// first; then the last 1312 slicer bits, the oldest in bit 0 of dword 256 (41 dwords: 1309 are read, whole dwords are
// kept); then zeros up to a multiple of 16 bytes
constexpr uint32_t kDcsHistDw = kDcsBlock / 2;                       // 256
constexpr uint32_t kDcsBitDw = (kDcsReach + 31) / 32;                // 41
constexpr uint32_t kDcsBitHist = 32 * kDcsBitDw;                     // 1312
constexpr uint32_t kDcsStateDw = 300;
static_assert(kDcsHistDw + kDcsBitDw <= kDcsStateDw && kDcsStateDw % 4 == 0, "the state row holds both histories");
static_assert(kDcsMaxTaps - 1 <= kDcsBlock, "the filter reaches no further back than the samples kept");

// ---- 4. the canonical word: the least of the 23 rotations
HRFD_DCS_HD uint32_t dcs_rot23(uint32_t w, uint32_t r) { return ((w >> r) | (w << (kDcsWordBits - r))) & kDcsWordMask; }

HRFD_DCS_HD uint32_t dcs_canonical(uint32_t w)
{
  uint32_t c = w;
  for (uint32_t r = 1; r < kDcsWordBits; r++)
  {
    const uint32_t v = dcs_rot23(w, r);
    c = v < c ? v : c;
  }
  return c;
}

// ---- 5. the code words: (p << 12) | 0x800 | code, p the remainder of (0x800 | code) x^11 modulo g; inverted: the
// complement in 23 bits
HRFD_DCS_HD uint32_t dcs_word(uint32_t code, bool inverted)
{
  const uint32_t data = 0x800u | (code & 0x1ffu);
  uint32_t p = data << 11;                     // degree 22 at the most
  for (int i = 22; i >= 11; i--)
  {
    if ((p >> i) & 1u)
    {
      p ^= kDcsGenerator << (i - 11);
    }
  }
  const uint32_t w = (p << 12) | data;
  return inverted ? w ^ kDcsWordMask : w;
}

// the remainder of w(x) modulo g: 0 for every code word and every rotation of one
HRFD_DCS_HD uint32_t dcs_syndrome(uint32_t w)
{
  for (int i = 22; i >= 11; i--)
  {
    if ((w >> i) & 1u)
    {
      w ^= kDcsGenerator << (i - 11);
    }
  }
  return w;
}

// ---- 8. the verdict of one block and group from the block's K counts: the entry of the group with the most hits, the
// lowest index on a tie; kDcsNoBest and absent for a group without entries, as the tone bank has it
HRFD_DCS_HD uint32_t dcs_best(const uint16_t *hits, const uint8_t *groups, uint32_t K, uint32_t g)
{
  uint32_t best = kDcsNoBest, top = 0;
  for (uint32_t k = 0; k < K; k++)
  {
    if (groups[k] == g && (best == kDcsNoBest || hits[k] > top))
    {
      best = k;
      top = hits[k];
    }
  }
  return best;
}

// ---- one channel, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512]; n_pcm_row: its [n_blocks] or NULL; taps: T of them; canon, groups: the K entries in
// list order; state: kDcsStateDw dwords, read and replaced; hits [n_blocks][K], best and present [n_blocks][4], each or NULL
inline void dcs_channel_slow(const int16_t *pcm_row, const uint32_t *n_pcm_row, uint32_t n_blocks, const int16_t *taps, uint32_t T,
                             const uint32_t *canon, const uint8_t *groups, uint32_t K, const uint32_t *min_hits, uint32_t *state,
                             uint16_t *hits, uint8_t *best, uint8_t *present)
{
  const uint32_t n = n_blocks * kDcsBlock;
  std::vector<int32_t> x(kDcsBlock + n);
  std::vector<uint8_t> s(kDcsBitHist + n);
  for (uint32_t i = 0; i < kDcsBlock; i++)
  {
    x[i] = (int16_t)(state[i / 2] >> (16 * (i & 1)));
  }
  for (uint32_t i = 0; i < kDcsBitHist; i++)
  {
    s[i] = (uint8_t)((state[kDcsHistDw + i / 32] >> (i & 31)) & 1u);
  }
  uint16_t count[kDcsMaxCodes];
  for (uint32_t b = 0; b < n_blocks; b++)
  {
    const uint32_t lim = pcm_block_limit(n_pcm_row, b);
    for (uint32_t k = 0; k < K; k++)
    {
      count[k] = 0;
    }
    for (uint32_t pos = 0; pos < kDcsBlock; pos++)
    {
      const uint32_t m = b * kDcsBlock + pos;
      x[kDcsBlock + m] = pos < lim ? pcm_row[m] : 0;
      int32_t acc = 0;                         // sum |h| <= 65535 and |x| <= 32768: every partial sum fits
      for (uint32_t j = 0; j < T; j++)
      {
        acc += (int32_t)taps[j] * x[kDcsBlock + m - j];
      }
      s[kDcsBitHist + m] = acc > 0 ? 1 : 0;
      uint32_t w = 0;
      for (uint32_t k = 0; k < kDcsWordBits; k++)
      {
        w |= (uint32_t)s[kDcsBitHist + m - dcs_delay(k)] << (kDcsWordBits - 1 - k);
      }
      const uint32_t c = dcs_canonical(w);
      for (uint32_t k = 0; k < K; k++)
      {
        count[k] += canon[k] == c ? 1 : 0;       // the list holds no word twice
      }
    }
    for (uint32_t k = 0; k < K && hits != nullptr; k++)
    {
      hits[(size_t)b * K + k] = count[k];
    }
    for (uint32_t g = 0; g < kDcsGroups; g++)
    {
      const uint32_t bi = dcs_best(count, groups, K, g);
      if (best != nullptr)
      {
        best[b * kDcsGroups + g] = (uint8_t)bi;
      }
      if (present != nullptr)
      {
        present[b * kDcsGroups + g] = bi != kDcsNoBest && count[bi] >= min_hits[g] ? 1 : 0;
      }
    }
  }
  for (uint32_t i = 0; i < kDcsStateDw; i++)
  {
    state[i] = 0;
  }
  for (uint32_t i = 0; i < kDcsBlock; i++)
  {
    state[i / 2] |= (uint32_t)(uint16_t)x[n + i] << (16 * (i & 1));
  }
  for (uint32_t i = 0; i < kDcsBitHist; i++)
  {
    state[kDcsHistDw + i / 32] |= (uint32_t)s[n + i] << (i & 31);
  }
}

// ---- the checks, each under `who`, the public function's name
inline int dcs_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

inline int dcs_check_taps(const char *who, const int16_t *taps, uint32_t n)
{
  if (n == 0 || n > kDcsMaxTaps || taps == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u taps and their array (got %u)", who, kDcsMaxTaps, n);
  }
  return bank_tap_sums_ok(who, taps, n, 1);
}

// K = 0..128 entries; inverted and groups may be NULL (none inverted, all in group 0).  Two entries with one canonical word
// are aliases (023 = 340 = 766, D023I = D047N): a sample must match at most one entry
inline int dcs_check_codes(const char *who, const uint16_t *codes, const uint8_t *inverted, const uint8_t *groups, uint32_t n)
{
  if (n > kDcsMaxCodes || (n > 0 && codes == nullptr))
  {
    return fail(HRFD_EINVAL, "%s: a list of %u codes (at most %u, and their array when n > 0)", who, n, kDcsMaxCodes);
  }
  uint32_t canon[kDcsMaxCodes];
  for (uint32_t k = 0; k < n; k++)
  {
    if (codes[k] > 0777)
    {
      return fail(HRFD_EINVAL, "%s: entry %u has code %u (three octal digits: 0..511)", who, k, codes[k]);
    }
    if (groups != nullptr && groups[k] >= kDcsGroups)
    {
      return fail(HRFD_EINVAL, "%s: entry %u has group %u (0..%u)", who, k, groups[k], kDcsGroups - 1);
    }
    canon[k] = dcs_canonical(dcs_word(codes[k], inverted != nullptr && inverted[k] != 0));
    for (uint32_t j = 0; j < k; j++)
    {
      if (canon[j] == canon[k])
      {
        return fail(HRFD_EINVAL, "%s: entries %u (D%03o%c) and %u (D%03o%c) are aliases: both have the canonical word 0x%06x", who,
                    j, codes[j], inverted != nullptr && inverted[j] != 0 ? 'I' : 'N', k, codes[k],
                    inverted != nullptr && inverted[k] != 0 ? 'I' : 'N', canon[k]);
      }
    }
  }
  return HRFD_OK;
}

inline int dcs_check_min_hits(const char *who, uint32_t group, uint32_t n)
{
  if (group >= kDcsGroups && group != HRFD_ALL_CHANNELS)
  {
    return fail(HRFD_EINVAL, "%s: group %u (0..%u or HRFD_ALL_CHANNELS)", who, group, kDcsGroups - 1);
  }
  if (n == 0 || n > kDcsBlock)
  {
    return fail(HRFD_EINVAL, "%s: min_hits %u (1..%u: a block has %u samples)", who, n, kDcsBlock, kDcsBlock);
  }
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle.  The dense host entry has no stride.
inline int dcs_check_call(const char *who, const void *pcm, uint64_t stride, bool device_entry, const void *n_pcm, uint32_t n_blocks,
                          const void *hits, const void *best, const void *present)
{
  if (n_blocks == 0 || n_blocks > kDcsMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kDcsMaxBlocks, n_blocks);
  }
  if (hits == nullptr && best == nullptr && present == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: no output asked for (hits, best and present are all NULL)", who);
  }
  if (device_entry)
  {
    BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", stride, 2ull * kDcsBlock * n_blocks));
  }
  if (!pcm_aligned(pcm, 2) || !pcm_aligned(hits, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM and hits must sit at even addresses", who);
  }
  if (!pcm_aligned(n_pcm, 4))
  {
    return fail(HRFD_EINVAL, "%s: n_pcm must be 4-byte aligned", who);
  }
  if (pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return HRFD_OK;
}

// the K canonical words in rising order with the entry each belongs to, padded with kDcsNoEntry to kDcsMaxCodes: what the
// kernel searches
inline void dcs_sorted_list(const uint32_t *canon, uint32_t K, uint32_t *sorted, uint8_t *entry)
{
  for (uint32_t i = 0; i < kDcsMaxCodes; i++)
  {
    sorted[i] = kDcsNoEntry;
    entry[i] = 0;
  }
  for (uint32_t k = 0; k < K; k++)               // insertion: K <= 128
  {
    uint32_t at = k;
    while (at > 0 && sorted[at - 1] > canon[k])
    {
      sorted[at] = sorted[at - 1];
      entry[at] = entry[at - 1];
      at--;
    }
    sorted[at] = canon[k];
    entry[at] = (uint8_t)k;
  }
}

} // namespace hrfd
