// hackrfdiags_amd/csrc/hrfd_afsk.h -- what the AFSK bank (hrfd_afsk_*) needs no HIP for: the limits, the laws (taps, power,
// decision, clock, bit), the bound on a row of bits, the argument checks, and a slow loop over one channel that restates the
// contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_level.h (tests/cpp/san_afsk.cc compiles it on the CPU;
// hrfd_afsk.hip includes it for the host side and the kernel); the includer declares `int fail(int code, const char *fmt,
// ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_pcm.h"

#define HRFD_AFSK_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kAfskBlock = kPcmBlock;
constexpr uint32_t kAfskMinWindow = 2;
constexpr uint32_t kAfskMaxWindow = 32;        // W
constexpr uint32_t kAfskMinShift = 1;
constexpr uint32_t kAfskMaxShift = 8;          // A
constexpr uint32_t kAfskMaxBaudStep = 1u << 31;                // at most one bit per sample
constexpr uint32_t kAfskMaxToneStep = 1u << 31;                // mark and space: up to half the sample rate
constexpr uint32_t kAfskMaxBlocks = 1024;
constexpr uint32_t kAfskHardPerBlock = kAfskBlock / 8;         // 64 bytes of decisions per block
constexpr uint32_t kAfskHistSamples = kAfskMaxWindow;          // samples kept per channel, of which the last W - 1 count
constexpr uint32_t kAfskStateDw = kAfskHistSamples / 2 + 2;    // 18: 16 dwords of sample pairs, phi, the two flags
constexpr int32_t kAfskMaxTap = 2047;
constexpr uint32_t kAfskDefaultMark = 644245094u;              // round(1200 / 8000 * 2^32)
constexpr uint32_t kAfskDefaultSpace = 1181116006u;            // round(2200 / 8000 * 2^32)
constexpr uint32_t kAfskDefaultBaud = kAfskDefaultMark;        // 1200 baud
constexpr uint32_t kAfskDefaultWindow = 8;
constexpr uint32_t kAfskDefaultShift = 2;
// |I| <= W x 32768 x 2047 < 2^31: every partial sum of a filter fits an int32
static_assert((uint64_t)kAfskMaxWindow * 32768u * (uint64_t)kAfskMaxTap < (1ull << 31), "the filters sum in int32");

// filter f of the four: the cosine and sine taps of the mark tone, then of the space tone
enum
{
  kAfskMarkC = 0,
  kAfskMarkS = 1,
  kAfskSpaceC = 2,
  kAfskSpaceS = 3,
  kAfskFilters = 4
};

// one channel's state between calls: the last 32 samples as the filter saw them (x[-32] first; the last W - 1 count), the
// clock's phase, the last decision and the last sampled decision
struct AfskState
{
  int16_t x[kAfskHistSamples];
  uint32_t phi;
  uint32_t flags;                              // bit 0: h[n-1]; bit 1: last
};
static_assert(sizeof(AfskState) == 4 * kAfskStateDw, "the kernel reads this layout");

struct AfskModem
{
  uint32_t mark_step, space_step, baud_step, W, A, nrzi;
};

// ---- 1. taps: i = (((step k) mod 2^32 + 2^19) >> 20) & 4095, C[k] = clamp((COS[i] + 8) >> 4, -2047, 2047), S[k] the same
// from COS[(i - 1024) & 4095].  cos4096: the "DDC_COS" table
inline int32_t afsk_tap_round(int32_t v)
{
  v = (v + 8) >> 4;
  return v < -kAfskMaxTap ? -kAfskMaxTap : (v > kAfskMaxTap ? kAfskMaxTap : v);
}

// taps [4][32] in the order of the enum above, zero from W on
inline void afsk_taps(const int16_t *cos4096, uint32_t mark_step, uint32_t space_step, uint32_t W, int16_t *taps)
{
  for (uint32_t t = 0; t < 2; t++)
  {
    const uint32_t step = t == 0 ? mark_step : space_step;
    for (uint32_t k = 0; k < kAfskMaxWindow; k++)
    {
      const uint32_t i = ((step * k + (1u << 19)) >> 20) & 4095u;
      taps[(2 * t) * kAfskMaxWindow + k] = (int16_t)(k < W ? afsk_tap_round(cos4096[i]) : 0);
      taps[(2 * t + 1) * kAfskMaxWindow + k] = (int16_t)(k < W ? afsk_tap_round(cos4096[(i - 1024u) & 4095u]) : 0);
    }
  }
}

// ---- 2. power: P = I^2 + Q^2.  |I|, |Q| <= 32 x 32768 x 2047 < 2^31 give I^2, Q^2 < 2^62 and P < 2^63; the sum of two
// powers stays below 2^64
HRFD_AFSK_HD uint64_t afsk_power(int32_t i, int32_t q) { return (uint64_t)((int64_t)i * i) + (uint64_t)((int64_t)q * q); }

// ---- 3. decision: h = P_mark > P_space (d = P_mark - P_space > 0 in int64); carrier = P_mark + P_space > min_power
HRFD_AFSK_HD uint32_t afsk_decide(uint64_t p_mark, uint64_t p_space) { return p_mark > p_space ? 1u : 0u; }
HRFD_AFSK_HD uint32_t afsk_carrier(uint64_t p_mark, uint64_t p_space, uint64_t min_power) { return p_mark + p_space > min_power ? 1u : 0u; }

// ---- 4. clock: the nudge of a phase at a transition, towards 2^31 (mid-bit) by 1 / 2^A of the distance.  It never crosses 0
// (a phase below 2^31 grows, but by less than its distance to 2^31) and never moves past 2^31
HRFD_AFSK_HD uint32_t afsk_nudge(uint32_t phase, uint32_t A) { return phase - (uint32_t)(((int32_t)(phase - (1u << 31))) >> A); }

// ---- 5. bit: the byte of a sampled decision h with the carrier flag; with nrzi a 1 is "no change since the last sample"
HRFD_AFSK_HD uint32_t afsk_bit(uint32_t h, uint32_t last, bool nrzi, uint32_t carrier)
{
  return (nrzi ? 1u - (h ^ last) : h) | (carrier << 1);
}

// the most bits 512 n_blocks samples give: the phase advances by at most baud_step + (2^31 >> A) a sample, and the count
// of wraps is the floor of the advance over 2^32, one more for the phase the call starts at
HRFD_AFSK_HD uint32_t afsk_max_bits(uint32_t baud_step, uint32_t A, uint32_t n_blocks)
{
  return (uint32_t)(((uint64_t)kAfskBlock * n_blocks * ((uint64_t)baud_step + ((1u << 31) >> A))) >> 32) + 1u;
}

// ---- one channel, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512]; n_pcm_row: its [n_blocks] or NULL; taps: afsk_taps' [4][32]; st: read and replaced;
// bits (with n_bits) and hard: each or NULL.  A call without bits does not run the clock: phi and last stay
inline void afsk_channel_slow(const int16_t *pcm_row, const uint32_t *n_pcm_row, uint32_t n_blocks, const AfskModem &m,
                              const int16_t *taps, uint64_t min_power, AfskState *st, uint8_t *bits, uint32_t *n_bits, uint8_t *hard)
{
  int32_t x[kAfskHistSamples + 1];             // x[32] is the sample at hand, x[32 - k] the one k back
  for (uint32_t i = 0; i < kAfskHistSamples; i++)
  {
    x[i] = st->x[i];
  }
  uint32_t phi = st->phi, h_prev = st->flags & 1u, last = (st->flags >> 1) & 1u, count = 0;
  for (uint32_t n = 0; n < kAfskBlock * n_blocks; n++)
  {
    const uint32_t b = n / kAfskBlock, pos = n % kAfskBlock;
    x[kAfskHistSamples] = pos < pcm_block_limit(n_pcm_row, b) ? pcm_row[n] : 0;
    int32_t acc[kAfskFilters];
    for (uint32_t f = 0; f < kAfskFilters; f++)
    {
      acc[f] = 0;
      for (uint32_t k = 0; k < m.W; k++)
      {
        acc[f] += x[kAfskHistSamples - k] * taps[f * kAfskMaxWindow + k];
      }
    }
    const uint64_t p_mark = afsk_power(acc[kAfskMarkC], acc[kAfskMarkS]), p_space = afsk_power(acc[kAfskSpaceC], acc[kAfskSpaceS]);
    const uint32_t h = afsk_decide(p_mark, p_space);
    if (hard != nullptr)
    {
      if ((n & 7u) == 0)
      {
        hard[n >> 3] = 0;
      }
      hard[n >> 3] |= (uint8_t)(h << (n & 7u));
    }
    if (bits != nullptr)
    {
      uint32_t next = phi + m.baud_step;
      if (next < phi)
      {
        bits[count++] = (uint8_t)afsk_bit(h, last, m.nrzi != 0, afsk_carrier(p_mark, p_space, min_power));
        last = m.nrzi != 0 ? h : last;
      }
      if (h != h_prev)
      {
        next = afsk_nudge(next, m.A);
      }
      phi = next;
    }
    h_prev = h;
    for (uint32_t i = 0; i < kAfskHistSamples; i++)
    {
      x[i] = x[i + 1];
    }
  }
  for (uint32_t i = 0; i < kAfskHistSamples; i++)
  {
    st->x[i] = (int16_t)x[i];
  }
  st->phi = phi;
  st->flags = h_prev | (last << 1);
  if (n_bits != nullptr)
  {
    *n_bits = count;
  }
}

// ---- the checks, each under `who`, the public function's name
inline int afsk_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

inline int afsk_check_modem(const char *who, const AfskModem &m)
{
  if (m.W < kAfskMinWindow || m.W > kAfskMaxWindow)
  {
    return fail(HRFD_EINVAL, "%s: window %u (%u..%u samples)", who, m.W, kAfskMinWindow, kAfskMaxWindow);
  }
  if (m.A < kAfskMinShift || m.A > kAfskMaxShift)
  {
    return fail(HRFD_EINVAL, "%s: loop shift %u (%u..%u)", who, m.A, kAfskMinShift, kAfskMaxShift);
  }
  if (m.baud_step == 0 || m.baud_step > kAfskMaxBaudStep)
  {
    return fail(HRFD_EINVAL, "%s: baud_step %u (1..2^31: at most one bit per sample)", who, m.baud_step);
  }
  if (m.mark_step == 0 || m.mark_step > kAfskMaxToneStep)
  {
    return fail(HRFD_EINVAL, "%s: mark_step %u (1..2^31: a tone up to 4 kHz)", who, m.mark_step);
  }
  if (m.space_step == 0 || m.space_step > kAfskMaxToneStep)
  {
    return fail(HRFD_EINVAL, "%s: space_step %u (1..2^31: a tone up to 4 kHz)", who, m.space_step);
  }
  return HRFD_OK;
}

// what the block count decides on its own (hrfd_afsk_max_bits asks for no more)
inline int afsk_check_blocks(const char *who, uint32_t n_blocks)
{
  if (n_blocks == 0 || n_blocks > kAfskMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kAfskMaxBlocks, n_blocks);
  }
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle.  The dense host entry has no strides
inline int afsk_check_call(const char *who, const void *pcm, uint64_t in_stride, bool device_entry, const void *n_pcm,
                           uint32_t n_blocks, const void *bits, const void *n_bits, const void *hard)
{
  BANK_TRY(afsk_check_blocks(who, n_blocks));
  if (bits == nullptr && n_bits == nullptr && hard == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: no output asked for (bits, n_bits and hard are all NULL)", who);
  }
  if ((bits == nullptr) != (n_bits == nullptr))
  {
    return fail(HRFD_EINVAL, "%s: bits and n_bits go together (both or neither)", who);
  }
  if (device_entry)
  {
    BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", in_stride, 2ull * kAfskBlock * n_blocks));
  }
  if (!pcm_aligned(pcm, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM must sit at an even address", who);
  }
  if (!pcm_aligned(n_pcm, 4) || !pcm_aligned(n_bits, 4))
  {
    return fail(HRFD_EINVAL, "%s: n_pcm and n_bits must be 4-byte aligned", who);
  }
  if (pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return HRFD_OK;
}

// a row of bits must hold what the handle's modem can give in the call
// (or, where there is no handle yet, what the slowest modem there is can give: `of` says which)
inline int afsk_check_bits_stride(const char *who, uint64_t bits_stride, uint32_t max_bits, const char *of = "this modem")
{
  if (bits_stride < max_bits)
  {
    return fail(HRFD_EINVAL, "%s: bits_stride_bytes %llu is below hrfd_afsk_max_bits = %u of %s", who,
                (unsigned long long)bits_stride, max_bits, of);
  }
  return HRFD_OK;
}

} // namespace hrfd
