// hackrfdiags_amd/csrc/hrfd_resamp.h -- what the resampler bank (hrfd_resamp_*) needs no HIP for: the limits, the argument
// checks, the count and phase law, the rounding, and a slow loop over one channel that restates the contract of
// include/hrfd.h sample by sample.  Plain C++ like hrfd_audio.h (tests/cpp/san_resamp.cc compiles it on the CPU;
// hrfd_resamp.hip includes it for the host side and the kernel); the includer declares `int fail(int code, const char *fmt,
// ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_pcm.h"

#define HRFD_RESAMP_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kResampBlock = kPcmBlock;   // samples per n_pcm block
constexpr uint32_t kResampMaxRatio = 512;      // L and M
constexpr uint32_t kResampMaxDown = 8;         // M <= 8 L
constexpr uint32_t kResampMaxTaps = 16384;     // T
constexpr uint32_t kResampMaxBranch = 512;     // K = ceil(T / L)
constexpr uint32_t kResampMaxIn = 524288;      // n_in of one call
constexpr uint32_t kResampHist = 512;          // samples of history kept per channel, whatever K is

// ---- 1. input (pcm_block_limit) and 3. rounding (pcm_fir_round, over every branch's sum |h| <= 65535): hrfd_pcm.h

HRFD_RESAMP_HD uint32_t resamp_gcd(uint32_t a, uint32_t b)
{
  while (b != 0)
  {
    const uint32_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

HRFD_RESAMP_HD uint32_t resamp_branch_taps(uint32_t T, uint32_t L) { return (T + L - 1) / L; }

// ---- 2. time: a call of n_in samples at phase d (0 <= d < M) gives the outputs whose q = d + j M lies below n_in L
HRFD_RESAMP_HD uint32_t resamp_out_count(uint32_t n_in, uint32_t L, uint32_t M, uint32_t d)
{
  const uint64_t span = (uint64_t)n_in * L;
  return span <= d ? 0u : (uint32_t)((span - d + M - 1) / M);
}

// d behind the call: d + n_out M - n_in L, again in 0..M-1
HRFD_RESAMP_HD uint32_t resamp_advance(uint32_t d, uint32_t n_in, uint32_t n_out, uint32_t L, uint32_t M)
{
  return (uint32_t)((int64_t)d + (int64_t)n_out * M - (int64_t)n_in * L);
}

// ---- one channel, output by output (the contract as a loop; the kernel must agree bit for bit)
// x_row: the channel's n_in samples; n_pcm_row: its [n_in / 512] or NULL; h: T taps; hist: the last 512 values of x in time
// order (hist[511] is the newest), read and replaced; y: resamp_out_count(n_in, L, M, d) outputs.  Returns the next d.
inline uint32_t resamp_channel_slow(const int16_t *x_row, const uint32_t *n_pcm_row, uint32_t n_in, const int16_t *h, uint32_t T,
                                    uint32_t L, uint32_t M, uint32_t d, int16_t *hist, int16_t *y)
{
  const uint32_t K = resamp_branch_taps(T, L), n_out = resamp_out_count(n_in, L, M, d);
  auto x = [&](int64_t s) -> int32_t {
    if (s < 0)
    {
      return hist[(int64_t)kResampHist + s];
    }
    const uint32_t b = (uint32_t)s / kResampBlock, pos = (uint32_t)s % kResampBlock;
    return pos < pcm_block_limit(n_pcm_row, b) ? x_row[s] : 0;
  };
  for (uint32_t j = 0; j < n_out; j++)
  {
    const uint64_t q = (uint64_t)d + (uint64_t)j * M;
    const int64_t i = (int64_t)(q / L);
    const uint32_t p = (uint32_t)(q % L);
    int32_t acc = 0;
    for (uint32_t k = 0; k < K; k++)
    {
      const uint32_t t = p + k * L;
      acc += (t < T ? (int32_t)h[t] : 0) * x(i - (int64_t)k);
    }
    y[j] = (int16_t)pcm_fir_round(acc);
  }
  int16_t next[kResampHist];
  for (uint32_t m = 0; m < kResampHist; m++)
  {
    next[m] = (int16_t)x((int64_t)n_in - kResampHist + m);
  }
  for (uint32_t m = 0; m < kResampHist; m++)
  {
    hist[m] = next[m];
  }
  return resamp_advance(d, n_in, n_out, L, M);
}

// ---- the checks, each under `who`, the public function's name
inline int resamp_check_create(const char *who, uint32_t n_channels, uint32_t L, uint32_t M, const void *out)
{
  BANK_TRY(pcm_check_channels(who, n_channels, out));
  if (L == 0 || L > kResampMaxRatio || M == 0 || M > kResampMaxRatio)
  {
    return fail(HRFD_EINVAL, "%s: up and down must be 1..%u (got %u / %u)", who, kResampMaxRatio, L, M);
  }
  if (resamp_gcd(L, M) != 1)
  {
    return fail(HRFD_EINVAL, "%s: up / down = %u / %u is not in lowest terms (gcd %u)", who, L, M, resamp_gcd(L, M));
  }
  if (M > kResampMaxDown * L)
  {
    return fail(HRFD_EINVAL, "%s: down %u is more than %u x up %u", who, M, kResampMaxDown, L);
  }
  return HRFD_OK;
}

// what the list decides without a handle: T = 1..16384 and its array
inline int resamp_check_tap_list(const char *who, const int16_t *taps, uint32_t n)
{
  if (n == 0 || n > kResampMaxTaps || taps == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u taps and their array (got %u)", who, kResampMaxTaps, n);
  }
  return HRFD_OK;
}

// and with the handle's L: K = ceil(T / L) <= 512 and the bank core's tap check over the L branches
inline int resamp_check_taps(const char *who, const int16_t *taps, uint32_t n, uint32_t L)
{
  BANK_TRY(resamp_check_tap_list(who, taps, n));
  if (resamp_branch_taps(n, L) > kResampMaxBranch)
  {
    return fail(HRFD_EINVAL, "%s: %u taps over %u branches are %u taps per branch (at most %u)", who, n, L, resamp_branch_taps(n, L),
                kResampMaxBranch);
  }
  return bank_tap_sums_ok(who, taps, n, L);
}

inline int resamp_check_n_in(const char *who, uint32_t n_in)
{
  if (n_in == 0 || n_in > kResampMaxIn)
  {
    return fail(HRFD_EINVAL, "%s: n_in must be 1..%u (got %u)", who, kResampMaxIn, n_in);
  }
  return HRFD_OK;
}

// with the handle's L: q = d + j M < n_in L + M must fit 32 bits with room to spare
inline int resamp_check_span(const char *who, uint32_t n_in, uint32_t L)
{
  if ((uint64_t)n_in * L >= (1ull << 31))
  {
    return fail(HRFD_EINVAL, "%s: n_in x up = %u x %u must stay below 2^31", who, n_in, L);
  }
  return HRFD_OK;
}

inline int resamp_check_capacity(const char *who, uint32_t n_out, uint32_t out_capacity)
{
  if (out_capacity < n_out)
  {
    return fail(HRFD_EINVAL, "%s: out_capacity %u is below the %u outputs of this call", who, out_capacity, n_out);
  }
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle; n_channels: the handle's, or 1 where there is none
// yet (the ranges that must not overlap grow with it).  The dense host entry has no strides: its rows are n_in and
// out_capacity samples long.
inline int resamp_check_call(const char *who, const void *pcm, uint64_t in_stride, bool device_entry, const void *n_pcm, uint32_t n_in,
                             const void *out, uint64_t out_stride, uint32_t out_capacity, const void *n_out, uint32_t n_channels)
{
  BANK_TRY(resamp_check_n_in(who, n_in));
  if (n_pcm != nullptr && n_in % kResampBlock != 0)
  {
    return fail(HRFD_EINVAL, "%s: n_pcm needs n_in to be a multiple of %u (got %u)", who, kResampBlock, n_in);
  }
  const uint64_t row = 2ull * n_in, out_row = 2ull * out_capacity;
  if (device_entry)
  {
    BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", in_stride, row));
    BANK_TRY(pcm_check_stride(who, "out_stride_bytes", out_stride, out_row, " (2 x out_capacity)"));
  }
  if (!pcm_aligned(pcm, 2) || !pcm_aligned(out, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM and out must sit at even addresses", who);
  }
  if (!pcm_aligned(n_pcm, 4))
  {
    return fail(HRFD_EINVAL, "%s: n_pcm must be 4-byte aligned", who);
  }
  if (pcm == nullptr || out == nullptr || n_out == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return pcm_check_no_overlap(who, pcm, device_entry ? in_stride : row, row, out, device_entry ? out_stride : out_row, out_row,
                              n_channels, "other workgroups still read it");
}

} // namespace hrfd
