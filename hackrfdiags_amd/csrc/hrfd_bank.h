// hackrfdiags_amd/csrc/hrfd_bank.h -- what the banks share and no HIP is needed for: BANK_TRY, the tuning record of the DDC
// and the DUC and its phase law, the tap check and tap packing of every FIR, the cut of a call into launches
// (bank_each_chunk), and the DUC's per-capture channel lists.
// hrfd_pcm.h adds the PCM contract on top.  Plain C++ (tests/cpp/san_bank.cc compiles it on the CPU); the includer
// declares `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define HRFD_BANK_HD __host__ __device__ __forceinline__
#else
#define HRFD_BANK_HD inline
#endif

// return what a check or a step answered unless it is HRFD_OK
#define BANK_TRY(expr)                                                                   \
  do                                                                                     \
  {                                                                                      \
    const int rc_ = (expr);                                                              \
    if (rc_ != HRFD_OK) return rc_;                                                      \
  } while (0)

namespace hrfd {

// One channel's tuning, as the kernels read it (24 bytes): theta(n) = theta_ref + (n - n_ref) * step modulo 2^32, n the
// absolute wideband sample index.  `word` is the bank's own: the DDC's gain shift g, the DUC's amplitude A.
struct BankTuning
{
  uint32_t capture;
  uint32_t step;
  uint32_t theta_ref;
  uint32_t word;
  uint64_t n_ref;
};
static_assert(sizeof(BankTuning) == 24, "the kernels read this layout");

HRFD_BANK_HD uint32_t bank_phase_at(const BankTuning &c, uint64_t N) { return c.theta_ref + (uint32_t)(N - c.n_ref) * c.step; }

// phase-continuous at the change point: theta_ref = theta(N) under the old tuning
inline void bank_retune(BankTuning &c, uint64_t N, uint32_t capture, uint32_t step)
{
  c.theta_ref = bank_phase_at(c, N);
  c.n_ref = N;
  c.step = step;
  c.capture = capture;
}

inline void bank_reset(BankTuning &c)
{
  c.theta_ref = 0u;
  c.n_ref = 0ull;
}

inline int bank_tap_count_ok(const char *who, const int16_t *taps, uint32_t n, uint32_t max_n)
{
  if (n > max_n || (n > 0 && taps == nullptr))
  {
    return fail(HRFD_EINVAL, "%s: %u taps (at most %u, and a tap array when n > 0)", who, n, max_n);
  }
  return HRFD_OK;
}

// sum |h| <= 65535 over every one of the `branches` polyphase branches (taps p, p + branches, ..): the int32 accumulator
// of a FIR over int16 samples then cannot overflow
inline int bank_tap_sums_ok(const char *who, const int16_t *taps, uint32_t n, uint32_t branches)
{
  for (uint32_t p = 0; p < branches; p++)
  {
    int64_t sum = 0;
    for (uint32_t k = p; k < n; k += branches)
    {
      sum += taps[k] < 0 ? -(int64_t)taps[k] : (int64_t)taps[k];
    }
    if (sum > 65535)
    {
      return fail(HRFD_EINVAL, "%s: branch %u of %u has sum |h| = %lld > 65535 (the int32 accumulator could overflow)", who,
                  p, branches, (long long)sum);
    }
  }
  return HRFD_OK;
}

inline int bank_packed_len(int T) { return T > 0 ? T / 2 + 1 : 0; }

// J (even, odd) packed pairs of the T time-reversed taps g: x = (g[2j], g[2j+1]) for a window that starts on an even
// sample, y = (g'[2j], g'[2j+1]) with g' = 0, g for one that starts on the odd sample above the dword.  Pair: uint2.
template <class Pair>
inline void bank_pack_taps(const int16_t *h, int T, Pair *out, int J)
{
  auto g = [&](int i) -> uint32_t { return (i >= 0 && i < T) ? (uint16_t)h[T - 1 - i] : 0u; };
  for (int j = 0; j < J; j++)
  {
    out[j].x = g(2 * j) | (g(2 * j + 1) << 16);
    out[j].y = g(2 * j - 1) | (g(2 * j) << 16);
  }
}

// look-back of an interpolating stage of T taps in samples at the low rate
inline int bank_branch_lookback(int T, int R) { return T > 0 ? (T - 1) / R : 0; }

// an interpolating stage's taps as R branches of LA + 1 taps each, every branch packed like bank_pack_taps into J pairs:
// branch p, tap j = h[p + j R]
template <class Pair>
inline void bank_pack_branch_taps(const int16_t *h, int T, int R, Pair *out, int J)
{
  const int LA = bank_branch_lookback(T, R);
  std::vector<int16_t> hp(LA + 1);
  for (int p = 0; p < R; p++)
  {
    for (int j = 0; j <= LA; j++)
    {
      hp[j] = (p + j * R < T) ? h[p + j * R] : (int16_t)0;
    }
    bank_pack_taps(hp.data(), LA + 1, out + p * J, J);
  }
}

constexpr uint32_t kBankMaxWgs = 1u << 22; // workgroups of one launch
static_assert((uint64_t)kBankMaxWgs * 256 <= (1ull << 30), "a launch of 256-thread workgroups stays at 2^30 work-items");

// The launches of a call of n_wgs workgroups, at most max_wgs each: f(first, count) for every launch in order, contiguous
// from 0 and none empty; n_wgs = 0 gives none.  First is the type the kernel's parameters hold `first` in: a call whose last
// launch would start above its range is refused in front of the first launch, never truncated.  f answers HRFD_OK or the
// failure that ends the call.
template <class First, class F>
inline int bank_each_chunk(const char *kernel, uint64_t n_wgs, uint32_t max_wgs, F f)
{
  if (max_wgs < 1 || max_wgs > kBankMaxWgs)
  {
    return fail(HRFD_EINVAL, "%s: %u workgroups per launch (1..%u)", kernel, max_wgs, kBankMaxWgs);
  }
  constexpr uint64_t top = (uint64_t)(First)~(First)0;
  static_assert((First)~(First)0 > (First)0 && sizeof(First) <= 8, "first_wg is unsigned");
  if (n_wgs > 0 && (n_wgs - 1) / max_wgs * max_wgs > top)
  {
    return fail(HRFD_EINVAL, "%s: %llu workgroups in launches of %u: the last launch starts above the %u bits of first_wg", kernel,
                (unsigned long long)n_wgs, max_wgs, 8u * (uint32_t)sizeof(First));
  }
  for (uint64_t first = 0; first < n_wgs; first += max_wgs)
  {
    const uint64_t left = n_wgs - first;
    BANK_TRY(f((First)first, (uint32_t)(left < max_wgs ? left : max_wgs)));
  }
  return HRFD_OK;
}

// the channels of every capture, in channel order (a counting sort): those of capture w are
// list[off[w] .. off[w + 1]); off has W + 1 entries, list C
inline void bank_channel_lists(const BankTuning *chan, uint32_t C, uint32_t W, uint32_t *off, uint32_t *list)
{
  std::vector<uint32_t> count(W, 0u);
  for (uint32_t c = 0; c < C; c++)
  {
    count[chan[c].capture]++;
  }
  off[0] = 0;
  for (uint32_t w = 0; w < W; w++)
  {
    off[w + 1] = off[w] + count[w];
    count[w] = off[w];
  }
  for (uint32_t c = 0; c < C; c++)
  {
    list[count[chan[c].capture]++] = c;
  }
}

} // namespace hrfd
