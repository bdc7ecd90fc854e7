// Sanitizer harness for the HIP-free part of the bank core (hackrfdiags_amd/csrc/hrfd_bank.h), CPU only: compiled as plain
// C++ under -fsanitize=address,undefined (tests/test_sanitizers.py).  The packed taps against the direct FIR for every tap
// count, the tap check at its bound, the tuning record across 2^32 and 2^33 samples, the channel lists against brute force.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../../include/hrfd.h"
static int fail(int code, const char *, ...) { return code; }
#include "../../hackrfdiags_amd/csrc/hrfd_bank.h"

using namespace hrfd;

struct Pair
{
  uint32_t x, y;
};

#define CHECK(cond)                                                \
  do                                                               \
  {                                                                \
    if (!(cond))                                                   \
    {                                                              \
      printf("san_bank: line %d: %s\n", __LINE__, #cond);          \
      return 1;                                                    \
    }                                                              \
  } while (0)

static int64_t dot2(uint32_t a, uint32_t b) { return (int64_t)(int16_t)a * (int16_t)b + (int64_t)(int16_t)(a >> 16) * (int16_t)(b >> 16); }

// J packed pairs over the rail x (int16 samples as dwords), window from sample s: what ddc_fir sums
static int64_t packed_fir(const std::vector<int16_t> &x, const Pair *t, int J, int s)
{
  int64_t acc = 0;
  for (int j = 0; j < J; j++)
  {
    const int i = 2 * ((s >> 1) + j);
    const uint32_t w = (uint16_t)x[i] | ((uint32_t)(uint16_t)x[i + 1] << 16);
    acc += dot2(w, (s & 1) ? t[j].y : t[j].x);
  }
  return acc;
}

// sum over k of h[k] x[end - k]
static int64_t direct_fir(const std::vector<int16_t> &x, const int16_t *h, int T, int end)
{
  int64_t acc = 0;
  for (int k = 0; k < T; k++)
  {
    acc += (int64_t)h[k] * x[end - k];
  }
  return acc;
}

static int check_taps(const std::vector<int16_t> &h, const std::vector<int16_t> &x)
{
  const int T = (int)h.size();
  // the DDC's packing: the window of T samples that ends at `end` starts at s = end - (T - 1)
  const int J = bank_packed_len(T);
  std::vector<Pair> t(J);
  bank_pack_taps(h.data(), T, t.data(), J);
  for (int s = 10; s < 12 && T > 0; s++)
  {
    CHECK(packed_fir(x, t.data(), J, s) == direct_fir(x, h.data(), T, s + T - 1));
  }
  // the DUC's: output R q + p of the zero-stuffed interpolation sums h[p + j R] v[q - j].  k_duc reads one window of v
  // for the positions m (even) and m + 1, from position m - LA on: x variant for m, y variant for m + 1
  for (int R = 1; R <= 8 && T > 0 && T <= 64; R *= 2)
  {
    const int LA = bank_branch_lookback(T, R), JA = bank_packed_len(LA + 1), m = 64;
    std::vector<Pair> tb((size_t)R * JA);
    bank_pack_branch_taps(h.data(), T, R, tb.data(), JA);
    const std::vector<int16_t> rail(x.begin() + (m - LA), x.end());
    for (int p = 0; p < R; p++)
    {
      for (int odd = 0; odd < 2; odd++)
      {
        int64_t want = 0;
        for (int j = 0; p + j * R < T; j++)
        {
          want += (int64_t)h[p + j * R] * x[m + odd - j];
        }
        CHECK(packed_fir(rail, tb.data() + (size_t)p * JA, JA, odd) == want);
      }
    }
  }
  return 0;
}

// bank_each_chunk over (n_wgs, max_wgs) with `first` held in First: the launches are contiguous from 0, none is empty, none
// exceeds max_wgs, they cover [0, n_wgs) exactly once and there are ceil(n_wgs / max_wgs) of them
template <class First>
static int check_chunks(uint64_t n_wgs, uint32_t max_wgs)
{
  uint64_t next = 0, launches = 0;
  bool ok = true;
  const int rc = bank_each_chunk<First>("t", n_wgs, max_wgs, [&](First first, uint32_t count) {
    ok = ok && (uint64_t)first == next && count >= 1 && count <= max_wgs;
    next += count;
    launches++;
    return HRFD_OK;
  });
  CHECK(rc == HRFD_OK && ok);
  CHECK(next == n_wgs);
  CHECK(launches == (n_wgs + max_wgs - 1) / max_wgs);
  return 0;
}

// a call that bank_each_chunk must refuse, in front of the first launch
template <class First>
static int check_chunks_refused(uint64_t n_wgs, uint32_t max_wgs)
{
  uint64_t launches = 0;
  const int rc = bank_each_chunk<First>("t", n_wgs, max_wgs, [&](First, uint32_t) {
    launches++;
    return HRFD_OK;
  });
  CHECK(rc == HRFD_EINVAL && launches == 0);
  return 0;
}

static int check_chunking()
{
  const uint32_t max = kBankMaxWgs;
  CHECK(max == (1u << 22));
  const uint64_t m64 = max;
  for (uint64_t n : std::vector<uint64_t>{0, 1, m64 - 1, m64, m64 + 1, 2 * m64, 2 * m64 + 1})
  {
    if (check_chunks<uint32_t>(n, max) != 0 || check_chunks<uint64_t>(n, max) != 0) return 1;
  }
  // 2^34 workgroups (the resampler's most): 4096 launches where first_wg has 64 bits; 32 bits cannot number a launch that
  // starts at 2^32, so 2^32 workgroups (the last launch starts at 2^32 - 2^22) are the most they take
  if (check_chunks<uint64_t>(1ull << 34, max) != 0 || check_chunks_refused<uint32_t>(1ull << 34, max) != 0) return 1;
  if (check_chunks<uint32_t>(1ull << 32, max) != 0 || check_chunks_refused<uint32_t>((1ull << 32) + 1, max) != 0) return 1;
  for (uint32_t m : {1u, 2u, 3u, 7u})
  {
    for (uint64_t n = 0; n <= 50; n++)
    {
      if (check_chunks<uint32_t>(n, m) != 0 || check_chunks<uint64_t>(n, m) != 0) return 1;
    }
  }
  // a narrow first_wg at small sizes: 255 is the last start a byte holds
  if (check_chunks<uint8_t>(256, 1) != 0 || check_chunks_refused<uint8_t>(257, 1) != 0) return 1;
  if (check_chunks<uint8_t>(7 * 37, 7) != 0 || check_chunks_refused<uint8_t>(7 * 37 + 1, 7) != 0) return 1;      // 252 / 259
  // n_wgs = 0 launches nothing whatever the limit; a limit outside 1 .. kBankMaxWgs is refused
  if (check_chunks<uint32_t>(0, 1) != 0 || check_chunks_refused<uint32_t>(5, 0) != 0 || check_chunks_refused<uint64_t>(5, max + 1) != 0)
    return 1;
  // a launch that fails ends the call there, with its code
  {
    uint64_t launches = 0;
    const int rc = bank_each_chunk<uint32_t>("t", 10, 3, [&](uint32_t, uint32_t) { return ++launches == 2 ? HRFD_ENODEV : HRFD_OK; });
    CHECK(rc == HRFD_ENODEV && launches == 2);
  }
  return 0;
}

int main()
{
  if (check_chunking() != 0)
  {
    return 1;
  }
  std::mt19937 rng(7);
  std::vector<int16_t> x(700);
  for (int16_t &v : x)
  {
    v = (int16_t)(rng() & 0xffff);
  }
  // 1. every tap count: random taps, and all-extreme ones over extreme samples
  for (int T = 0; T <= 256; T++)
  {
    std::vector<int16_t> h(T), hx(T, (int16_t)-32768);
    for (int16_t &v : h)
    {
      v = (int16_t)(rng() & 0xffff);
    }
    if (check_taps(h, x) != 0)
    {
      return 1;
    }
    std::vector<int16_t> xx(700, (int16_t)-32768);
    if (check_taps(hx, xx) != 0)
    {
      return 1;
    }
  }
  // 2. the tap check at its bound
  {
    const int16_t ok[3] = {32767, -32768, 0}, bad[3] = {32767, -32768, 1};
    CHECK(bank_tap_sums_ok("t", ok, 3, 1) == HRFD_OK && bank_tap_sums_ok("t", bad, 3, 1) == HRFD_EINVAL);
    CHECK(bank_tap_count_ok("t", ok, 3, 3) == HRFD_OK && bank_tap_count_ok("t", ok, 4, 3) == HRFD_EINVAL);
    CHECK(bank_tap_count_ok("t", nullptr, 0, 3) == HRFD_OK && bank_tap_count_ok("t", nullptr, 1, 3) == HRFD_EINVAL);
    for (uint32_t R = 1; R <= 8; R *= 2)
    {
      // every branch at 65535, then one branch at 65536
      std::vector<int16_t> h(3 * R);
      for (uint32_t p = 0; p < R; p++)
      {
        h[p] = 32767;
        h[p + R] = -32768;
        h[p + 2 * R] = 0;
      }
      CHECK(bank_tap_sums_ok("t", h.data(), 3 * R, R) == HRFD_OK);
      CHECK(R == 1 || bank_tap_sums_ok("t", h.data(), 3 * R, 1) == HRFD_EINVAL);
      h[3 * R - 1] = -1;
      CHECK(bank_tap_sums_ok("t", h.data(), 3 * R, R) == HRFD_EINVAL);
    }
  }
  // 3. retune keeps the phase continuous while N passes 2^32 and 2^33
  {
    BankTuning c{0u, 0u, 0u, 5u, 0ull};
    uint64_t N = 0;
    uint32_t theta = 0, step = 0x9E3779B9u;
    bank_retune(c, N, 1u, step);
    for (int i = 0; i < 40; i++)
    {
      const uint64_t adv = (1ull << 28) + (rng() & 0xfffff);
      N += adv;
      theta += (uint32_t)adv * step;                       // the phase the samples in between have advanced
      CHECK(bank_phase_at(c, N) == theta);
      if (i % 3 == 0)
      {
        step = (uint32_t)rng();
        bank_retune(c, N, (uint32_t)(i & 1), step);
        CHECK(bank_phase_at(c, N) == theta && c.n_ref == N && c.step == step && c.capture == (uint32_t)(i & 1) && c.word == 5u);
      }
    }
    CHECK(N > (1ull << 33));
    bank_reset(c);
    CHECK(c.theta_ref == 0u && c.n_ref == 0ull && c.step == step && c.word == 5u);
  }
  // 4. the channel lists against brute force
  for (int trial = 0; trial < 60; trial++)
  {
    const uint32_t W = 1 + rng() % 9, C = 1 + rng() % 70;
    std::vector<BankTuning> chan(C, BankTuning{0u, 0u, 0u, 0u, 0ull});
    for (BankTuning &c : chan)
    {
      c.capture = trial % 3 == 0 ? W - 1 : trial % 3 == 1 ? (rng() % W) / 2 * 2 % W : rng() % W;   // one, even ones, any
    }
    std::vector<uint32_t> off(W + 1, 77u), list(C, 77u), want;
    bank_channel_lists(chan.data(), C, W, off.data(), list.data());
    CHECK(off[0] == 0 && off[W] == C);
    for (uint32_t w = 0; w < W; w++)
    {
      CHECK(off[w] == want.size());
      for (uint32_t c = 0; c < C; c++)
      {
        if (chan[c].capture == w) want.push_back(c);
      }
    }
    CHECK(want == list);
  }
  printf("san_bank ok\n");
  return 0;
}
