// Sanitizer harness for the HIP-free part of the resampler bank (hackrfdiags_amd/csrc/hrfd_resamp.h), CPU only: compiled as
// plain C++ under -fsanitize=address,undefined (tests/test_resamp_sanitizers.py).  Every check at its limit with its text,
// the count and phase law over every ratio's edge (the rounding on its boundaries: san_pcm.cc), the slow loop at the largest sums the laws
// allow (a branch sum of 65535 against +-32768 samples, K = 512), a stream cut into calls against one long call with calls
// that give no output, and n_pcm with other bytes behind it.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/hrfd.h"
static char g_err[512];
static int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
#include "../../hackrfdiags_amd/csrc/hrfd_resamp.h"

using namespace hrfd;

#define CHECK(cond)                                                  \
  do                                                                 \
  {                                                                  \
    if (!(cond))                                                     \
    {                                                                \
      printf("san_resamp: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                      \
    }                                                                \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_the_checks()
{
  static_assert(kResampMaxRatio == HRFD_RESAMP_MAX_RATIO && kResampMaxTaps == HRFD_RESAMP_MAX_TAPS &&
                    kResampMaxBranch == HRFD_RESAMP_MAX_BRANCH && kResampMaxIn == HRFD_RESAMP_MAX_IN,
                "the header's limits are the public ones");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(resamp_check_create("who", c, 1, 1, &out), "channels"));
  }
  CHECK(refused(resamp_check_create("who", 1, 1, 1, nullptr), "result pointer"));
  CHECK(refused(resamp_check_create("who", 1, 0, 1, &out), "1..512") && refused(resamp_check_create("who", 1, 1, 0, &out), "1..512"));
  CHECK(refused(resamp_check_create("who", 1, 513, 1, &out), "1..512") && refused(resamp_check_create("who", 1, 1, 513, &out), "1..512"));
  CHECK(refused(resamp_check_create("who", 1, 6, 4, &out), "gcd 2") && refused(resamp_check_create("who", 1, 512, 512, &out), "gcd 512"));
  CHECK(refused(resamp_check_create("who", 1, 1, 9, &out), "more than 8 x up") && refused(resamp_check_create("who", 1, 63, 512, &out), "more than"));
  for (uint32_t L = 1; L <= 512; L++)
  {
    for (uint32_t M = 1; M <= 512; M++)
    {
      const bool ok = resamp_gcd(L, M) == 1 && M <= 8 * L;
      CHECK((resamp_check_create("who", 65536, L, M, &out) == HRFD_OK) == ok);
    }
  }

  std::vector<int16_t> h(16385, 1);
  CHECK(refused(resamp_check_tap_list("who", h.data(), 0), "taps") && refused(resamp_check_tap_list("who", h.data(), 16385), "taps"));
  CHECK(refused(resamp_check_tap_list("who", nullptr, 1), "taps"));
  CHECK(resamp_check_taps("who", h.data(), 16384, 32) == HRFD_OK && resamp_check_taps("who", h.data(), 16384, 512) == HRFD_OK);
  CHECK(refused(resamp_check_taps("who", h.data(), 16384, 31), "529 taps per branch"));
  CHECK(resamp_check_taps("who", h.data(), 512, 1) == HRFD_OK && refused(resamp_check_taps("who", h.data(), 513, 1), "513 taps per branch"));
  CHECK(resamp_check_taps("who", h.data(), 6 * 512, 6) == HRFD_OK && refused(resamp_check_taps("who", h.data(), 6 * 512 + 1, 6), "513 taps per branch"));
  // branch 1 of 3: 32767 + 32767 + 1 passes, + 2 does not; the other branches do not count towards it
  std::vector<int16_t> b = {30000, 32767, -30000, 5000, -32767, 5000, 535, 1, 535};
  CHECK(resamp_check_taps("who", b.data(), 9, 3) == HRFD_OK);
  b[7] = 2;
  CHECK(refused(resamp_check_taps("who", b.data(), 9, 3), "branch 1 of 3 has sum |h| = 65536"));
  CHECK(resamp_check_taps("who", b.data(), 7, 3) == HRFD_OK);           // h[k] = 0 for k >= T

  CHECK(refused(pcm_check_channel("who", 5, 5), "channel 5") && pcm_check_channel("who", 4, 5) == HRFD_OK);
  CHECK(pcm_check_channel("who", HRFD_ALL_CHANNELS, 1) == HRFD_OK);
  CHECK(refused(resamp_check_n_in("who", 0), "n_in") && refused(resamp_check_n_in("who", 524289), "n_in"));
  CHECK(resamp_check_n_in("who", 1) == HRFD_OK && resamp_check_n_in("who", 524288) == HRFD_OK);
  // no call can reach this one (524288 x 512 = 2^28); the kernel's 32-bit q rests on it all the same
  CHECK(resamp_check_span("who", 524288, 512) == HRFD_OK && resamp_check_span("who", 0x7fffffffu, 1) == HRFD_OK);
  CHECK(refused(resamp_check_span("who", 0x80000000u, 1), "2^31") && refused(resamp_check_span("who", 1u << 22, 512), "2^31"));
  CHECK(resamp_check_capacity("who", 0, 0) == HRFD_OK && resamp_check_capacity("who", 48, 48) == HRFD_OK);
  CHECK(refused(resamp_check_capacity("who", 48, 47), "out_capacity 47 is below the 48") && refused(resamp_check_capacity("who", 1, 0), "below"));

  alignas(16) static char buf[32768];
  const void *in = buf + 8192, *far = buf + 24576;
  uint32_t n = 0;
  CHECK(refused(resamp_check_call("who", in, 200, true, nullptr, 0, far, 16, 8, &n, 1), "n_in"));
  CHECK(refused(resamp_check_call("who", in, 1u << 21, true, nullptr, 524289, far, 16, 8, &n, 1), "n_in"));
  CHECK(refused(resamp_check_call("who", in, 1022, true, buf, 511, far, 16, 8, &n, 1), "multiple of 512"));
  CHECK(resamp_check_call("who", in, 1024, true, buf, 512, far, 16, 8, &n, 1) == HRFD_OK);
  CHECK(refused(resamp_check_call("who", in, 1024, true, buf + 2, 512, far, 16, 8, &n, 1), "4-byte aligned"));
  CHECK(refused(resamp_check_call("who", in, 198, true, nullptr, 100, far, 16, 8, &n, 1), "channel_stride_bytes"));
  CHECK(refused(resamp_check_call("who", in, 201, true, nullptr, 100, far, 16, 8, &n, 1), "channel_stride_bytes"));
  CHECK(refused(resamp_check_call("who", in, 200, true, nullptr, 100, far, 14, 8, &n, 1), "out_stride_bytes"));
  CHECK(refused(resamp_check_call("who", in, 200, true, nullptr, 100, far, 17, 8, &n, 1), "out_stride_bytes"));
  CHECK(resamp_check_call("who", in, 0, false, nullptr, 100, far, 0, 8, &n, 2) == HRFD_OK);   // the host entry has no strides
  CHECK(refused(resamp_check_call("who", buf + 8193, 200, true, nullptr, 100, far, 16, 8, &n, 1), "even address"));
  CHECK(refused(resamp_check_call("who", in, 200, true, nullptr, 100, buf + 24577, 16, 8, &n, 1), "even address"));
  CHECK(refused(resamp_check_call("who", nullptr, 200, true, nullptr, 100, far, 16, 8, &n, 1), "NULL argument"));
  CHECK(refused(resamp_check_call("who", in, 200, true, nullptr, 100, nullptr, 16, 8, &n, 1), "NULL argument"));
  CHECK(refused(resamp_check_call("who", in, 200, true, nullptr, 100, far, 16, 8, nullptr, 1), "NULL argument"));
  // out against the input's rows: [8192, 8192 + 3 x 206 + 200) with 4 channels, out rows of 600 samples 1204 bytes apart
  CHECK(resamp_check_call("who", in, 206, true, nullptr, 100, buf + 8192 - 3 * 1204 - 1200, 1204, 600, &n, 4) == HRFD_OK);
  CHECK(refused(resamp_check_call("who", in, 206, true, nullptr, 100, buf + 8192 - 3 * 1204 - 1198, 1204, 600, &n, 4), "overlaps"));
  CHECK(resamp_check_call("who", in, 206, true, nullptr, 100, buf + 8192 + 3 * 206 + 200, 1204, 600, &n, 4) == HRFD_OK);
  CHECK(refused(resamp_check_call("who", in, 206, true, nullptr, 100, buf + 8192 + 3 * 206 + 198, 1204, 600, &n, 4), "overlaps"));
  CHECK(resamp_check_call("who", in, 206, true, nullptr, 100, buf + 8192 + 3 * 206 + 198, 1204, 600, &n, 1) == HRFD_OK);
  CHECK(refused(resamp_check_call("who", in, 0, false, nullptr, 100, buf + 8192 + 198, 0, 600, &n, 1), "overlaps"));
  CHECK(resamp_check_call("who", in, 0, false, nullptr, 100, buf + 8192 + 200, 0, 600, &n, 1) == HRFD_OK);
  return 0;
}

static int check_laws()
{
  // rounding and saturation (pcm_fir_round): tests/cpp/san_pcm.cc
  // count and phase: the outputs are those whose q lies below n_in L, and d stays in 0..M-1; a stream of single samples
  // and one of the largest calls give every output once
  for (uint32_t L : {1u, 2u, 3u, 5u, 7u, 80u, 147u, 441u, 511u, 512u})
  {
    for (uint32_t M : {1u, 2u, 3u, 6u, 8u, 80u, 160u, 441u, 511u, 512u})
    {
      if (resamp_gcd(L, M) != 1 || M > 8 * L)
      {
        continue;
      }
      for (uint32_t d = 0; d < M; d += (M > 16 ? M / 7 : 1))
      {
        for (uint32_t n_in : {1u, 2u, 3u, 511u, 512u, 513u, 524288u})
        {
          const uint32_t n_out = resamp_out_count(n_in, L, M, d);
          const uint64_t span = (uint64_t)n_in * L;
          CHECK(n_out == 0 ? span <= d : ((uint64_t)d + (uint64_t)(n_out - 1) * M < span && (uint64_t)d + (uint64_t)n_out * M >= span));
          CHECK(resamp_advance(d, n_in, n_out, L, M) < M);
        }
      }
      uint32_t d = 0, total = 0;
      for (uint32_t s = 0; s < 1000; s++)
      {
        const uint32_t n_out = resamp_out_count(1, L, M, d);
        d = resamp_advance(d, 1, n_out, L, M);
        total += n_out;
      }
      CHECK(total == (1000 * L + M - 1) / M && total == resamp_out_count(1000, L, M, 0) && d == resamp_advance(0, 1000, total, L, M));
    }
  }
  return 0;
}

static int check_extremes()
{
  // K = 512 on each of L = 2 branches, every branch sum 65535: 511 taps of 128 and one of 127 per branch, the signs of branch
  // 1 turned over.  Full-scale input of one sign: every product of a branch has one sign, acc = +-65535 x 32768
  const uint32_t L = 2, K = 512, T = L * K, n_in = 1100;
  std::vector<int16_t> h(T), hist(kResampHist, 0), x(n_in, (int16_t)-32768), y(L * n_in);
  for (uint32_t k = 0; k < K; k++)
  {
    const int16_t v = (int16_t)(k == K - 1 ? 127 : 128);
    h[2 * k] = v;
    h[2 * k + 1] = (int16_t)-v;
  }
  CHECK(resamp_check_taps("who", h.data(), T, L) == HRFD_OK);
  uint32_t d = resamp_channel_slow(x.data(), nullptr, n_in, h.data(), T, L, 1, 0, hist.data(), y.data());
  CHECK(d == 0 && y[2 * 511] == -32768 && y[2 * 511 + 1] == 32767 && y[2 * n_in - 2] == -32768 && y[2 * n_in - 1] == 32767);
  CHECK(hist[0] == -32768 && hist[511] == -32768);
  std::fill(x.begin(), x.end(), (int16_t)32767);
  std::fill(hist.begin(), hist.end(), (int16_t)0);
  resamp_channel_slow(x.data(), nullptr, n_in, h.data(), T, L, 1, 0, hist.data(), y.data());
  CHECK(y[2 * n_in - 2] == 32767 && y[2 * n_in - 1] == -32768);
  // two taps of one sign against -32768: the bound itself
  std::vector<int16_t> two = {-32768, -32767};
  std::fill(x.begin(), x.end(), (int16_t)-32768);
  std::fill(hist.begin(), hist.end(), (int16_t)0);
  resamp_channel_slow(x.data(), nullptr, n_in, two.data(), 2, 1, 1, 0, hist.data(), y.data());
  CHECK(y[0] == 32767 && y[1] == 32767 && y[n_in - 1] == 32767);
  return 0;
}

static int check_cutting_and_n_pcm()
{
  const uint32_t n = 700 + 1024;
  const uint32_t cuts[] = {1, 1, 2, 3, 1, 5, 64, 1, 100, 511, 11, 1024};        // the last with n_pcm
  uint32_t s = 4711u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 16; };
  const uint32_t ratios[][2] = {{1, 1}, {1, 6}, {1, 8}, {2, 1}, {2, 3}, {3, 2}, {6, 1}, {7, 8}, {80, 441}, {441, 80}};
  for (const auto &ratio : ratios)
  {
    {
      const uint32_t L = ratio[0], M = ratio[1];
      for (uint32_t K : {1u, 2u, 37u, 512u})
      {
        const uint32_t T = L * K - (K > 1 ? 1 : 0);
        if (T > kResampMaxTaps)
        {
          continue;
        }
        std::vector<int16_t> h(T), x(n), other(n);
        for (auto &v : h)
        {
          v = (int16_t)((int)(next() % (2 * (65535 / K) + 1)) - (int)(65535 / K));
        }
        CHECK(resamp_check_taps("who", h.data(), T, L) == HRFD_OK);
        for (auto &v : x)
        {
          v = (int16_t)next();
        }
        const uint32_t n_pcm[2] = {0xffffffffu, 300};
        other = x;
        for (uint32_t i = 700 + 512 + 300; i < n; i++)
        {
          other[i] ^= 0x5a5a;
        }
        const uint32_t total = resamp_out_count(n, L, M, 0);
        std::vector<int16_t> y(total + 1), yc(total + 1), yo(total + 1), hist(kResampHist, 0), hist_c(kResampHist, 0), hist_o(kResampHist, 0);
        // one call of 700 and one of 1024 under n_pcm; the same cut into calls; the same with other bytes behind n_pcm
        uint32_t d = resamp_channel_slow(x.data(), nullptr, 700, h.data(), T, L, M, 0, hist.data(), y.data());
        const uint32_t first = resamp_out_count(700, L, M, 0);
        CHECK(first == (700 * L + M - 1) / M);
        d = resamp_channel_slow(x.data() + 700, n_pcm, 1024, h.data(), T, L, M, d, hist.data(), y.data() + first);
        uint32_t dc = 0, dd = 0, at = 0, made = 0, made_o = 0, empty = 0;
        for (uint32_t k : cuts)
        {
          const uint32_t n_out = resamp_out_count(k, L, M, dc);
          empty += n_out == 0;
          CHECK(made + n_out <= total);
          dc = resamp_channel_slow(x.data() + at, k == 1024 ? n_pcm : nullptr, k, h.data(), T, L, M, dc, hist_c.data(), yc.data() + made);
          dd = resamp_channel_slow(other.data() + at, k == 1024 ? n_pcm : nullptr, k, h.data(), T, L, M, dd, hist_o.data(), yo.data() + made_o);
          made += n_out;
          made_o += n_out;
          at += k;
        }
        CHECK(at == n && dc == d && dd == d && made <= total);
        y.resize(made);
        yc.resize(made);
        yo.resize(made);
        CHECK(y == yc && y == yo && hist == hist_c && hist == hist_o);
        CHECK(empty > 0 || L > 1 || M == 1);
        // the history is the input's tail as the filter saw it: zero behind n_pcm
        CHECK(hist[0] == x[n - 512] && hist[299] == x[n - 512 + 299] && hist[300] == 0 && hist[511] == 0);
      }
    }
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_extremes() || check_cutting_and_n_pcm())
  {
    return 1;
  }
  printf("san_resamp ok\n");
  return 0;
}
