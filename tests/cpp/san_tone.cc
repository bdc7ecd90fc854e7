// Sanitizer harness for the HIP-free part of the tone bank (hackrfdiags_amd/csrc/hrfd_tone.h), CPU only: compiled as plain
// C++ under -fsanitize=address,undefined (tests/test_tone_sanitizers.py).  Every check at its limit with its text, the
// valid count against a count sample by sample, the slow loop at the largest sums the law allows (L = 8192, full-scale
// input of either sign under a flat window of 32767, steps 0, 1, 2^31, 2^32 - 1), the verdict on its boundaries, and the
// byte split the kernel sums with (c = 256 (c >> 8) + (c & 255)) over the whole cosine table.
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
#include "../../hackrfdiags_amd/csrc/hrfd_ddc_tables.h"
#include "../../hackrfdiags_amd/csrc/hrfd_tone.h"

using namespace hrfd;

#define CHECK(cond)                                                \
  do                                                               \
  {                                                                \
    if (!(cond))                                                   \
    {                                                              \
      printf("san_tone: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                    \
    }                                                              \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_the_checks()
{
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(tone_check_create("who", c, 256, &out), "channels"));
  }
  CHECK(refused(tone_check_create("who", 1, 256, nullptr), "result pointer"));
  for (uint32_t L : {0u, 1u, 64u, 192u, 255u, 16384u, 0x80000000u})
  {
    CHECK(refused(tone_check_create("who", 1, L, &out), "frame_len"));
  }
  for (uint32_t L = 128; L <= 8192; L *= 2)
  {
    CHECK(tone_check_create("who", 1, L, &out) == HRFD_OK && tone_check_create("who", 65536, L, &out) == HRFD_OK);
  }
  std::vector<uint32_t> steps(129, 7u);
  std::vector<uint8_t> groups(129, 3);
  CHECK(refused(tone_check_tones("who", steps.data(), nullptr, 0), "tones"));
  CHECK(refused(tone_check_tones("who", steps.data(), groups.data(), 129), "tones"));
  CHECK(refused(tone_check_tones("who", nullptr, nullptr, 1), "tones"));
  CHECK(tone_check_tones("who", steps.data(), groups.data(), 128) == HRFD_OK && tone_check_tones("who", steps.data(), nullptr, 1) == HRFD_OK);
  groups[127] = 4;
  CHECK(refused(tone_check_tones("who", steps.data(), groups.data(), 128), "group 4"));
  CHECK(tone_check_tones("who", steps.data(), groups.data(), 127) == HRFD_OK);
  std::vector<int16_t> w(8192, 32767);
  w[100] = -32767;
  CHECK(tone_check_window("who", w.data(), 8192) == HRFD_OK && tone_check_window("who", nullptr, 8192) == HRFD_OK);
  w[8191] = -32768;
  CHECK(refused(tone_check_window("who", w.data(), 8192), "entry 8191"));
  CHECK(tone_check_window("who", w.data(), 4096) == HRFD_OK);
  CHECK(refused(tone_check_threshold("who", 4, 0, 0), "group"));
  CHECK(refused(tone_check_threshold("who", 0, HRFD_TONE_MAX_RATIO + 1, 0), "ratio_q8"));
  CHECK(refused(tone_check_threshold("who", HRFD_ALL_CHANNELS, 0, HRFD_TONE_MAX_ENERGY + 1), "min_energy"));
  CHECK(tone_check_threshold("who", 3, HRFD_TONE_MAX_RATIO, HRFD_TONE_MAX_ENERGY) == HRFD_OK);
  CHECK(tone_check_threshold("who", HRFD_ALL_CHANNELS, 0, 0) == HRFD_OK);
  alignas(16) static char buf[64];
  const void *p = buf, *q = buf + 16;
  CHECK(refused(tone_check_call("who", p, 1024, true, 0, q, q, q, q, q), "n_blocks"));
  CHECK(refused(tone_check_call("who", p, 1 << 21, true, 1025, q, q, q, q, q), "n_blocks"));
  CHECK(refused(tone_check_call("who", p, 1024, true, 1, nullptr, nullptr, nullptr, nullptr, nullptr), "no output"));
  CHECK(refused(tone_check_call("who", p, 1022, true, 1, q, q, q, q, q), "channel_stride_bytes"));
  CHECK(refused(tone_check_call("who", p, 1025, true, 1, q, q, q, q, q), "channel_stride_bytes"));
  CHECK(refused(tone_check_call("who", p, 1024 * 1024 - 2, true, 1024, q, q, q, q, q), "channel_stride_bytes"));
  CHECK(tone_check_call("who", p, 0, false, 1024, q, q, q, q, q) == HRFD_OK);             // the host entry has no stride
  CHECK(refused(tone_check_call("who", buf + 1, 1024, true, 1, q, q, q, q, q), "even address"));
  CHECK(refused(tone_check_call("who", p, 1024, true, 1, buf + 20, q, q, q, q), "aligned"));
  CHECK(refused(tone_check_call("who", p, 1024, true, 1, q, buf + 12, q, q, q), "aligned"));
  CHECK(refused(tone_check_call("who", p, 1024, true, 1, q, q, buf + 18, q, q), "aligned"));
  CHECK(refused(tone_check_call("who", nullptr, 1024, true, 1, q, q, q, q, q), "NULL argument"));
  CHECK(tone_check_call("who", buf + 2, 1026, true, 1, nullptr, nullptr, buf + 20, buf + 1, buf + 3) == HRFD_OK);
  for (uint32_t L = 128; L <= 8192; L *= 2)
  {
    for (uint32_t nb = 1; nb <= 1024; nb++)
    {
      const bool whole = (512 * nb) % L == 0;
      CHECK(whole ? tone_check_frames("who", L, nb, 1) == HRFD_OK : refused(tone_check_frames("who", L, nb, 1), "frames"));
    }
    CHECK(refused(tone_check_frames("who", L, 16, 0), "no tones"));
  }
  return 0;
}

static int check_valid()
{
  const uint32_t edges[] = {0, 1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 0xffffffffu};
  const uint32_t n_blocks = 16;
  uint32_t n_pcm[16];
  for (uint32_t round = 0; round < 13; round++)
  {
    for (uint32_t b = 0; b < n_blocks; b++)
    {
      n_pcm[b] = edges[(b * 5 + round) % 13];
    }
    for (uint32_t L = 128; L <= 8192; L *= 2)
    {
      for (uint32_t f = 0; f < 512 * n_blocks / L; f++)
      {
        uint32_t want = 0;
        for (uint32_t n = 0; n < L; n++)
        {
          const uint32_t j = f * L + n;
          want += j % 512 < pcm_block_limit(n_pcm, j / 512) ? 1 : 0;
        }
        CHECK(tone_frame_valid(n_pcm, f, L) == want);
        CHECK(tone_frame_valid(nullptr, f, L) == L);
      }
    }
  }
  return 0;
}

static int check_extremes()
{
  const uint32_t L = 8192;
  const uint32_t steps[4] = {0u, 1u, 1u << 31, 0xffffffffu};
  const uint8_t groups[4] = {0, 1, 2, 2};
  std::vector<int16_t> window(L, 32767), pcm(2 * L);
  for (int v : {-32768, 32767})
  {
    for (auto &x : pcm)
    {
      x = (int16_t)v;
    }
    const int64_t u = ((int64_t)v * 32767 + (1 << 14)) >> 15;
    CHECK(tone_window(v, 32767) == u && (u == 32766 || u == -32767));
    const uint64_t E = (uint64_t)L * (uint64_t)(u * u);
    CHECK(E < (1ull << 43));
    ToneThresholds th = {{E, E + 1, 0, 0}, {0, 0, HRFD_TONE_MAX_RATIO, 0}};
    uint64_t power[4], energy = 0;
    uint32_t valid = 0;
    uint8_t best[4], present[4];
    for (uint32_t f = 0; f < 2; f++)
    {
      tone_frame_slow(pcm.data(), nullptr, f, L, window.data(), steps, groups, 4, th, Q_DDC_COS, power, &energy, &valid, best, present);
      CHECK(energy == E && valid == L);
      const int64_t I0 = tone_round15((int64_t)L * u * 32767);      // step 0: every c is COS[0], every s is COS[3072] = 0
      CHECK(power[0] == (uint64_t)(I0 * I0) && power[0] < (1ull << 57));
      // step 2^31 alternates +-32767: the sum is 0
      CHECK(power[2] == 0);
      CHECK(best[0] == 0 && best[1] == 1 && best[3] == kToneNoBest && present[3] == 0);
      CHECK(present[0] == 1);                              // E_min = E passes
      CHECK(present[1] == 0);                              // E_min = E + 1 does not
      // steps 1 and 2^32 - 1 stay on COS[0] for all 8192 samples: the power of step 0.  P is about 8192 E, above the
      // (E 2^20) >> 8 = 4096 E of the largest ratio
      CHECK(power[1] == power[0] && power[3] == power[0] && best[2] == 3 && present[2] == 1);
    }
    // a squelched second block of the first frame: valid < L, never present, and the samples there do not count
    uint32_t n_pcm[32];
    for (auto &n : n_pcm)
    {
      n = 512;
    }
    n_pcm[1] = 0;
    th.min_energy[0] = 0;
    tone_frame_slow(pcm.data(), n_pcm, 0, L, window.data(), steps, groups, 4, th, Q_DDC_COS, power, &energy, &valid, best, present);
    CHECK(valid == L - 512 && energy == E / L * (L - 512) && present[0] == 0);
  }
  return 0;
}

static int check_verdict()
{
  // P_best == (E T) >> 8 passes, one below does not; E = 256 makes (E T) >> 8 = T
  CHECK(tone_present(128, 128, 256, 0, 300, 300) && !tone_present(128, 128, 256, 0, 300, 301) && tone_present(128, 128, 256, 0, 300, 299));
  CHECK(!tone_present(127, 128, 256, 0, 300, 0) && !tone_present(128, 128, 256, 257, 300, 0) && tone_present(128, 128, 256, 256, 0, 0));
  // the largest product: E = 2^43 - 1, T = 2^20 stays inside 64 bits
  const uint64_t E = (1ull << 43) - 1;
  const unsigned __int128 wide = ((unsigned __int128)E * HRFD_TONE_MAX_RATIO) >> 8;
  CHECK(wide < ((unsigned __int128)1 << 64));
  CHECK(tone_present(8192, 8192, E, E, (uint64_t)wide, HRFD_TONE_MAX_RATIO) && !tone_present(8192, 8192, E, E, (uint64_t)wide - 1, HRFD_TONE_MAX_RATIO));
  // ties and empty groups
  const uint64_t P[5] = {5, 9, 9, 9, 1};
  const uint8_t g[5] = {0, 1, 1, 3, 3};
  CHECK(tone_best(P, g, 5, 0) == 0 && tone_best(P, g, 5, 1) == 1 && tone_best(P, g, 5, 2) == kToneNoBest && tone_best(P, g, 5, 3) == 3);
  const uint64_t Z[3] = {0, 0, 0};
  CHECK(tone_best(Z, g, 3, 1) == 1);
  return 0;
}

static int check_table_law()
{
  for (int i = 0; i < 4096; i++)
  {
    const int c = Q_DDC_COS[i];
    CHECK(c >= -32767 && c <= 32767);
    CHECK(256 * (c >> 8) + (c & 255) == c && (c >> 8) >= -128 && (c >> 8) <= 127);
    CHECK(Q_DDC_COS[tone_sin_index((uint32_t)i)] == Q_DDC_COS[(i + 3072) & 4095]);
  }
  CHECK(tone_cos_index(0) == 0 && tone_cos_index(0xffffffffu) == 0 && tone_cos_index(1u << 31) == 2048 &&
        tone_cos_index((1u << 19) - 1) == 0 && tone_cos_index(1u << 19) == 1);
  // 64 steps of a lane at the largest magnitudes stay inside int32: what lets the kernel sum without widening
  CHECK(64ll * 2 * 32767 * 255 < (1ll << 31) && 64ll * 2 * 32767 * 128 < (1ll << 31));
  CHECK(tone_round15(-1) == 0 && tone_round15(-(1 << 14)) == 0 && tone_round15(-(1 << 14) - 1) == -1 && tone_round15((1 << 14) - 1) == 0);
  return 0;
}

int main()
{
  if (check_the_checks() || check_valid() || check_extremes() || check_verdict() || check_table_law())
  {
    return 1;
  }
  printf("san_tone ok\n");
  return 0;
}
