// Sanitizer harness for the HIP-free part of the DDC bank's receive key (hackrfdiags_amd/csrc/hrfd_ddc_key.h), CPU only:
// compiled as plain C++ under -fsanitize=address,undefined (tests/test_ddc_key_sanitizers.py).  Every check at its limit with
// its text, n_keys around a block's end for the smallest and the largest key block, the skip rule at tile 0 and at a block's
// first and last tile, and the per-channel count of skipped units against a loop that restates the rule sample by sample.
// Every key row is a heap buffer of exactly n_keys bytes: the sanitizer sees an index past the call.
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
#include "../../hackrfdiags_amd/csrc/hrfd_ddc_key.h"

using namespace hrfd;

#define CHECK(cond)                                                    \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      printf("san_ddc_key: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_the_checks()
{
  static_assert(kDdcKeyMinLog2 == 10 && kDdcKeyMaxLog2 == 17 && kDdcKeyDefaultLog2 == 17, "the header's limits");
  for (uint32_t k : {0u, 9u, 18u, 0xffffffffu})
  {
    CHECK(refused(ddc_key_check_block("who", k), "key block"));
  }
  for (uint32_t k = 10; k <= 17; k++)
  {
    CHECK(ddc_key_check_block("who", k) == HRFD_OK);
  }
  int out = 0;
  CHECK(refused(ddc_key_check_result("who", nullptr), "NULL result") && ddc_key_check_result("who", &out) == HRFD_OK);
  CHECK(ddc_key_check_channel("who", 0, 5) == HRFD_OK && ddc_key_check_channel("who", 4, 5) == HRFD_OK);
  CHECK(ddc_key_check_channel("who", HRFD_ALL_CHANNELS, 5) == HRFD_OK);
  CHECK(refused(ddc_key_check_channel("who", 5, 5), "channel 5") && refused(ddc_key_check_channel("who", 0xfffffffeu, 5), "channel"));
  uint8_t key = 1;
  // 2 * (2^17 + 1) bytes: two keys at k = 17, 129 at k = 10
  const uint32_t ob = 2u * ((1u << 17) + 1u);
  CHECK(ddc_key_check_stride("who", nullptr, 0, ob, 17) == HRFD_OK);              // no key: the unkeyed call
  CHECK(refused(ddc_key_check_stride("who", &key, 0, ob, 17), "key_stride 0"));
  CHECK(refused(ddc_key_check_stride("who", &key, 1, ob, 17), "n_keys = 2"));
  CHECK(ddc_key_check_stride("who", &key, 2, ob, 17) == HRFD_OK);
  CHECK(refused(ddc_key_check_stride("who", &key, 128, ob, 10), "n_keys = 129"));
  CHECK(ddc_key_check_stride("who", &key, 129, ob, 10) == HRFD_OK && ddc_key_check_stride("who", &key, ~0ull, ob, 10) == HRFD_OK);
  return 0;
}

static int check_n_keys()
{
  for (uint32_t k : {10u, 17u})
  {
    const uint32_t B = 1u << k;
    CHECK(ddc_key_n(1, k) == 1 && ddc_key_n(B - 1, k) == 1 && ddc_key_n(B, k) == 1 && ddc_key_n(B + 1, k) == 2);
    CHECK(ddc_key_n(2 * B, k) == 2 && ddc_key_n(2 * B + 1, k) == 3);
    CHECK(ddc_key_block_of(0, k) == 0 && ddc_key_block_of(B - 1, k) == 0 && ddc_key_block_of(B, k) == 1);
  }
  CHECK(ddc_key_n(1024, 10) == 1 && ddc_key_n(1025, 10) == 2 && ddc_key_n(1024, 17) == 1 && ddc_key_n(1025, 17) == 1);
  CHECK(ddc_key_n(1u << 24, 10) == (1u << 14) && ddc_key_n(0xffffffffu, 10) == (1u << 22));    // no 32-bit wrap
  CHECK(ddc_key_tiles(1) == 1 && ddc_key_tiles(1024) == 1 && ddc_key_tiles(1025) == 2);
  return 0;
}

// a key row of exactly n bytes on the heap
static std::vector<uint8_t> row_of(std::initializer_list<int> v)
{
  std::vector<uint8_t> r;
  for (int x : v)
  {
    r.push_back((uint8_t)x);
  }
  r.shrink_to_fit();
  return r;
}

static int check_the_rule()
{
  // k = 10: a block is a tile, and a tile is skipped iff its own byte is off: no floor at tile 0, no look-back
  {
    const std::vector<uint8_t> r = row_of({0, 0, 1, 0, 0, 0x80, 0});
    const bool want[7] = {true, true, false, true, true, false, true};
    for (uint32_t t = 0; t < 7; t++)
    {
      CHECK(ddc_key_skip(r.data(), t, 10) == want[t]);
    }
  }
  // k = 11: two tiles per block
  {
    const std::vector<uint8_t> r = row_of({0, 0, 2, 0, 0});
    const bool want[10] = {true, true, true, true, false, false, true, true, true, true};
    for (uint32_t t = 0; t < 10; t++)
    {
      CHECK(ddc_key_skip(r.data(), t, 11) == want[t]);
    }
  }
  // k = 17: 128 tiles per block; M = 2^17 + 1024 has two keys and 129 tiles
  {
    const std::vector<uint8_t> off_on = row_of({0, 1}), on_off = row_of({1, 0});
    CHECK(ddc_key_skip(off_on.data(), 0, 17) && ddc_key_skip(off_on.data(), 127, 17) && !ddc_key_skip(off_on.data(), 128, 17));
    CHECK(!ddc_key_skip(on_off.data(), 0, 17) && !ddc_key_skip(on_off.data(), 127, 17) && ddc_key_skip(on_off.data(), 128, 17));
  }
  return 0;
}

// the rule restated from the samples: a unit is skipped iff every output sample of the tile is keyed off
static uint64_t brute(const std::vector<uint8_t> &key, uint64_t stride, uint32_t c, uint32_t M, uint32_t k)
{
  uint64_t n = 0;
  for (uint32_t m0 = 0; m0 < M; m0 += 1024)
  {
    bool any = false;
    for (uint32_t m = m0; m < m0 + 1024 && m < M; m++)
    {
      any = any || key[c * stride + (m >> k)] != 0;
    }
    n += any ? 0u : 1u;
  }
  return n;
}

static int check_the_count()
{
  uint32_t seed = 2025;
  for (uint32_t k : {10u, 11u, 13u})
  {
    for (uint32_t M : {1u, 1023u, 1024u, 1025u, 5u * 1024u + 37u, (1u << 13) + 1u, 3u * (1u << 13)})
    {
      const uint32_t C = 5, nk = ddc_key_n(M, k);
      for (uint32_t pad : {0u, 3u})
      {
        // rows nk + pad apart; the buffer ends with the last row's last key
        std::vector<uint8_t> key((size_t)(C - 1) * (nk + pad) + nk, 0xff);
        for (uint32_t c = 0; c < C; c++)
        {
          for (uint32_t j = 0; j < nk; j++)
          {
            seed = seed * 1664525u + 1013904223u;
            key[(size_t)c * (nk + pad) + j] = (seed >> 24) % 3 == 0 ? (uint8_t)(seed >> 16 | 1) : 0;
          }
        }
        key.shrink_to_fit();
        std::vector<uint64_t> per(C, 99);
        per.shrink_to_fit();
        const uint64_t sum = ddc_key_count_skips(key.data(), nk + pad, C, M, k, per.data());
        uint64_t want = 0;
        for (uint32_t c = 0; c < C; c++)
        {
          CHECK(per[c] == brute(key, nk + pad, c, M, k));
          want += per[c];
        }
        CHECK(sum == want && ddc_key_count_skips(key.data(), nk + pad, C, M, k, nullptr) == want);
      }
    }
  }
  // all off and all on at the default block: every tile of every channel, and none
  const uint32_t M = (1u << 17) + 1024;
  std::vector<uint8_t> off(2 * 2, 0), on(2 * 2, 1);
  CHECK(ddc_key_count_skips(off.data(), 2, 2, M, 17, nullptr) == 2 * 129 && ddc_key_count_skips(on.data(), 2, 2, M, 17, nullptr) == 0);
  return 0;
}

int main()
{
  if (check_the_checks() || check_n_keys() || check_the_rule() || check_the_count())
  {
    return 1;
  }
  printf("san_ddc_key ok\n");
  return 0;
}
