// Sanitizer harness for the HIP-free part of the DUC bank's transmit key (hackrfdiags_amd/csrc/hrfd_duc_key.h), CPU only:
// compiled as plain C++ under -fsanitize=address,undefined (tests/test_duc_key_sanitizers.py).  Every check at its limit with
// its text, n_keys around a block's end for the smallest and the largest key block, the skip rule at tile 0, at a block's
// first tile and behind an on block, and the count of skipped units against a loop that restates the rule sample by sample.
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
#include "../../hackrfdiags_amd/csrc/hrfd_duc_key.h"

using namespace hrfd;

#define CHECK(cond)                                                    \
  do                                                                   \
  {                                                                    \
    if (!(cond))                                                       \
    {                                                                  \
      printf("san_duc_key: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
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
  static_assert(kDucKeyMinLog2 == 10 && kDucKeyMaxLog2 == 17 && kDucKeyDefaultLog2 == 17, "the header's limits");
  for (uint32_t k : {0u, 9u, 18u, 0xffffffffu})
  {
    CHECK(refused(duc_key_check_block("who", k), "key block"));
  }
  for (uint32_t k = 10; k <= 17; k++)
  {
    CHECK(duc_key_check_block("who", k) == HRFD_OK);
  }
  int out = 0;
  CHECK(refused(duc_key_check_result("who", nullptr), "NULL result") && duc_key_check_result("who", &out) == HRFD_OK);
  uint8_t key = 1;
  // 2 * (2^17 + 1) bytes: two keys at k = 17, 129 at k = 10
  const uint32_t ib = 2u * ((1u << 17) + 1u);
  CHECK(duc_key_check_stride("who", nullptr, 0, ib, 17) == HRFD_OK);              // no key: the unkeyed call
  CHECK(refused(duc_key_check_stride("who", &key, 0, ib, 17), "key_stride 0"));
  CHECK(refused(duc_key_check_stride("who", &key, 1, ib, 17), "n_keys = 2"));
  CHECK(duc_key_check_stride("who", &key, 2, ib, 17) == HRFD_OK);
  CHECK(refused(duc_key_check_stride("who", &key, 128, ib, 10), "n_keys = 129"));
  CHECK(duc_key_check_stride("who", &key, 129, ib, 10) == HRFD_OK && duc_key_check_stride("who", &key, ~0ull, ib, 10) == HRFD_OK);
  return 0;
}

static int check_n_keys()
{
  for (uint32_t k : {10u, 17u})
  {
    const uint32_t B = 1u << k;
    CHECK(duc_key_n(1, k) == 1 && duc_key_n(B - 1, k) == 1 && duc_key_n(B, k) == 1 && duc_key_n(B + 1, k) == 2);
    CHECK(duc_key_n(2 * B, k) == 2 && duc_key_n(2 * B + 1, k) == 3);
    CHECK(duc_key_block_of(0, k) == 0 && duc_key_block_of(B - 1, k) == 0 && duc_key_block_of(B, k) == 1);
  }
  CHECK(duc_key_n(1u << 24, 10) == (1u << 14) && duc_key_n(0xffffffffu, 10) == (1u << 22));    // no 32-bit wrap
  CHECK(duc_key_tiles(1) == 1 && duc_key_tiles(1024) == 1 && duc_key_tiles(1025) == 2);
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
  // k = 10: a block is a tile.  Tile 0 is never skipped; a tile is skipped when it and the one in front are off
  {
    const std::vector<uint8_t> r = row_of({0, 0, 1, 0, 0, 0x80, 0});
    const bool want[7] = {false, true, false, false, true, false, false};       // behind an on block: computed
    for (uint32_t t = 0; t < 7; t++)
    {
      CHECK(duc_key_skip(r.data(), t, 10) == want[t]);
    }
  }
  // k = 11: two tiles per block.  A block's first tile looks back into the block in front
  {
    const std::vector<uint8_t> r = row_of({0, 0, 1, 0, 0});
    const bool want[10] = {false, true, true, true, false, false, false, true, true, true};
    for (uint32_t t = 0; t < 10; t++)
    {
      CHECK(duc_key_skip(r.data(), t, 11) == want[t]);
    }
  }
  // k = 17: 128 tiles per block; M = 2^17 + 1024 has two keys and 129 tiles
  {
    const std::vector<uint8_t> off_on = row_of({0, 1}), on_off = row_of({1, 0}), off_off = row_of({0, 0});
    CHECK(!duc_key_skip(off_on.data(), 0, 17) && duc_key_skip(off_on.data(), 1, 17) && duc_key_skip(off_on.data(), 127, 17));
    CHECK(!duc_key_skip(off_on.data(), 128, 17));
    CHECK(!duc_key_skip(on_off.data(), 127, 17) && !duc_key_skip(on_off.data(), 128, 17));    // its look-back is on
    CHECK(!duc_key_skip(off_off.data(), 0, 17) && duc_key_skip(off_off.data(), 128, 17));
  }
  // the mask: the row is indexed inside the call only
  {
    const std::vector<uint8_t> r = row_of({0, 7});
    const uint32_t M = 1024 + 5;
    CHECK(duc_key_on(r.data(), -1, M, 10) && duc_key_on(r.data(), -318, M, 10));               // the history
    CHECK(!duc_key_on(r.data(), 0, M, 10) && !duc_key_on(r.data(), 1023, M, 10));
    CHECK(duc_key_on(r.data(), 1024, M, 10) && duc_key_on(r.data(), M - 1, M, 10));
    CHECK(duc_key_on(r.data(), M, M, 10) && duc_key_on(r.data(), 1ll << 40, M, 10));           // beyond the call: zeros anyway
  }
  return 0;
}

// the rule restated from the samples: a unit is skipped iff it is not the call's first tile and every sample of the tile
// and of the 1024 samples in front of it is keyed off
static uint64_t brute(const std::vector<uint8_t> &key, uint64_t stride, uint32_t C, uint32_t M, uint32_t k)
{
  uint64_t n = 0;
  for (uint32_t c = 0; c < C; c++)
  {
    for (uint32_t m0 = 1024; m0 < M; m0 += 1024)
    {
      bool any = false;
      for (uint32_t m = m0 - 1024; m < m0 + 1024 && m < M; m++)
      {
        any = any || key[c * stride + (m >> k)] != 0;
      }
      n += any ? 0u : 1u;
    }
  }
  return n;
}

static int check_the_count()
{
  uint32_t seed = 2024;
  for (uint32_t k : {10u, 11u, 13u})
  {
    for (uint32_t M : {1u, 1024u, 1025u, 5u * 1024u + 600u, (1u << 13) + 1u, 3u * (1u << 13)})
    {
      const uint32_t C = 5, nk = duc_key_n(M, k);
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
        CHECK(duc_key_count_skips(key.data(), nk + pad, C, M, k) == brute(key, nk + pad, C, M, k));
      }
    }
  }
  // all off and all on at the default block: tiles - 1 per channel, and none
  const uint32_t M = (1u << 17) + 1024;
  std::vector<uint8_t> off(2 * 2, 0), on(2 * 2, 1);
  CHECK(duc_key_count_skips(off.data(), 2, 2, M, 17) == 2 * 128 && duc_key_count_skips(on.data(), 2, 2, M, 17) == 0);
  return 0;
}

int main()
{
  if (check_the_checks() || check_n_keys() || check_the_rule() || check_the_count())
  {
    return 1;
  }
  printf("san_duc_key ok\n");
  return 0;
}
