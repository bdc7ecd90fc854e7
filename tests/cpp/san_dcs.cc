// Sanitizer harness for the HIP-free part of the DCS bank (hackrfdiags_amd/csrc/hrfd_dcs.h), CPU only: compiled as plain C++
// under -fsanitize=address,undefined (tests/test_dcs_sanitizers.py).  Every check at its limit with its text, the laws on
// their anchors (the grid's ends, the rotations, the code words and their syndromes, the alias classes of 023), the sorted
// list the kernel searches, the verdict's ties and empty groups, and the slow loop over one channel: taps at both limits with
// the largest accumulator, n_pcm with other bytes behind it, a stream cut into calls against one long call, detection of a
// code sent and silence.
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
#include "../../hackrfdiags_amd/csrc/hrfd_dcs.h"

using namespace hrfd;

#define CHECK(cond)                                                 \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      printf("san_dcs: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                     \
    }                                                               \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_the_checks()
{
  static_assert(kDcsMaxTaps == HRFD_DCS_MAX_TAPS && kDcsMaxCodes == HRFD_DCS_MAX_CODES && kDcsMaxBlocks == HRFD_DCS_MAX_BLOCKS &&
                    kDcsGroups == HRFD_DCS_GROUPS && kDcsNoBest == HRFD_DCS_NO_BEST,
                "the header's limits are the public ones");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(dcs_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(dcs_check_create("who", 1, nullptr), "result pointer") && dcs_check_create("who", 65536, &out) == HRFD_OK);

  std::vector<int16_t> t(513, 127);
  CHECK(refused(dcs_check_taps("who", t.data(), 0), "1..512 taps") && refused(dcs_check_taps("who", t.data(), 513), "1..512 taps"));
  CHECK(refused(dcs_check_taps("who", nullptr, 1), "taps") && dcs_check_taps("who", t.data(), 1) == HRFD_OK);
  CHECK(dcs_check_taps("who", t.data(), 512) == HRFD_OK);                               // 65024
  t[0] = 127 + 511;
  CHECK(dcs_check_taps("who", t.data(), 512) == HRFD_OK);                               // 65535
  t[1] = -128;
  CHECK(refused(dcs_check_taps("who", t.data(), 512), "sum |h| = 65536"));

  uint16_t codes[129];
  uint8_t inv[129], grp[129];
  for (uint32_t k = 0; k < 129; k++)
  {
    codes[k] = 0;
    inv[k] = 0;
    grp[k] = (uint8_t)(k % 4);
  }
  CHECK(dcs_check_codes("who", nullptr, nullptr, nullptr, 0) == HRFD_OK && dcs_check_codes("who", codes, inv, grp, 1) == HRFD_OK);
  CHECK(refused(dcs_check_codes("who", codes, inv, grp, 129), "at most 128") && refused(dcs_check_codes("who", nullptr, inv, grp, 1), "their array"));
  codes[1] = 512;
  CHECK(refused(dcs_check_codes("who", codes, inv, grp, 2), "entry 1 has code 512") && dcs_check_codes("who", codes, inv, grp, 1) == HRFD_OK);
  codes[1] = 0777;
  grp[1] = 4;
  CHECK(refused(dcs_check_codes("who", codes, inv, grp, 2), "entry 1 has group 4") && dcs_check_codes("who", codes, inv, nullptr, 2) == HRFD_OK);
  grp[1] = 3;
  const uint16_t three[3] = {023, 0754, 0340};
  CHECK(refused(dcs_check_codes("who", three, nullptr, nullptr, 3), "entries 0 (D023N) and 2 (D340N) are aliases"));
  CHECK(dcs_check_codes("who", three, nullptr, nullptr, 2) == HRFD_OK);
  const uint16_t pair[2] = {023, 047};
  const uint8_t second[2] = {0, 1}, both[2] = {9, 1};
  CHECK(refused(dcs_check_codes("who", pair, second, nullptr, 2), "entries 0 (D023N) and 1 (D047I)"));
  CHECK(dcs_check_codes("who", pair, nullptr, nullptr, 2) == HRFD_OK && dcs_check_codes("who", pair, both, nullptr, 2) == HRFD_OK);
  // the largest list there is: one entry of every class, until 128 are found
  uint32_t K = 0;
  for (uint32_t c = 0; c < 512 && K < 128; c++)
  {
    codes[K] = (uint16_t)c;
    inv[K] = 0;
    K += dcs_check_codes("who", codes, inv, nullptr, K + 1) == HRFD_OK ? 1 : 0;
  }
  CHECK(K == 128 && dcs_check_codes("who", codes, inv, grp, 128) == HRFD_OK);

  CHECK(dcs_check_min_hits("who", 0, 1) == HRFD_OK && dcs_check_min_hits("who", 3, 512) == HRFD_OK);
  CHECK(dcs_check_min_hits("who", HRFD_ALL_CHANNELS, 128) == HRFD_OK);
  CHECK(refused(dcs_check_min_hits("who", 4, 128), "group 4") && refused(dcs_check_min_hits("who", 0, 0), "min_hits 0"));
  CHECK(refused(dcs_check_min_hits("who", 0, 513), "min_hits 513"));

  alignas(16) static char buf[65536];
  const void *in = buf + 16384, *h = buf + 2, *b = buf + 8193, *p = buf + 12291, *n = buf + 4096;
  CHECK(dcs_check_call("who", in, 1024, true, n, 1, h, b, p) == HRFD_OK && dcs_check_call("who", in, 0, false, nullptr, 1024, h, b, p) == HRFD_OK);
  CHECK(refused(dcs_check_call("who", in, 1024, true, n, 0, h, b, p), "n_blocks"));
  CHECK(refused(dcs_check_call("who", in, 1 << 21, true, n, 1025, h, b, p), "n_blocks"));
  CHECK(refused(dcs_check_call("who", in, 1024, true, n, 1, nullptr, nullptr, nullptr), "no output"));
  CHECK(dcs_check_call("who", in, 1024, true, n, 1, h, nullptr, nullptr) == HRFD_OK && dcs_check_call("who", in, 1024, true, n, 1, nullptr, b, nullptr) == HRFD_OK);
  CHECK(dcs_check_call("who", in, 1024, true, n, 1, nullptr, nullptr, p) == HRFD_OK);
  CHECK(refused(dcs_check_call("who", in, 1022, true, n, 1, h, b, p), "channel_stride_bytes"));
  CHECK(refused(dcs_check_call("who", in, 1025, true, n, 1, h, b, p), "channel_stride_bytes"));
  CHECK(dcs_check_call("who", in, 1026, true, n, 1, h, b, p) == HRFD_OK);
  CHECK(refused(dcs_check_call("who", buf + 16385, 1024, true, n, 1, h, b, p), "even addresses"));
  CHECK(refused(dcs_check_call("who", in, 1024, true, n, 1, buf + 3, b, p), "even addresses"));
  CHECK(refused(dcs_check_call("who", in, 1024, true, buf + 4098, 1, h, b, p), "4-byte aligned"));
  CHECK(refused(dcs_check_call("who", nullptr, 1024, true, n, 1, h, b, p), "NULL argument"));
  return 0;
}

static int check_laws()
{
  CHECK(dcs_delay(0) == 0 && dcs_delay(1) == 59 && dcs_delay(2) == 119 && dcs_delay(21) == 1250 && dcs_delay(22) == 1309 && kDcsReach == 1309);
  CHECK(dcs_rot23(1, 1) == 1u << 22 && dcs_rot23(1u << 22, 22) == 1 && dcs_rot23(0x7fffff, 7) == 0x7fffff && dcs_rot23(0x123456, 0) == 0x123456);
  CHECK(dcs_canonical(0) == 0 && dcs_canonical(0x7fffff) == 0x7fffff && dcs_canonical(1u << 22) == 1 && dcs_canonical(0x600001) == 7);
  CHECK(dcs_word(023, false) == 0x763813 && dcs_word(023, true) == (0x763813 ^ 0x7fffff));
  uint32_t same[4], n_same = 0, comp[4], n_comp = 0;
  const uint32_t c023 = dcs_canonical(dcs_word(023, false)), i023 = dcs_canonical(dcs_word(023, true));
  for (uint32_t c = 0; c < 512; c++)
  {
    const uint32_t w = dcs_word(c, false);
    CHECK((w & 0xfff) == (0x800 | c) && w <= kDcsWordMask);
    for (uint32_t r = 0; r < kDcsWordBits; r++)
    {
      CHECK(dcs_syndrome(dcs_rot23(w, r)) == 0 && dcs_canonical(dcs_rot23(w, r)) == dcs_canonical(w));
    }
    CHECK(dcs_syndrome(w ^ 1) != 0 && dcs_canonical(w) != 0 && dcs_canonical(w ^ kDcsWordMask) != kDcsWordMask);
    if (dcs_canonical(w) == c023 && n_same < 4)
    {
      same[n_same++] = c;
    }
    if (dcs_canonical(w) == i023 && n_comp < 4)
    {
      comp[n_comp++] = c;
    }
  }
  CHECK(n_same == 3 && same[0] == 023 && same[1] == 0340 && same[2] == 0766);
  CHECK(n_comp == 3 && comp[0] == 047 && comp[1] == 0375 && comp[2] == 0707);

  const uint32_t canon[5] = {900, 5, 70000, 6, 1};
  uint32_t sorted[kDcsMaxCodes];
  uint8_t entry[kDcsMaxCodes];
  dcs_sorted_list(canon, 5, sorted, entry);
  CHECK(sorted[0] == 1 && sorted[1] == 5 && sorted[2] == 6 && sorted[3] == 900 && sorted[4] == 70000 && sorted[5] == kDcsNoEntry && sorted[127] == kDcsNoEntry);
  CHECK(entry[0] == 4 && entry[1] == 1 && entry[2] == 3 && entry[3] == 0 && entry[4] == 2);
  dcs_sorted_list(canon, 0, sorted, entry);
  CHECK(sorted[0] == kDcsNoEntry);

  const uint16_t hits[6] = {0, 7, 7, 0, 512, 0};
  const uint8_t grp[6] = {0, 1, 1, 0, 2, 0};
  CHECK(dcs_best(hits, grp, 6, 0) == 0 && dcs_best(hits, grp, 6, 1) == 1 && dcs_best(hits, grp, 6, 2) == 4 && dcs_best(hits, grp, 6, 3) == kDcsNoBest);
  CHECK(dcs_best(hits, grp, 0, 0) == kDcsNoBest && dcs_best(hits, grp, 3, 1) == 1);
  return 0;
}

static uint32_t g_seed = 754u;
static uint32_t next() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// the NRZ row of a word from stream time t0 on
static void levels(uint32_t word, int16_t amp, uint32_t t0, int16_t *x, uint32_t n)
{
  for (uint32_t i = 0; i < n; i++)
  {
    x[i] = (word >> ((((uint64_t)(t0 + i) * 21) / 1250) % 23)) & 1 ? amp : (int16_t)-amp;
  }
}

static int check_the_slow_loop()
{
  const uint32_t B = 9, n = B * kDcsBlock;
  const uint16_t codes[3] = {0754, 023, 0411};
  const uint8_t grp[3] = {0, 0, 2};
  uint32_t canon[3];
  for (int k = 0; k < 3; k++)
  {
    canon[k] = dcs_canonical(dcs_word(codes[k], k == 1));
  }
  const uint32_t min_hits[4] = {128, 1, 512, 1};
  // the largest accumulator both ways: sum |h| = 65535 against full scale, T = 512 and T = 1
  std::vector<int16_t> big(512, 127), one(1, 16384), x(n), other(n);
  big[0] = 127 + 511;
  for (uint32_t i = 0; i < n; i++)
  {
    x[i] = (i / 700) % 2 ? -32768 : 32767;
  }
  std::vector<uint32_t> st(kDcsStateDw, 0);
  std::vector<uint16_t> hits(B * 3);
  std::vector<uint8_t> best(B * 4), present(B * 4);
  dcs_channel_slow(x.data(), nullptr, B, big.data(), 512, canon, grp, 3, min_hits, st.data(), hits.data(), best.data(), present.data());
  for (int16_t &v : big)
  {
    v = (int16_t)-v;
  }
  dcs_channel_slow(x.data(), nullptr, B, big.data(), 512, canon, grp, 3, min_hits, st.data(), hits.data(), best.data(), present.data());

  // D754 at 2000 with a little noise: found from block 4 on, group 1 empty, group 2's entry unseen; silence after a reset
  levels(dcs_word(0754, false), 2000, 0, x.data(), n);
  for (uint32_t i = 0; i < n; i++)
  {
    x[i] = (int16_t)(x[i] + (int32_t)(next() % 401) - 200);
  }
  std::fill(st.begin(), st.end(), 0u);
  dcs_channel_slow(x.data(), nullptr, B, one.data(), 1, canon, grp, 3, min_hits, st.data(), hits.data(), best.data(), present.data());
  for (uint32_t b = 0; b < B; b++)
  {
    CHECK(best[4 * b] == 0 && best[4 * b + 1] == kDcsNoBest && best[4 * b + 2] == 2 && best[4 * b + 3] == kDcsNoBest);
    CHECK(present[4 * b + 1] == 0 && present[4 * b + 2] == 0 && present[4 * b + 3] == 0 && hits[3 * b + 1] == 0 && hits[3 * b + 2] == 0);
    CHECK(present[4 * b] == (b >= 4 ? 1 : present[4 * b]) && (b >= 2 || hits[3 * b] == 0) && hits[3 * b] <= 512);
  }
  CHECK(st[kDcsStateDw - 1] == 0 && st[kDcsStateDw - 3] == 0 && (uint16_t)st[255] == (uint16_t)x[n - 2] && (uint16_t)(st[255] >> 16) == (uint16_t)x[n - 1]);
  CHECK((st[kDcsHistDw + kDcsBitDw - 1] >> 31) == (x[n - 1] > 0 ? 1u : 0u));

  // cut 4 + 1 + 3 + 1 against one call, with n_pcm and other bytes behind it; each output alone
  const uint32_t n_pcm[B] = {512, 0xffffffffu, 300, 512, 512, 0, 511, 512, 1};
  other = x;
  for (uint32_t b = 0; b < B; b++)
  {
    for (uint32_t i = pcm_block_limit(n_pcm, b); i < kDcsBlock; i++)
    {
      other[b * kDcsBlock + i] ^= 0x5a5a;
    }
  }
  std::vector<uint32_t> st_a(kDcsStateDw, 0), st_b(kDcsStateDw, 0), st_c(kDcsStateDw, 0);
  std::vector<uint16_t> hits_b(B * 3), hits_c(B * 3);
  std::vector<uint8_t> best_b(B * 4), present_b(B * 4);
  dcs_channel_slow(x.data(), n_pcm, B, one.data(), 1, canon, grp, 3, min_hits, st_a.data(), hits.data(), best.data(), present.data());
  const uint32_t cuts[] = {4, 1, 3, 1};
  uint32_t at = 0;
  for (uint32_t k : cuts)
  {
    dcs_channel_slow(other.data() + at * kDcsBlock, n_pcm + at, k, one.data(), 1, canon, grp, 3, min_hits, st_b.data(), hits_b.data() + at * 3,
                     best_b.data() + at * 4, present_b.data() + at * 4);
    dcs_channel_slow(x.data() + at * kDcsBlock, n_pcm + at, k, one.data(), 1, canon, grp, 3, min_hits, st_c.data(), hits_c.data() + at * 3, nullptr,
                     nullptr);
    at += k;
  }
  CHECK(hits == hits_b && best == best_b && present == present_b && st_a == st_b && hits == hits_c && st_a == st_c);
  // an empty list, verdicts only
  dcs_channel_slow(x.data(), nullptr, 2, one.data(), 1, nullptr, nullptr, 0, min_hits, st_a.data(), nullptr, best.data(), present.data());
  CHECK(best[0] == kDcsNoBest && best[7] == kDcsNoBest && present[0] == 0 && present[7] == 0);
  // silence: no hits
  std::fill(st.begin(), st.end(), 0u);
  std::fill(x.begin(), x.end(), (int16_t)0);
  dcs_channel_slow(x.data(), nullptr, B, one.data(), 1, canon, grp, 3, min_hits, st.data(), hits.data(), best.data(), present.data());
  for (uint32_t i = 0; i < B * 3; i++)
  {
    CHECK(hits[i] == 0);
  }
  for (uint32_t i = 0; i < kDcsStateDw; i++)
  {
    CHECK(st[i] == 0);
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_the_slow_loop())
  {
    return 1;
  }
  printf("san_dcs ok\n");
  return 0;
}
