// Sanitizer harness for the HIP-free part of the AFSK bank (hackrfdiags_amd/csrc/hrfd_afsk.h), CPU only: compiled as plain
// C++ under -fsanitize=address,undefined (tests/test_afsk_sanitizers.py).  Every check at its limit with its text, the laws
// on their boundaries (the tap clamp, the nudge on both sides of mid-bit and at the ends of the phase circle, the bit byte,
// the row bound), full-scale input whose signs follow the taps so that |I| reaches its bound and the powers need their 64
// bits, and the slow loop over random input: the row bound, a stream cut into calls against one long call, a call without
// bits, and n_pcm with other bytes behind it.
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
#include "../../hackrfdiags_amd/csrc/hrfd_afsk.h"
#include "../../hackrfdiags_amd/csrc/hrfd_ddc_tables.h"

using namespace hrfd;

#define CHECK(cond)                                                 \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      printf("san_afsk: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                     \
    }                                                               \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static const AfskModem kBell202 = {kAfskDefaultMark, kAfskDefaultSpace, kAfskDefaultBaud, 8, 2, 1};

static int check_the_checks()
{
  static_assert(kAfskMaxWindow == HRFD_AFSK_MAX_WINDOW && kAfskMaxBlocks == HRFD_AFSK_MAX_BLOCKS, "the header's limits are the public ones");
  static_assert(sizeof(AfskState) == 72, "18 dwords of state");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(afsk_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(afsk_check_create("who", 1, nullptr), "result pointer") && afsk_check_create("who", 65536, &out) == HRFD_OK);

  CHECK(afsk_check_modem("who", kBell202) == HRFD_OK);
  AfskModem m = kBell202;
  for (uint32_t W : {0u, 1u, 33u})
  {
    m.W = W;
    CHECK(refused(afsk_check_modem("who", m), "window"));
  }
  m = kBell202;
  for (uint32_t A : {0u, 9u})
  {
    m.A = A;
    CHECK(refused(afsk_check_modem("who", m), "loop shift"));
  }
  for (uint32_t s : {0u, (1u << 31) + 1u, 0xffffffffu})
  {
    m = kBell202;
    m.baud_step = s;
    CHECK(refused(afsk_check_modem("who", m), "baud_step"));
    m = kBell202;
    m.mark_step = s;
    CHECK(refused(afsk_check_modem("who", m), "mark_step"));
    m = kBell202;
    m.space_step = s;
    CHECK(refused(afsk_check_modem("who", m), "space_step"));
  }
  m = AfskModem{1u << 31, 1u, 1u << 31, 2, 1, 0};
  CHECK(afsk_check_modem("who", m) == HRFD_OK);
  m = AfskModem{1u, 1u << 31, 1u, 32, 8, 1};
  CHECK(afsk_check_modem("who", m) == HRFD_OK);

  alignas(16) static char buf[65536];
  const void *in = buf + 16384, *b = buf + 1, *n = buf + 4096, *h = buf + 8193;
  CHECK(refused(afsk_check_call("who", in, 1024, true, nullptr, 0, b, n, h), "n_blocks"));
  CHECK(refused(afsk_check_call("who", in, 1 << 21, true, nullptr, 1025, b, n, h), "n_blocks"));
  CHECK(refused(afsk_check_call("who", in, 1024, true, nullptr, 1, nullptr, nullptr, nullptr), "no output"));
  CHECK(refused(afsk_check_call("who", in, 1024, true, nullptr, 1, b, nullptr, h), "go together"));
  CHECK(refused(afsk_check_call("who", in, 1024, true, nullptr, 1, nullptr, n, nullptr), "go together"));
  CHECK(afsk_check_call("who", in, 1024, true, nullptr, 1, nullptr, nullptr, h) == HRFD_OK);
  CHECK(afsk_check_call("who", in, 1024, true, nullptr, 1, b, n, nullptr) == HRFD_OK);
  CHECK(refused(afsk_check_call("who", in, 1022, true, nullptr, 1, b, n, h), "channel_stride_bytes"));
  CHECK(refused(afsk_check_call("who", in, 1025, true, nullptr, 1, b, n, h), "channel_stride_bytes"));
  CHECK(afsk_check_call("who", in, 0, false, nullptr, 1, b, n, h) == HRFD_OK);                  // the host entry has no strides
  CHECK(refused(afsk_check_call("who", buf + 16385, 1024, true, nullptr, 1, b, n, h), "even address"));
  CHECK(afsk_check_call("who", buf + 16386, 1030, true, buf + 8, 1, b, n, h) == HRFD_OK);
  CHECK(refused(afsk_check_call("who", in, 1024, true, buf + 2, 1, b, n, h), "4-byte aligned"));
  CHECK(refused(afsk_check_call("who", in, 1024, true, nullptr, 1, b, buf + 4098, h), "4-byte aligned"));
  CHECK(refused(afsk_check_call("who", nullptr, 1024, true, nullptr, 1, b, n, h), "NULL argument"));
  CHECK(refused(afsk_check_blocks("who", 0), "n_blocks") && afsk_check_blocks("who", 1024) == HRFD_OK);
  CHECK(refused(afsk_check_bits_stride("who", 615, 616), "bits_stride_bytes 615 is below") && afsk_check_bits_stride("who", 616, 616) == HRFD_OK);
  return 0;
}

static int check_laws()
{
  // 1. taps: cos 0 = 32767 -> 2048 clamps to 2047; the sine a quarter turn behind; zero from W on
  CHECK(afsk_tap_round(32767) == 2047 && afsk_tap_round(-32767) == -2047 && afsk_tap_round(0) == 0 && afsk_tap_round(-8) == 0);
  CHECK(afsk_tap_round(-9) == -1 && afsk_tap_round(7) == 0 && afsk_tap_round(8) == 1 && afsk_tap_round(-24) == -1 && afsk_tap_round(-25) == -2);
  int16_t taps[kAfskFilters * kAfskMaxWindow];
  afsk_taps(Q_DDC_COS, 1u << 30, 1u << 31, 5, taps);               // 2 kHz: 1 0 -1 0 1; 4 kHz: 1 -1 1 -1 1
  const int16_t want[4][6] = {{2047, 0, -2047, 0, 2047, 0}, {0, 2047, 0, -2047, 0, 0}, {2047, -2047, 2047, -2047, 2047, 0}, {0, 0, 0, 0, 0, 0}};
  for (int f = 0; f < 4; f++)
  {
    for (int k = 0; k < 6; k++)
    {
      CHECK(taps[f * kAfskMaxWindow + k] == want[f][k]);
    }
  }
  // 2. the powers at the bound: |I| = |Q| = 32 x 32768 x 2047 needs 62 bits a square, 63 a power, 64 the sum of two
  const int32_t top = 32 * 32768 * 2047;
  CHECK(afsk_power(top, -top) == 2ull * (uint64_t)top * (uint64_t)top && afsk_power(top, top) > (1ull << 62) && afsk_power(top, top) < (1ull << 63));
  CHECK(afsk_power(-top, 0) == (uint64_t)top * (uint64_t)top && afsk_power(0, 0) == 0);
  const uint64_t pt = afsk_power(top, top);
  CHECK(afsk_carrier(pt, pt, ~0ull) == 0 && afsk_carrier(pt, pt, 2 * pt - 1) == 1 && afsk_carrier(pt, pt, 2 * pt) == 0 && 2 * pt > (1ull << 63));
  CHECK(afsk_carrier(0, 0, 0) == 0 && afsk_carrier(1, 0, 0) == 1);
  // 3. the decision: strictly greater
  CHECK(afsk_decide(1, 0) == 1 && afsk_decide(0, 0) == 0 && afsk_decide(pt, pt) == 0 && afsk_decide(pt, pt - 1) == 1 && afsk_decide(0, pt) == 0);
  // 4. the nudge: towards 2^31 from both sides, by 1 / 2^A of the distance (the shift floors), fixed at 2^31, never across 0
  CHECK(afsk_nudge(1u << 31, 1) == 1u << 31 && afsk_nudge(0, 1) == 1u << 30 && afsk_nudge(0, 8) == 1u << 23);
  CHECK(afsk_nudge(0xffffffffu, 1) == 0xffffffffu - 0x3fffffffu && afsk_nudge(0xffffffffu, 8) == 0xffffffffu - 0x7fffffu);
  CHECK(afsk_nudge((1u << 31) + 1, 1) == (1u << 31) + 1 && afsk_nudge((1u << 31) - 1, 1) == 1u << 31 && afsk_nudge((1u << 31) + 2, 1) == (1u << 31) + 1);
  for (uint32_t A = 1; A <= 8; A++)
  {
    for (uint32_t p : {0u, 1u, 12345u, (1u << 31) - 2, (1u << 31) + 7, 0xfffffffeu, 0xffffffffu})
    {
      const uint32_t q = afsk_nudge(p, A);
      CHECK(p < (1u << 31) ? (q >= p && q <= (1u << 31) && q - p <= ((1u << 31) >> A)) : (q <= p && q >= (1u << 31)));
    }
  }
  // 5. the bit byte
  CHECK(afsk_bit(1, 0, false, 0) == 1 && afsk_bit(0, 1, false, 1) == 2 && afsk_bit(1, 1, false, 1) == 3);
  CHECK(afsk_bit(1, 0, true, 0) == 0 && afsk_bit(0, 1, true, 0) == 0 && afsk_bit(1, 1, true, 1) == 3 && afsk_bit(0, 0, true, 0) == 1);
  // the row bound: Bell 202 over 16 blocks; the extremes stay in 32 bits
  CHECK(afsk_max_bits(kAfskDefaultBaud, 2, 16) == 2253 && afsk_max_bits(1, 8, 1) == 2 && afsk_max_bits(1u << 31, 1, 1024) == 393217);
  return 0;
}

static uint32_t g_seed = 1202u;
static uint32_t next() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// |I| reaches W x 32768 x 2047 where the input is -32768 times the sign of the taps, and the sum stays an int32
static int check_the_bound_is_reached()
{
  const AfskModem m = {1u << 31, 1u << 30, 1u << 31, 32, 1, 0};     // mark at 4 kHz: every cosine tap is +-2047
  int16_t taps[kAfskFilters * kAfskMaxWindow];
  afsk_taps(Q_DDC_COS, m.mark_step, m.space_step, m.W, taps);
  std::vector<int16_t> x(kAfskBlock);
  for (uint32_t n = 0; n < kAfskBlock; n++)
  {
    x[n] = (int16_t)((n & 1u) ? -32768 : 32767);
  }
  x[100] = -32768;                                                  // (a slip: the decisions still hold)
  AfskState st = {};
  uint8_t hard[kAfskHardPerBlock], bits[520];
  uint32_t n_bits = 0;
  afsk_channel_slow(x.data(), nullptr, 1, m, taps, (1ull << 61), &st, bits, &n_bits, hard);
  CHECK(n_bits >= 255 && n_bits <= 257 && n_bits <= afsk_max_bits(m.baud_step, m.A, 1));      // a bit every other sample
  for (uint32_t i = 100; i < n_bits; i++)
  {
    CHECK(bits[i] == 3);                                            // mark, with a power above 2^61: no 32-bit square
  }
  // the very bound: all samples -32768 against taps of one sign (DC would need a zero step; the alternating tone's sign
  // pattern times alternating -32768 / 32767 comes within 32 of it): |I| = 16 x 32768 x 2047 + 16 x 32767 x 2047
  int32_t acc = 0;
  for (uint32_t k = 0; k < 32; k++)
  {
    acc += x[200 - k] * taps[kAfskMarkC * kAfskMaxWindow + k];
  }
  CHECK((acc < 0 ? -(int64_t)acc : (int64_t)acc) == 16ll * 32768 * 2047 + 16ll * 32767 * 2047);
  return 0;
}

// random modems over noisy two-tone input: the row bound, the cut into calls, a call without bits, other bytes behind n_pcm
static int check_bound_and_cutting()
{
  const uint32_t B = 16, n = B * kAfskBlock;
  const uint32_t cuts[] = {1, 4, 5, 6};
  for (int round = 0; round < 24; round++)
  {
    const uint32_t Ws[] = {2, 7, 8, 27, 32, 2 + next() % 31};
    const uint32_t bauds[] = {161061274u, 644245094u, 1u << 31, 1u + next() % (1u << 31)};
    AfskModem m = {1u + next() % (1u << 31), 1u + next() % (1u << 31), bauds[next() % 4], Ws[next() % 6], 1 + next() % 8, next() % 2};
    if (round < 3)
    {
      m = kBell202;
      m.A = round == 0 ? 2 : (round == 1 ? 1 : 8);
    }
    CHECK(afsk_check_modem("who", m) == HRFD_OK);
    int16_t taps[kAfskFilters * kAfskMaxWindow];
    afsk_taps(Q_DDC_COS, m.mark_step, m.space_step, m.W, taps);
    std::vector<int16_t> x(n), other(n);
    uint32_t phase = 0, tone = m.mark_step, amp = 1;
    for (uint32_t i = 0; i < n; i++)
    {
      if (next() % 7 == 0)
      {
        tone = (next() & 1u) ? m.mark_step : m.space_step;
      }
      if (i % 700 == 0)
      {
        const uint32_t amps[] = {0, 1, 300, 8000, 32767};
        amp = amps[next() % 5];
      }
      phase += tone;
      const int32_t v = (Q_DDC_COS[phase >> 20] * (int32_t)amp) / 32767 + (int32_t)(next() % 201) - 100;
      x[i] = (int16_t)(v > 32767 ? 32767 : (v < -32768 ? -32768 : v));
    }
    uint32_t n_pcm[B];
    for (uint32_t b = 0; b < B; b++)
    {
      const uint32_t kinds[] = {512, 512, 0xffffffffu, 300, 0, 511, 1};
      n_pcm[b] = kinds[next() % 7];
    }
    other = x;
    for (uint32_t b = 0; b < B; b++)
    {
      for (uint32_t i = pcm_block_limit(n_pcm, b); i < kAfskBlock; i++)
      {
        other[b * kAfskBlock + i] ^= 0x5a5a;
      }
    }
    const uint32_t cap = afsk_max_bits(m.baud_step, m.A, B);
    std::vector<uint8_t> bits(cap + 4, 0xEE), bits_c(cap + 4, 0xEE), hard(B * kAfskHardPerBlock), hard_c(B * kAfskHardPerBlock), hard_o(B * kAfskHardPerBlock);
    uint32_t n_bits = 0, n_c = 0;
    AfskState st = {}, st_c = {}, st_o = {};
    afsk_channel_slow(x.data(), n_pcm, B, m, taps, 1000000, &st, bits.data(), &n_bits, hard.data());
    CHECK(n_bits <= cap && n_bits <= n && bits[n_bits] == 0xEE && bits[cap] == 0xEE);
    uint32_t at = 0;
    for (uint32_t k : cuts)
    {
      const uint32_t cap_k = afsk_max_bits(m.baud_step, m.A, k);
      uint32_t got = 0;
      afsk_channel_slow(other.data() + at * kAfskBlock, n_pcm + at, k, m, taps, 1000000, &st_c, bits_c.data() + n_c, &got,
                        hard_c.data() + at * kAfskHardPerBlock);
      CHECK(got <= cap_k);
      n_c += got;
      at += k;
    }
    CHECK(n_c == n_bits && bits == bits_c && hard == hard_c && memcmp(&st, &st_c, sizeof(st)) == 0);
    // a call without bits: the same decisions and samples, the clock where it was
    afsk_channel_slow(x.data(), n_pcm, B, m, taps, 0, &st_o, nullptr, nullptr, hard_o.data());
    CHECK(hard == hard_o && st_o.phi == 0 && (st_o.flags & 2u) == 0 && (st_o.flags & 1u) == (st.flags & 1u) &&
          memcmp(st_o.x, st.x, sizeof(st.x)) == 0);
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_the_bound_is_reached() || check_bound_and_cutting())
  {
    return 1;
  }
  printf("san_afsk ok\n");
  return 0;
}
