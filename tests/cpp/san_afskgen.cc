// Sanitizer harness for the HIP-free part of the AFSK generator bank (hackrfdiags_amd/csrc/hrfd_afskgen.h), CPU only: compiled
// as plain C++ under -fsanitize=address,undefined (tests/test_afskgen_sanitizers.py).  Every check at its limit with its text,
// the laws on their boundaries (the levels with and without NRZI, the length at 2^31 - 1 and at 2^31, the bit of the last
// sample, the phase against a walk over the samples, the largest amp), every rule of the queue (append, insertion, overlap,
// the four messages, their slots, times near 2^63), the cut, and the slow loop: against a restatement written out here, a
// stream cut into calls against one long call with exactly sized buffers, in place against out of place, generate only,
// saturation with its count, the active bytes, and one tone against the tone generator's slow loop.
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
#include "../../hackrfdiags_amd/csrc/hrfd_afskgen.h"
#include "../../hackrfdiags_amd/csrc/hrfd_tonegen.h"         // for the one tone against the tone generator's slow loop
#include "../../hackrfdiags_amd/csrc/hrfd_ddc_tables.h"

using namespace hrfd;

#define CHECK(cond)                                                   \
  do                                                                  \
  {                                                                   \
    if (!(cond))                                                      \
    {                                                                 \
      printf("san_afskgen: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static uint32_t g_seed = 1202u;
static uint32_t next() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static const uint32_t kBaud1200 = 644245094u, kBaud300 = 161061274u, kOdd = 0x01234567u, kTop = 1u << 31;

static hrfd_afskgen_message msg(uint32_t n_bits, uint32_t baud = kBaud1200, uint32_t amp = 8000, uint32_t gap = 0, uint32_t mark = 644245094u,
                                uint32_t space = 1181116006u, uint32_t flags = 1)
{
  return hrfd_afskgen_message{gap, n_bits, mark, space, baud, amp, flags, 0};
}

static int check_the_checks()
{
  static_assert(kAfskgenMaxMessages == HRFD_AFSKGEN_MAX_MESSAGES && kAfskgenMaxBits == HRFD_AFSKGEN_MAX_BITS &&
                    kGenMaxBlocks == HRFD_AFSKGEN_MAX_BLOCKS && kAfskgenNrzi == HRFD_AFSKGEN_NRZI && kGenAppend == HRFD_AFSKGEN_APPEND,
                "the header's limits are the public ones");
  static_assert(sizeof(hrfd_afskgen_message) == 32, "eight uint32");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(afskgen_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(afskgen_check_create("who", 1, nullptr), "result pointer") && afskgen_check_create("who", 65536, &out) == HRFD_OK);

  std::vector<uint8_t> bits(8192, 1);                      // exactly the most a message reads
  uint64_t L = 0;
  hrfd_afskgen_message m = msg(8192, kTop, 32767, 0xffffffffu, kTop, kTop);
  CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK && L == 16384);
  m = msg(1, 3, 0, 0, 1, 1, 0);
  CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK && L == 1431655766ull);
  CHECK(refused(afskgen_check_message("who", nullptr, bits.data(), &L), "NULL argument") &&
        refused(afskgen_check_message("who", &m, nullptr, &L), "NULL argument"));
  for (uint32_t n : {0u, 8193u, 0xffffffffu})
  {
    m = msg(n);
    CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "n_bits must be 1..8192"));
  }
  for (uint32_t v : {0u, kTop + 1, 0xffffffffu})
  {
    m = msg(3, kBaud1200, 0, 0, v);
    CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "mark_step must be 1..2^31"));
    m = msg(3, kBaud1200, 0, 0, 1, v);
    CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "space_step must be 1..2^31"));
    m = msg(3, v);
    CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "baud_step must be 1..2^31"));
  }
  m = msg(3, kBaud1200, 32768);
  CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "amp above 32767"));
  m = msg(3, kBaud1200, 0, 0, 1, 1, 2);
  CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "only bit 0 of flags"));
  m = msg(3);
  m.pad = 7;
  CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "a pad of 0"));
  m = msg(1, 1);
  CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "below 2^31"));
  m = msg(8192, 16384);
  CHECK(refused(afskgen_check_message("who", &m, bits.data(), &L), "below 2^31"));
  m = msg(8192, 16385);
  CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK && L == 2147352584ull);

  CHECK(gen_check_time("who", (1ull << 63) - 1) == HRFD_OK && refused(gen_check_time("who", 1ull << 63), "below 2^63"));
  alignas(16) static char buf[65536];
  const void *in = buf + 16384, *far = buf + 40960;
  CHECK(refused(gen_check_call("who", in, 1024, true, 0, far, 1024, 1), "n_blocks"));
  CHECK(refused(gen_check_call("who", in, 1 << 21, true, 1025, far, 1 << 21, 1), "n_blocks"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, nullptr, 1024, 1), "NULL argument"));
  CHECK(refused(gen_check_call("who", in, 1022, true, 1, far, 1024, 1), "channel_stride_bytes"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, far, 1027, 1), "out_stride_bytes"));
  CHECK(gen_check_call("who", nullptr, 0, true, 1, far, 1024, 7) == HRFD_OK);
  CHECK(refused(gen_check_call("who", buf + 16385, 1024, true, 1, far, 1024, 1), "even addresses"));
  CHECK(gen_check_call("who", in, 1030, true, 1, in, 1030, 4) == HRFD_OK && gen_check_call("who", in, 0, false, 3, in, 0, 4) == HRFD_OK);
  CHECK(refused(gen_check_call("who", in, 1030, true, 1, in, 1032, 4), "overlaps"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, buf + 16384 + 1024, 1024, 4), "overlaps"));
  CHECK(gen_check_call("who", in, 1024, true, 1, buf + 16384 + 4096, 1024, 4) == HRFD_OK);
  return 0;
}

static int check_laws()
{
  // 1. levels: plain, and NRZI from mark; whole words, the last one zero behind the last bit
  const uint8_t d[6] = {0, 0, 1, 0xfe, 0xff, 2};           // only bit 0 counts: 0 0 1 0 1 0
  uint32_t w[2] = {0xeeeeeeeeu, 0xeeeeeeeeu};
  afskgen_levels(d, 6, false, w);
  CHECK(w[0] == 0x14u && w[1] == 0xeeeeeeeeu);
  afskgen_levels(d, 6, true, w);                           // from 1: 0 1 1 0 0 1
  CHECK(w[0] == 0x26u && w[1] == 0xeeeeeeeeu);
  std::vector<uint8_t> ones(33, 1), zeros(33, 0);          // exactly 33 bytes are read
  afskgen_levels(ones.data(), 33, true, w);
  CHECK(w[0] == 0xffffffffu && w[1] == 1u);
  afskgen_levels(zeros.data(), 33, true, w);               // every bit turns the level over, the first to space
  CHECK(w[0] == 0xaaaaaaaau && w[1] == 0u);
  afskgen_levels(zeros.data(), 32, false, w);
  CHECK(w[0] == 0u && w[1] == 0u);                         // (the second word is not touched by 32 bits)

  // 2. the length at its edges, and the bit of the last sample
  struct { uint32_t B, r; uint64_t L; } cases[] = {{8192, kTop, 16384},          {3, kBaud1200, 21},           {3, kBaud1200 + 1, 20},
                                                   {1, kTop, 2},                 {1, 3, 1431655766ull},        {3u << 28, (3u << 29) + 1, (1ull << 31) - 1},
                                                   {8192, kBaud300, 218454},     {1, kOdd, 226},               {0xffffffffu, kTop, 0}};
  for (auto &c : cases)
  {
    uint64_t L = 0;
    if (c.L == 0)
    {
      CHECK(refused(afskgen_length("who", c.B, c.r, &L), "below 2^31"));
      continue;
    }
    CHECK(afskgen_length("who", c.B, c.r, &L) == HRFD_OK && L == c.L);
    CHECK(afskgen_bit((uint32_t)(L - 1), c.r) == c.B - 1 && (L == 1 || afskgen_bit((uint32_t)(L - 2), c.r) <= c.B - 1));
    CHECK(((L * c.r) >> 32) >= c.B && afskgen_first_sample(c.B, c.r) == L && afskgen_first_sample(0, c.r) == 0);
  }
  uint64_t L = 0;
  CHECK(refused(afskgen_length("who", 1, 1, &L), "below 2^31") && refused(afskgen_length("who", 1, 2, &L), "below 2^31"));
  CHECK(refused(afskgen_length("who", 3u << 28, 3u << 29, &L), "2147483648 samples"));
  CHECK(refused(afskgen_length("who", 0, 5, &L), "at least one bit") && refused(afskgen_length("who", 5, 0, &L), "a step of 1..2^31") &&
        refused(afskgen_length("who", 5, kTop + 1, &L), "a step of 1..2^31"));
  // a 32-bit product would lose the bit: k = 2^30 at the top step is bit 2^29
  CHECK(afskgen_bit(1u << 30, kTop) == (1u << 29) && afskgen_bit(0x7fffffffu, kTop) == 0x3fffffffu);

  // 3. the phase in closed form against the walk over the samples, at every k of messages of every baud rate
  for (uint32_t r : {kBaud300, kBaud1200, kTop, kOdd})
  {
    const uint32_t B = r == kOdd ? 9 : 70;
    std::vector<uint8_t> bits(B);
    for (auto &b : bits)
    {
      b = (uint8_t)next();
    }
    std::vector<uint32_t> lv((B + 31) / 32);               // exactly the words the law reads
    afskgen_levels(bits.data(), B, r != kTop, lv.data());
    CHECK(afskgen_length("who", B, r, &L) == HRFD_OK);
    const AfskgenSlot s = {5, 5 + L, next() << 7, next() << 7, r, 32767};
    uint32_t theta = 0;
    for (uint64_t k = 0; k <= L; k++)
    {
      CHECK(afskgen_theta_at(s, lv.data(), k) == theta);
      if (k < L)
      {
        CHECK(afskgen_bit((uint32_t)k, r) < B);
        theta += afskgen_step(s, lv.data(), (uint32_t)k);
      }
    }
  }
  // the phase far into the longest message there is, without the walk: one bit of 2^31 - 1 samples... of mark only
  {
    const uint8_t one = 1;
    uint32_t lv = 0;
    afskgen_levels(&one, 1, true, &lv);
    CHECK(afskgen_length("who", 1, 3, &L) == HRFD_OK);
    const AfskgenSlot s = {0, L, 0x12345679u, 77u, 3u, 32767};
    CHECK(lv == 1u && afskgen_theta_at(s, &lv, L) == (uint32_t)(L * 0x12345679ull) && afskgen_theta_at(s, &lv, 0) == 0);
  }
  // 4. a sample: k = 0 is the zero crossing; the largest amp at the sine's peaks, under both ramps
  const AfskgenSlot s = {100, 100 + 300, 1u << 30, 1u << 30, kBaud1200, 32767};
  CHECK(afskgen_sample(s, 100, 0, Q_DDC_COS) == 0);
  CHECK(afskgen_sample(s, 101, 1u << 30, Q_DDC_COS) == (32766 * 2 + 32) >> 6 && afskgen_sample(s, 163, 1u << 30, Q_DDC_COS) == (32766 * 64 + 32) >> 6);
  CHECK(afskgen_sample(s, 164, 3u << 30, Q_DDC_COS) == -32766 && afskgen_sample(s, 399, 3u << 30, Q_DDC_COS) == (-32766 + 32) >> 6);
  CHECK(afskgen_sample(s, 336, 1u << 30, Q_DDC_COS) == 32766 && afskgen_sample(s, 337, 1u << 30, Q_DDC_COS) == (32766 * 63 + 32) >> 6);
  return 0;
}

static int check_queue()
{
  AfskgenQueue q;
  AfskgenSlot s;
  uint64_t L = 0, end = 0;
  std::vector<uint8_t> bits(64, 1);
  hrfd_afskgen_message m = msg(3, kBaud1200, 8000, 10);    // L = 21
  CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK && L == 21);
  CHECK(afskgen_lay_out("who", q, 0, &m, L, 1000, &s) == HRFD_OK && s.start == 1010 && s.end == 1031 && s.amp == 8000);
  CHECK(afskgen_insert(q, s, std::vector<uint32_t>(1, 7u)) == 0);
  CHECK(afskgen_lay_out("who", q, 0, &m, L, kGenAppend, &s) == HRFD_OK && s.start == 1041 && s.end == 1062);
  CHECK(afskgen_insert(q, s, std::vector<uint32_t>(1, 7u)) == 1);
  CHECK(afskgen_lay_out("who", q, 0, &m, L, 0, &s) == HRFD_OK && s.start == 10);                 // in front
  CHECK(afskgen_insert(q, s, std::vector<uint32_t>(1, 7u)) == 2 && q[0].s.start == 10 && q[0].slot == 2 && q[1].slot == 0 && q[2].slot == 1);
  for (uint64_t start : {980ull, 1000ull, 1020ull, 1011ull, 1051ull})                            // [start + 10, start + 31)
  {
    CHECK(refused(afskgen_lay_out("who", q, 0, &m, L, start, &s), "would overlap"));
  }
  CHECK(afskgen_lay_out("who", q, 0, &m, L, 979, &s) == HRFD_OK && afskgen_lay_out("who", q, 0, &m, L, 1052, &s) == HRFD_OK);
  m.gap = 0;
  CHECK(refused(afskgen_lay_out("who", q, 0, &m, L, 1030, &s), "would overlap") && afskgen_lay_out("who", q, 0, &m, L, 1031, &s) != HRFD_OK);
  m.gap = 10;
  CHECK(refused(afskgen_lay_out("who", q, 50, &m, L, 49, &s), "before the stream time 50"));
  CHECK(afskgen_count_pending(q, 0, &end) == 3 && end == 1062 && afskgen_count_pending(q, 31, &end) == 2 && afskgen_count_pending(q, 1062, &end) == 0 &&
        end == 1062);
  // the four, and the slot a message that ended leaves
  CHECK(afskgen_lay_out("who", q, 0, &m, L, 2000, &s) == HRFD_OK && afskgen_insert(q, s, std::vector<uint32_t>(1, 7u)) == 3);
  CHECK(refused(afskgen_lay_out("who", q, 30, &m, L, kGenAppend, &s), "5 messages"));
  CHECK(afskgen_lay_out("who", q, 31, &m, L, kGenAppend, &s) == HRFD_OK && s.start == 2041);         // the first has ended
  afskgen_drop_ended(q, 31);
  CHECK(q.size() == 3 && afskgen_insert(q, s, std::vector<uint32_t>(1, 7u)) == 2 && q.back().s.start == 2041);
  // append where everything has ended: from N
  CHECK(afskgen_lay_out("who", q, 5000, &m, L, kGenAppend, &s) == HRFD_OK && s.start == 5010);
  // times near 2^63
  q.clear();
  CHECK(afskgen_lay_out("who", q, 0, &m, L, (1ull << 63) - 32, &s) == HRFD_OK && s.end == (1ull << 63) - 1);
  CHECK(refused(afskgen_lay_out("who", q, 0, &m, L, (1ull << 63) - 31, &s), "2^63") && refused(afskgen_lay_out("who", q, 0, &m, L, (1ull << 63) - 1, &s), "2^63"));
  m = msg(1, 3, 0, 0xffffffffu);
  CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK);
  CHECK(afskgen_lay_out("who", q, 0, &m, L, (1ull << 63) - 1431655766ull - 0x100000000ull, &s) == HRFD_OK && s.end == (1ull << 63) - 1);
  // the cut
  m = msg(60);                                             // 401 samples
  CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK && L == 401);
  for (uint64_t at : {0ull, 500ull, 1000ull})
  {
    CHECK(afskgen_lay_out("who", q, 0, &m, L, at, &s) == HRFD_OK);
    afskgen_insert(q, s, std::vector<uint32_t>(2, 7u));
  }
  AfskgenQueue c = q;
  afskgen_cut(c, 450);                                     // in the gap: everything left has not begun
  afskgen_drop_ended(c, 450);
  CHECK(c.empty());
  c = q;
  afskgen_drop_ended(c, 500);
  afskgen_cut(c, 500);                                     // the second has just begun
  CHECK(c.size() == 1 && c[0].s.start == 500 && c[0].s.end == 564 && c[0].slot == 1);
  c = q;
  afskgen_drop_ended(c, 880);
  afskgen_cut(c, 880);                                     // 21 samples left: the end stays
  CHECK(c.size() == 1 && c[0].s.end == 901);
  return 0;
}

// the contract written out again: the phase by a walk from the message's first sample, 64-bit arithmetic, divisions for
// the shifts
static int32_t restated(const AfskgenSlot &s, const uint8_t *level, uint64_t n, const uint64_t E)
{
  if (n < s.start || n >= E)
  {
    return 0;
  }
  const uint64_t k = n - s.start;
  uint64_t theta = 0;
  for (uint64_t j = 0; j < k; j++)
  {
    theta = (theta + (level[(j * s.baud_step) >> 32] ? s.mark_step : s.space_step)) & 0xffffffffull;
  }
  const uint64_t i = ((theta + (1u << 19)) >> 20) & 4095;
  const int64_t sum = (int64_t)s.amp * Q_DDC_COS[(i + 4096 - 1024) & 4095] + (1 << 14);
  const int64_t v = sum >= 0 ? sum / 32768 : -((-sum + 32767) / 32768);
  uint64_t e = k + 1 < 64 ? k + 1 : 64;
  e = E - n < e ? E - n : e;
  const int64_t w = v * (int64_t)e + 32;
  return (int32_t)(w >= 0 ? w / 64 : -((-w + 63) / 64));
}

static int check_slow_loop()
{
  const uint32_t B = 9, n = B * kGenBlock;
  const uint32_t bauds[4] = {kBaud1200, kBaud300, kTop, kOdd};
  for (int round = 0; round < 8; round++)
  {
    const uint64_t bases[] = {0, 1, (1ull << 32) - 1024, (1ull << 62) + 5};
    const uint64_t N = bases[round % 4];
    // up to four messages laid out around the call through the queue rules; the first starts before the call in some rounds
    AfskgenQueue q;
    std::vector<std::vector<uint8_t>> level;
    const uint32_t count = 1 + round % 4;
    for (uint32_t j = 0; j < count; j++)
    {
      const uint32_t r = bauds[(round + j) % 4];
      const uint32_t lens[] = {1, 2, 3, 31, 32, 33, 40, 200};
      const uint32_t n_bits = r == kOdd ? 1 + next() % 4 : lens[next() % 8];
      std::vector<uint8_t> bits(n_bits);                   // exactly sized
      for (auto &b : bits)
      {
        b = (uint8_t)next();
      }
      hrfd_afskgen_message m = msg(n_bits, r, round % 2 ? 32767 : next() % 32768, next() % 3 == 0 ? next() % 700 : 0, next() << 7, next() << 7, j & 1);
      uint64_t L = 0;
      AfskgenSlot s;
      CHECK(afskgen_check_message("who", &m, bits.data(), &L) == HRFD_OK);
      CHECK(afskgen_lay_out("who", q, N, &m, L, j == 0 ? N + next() % 600 : kGenAppend, &s) == HRFD_OK);
      std::vector<uint32_t> lv((n_bits + 31) / 32);
      afskgen_levels(bits.data(), n_bits, (m.flags & 1) != 0, lv.data());
      std::vector<uint8_t> plain(n_bits);
      uint8_t cur = 1;
      for (uint32_t i = 0; i < n_bits; i++)
      {
        cur = (m.flags & 1) ? ((bits[i] & 1) ? cur : 1 - cur) : (bits[i] & 1);
        plain[i] = cur;
      }
      afskgen_insert(q, s, std::move(lv));
      level.push_back(plain);
    }
    if (round >= 4)
    {
      // the first message began before the call, and is cut inside it
      const uint64_t back = q[0].s.start - N + std::min<uint64_t>(N, 100);
      for (auto &m : q)
      {
        m.s.start -= back;
        m.s.end -= back;
      }
      q[0].s.end = std::min(q[0].s.end, N + 64 + round);
    }
    AfskgenSlot slots[kAfskgenMaxMessages];
    const uint32_t *lv[kAfskgenMaxMessages];
    for (uint32_t j = 0; j < count; j++)
    {
      slots[j] = q[j].s;
      lv[j] = q[j].levels.data();
    }
    std::vector<int16_t> x(n), y(n), yc(n), io(n), gen(n), genc(n);
    for (uint32_t i = 0; i < n; i++)
    {
      const uint32_t r = next();
      x[i] = (int16_t)(r % 5 == 0 ? 32767 : (r % 5 == 1 ? -32768 : (int32_t)(r % 65536) - 32768));
    }
    uint8_t act[B], actc[B], actg[B];
    const uint64_t clips = afskgen_channel_slow(x.data(), B, slots, lv, count, N, Q_DDC_COS, y.data(), act);
    uint64_t want_clips = 0;
    for (uint32_t i = 0; i < n; i++)
    {
      int64_t sum = x[i];
      for (uint32_t j = 0; j < count; j++)
      {
        sum += restated(slots[j], level[j].data(), N + i, slots[j].end);
      }
      const int64_t sat = sum < -32768 ? -32768 : (sum > 32767 ? 32767 : sum);
      want_clips += sat != sum;
      CHECK(y[i] == sat);
    }
    CHECK(clips == want_clips);
    for (uint32_t b = 0; b < B; b++)
    {
      uint8_t on = 0;
      for (uint32_t j = 0; j < count; j++)
      {
        for (uint32_t i = 0; i < kGenBlock && !on; i++)
        {
          const uint64_t at = N + (uint64_t)b * kGenBlock + i;
          on = at >= slots[j].start && at < slots[j].end;
        }
      }
      CHECK(act[b] == on);
    }
    // cut 1 + 3 + 5 with exactly sized buffers, in place; generate only whole and cut
    const uint32_t cuts[] = {1, 3, 5};
    uint32_t at = 0;
    uint64_t clips_c = 0, clips_io = 0;
    for (uint32_t k : cuts)
    {
      const uint64_t Nk = N + (uint64_t)at * kGenBlock;
      std::vector<int16_t> in(x.begin() + at * kGenBlock, x.begin() + (at + k) * kGenBlock), out(k * kGenBlock), g(k * kGenBlock);
      std::vector<uint8_t> a(k);
      clips_c += afskgen_channel_slow(in.data(), k, slots, lv, count, Nk, Q_DDC_COS, out.data(), a.data());
      memcpy(yc.data() + at * kGenBlock, out.data(), 2 * out.size());
      memcpy(actc + at, a.data(), k);
      clips_io += afskgen_channel_slow(in.data(), k, slots, lv, count, Nk, Q_DDC_COS, in.data(), nullptr);
      memcpy(io.data() + at * kGenBlock, in.data(), 2 * in.size());
      afskgen_channel_slow(nullptr, k, slots, lv, count, Nk, Q_DDC_COS, g.data(), nullptr);
      memcpy(genc.data() + at * kGenBlock, g.data(), 2 * g.size());
      at += k;
    }
    afskgen_channel_slow(nullptr, B, slots, lv, count, N, Q_DDC_COS, gen.data(), actg);
    CHECK(y == yc && y == io && clips == clips_c && clips == clips_io && gen == genc);
    CHECK(memcmp(act, actc, B) == 0 && memcmp(act, actg, B) == 0);
  }
  // one tone: the tone generator's segment of the same start, length, step and amp, through its own slow loop
  {
    const uint8_t bits[3] = {1, 0, 1};
    uint32_t lv = 0;
    afskgen_levels(bits, 3, true, &lv);
    const AfskgenSlot s = {7, 7 + 21, 0x23456789u, 0x23456789u, kBaud1200, 32767};
    const uint32_t *plv = &lv;
    TonegenTrack tr[2];
    tr[0].push_back(TonegenSlot{7, 7 + 21, 0x23456789u, 0u, 32767u, 0u});
    TonegenSlot slots[kTonegenSlots];
    tonegen_fill_slots(tr, slots);
    std::vector<int16_t> a(512), t(512);
    CHECK(afskgen_channel_slow(nullptr, 1, &s, &plv, 1, 0, Q_DDC_COS, a.data(), nullptr) == 0);
    CHECK(tonegen_channel_slow(nullptr, 1, slots, 0, Q_DDC_COS, t.data(), nullptr) == 0 && a == t && a[8] != 0);
  }
  // a channel without messages passes its input through and generates silence
  std::vector<int16_t> x(512), y(512, 1);
  for (uint32_t i = 0; i < 512; i++)
  {
    x[i] = (int16_t)(i * 127 - 32768);
  }
  uint8_t act = 9;
  CHECK(afskgen_channel_slow(x.data(), 1, nullptr, nullptr, 0, 12345, Q_DDC_COS, y.data(), &act) == 0 && x == y && act == 0);
  CHECK(afskgen_channel_slow(nullptr, 1, nullptr, nullptr, 0, 0, Q_DDC_COS, y.data(), nullptr) == 0 && y == std::vector<int16_t>(512, 0));
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_queue() || check_slow_loop())
  {
    return 1;
  }
  printf("san_afskgen ok\n");
  return 0;
}
