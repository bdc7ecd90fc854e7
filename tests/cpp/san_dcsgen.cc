// Sanitizer harness for the HIP-free part of the DCS generator bank (hackrfdiags_amd/csrc/hrfd_dcsgen.h, and hrfd_gen.h, which it
// shares with the tone and AFSK generators), CPU only: compiled as plain C++ under -fsanitize=address,undefined
// (tests/test_dcsgen_sanitizers.py).  Every check at its limit with its text, the grids over a whole period and across u's wrap
// at 28750 against a restatement in 64 bits written out here, every rule of the queue (append, insertion, overlap, FOREVER, the
// 8 segments, times near 2^63), the cut case by case, the largest accumulator at T = 512, and the slow loop: a stream cut into
// calls against one long call, in place against out of place, generate only, saturation with its count, the active bytes.
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
#include "../../hackrfdiags_amd/csrc/hrfd_dcsgen.h"

using namespace hrfd;

#define CHECK(cond)                                                  \
  do                                                                 \
  {                                                                  \
    if (!(cond))                                                     \
    {                                                                \
      printf("san_dcsgen: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                      \
    }                                                                \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static hrfd_dcsgen_segment seg(uint32_t length, uint32_t tail = 0, uint32_t word = 0, uint32_t amp = 0, uint32_t gap = 0)
{
  return hrfd_dcsgen_segment{gap, length, tail, word, amp};
}

static const uint32_t kWord = 0x763813;    // D023N

static int check_the_checks()
{
  static_assert(kDcsgenMaxSegments == HRFD_DCSGEN_MAX_SEGMENTS && kGenMaxBlocks == HRFD_DCSGEN_MAX_BLOCKS &&
                    kDcsgenMaxTaps == HRFD_DCSGEN_MAX_TAPS && kDcsgenForever == HRFD_DCSGEN_FOREVER &&
                    kDcsgenDefaultTail == HRFD_DCSGEN_DEFAULT_TAIL && kGenAppend == HRFD_DCSGEN_APPEND,
                "the header's limits are the public ones");
  static_assert(sizeof(hrfd_dcsgen_segment) == 20, "five uint32");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(dcsgen_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(dcsgen_check_create("who", 1, nullptr), "result pointer") && dcsgen_check_create("who", 65536, &out) == HRFD_OK);

  hrfd_dcsgen_segment s9[9];
  for (auto &s : s9)
  {
    s = seg(1);
  }
  CHECK(dcsgen_check_segments("who", s9, 1) == HRFD_OK && dcsgen_check_segments("who", s9, 8) == HRFD_OK);
  CHECK(refused(dcsgen_check_segments("who", s9, 0), "1..8 segments") && refused(dcsgen_check_segments("who", s9, 9), "1..8 segments"));
  CHECK(refused(dcsgen_check_segments("who", nullptr, 1), "segments"));
  s9[3] = seg(1, 0, 0, 32768);
  CHECK(refused(dcsgen_check_segments("who", s9, 4), "segment 3 has an amp above 32767") && dcsgen_check_segments("who", s9, 3) == HRFD_OK);
  s9[3] = seg(1, 0, 0x800000, 0);
  CHECK(refused(dcsgen_check_segments("who", s9, 4), "segment 3 has the word 0x800000"));
  s9[3] = seg(0xfffffffeu, 0xfffffffeu, 0x7fffff, 32767, 0xffffffffu);
  CHECK(dcsgen_check_segments("who", s9, 4) == HRFD_OK);
  s9[3] = seg(0);
  CHECK(refused(dcsgen_check_segments("who", s9, 4), "segment 3 has length 0"));
  s9[3] = seg(1, 0xffffffffu);
  CHECK(refused(dcsgen_check_segments("who", s9, 4), "segment 3 has a tail of 2^32-1"));
  s9[3] = seg(kDcsgenForever, 1440);
  CHECK(dcsgen_check_segments("who", s9, 4) == HRFD_OK && refused(dcsgen_check_segments("who", s9, 5), "segment 4 lies behind a FOREVER"));

  int16_t taps[513];
  for (auto &t : taps)
  {
    t = 0;
  }
  CHECK(refused(dcsgen_check_taps("who", taps, 0), "1..512 taps") && refused(dcsgen_check_taps("who", taps, 513), "1..512 taps"));
  CHECK(refused(dcsgen_check_taps("who", nullptr, 1), "taps") && dcsgen_check_taps("who", taps, 512) == HRFD_OK);
  taps[0] = 32767;
  taps[511] = -32768;
  CHECK(dcsgen_check_taps("who", taps, 512) == HRFD_OK);   // sum |h| = 65535
  taps[100] = 1;
  CHECK(refused(dcsgen_check_taps("who", taps, 512), "sum |h| = 65536 > 65535"));

  CHECK(gen_check_time("who", (1ull << 63) - 1) == HRFD_OK && refused(gen_check_time("who", 1ull << 63), "below 2^63"));
  int16_t buf[1024];
  CHECK(gen_check_call("who", buf, 0, false, 1, buf + 512, 0, 1) == HRFD_OK && gen_check_call("who", buf, 0, false, 1, buf, 0, 1) == HRFD_OK);
  CHECK(refused(gen_check_call("who", buf, 0, false, 0, buf, 0, 1), "n_blocks") && refused(gen_check_call("who", buf, 0, false, 1025, buf, 0, 1), "n_blocks"));
  CHECK(refused(gen_check_call("who", buf, 0, false, 1, buf + 1, 0, 1), "overlaps the input"));
  CHECK(refused(gen_check_call("who", buf, 1024, true, 1, buf, 1026, 1), "overlaps the input"));
  CHECK(refused(gen_check_call("who", nullptr, 0, true, 1, buf, 1022, 1), "out_stride_bytes"));
  return 0;
}

// the grids in 64 bits on the absolute time, where 21 n and 42 n fit
static int32_t bit_ref(uint32_t word, uint64_t n) { return ((word >> ((21 * n / 1250) % 23)) & 1u) ? 1 : -1; }
static int32_t sq_ref(uint64_t n) { return ((42 * n / 1250) & 1u) ? -1 : 1; }

static int check_the_grids()
{
  // a whole period and the wrap: the reduced grid is the absolute one, because 28750 samples are 483 bit times exactly
  CHECK(21ull * kDcsgenPeriod == 483ull * 1250 && 483 % 23 == 0 && (2 * 483) % 2 == 0);
  const DcsgenSlot code = {0, kDcsgenNoEnd, kDcsgenNoEnd, kWord, 7};
  const DcsgenSlot tail = {0, 0, kDcsgenNoEnd, kWord, 7};
  for (uint64_t base : {0ull, 28750ull - 5, 28750ull * 40000ull - 3, (1ull << 40) + 12345})
  {
    for (uint64_t n = base; n < base + 2 * kDcsgenPeriod + 10; n++)
    {
      const uint32_t u = dcsgen_u(n);
      CHECK(u < kDcsgenPeriod && dcsgen_bit_index(u) == (21 * n / 1250) % 23);
      CHECK(dcsgen_slot_at(code, n, u) == 7 * bit_ref(kWord, n) && dcsgen_slot_at(tail, n, u) == 7 * sq_ref(n));
    }
  }
  // u at the top of the clock, where only the reduced grid can be computed
  const uint64_t top = (1ull << 63) - 1;
  CHECK(dcsgen_u(top) == (uint32_t)(top % 28750) && dcsgen_u(28749) == 28749 && dcsgen_u(28750) == 0);
  // the bit times are 59 or 60 samples, the turn-off code's halves 29 or 30
  uint32_t run = 0, last = 0;
  for (uint32_t u = 0; u < kDcsgenPeriod; u++)
  {
    const uint32_t h = 42u * u / 1250u;
    if (h != last)
    {
      CHECK(run == 29 || run == 30);
      run = 0;
      last = h;
    }
    run++;
  }
  // a slot's three ranges
  const DcsgenSlot s = {100, 200, 250, 0x7fffff, 9};
  CHECK(dcsgen_slot_at(s, 99, 99) == 0 && dcsgen_slot_at(s, 100, 100) == 9 && dcsgen_slot_at(s, 199, 199) == 9);
  CHECK(dcsgen_slot_at(s, 200, 200) == 9 * sq_ref(200) && dcsgen_slot_at(s, 249, 249) == 9 * sq_ref(249) && dcsgen_slot_at(s, 250, 250) == 0);
  CHECK(dcsgen_slot_at(kDcsgenEmptySlot, 0, 0) == 0 && dcsgen_slot_at(kDcsgenEmptySlot, ~0ull - 1, 5) == 0);
  CHECK(dcsgen_round(0) == 0 && dcsgen_round(8191) == 0 && dcsgen_round(8192) == 1 && dcsgen_round(-8192) == 0 && dcsgen_round(-8193) == -1);
  CHECK(dcsgen_round(65535 * 32767) == 131066 && dcsgen_round(-65535 * 32767) == -131066);
  return 0;
}

static bool same(const DcsgenQueue &q, std::vector<std::vector<uint64_t>> want)
{
  if (q.size() != want.size())
  {
    return false;
  }
  for (size_t i = 0; i < q.size(); i++)
  {
    if (q[i].s.start != want[i][0] || q[i].s.mid != want[i][1] || q[i].s.end != want[i][2])
    {
      return false;
    }
  }
  return true;
}

static int check_the_queue()
{
  const uint64_t X = kDcsgenNoEnd;
  DcsgenQueue q, m;
  hrfd_dcsgen_segment a[2] = {seg(100, 20, kWord, 5, 10), seg(50, 0, kWord, 6, 3)};
  CHECK(dcsgen_lay_out("who", q, 1000, a, 2, kGenAppend, m) == HRFD_OK && same(m, {{1010, 1110, 1130}, {1133, 1183, 1183}}));
  CHECK(m[0].tail == 20 && m[1].s.amp == 6 && q.empty());
  q = m;
  CHECK(refused(dcsgen_lay_out("who", q, 1000, a, 1, 999, m), "start 999 lies before the stream time 1000"));
  hrfd_dcsgen_segment one = seg(10, 0, kWord, 1);
  CHECK(refused(dcsgen_lay_out("who", q, 1000, &one, 1, 1129, m), "the segments at 1010 and 1129 would overlap"));
  CHECK(dcsgen_lay_out("who", q, 1000, &one, 1, 1000, m) == HRFD_OK && same(m, {{1000, 1010, 1010}, {1010, 1110, 1130}, {1133, 1183, 1183}}));
  hrfd_dcsgen_segment three = seg(3);
  CHECK(dcsgen_lay_out("who", q, 1000, &three, 1, 1130, m) == HRFD_OK && m.size() == 3 && m[1].s.start == 1130);     // abuts both
  hrfd_dcsgen_segment four = seg(4);
  CHECK(refused(dcsgen_lay_out("who", q, 1000, &four, 1, 1130, m), "would overlap"));
  hrfd_dcsgen_segment ever = seg(kDcsgenForever, 1440, kWord, 5);
  CHECK(dcsgen_lay_out("who", q, 1000, &ever, 1, kGenAppend, m) == HRFD_OK && same(m, {{1010, 1110, 1130}, {1133, 1183, 1183}, {1183, X, X}}));
  CHECK(m[2].tail == 1440);
  DcsgenQueue spare;
  CHECK(refused(dcsgen_lay_out("who", q, 1000, &ever, 1, 1000, spare), "behind the FOREVER segment at 1000"));
  q = m;
  CHECK(refused(dcsgen_lay_out("who", q, 1000, &one, 1, kGenAppend, m), "nothing can be appended behind a FOREVER"));
  CHECK(refused(dcsgen_lay_out("who", q, 1000, &one, 1, 5000, m), "behind the FOREVER segment at 1183"));
  // what has ended makes room: E + 511 <= N
  CHECK(dcsgen_ended(q[0].s, 1130 + 511) && !dcsgen_ended(q[0].s, 1130 + 510) && !dcsgen_ended(q[2].s, ~0ull - 1));
  CHECK(dcsgen_next_end(q) == 1130 + 511);
  dcsgen_drop_ended(q, 1183 + 510);
  CHECK(q.size() == 2);
  dcsgen_drop_ended(q, 1183 + 511);
  CHECK(q.size() == 1 && dcsgen_next_end(q) == X);
  // the eight
  q.clear();
  hrfd_dcsgen_segment s8[8];
  for (auto &s : s8)
  {
    s = seg(5, 5);
  }
  CHECK(dcsgen_lay_out("who", q, 0, s8, 8, 100, m) == HRFD_OK && m.size() == 8 && m[7].s.end == 180);
  q = m;
  CHECK(refused(dcsgen_lay_out("who", q, 110 + 510, &one, 1, kGenAppend, m), "9 segments that have not ended on one channel (at most 8)"));
  CHECK(dcsgen_lay_out("who", q, 110 + 511, &one, 1, kGenAppend, m) == HRFD_OK && m.size() == 8 && m[7].s.start == 621);
  // near 2^63
  const uint64_t top = (1ull << 63) - 10;
  q.clear();
  hrfd_dcsgen_segment t = seg(4, 5);
  CHECK(dcsgen_lay_out("who", q, top, &t, 1, top, m) == HRFD_OK && m[0].s.end == (1ull << 63) - 1);
  t = seg(5, 5);
  CHECK(refused(dcsgen_lay_out("who", q, top, &t, 1, kGenAppend, m), "segment 0 would lie at or above stream time 2^63"));
  t = seg(1, 0, 0, 0, 10);
  CHECK(refused(dcsgen_lay_out("who", q, top, &t, 1, top, m), "segment 0 would lie at or above"));
  t = seg(0xfffffffeu, 0xfffffffeu, 0, 0, 0xffffffffu);
  CHECK(dcsgen_lay_out("who", q, 0, &t, 1, (1ull << 63) - (3ull << 32), m) == HRFD_OK);
  CHECK(dcsgen_lay_out("who", q, 0, &ever, 1, (1ull << 63) - 1, m) == HRFD_OK);
  return 0;
}

static int check_the_cut()
{
  const uint64_t X = kDcsgenNoEnd, N = 10000;
  auto one = [](uint64_t s, uint64_t m, uint64_t e, uint32_t tail) { return DcsgenQueue{DcsgenSeg{DcsgenSlot{s, m, e, kWord, 5}, tail}}; };
  DcsgenQueue q = one(9000, 12000, 12500, 500);
  dcsgen_cut(q, N, true);
  CHECK(same(q, {{9000, N, N + 500}}));
  q = one(9000, 12000, 12500, 500);
  dcsgen_cut(q, N, false);
  CHECK(same(q, {{9000, N, N}}));
  q = one(9000, X, X, 1440);
  dcsgen_cut(q, N, true);
  CHECK(same(q, {{9000, N, N + 1440}}));
  q = one(N, 12000, 12500, 500);
  dcsgen_cut(q, N, true);
  CHECK(q.empty());
  q = one(N + 1, X, X, 0);
  dcsgen_cut(q, N, false);
  CHECK(q.empty());
  q = one(9000, 9900, 10400, 500);
  dcsgen_cut(q, N, true);
  CHECK(same(q, {{9000, 9900, 10400}}));
  dcsgen_cut(q, N, false);
  CHECK(same(q, {{9000, 9900, N}}));
  dcsgen_cut(q, N, false);
  CHECK(same(q, {{9000, 9900, N}}));                       // E <= N: untouched
  q = one(9000, 9400, N - 511, 100);
  dcsgen_cut(q, N, true);
  CHECK(q.empty());                                        // ended: it leaves
  q = one((1ull << 63) - 700, X, X, 1440);
  dcsgen_cut(q, (1ull << 63) - 512, true);
  CHECK(same(q, {{(1ull << 63) - 700, (1ull << 63) - 512, (1ull << 63) - 1}}));
  return 0;
}

static int check_the_slow_loop()
{
  // the largest accumulator: 512 taps of sum |h| = 65535 whose signs follow the turn-off code's, over it at amp 32767
  {
    std::vector<int16_t> h(512);
    int64_t left = 65535;
    const uint64_t at = 3000;                              // the output sample that sees the largest sum
    for (uint32_t j = 0; j < 512; j++)
    {
      const int64_t mag = j < 511 ? 128 : left;
      left -= mag;
      h[j] = (int16_t)(sq_ref(at - j) * mag);
    }
    CHECK(left == 0 && dcsgen_check_taps("who", h.data(), 512) == HRFD_OK);
    DcsgenSlot slots[kDcsgenMaxSegments];
    DcsgenQueue q{DcsgenSeg{DcsgenSlot{0, 1, kDcsgenNoEnd, 0, 32767}, 0}};
    dcsgen_fill_slots(q, slots);
    std::vector<int16_t> x(6 * 512, (int16_t)32767), out(6 * 512);
    std::vector<uint8_t> active(6);
    const uint64_t clips = dcsgen_channel_slow(x.data(), 6, slots, h.data(), 512, 512, out.data(), active.data());
    CHECK(out[at - 512] == 32767 && clips > 0 && active[0] == 1 && active[5] == 1);      // g = (65535 * 32767 + 2^13) >> 14 on top of 32767
    for (auto &v : x)
    {
      v = -32768;
    }
    dcsgen_channel_slow(x.data(), 6, slots, h.data(), 512, 512, out.data(), nullptr);
    CHECK(out[at - 512] == 32767);                         // -32768 + 131066 saturates as well
    for (auto &v : h)
    {
      v = (int16_t)-v;
    }
    dcsgen_channel_slow(nullptr, 6, slots, h.data(), 512, 512, out.data(), nullptr);
    CHECK(out[at - 512] == -32768);
  }
  // a stream across u's wrap cut into calls, against one call; in place; generate only
  for (uint32_t T : {1u, 2u, 255u, 512u})
  {
    std::vector<int16_t> h(T);
    for (uint32_t j = 0; j < T; j++)
    {
      h[j] = (int16_t)((int)((j * 2654435761u) >> 20) % 255 - 127);
    }
    h[0] = 16384;
    const uint64_t N = 28750ull * 77 - 1300;
    DcsgenQueue q;
    hrfd_dcsgen_segment run[3] = {seg(900, 300, kWord, 32767, 17), seg(1, 0, 0x7fffff, 20000), seg(kDcsgenForever, 0, kWord ^ 0x7fffff, 9000, 600)};
    DcsgenQueue m;
    CHECK(dcsgen_lay_out("who", q, N, run, 3, kGenAppend, m) == HRFD_OK);
    DcsgenSlot slots[kDcsgenMaxSegments];
    dcsgen_fill_slots(m, slots);
    const uint32_t B = 8;
    std::vector<int16_t> x(B * 512), whole(B * 512), parts(B * 512), gen(B * 512);
    for (size_t i = 0; i < x.size(); i++)
    {
      x[i] = (int16_t)((i * 40503u) ^ (i >> 3));
    }
    std::vector<uint8_t> act_whole(B), act_parts(B);
    const uint64_t clips = dcsgen_channel_slow(x.data(), B, slots, h.data(), T, N, whole.data(), act_whole.data());
    uint64_t sum = 0, at = 0;
    for (uint32_t nb : {1u, 3u, 1u, 2u, 1u})
    {
      DcsgenQueue live = m;
      dcsgen_drop_ended(live, N + at * 512);               // what a call does first
      dcsgen_fill_slots(live, slots);
      sum += dcsgen_channel_slow(x.data() + at * 512, nb, slots, h.data(), T, N + at * 512, parts.data() + at * 512, act_parts.data() + at);
      at += nb;
    }
    CHECK(at == B && whole == parts && act_whole == act_parts && sum == clips);
    dcsgen_fill_slots(m, slots);
    std::vector<int16_t> y = x;
    CHECK(dcsgen_channel_slow(y.data(), B, slots, h.data(), T, N, y.data(), nullptr) == clips && y == whole);      // in place
    dcsgen_channel_slow(nullptr, B, slots, h.data(), T, N, gen.data(), nullptr);
    if (T == 1)
    {
      for (uint32_t i = 0; i < B * 512; i++)
      {
        const uint64_t n = N + i;
        const int32_t want = n < N + 17 ? 0 : n < N + 917 ? 32767 * bit_ref(kWord, n) : n < N + 1217 ? 32767 * sq_ref(n) : n < N + 1218 ? 20000
                             : n < N + 1818 ? 0 : 9000 * bit_ref(kWord ^ 0x7fffff, n);
        CHECK(gen[i] == want);
      }
    }
  }
  // the stream's start: nothing lies in front of time 0
  {
    int16_t h[512];
    for (auto &v : h)
    {
      v = 100;
    }
    DcsgenSlot slots[kDcsgenMaxSegments];
    dcsgen_fill_slots(DcsgenQueue{DcsgenSeg{DcsgenSlot{0, kDcsgenNoEnd, kDcsgenNoEnd, 0x7fffff, 1000}, 0}}, slots);
    int16_t out[512];
    dcsgen_channel_slow(nullptr, 1, slots, h, 512, 0, out, nullptr);
    CHECK(out[0] == dcsgen_round(100 * 1000) && out[511] == dcsgen_round(512 * 100 * 1000));
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_the_grids() || check_the_queue() || check_the_cut() || check_the_slow_loop())
  {
    return 1;
  }
  printf("san_dcsgen ok\n");
  return 0;
}
