// Sanitizer harness for the HIP-free part of the tone generator bank (hackrfdiags_amd/csrc/hrfd_tonegen.h, and hrfd_gen.h,
// which it shares with the AFSK generator), CPU only: compiled
// as plain C++ under -fsanitize=address,undefined (tests/test_tonegen_sanitizers.py).  Every check at its limit with its text,
// the laws on their boundaries (the zero crossing at k = 0, both signs of the rounding, the largest mix, the ramp's ends),
// every rule of the queue (append, insertion, overlap, FOREVER, the 32 segments, times near 2^63), the cut, and the slow loop:
// against a restatement written out here, a stream cut into calls against one long call, in place against out of place,
// generate only, k across and above 2^32, saturation with its count, and the active bits.
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
#include "../../hackrfdiags_amd/csrc/hrfd_tonegen.h"
#include "../../hackrfdiags_amd/csrc/hrfd_ddc_tables.h"

using namespace hrfd;

#define CHECK(cond)                                                   \
  do                                                                  \
  {                                                                   \
    if (!(cond))                                                      \
    {                                                                 \
      printf("san_tonegen: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static hrfd_tonegen_segment seg(uint32_t length, uint32_t step_a = 0, uint32_t amp_a = 0, uint32_t step_b = 0, uint32_t amp_b = 0,
                                uint32_t gap = 0)
{
  return hrfd_tonegen_segment{gap, length, step_a, step_b, amp_a, amp_b};
}

static int check_the_checks()
{
  static_assert(kTonegenTracks == HRFD_TONEGEN_TRACKS && kTonegenMaxSegments == HRFD_TONEGEN_MAX_SEGMENTS &&
                    kGenMaxBlocks == HRFD_TONEGEN_MAX_BLOCKS && kTonegenForever == HRFD_TONEGEN_FOREVER &&
                    kGenAppend == HRFD_TONEGEN_APPEND,
                "the header's limits are the public ones");
  static_assert(sizeof(hrfd_tonegen_segment) == 24, "six uint32");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(tonegen_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(tonegen_check_create("who", 1, nullptr), "result pointer") && tonegen_check_create("who", 65536, &out) == HRFD_OK);

  hrfd_tonegen_segment s33[33];
  for (auto &s : s33)
  {
    s = seg(1);
  }
  CHECK(tonegen_check_segments("who", s33, 1, 0) == HRFD_OK && tonegen_check_segments("who", s33, 32, 1) == HRFD_OK);
  CHECK(refused(tonegen_check_segments("who", s33, 1, 2), "track 2"));
  CHECK(refused(tonegen_check_segments("who", s33, 0, 0), "1..32 segments") && refused(tonegen_check_segments("who", s33, 33, 0), "1..32 segments"));
  CHECK(refused(tonegen_check_segments("who", nullptr, 1, 0), "segments"));
  s33[3] = seg(1, 0, 32768);
  CHECK(refused(tonegen_check_segments("who", s33, 4, 0), "segment 3 has an amp above 32767") && tonegen_check_segments("who", s33, 3, 0) == HRFD_OK);
  s33[3] = seg(1, 0, 32767, 0, 32768);
  CHECK(refused(tonegen_check_segments("who", s33, 4, 0), "amp above"));
  s33[3] = seg(1, 0xffffffffu, 32767, 0xffffffffu, 32767, 0xffffffffu);
  CHECK(tonegen_check_segments("who", s33, 4, 0) == HRFD_OK);
  s33[3] = seg(0);
  CHECK(refused(tonegen_check_segments("who", s33, 4, 0), "segment 3 has length 0"));
  s33[3] = seg(kTonegenForever);
  CHECK(tonegen_check_segments("who", s33, 4, 0) == HRFD_OK && refused(tonegen_check_segments("who", s33, 5, 0), "segment 4 lies behind a FOREVER"));
  s33[3] = seg(0xfffffffeu);
  CHECK(tonegen_check_segments("who", s33, 5, 0) == HRFD_OK);

  CHECK(gen_check_time("who", 0) == HRFD_OK && gen_check_time("who", (1ull << 63) - 1) == HRFD_OK);
  CHECK(refused(gen_check_time("who", 1ull << 63), "below 2^63") && refused(gen_check_time("who", ~0ull), "below 2^63"));
  CHECK(gen_check_one_channel("who", 0, 1) == HRFD_OK && gen_check_one_channel("who", 65535, 65536) == HRFD_OK);
  CHECK(refused(gen_check_one_channel("who", 5, 5), "channel 5 (0..4)") && refused(gen_check_one_channel("who", HRFD_ALL_CHANNELS, 65536), "(0..65535)"));
  CHECK(tonegen_check_track("who", 4, 1, 5) == HRFD_OK && tonegen_check_track("who", HRFD_ALL_CHANNELS, 0, 1) == HRFD_OK);
  CHECK(refused(tonegen_check_track("who", 5, 0, 5), "channel 5") && refused(tonegen_check_track("who", 0, 2, 5), "track 2"));

  alignas(16) static char buf[65536];
  const void *in = buf + 16384, *far = buf + 40960;
  CHECK(refused(gen_check_call("who", in, 1024, true, 0, far, 1024, 1), "n_blocks"));
  CHECK(refused(gen_check_call("who", in, 1 << 21, true, 1025, far, 1 << 21, 1), "n_blocks"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, nullptr, 1024, 1), "NULL argument"));
  CHECK(refused(gen_check_call("who", in, 1022, true, 1, far, 1024, 1), "channel_stride_bytes"));
  CHECK(refused(gen_check_call("who", in, 1025, true, 1, far, 1024, 1), "channel_stride_bytes"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, far, 1022, 1), "out_stride_bytes"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, far, 1027, 1), "out_stride_bytes"));
  CHECK(gen_check_call("who", nullptr, 0, true, 1, far, 1024, 7) == HRFD_OK);          // generate only: no input stride
  CHECK(refused(gen_check_call("who", nullptr, 0, true, 1, far, 1022, 7), "out_stride_bytes"));
  CHECK(gen_check_call("who", in, 0, false, 1, far, 0, 2) == HRFD_OK);                 // the host entry has no strides
  CHECK(gen_check_call("who", nullptr, 0, false, 1024, far, 0, 1) == HRFD_OK);
  CHECK(refused(gen_check_call("who", buf + 16385, 1024, true, 1, far, 1024, 1), "even addresses"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, buf + 40961, 1024, 1), "even addresses"));
  // in place: the input's own address and stride, and nothing else that overlaps
  CHECK(gen_check_call("who", in, 1030, true, 1, in, 1030, 4) == HRFD_OK);
  CHECK(gen_check_call("who", in, 0, false, 3, in, 0, 4) == HRFD_OK);
  CHECK(refused(gen_check_call("who", in, 1030, true, 1, in, 1032, 4), "overlaps"));
  CHECK(refused(gen_check_call("who", in, 1030, true, 1, in, 1032, 1), "in place means"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, buf + 16386, 1024, 1), "overlaps"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, buf + 16384 - 2, 1024, 1), "overlaps"));
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, buf + 16384 + 1022, 1024, 1), "overlaps"));
  CHECK(gen_check_call("who", in, 1024, true, 1, buf + 16384 + 1024, 1024, 1) == HRFD_OK);
  CHECK(gen_check_call("who", in, 1024, true, 1, buf + 16384 - 1024, 1024, 1) == HRFD_OK);
  CHECK(refused(gen_check_call("who", in, 1024, true, 1, buf + 16384 + 1024, 1024, 4), "overlaps"));      // inside the rows of four
  CHECK(gen_check_call("who", in, 1024, true, 1, buf + 16384 + 4096, 1024, 4) == HRFD_OK);
  return 0;
}

static int check_laws()
{
  // 1. the index: rounded to the nearest of 4096, the sine a quarter turn behind the cosine, zero at theta = 0
  CHECK(gen_cos_index(0) == 0 && gen_cos_index((1u << 19) - 1) == 0 && gen_cos_index(1u << 19) == 1);
  CHECK(gen_cos_index(0xfff80000u) == 0 && gen_cos_index(0xfff7ffffu) == 4095);
  CHECK(gen_sin_index(0) == 3072 && Q_DDC_COS[3072] == 0 && Q_DDC_COS[gen_sin_index(1u << 30)] == 32767);
  CHECK(Q_DDC_COS[gen_sin_index(3u << 30)] == -32767 && Q_DDC_COS[gen_sin_index(1u << 31)] == 0);
  // 2. the mix: the largest sums, the rounding on both signs (the shift is arithmetic)
  CHECK(gen_mix(32767, 32767, 32767, 32767) == 65532 && gen_mix(32767, -32767, 32767, -32767) == -65532);
  CHECK(gen_mix(1, 16384, 0, 0) == 1 && gen_mix(1, 16383, 0, 0) == 0 && gen_mix(1, -16384, 0, 0) == 0 &&
        gen_mix(1, -16385, 0, 0) == -1);
  CHECK(gen_mix(0, 32767, 0, -32767) == 0 && gen_mix(32767, 32767, 32767, -32767) == 0);
  // 3. the ramp: e = 64 gives v itself; the ends; the rounding
  for (int32_t v : {-65534, -1, 0, 1, 77, 65534})
  {
    CHECK(gen_ramp(v, 64, 64) == v && gen_ramp(v, 1000, 64) == v && gen_ramp(v, 64, 1u << 20) == v);
  }
  CHECK(gen_ramp(6400, 1, 64) == 100 && gen_ramp(6400, 64, 1) == 100 && gen_ramp(6400, 63, 2) == 200 &&
        gen_ramp(6400, 32, 33) == 3200);
  CHECK(gen_ramp(1, 32, 64) == 1 && gen_ramp(1, 31, 64) == 0 && gen_ramp(-1, 32, 64) == 0 && gen_ramp(-1, 33, 64) == -1);
  CHECK(gen_ramp(65534, 63, 64) == 64510 && gen_ramp(-65534, 64, 63) == -64510);
  // 4. the output
  bool clip;
  CHECK(gen_output(32767, 0, &clip) == 32767 && !clip && gen_output(32767, 1, &clip) == 32767 && clip);
  CHECK(gen_output(-32768, 0, &clip) == -32768 && !clip && gen_output(-32768, -1, &clip) == -32768 && clip);
  CHECK(gen_output(-32768, 131068, &clip) == 32767 && clip && gen_output(32767, -131068, &clip) == -32768 && clip);
  CHECK(gen_output(-32768, 65535, &clip) == 32767 && !clip && gen_output(100, -200, &clip) == -100 && !clip);
  return 0;
}

static int check_queue()
{
  TonegenTrack q, m;
  hrfd_tonegen_segment two[2] = {seg(100), seg(50, 0, 0, 0, 0, 10)};
  CHECK(tonegen_lay_out("who", q, 0, two, 2, 1000, m) == HRFD_OK && m.size() == 2);
  CHECK(m[0].start == 1000 && m[0].end == 1100 && m[1].start == 1110 && m[1].end == 1160);
  q = m;
  hrfd_tonegen_segment one = seg(10);
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, 1100, m) == HRFD_OK && m.size() == 3 && m[1].start == 1100);       // into the gap
  q = m;
  one = seg(1000);
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, 0, m) == HRFD_OK && m.size() == 4 && m[0].start == 0 && m[3].end == 1160);      // in front
  q = m;
  one = seg(2);
  for (uint64_t start : {999ull, 1099ull, 1101ull, 1159ull})
  {
    CHECK(refused(tonegen_lay_out("who", q, 0, &one, 1, start, m), "overlap"));
  }
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, 1160, m) == HRFD_OK);
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, kGenAppend, m) == HRFD_OK && m.back().start == 1160 && m.back().end == 1162);
  CHECK(tonegen_lay_out("who", q, 5000, &one, 1, kGenAppend, m) == HRFD_OK && m.size() == 1 && m[0].start == 5000);       // all ended
  CHECK(refused(tonegen_lay_out("who", q, 1050, &one, 1, 1049, m), "before the stream time 1050"));
  CHECK(tonegen_lay_out("who", q, 1050, &one, 1, 1160, m) == HRFD_OK && m.size() == 4 && m[0].start == 1000);    // [0, 1000) has ended
  one = seg(kTonegenForever, 5, 6, 7, 8, 3);
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, kGenAppend, m) == HRFD_OK && m.back().start == 1163 && m.back().end == kTonegenNoEnd);
  CHECK(m.back().step_a == 5 && m.back().step_b == 7 && m.back().amps == (6u | (8u << 16)));
  q = m;
  one = seg(1);
  CHECK(refused(tonegen_lay_out("who", q, 0, &one, 1, kGenAppend, m), "appended behind a FOREVER"));
  CHECK(refused(tonegen_lay_out("who", q, 0, &one, 1, 1ull << 40, m), "behind the FOREVER segment at 1163"));
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, 1160, m) == HRFD_OK);                        // in front of it still
  CHECK(tonegen_track_end(q) == kTonegenNoEnd);
  // the 32
  q.clear();
  hrfd_tonegen_segment many[32];
  for (auto &s : many)
  {
    s = seg(1);
  }
  CHECK(tonegen_lay_out("who", q, 0, many, 32, kGenAppend, m) == HRFD_OK && m.size() == 32 && m[31].end == 32);
  q = m;
  CHECK(refused(tonegen_lay_out("who", q, 0, many, 1, kGenAppend, m), "33 segments"));
  CHECK(refused(tonegen_lay_out("who", q, 31, many, 32, kGenAppend, m), "33 segments"));          // one has not ended
  CHECK(tonegen_lay_out("who", q, 32, many, 32, kGenAppend, m) == HRFD_OK && m.size() == 32 && m[0].start == 32);
  // times near 2^63
  q.clear();
  one = seg(0xfffffffeu, 0, 0, 0, 0, 0xffffffffu);
  CHECK(tonegen_lay_out("who", q, 0, &one, 1, (1ull << 63) - 0x200000000ull, m) == HRFD_OK);
  CHECK(refused(tonegen_lay_out("who", q, 0, &one, 1, (1ull << 63) - 0x1fffffffdull, m), "2^63"));
  CHECK(refused(tonegen_lay_out("who", q, 0, &one, 1, (1ull << 63) - 1, m), "2^63"));
  // the cut
  q.clear();
  hrfd_tonegen_segment three[3] = {seg(100), seg(200, 0, 0, 0, 0, 50), seg(kTonegenForever)};
  CHECK(tonegen_lay_out("who", q, 0, three, 3, 0, q) == HRFD_OK && q.size() == 3);
  TonegenTrack c = q;
  tonegen_cut(c, 120);                                     // in the gap: everything left has not begun
  CHECK(c.empty());
  c = q;
  tonegen_cut(c, 150);                                     // the second has just begun
  CHECK(c.size() == 1 && c[0].start == 150 && c[0].end == 214);
  c = q;
  tonegen_cut(c, 300);                                     // 50 samples left: the end stays
  CHECK(c.size() == 1 && c[0].end == 350);
  c = q;
  tonegen_cut(c, (1ull << 33) + 7);                        // the endless one, further than 2^32 from its start
  CHECK(c.size() == 1 && c[0].start == 350 && c[0].end == (1ull << 33) + 71);
  tonegen_drop_ended(c, (1ull << 33) + 70);
  CHECK(c.size() == 1);
  tonegen_drop_ended(c, (1ull << 33) + 71);
  CHECK(c.empty());
  return 0;
}

static uint32_t g_seed = 4711u;
static uint32_t next() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// the contract written out again, with the length where the header keeps the end
static int32_t restated(const TonegenSlot &s, uint64_t n)
{
  if (n < s.start || n >= s.end)
  {
    return 0;
  }
  const uint64_t k = n - s.start;
  int64_t S[2];
  const uint32_t steps[2] = {s.step_a, s.step_b};
  for (int x = 0; x < 2; x++)
  {
    const uint64_t theta = ((uint64_t)steps[x] * (k & 0xffffffffull)) & 0xffffffffull;
    const uint64_t i = ((theta + (1u << 19)) >> 20) & 4095;
    S[x] = Q_DDC_COS[(i + 4096 - 1024) & 4095];
  }
  const int64_t sum = (int64_t)(s.amps & 0xffff) * S[0] + (int64_t)(s.amps >> 16) * S[1] + (1 << 14);
  const int64_t v = sum >= 0 ? sum / 32768 : -((-sum + 32767) / 32768);                 // floor(sum / 2^15)
  uint64_t e = k + 1 < 64 ? k + 1 : 64;
  if (s.end != kTonegenNoEnd)
  {
    const uint64_t length = s.end - s.start;
    e = length - k < e ? length - k : e;
  }
  const int64_t w = v * (int64_t)e + 32;
  return (int32_t)(w >= 0 ? w / 64 : -((-w + 63) / 64));
}

static int check_slow_loop()
{
  const uint32_t B = 9, n = B * kGenBlock;
  for (int round = 0; round < 12; round++)
  {
    const uint64_t bases[] = {0, 1, (1ull << 32) - 1024, (1ull << 32) + 5, (1ull << 40) + 333, 1ull << 62};
    const uint64_t N = bases[round % 6];
    // two tracks laid out around the call through the queue rules; the second starts long before the call in some rounds
    TonegenTrack tr[2];
    for (uint32_t t = 0; t < 2; t++)
    {
      std::vector<hrfd_tonegen_segment> segs;
      const uint32_t lens[] = {1, 2, 63, 64, 65, 127, 128, 129, 512, 2048, 1 + next() % 3000};
      const uint32_t count = 1 + next() % 12;
      for (uint32_t i = 0; i < count; i++)
      {
        segs.push_back(seg(lens[next() % 11], next() << 8, next() % 32768, next() << 8, round % 2 ? 32767 : next() % 32768,
                           next() % 4 == 0 ? next() % 700 : 0));
      }
      if (next() % 2 == 0)
      {
        segs.push_back(seg(kTonegenForever, next() << 8, 32767, next() << 8, 32767));
      }
      TonegenTrack m;
      CHECK(tonegen_lay_out("who", tr[t], N, segs.data(), (uint32_t)segs.size(), N + (t == 0 ? 0 : next() % 600), m) == HRFD_OK);
      tr[t] = m;
      if (t == 1 && N > (1ull << 33))
      {
        tr[t][0].start -= (1ull << 32) + 17;               // k above 2^32 inside the call
      }
    }
    TonegenSlot slots[kTonegenSlots];
    tonegen_fill_slots(tr, slots);
    std::vector<int16_t> x(n), y(n), yc(n), io(n), gen(n), genc(n);
    for (uint32_t i = 0; i < n; i++)
    {
      const uint32_t r = next();
      x[i] = (int16_t)(r % 5 == 0 ? 32767 : (r % 5 == 1 ? -32768 : (int32_t)(r % 65536) - 32768));
    }
    uint8_t act[B], actc[B], actg[B];
    const uint64_t clips = tonegen_channel_slow(x.data(), B, slots, N, Q_DDC_COS, y.data(), act);
    // the restatement, sample by sample
    uint64_t want_clips = 0;
    for (uint32_t i = 0; i < n; i++)
    {
      int64_t sum = x[i];
      for (uint32_t j = 0; j < kTonegenSlots; j++)
      {
        sum += restated(slots[j], N + i);
      }
      const int64_t sat = sum < -32768 ? -32768 : (sum > 32767 ? 32767 : sum);
      want_clips += sat != sum;
      CHECK(y[i] == sat);
    }
    CHECK(clips == want_clips);
    for (uint32_t b = 0; b < B; b++)
    {
      uint8_t bits = 0;
      for (uint32_t j = 0; j < kTonegenSlots; j++)
      {
        for (uint32_t i = 0; i < kGenBlock && !(bits >> (j / 32) & 1); i++)
        {
          const uint64_t at = N + (uint64_t)b * kGenBlock + i;
          bits |= (uint8_t)((at >= slots[j].start && at < slots[j].end ? 1 : 0) << (j / 32));
        }
      }
      CHECK(act[b] == bits);
    }
    // cut 1 + 3 + 5, in place; generate only whole and cut
    const uint32_t cuts[] = {1, 3, 5};
    io = x;
    uint32_t at = 0;
    uint64_t clips_c = 0, clips_io = 0;
    for (uint32_t k : cuts)
    {
      const uint64_t Nk = N + (uint64_t)at * kGenBlock;
      clips_c += tonegen_channel_slow(x.data() + at * kGenBlock, k, slots, Nk, Q_DDC_COS, yc.data() + at * kGenBlock, actc + at);
      int16_t *p = io.data() + at * kGenBlock;
      clips_io += tonegen_channel_slow(p, k, slots, Nk, Q_DDC_COS, p, nullptr);
      tonegen_channel_slow(nullptr, k, slots, Nk, Q_DDC_COS, genc.data() + at * kGenBlock, nullptr);
      at += k;
    }
    tonegen_channel_slow(nullptr, B, slots, N, Q_DDC_COS, gen.data(), actg);
    CHECK(y == yc && y == io && clips == clips_c && clips == clips_io && gen == genc);
    CHECK(memcmp(act, actc, B) == 0 && memcmp(act, actg, B) == 0);
  }
  // a channel of empty slots passes its input through and generates silence
  TonegenTrack none[2];
  TonegenSlot slots[kTonegenSlots];
  tonegen_fill_slots(none, slots);
  std::vector<int16_t> x(512), y(512, 1);
  for (uint32_t i = 0; i < 512; i++)
  {
    x[i] = (int16_t)(i * 127 - 32768);
  }
  uint8_t act = 9;
  CHECK(tonegen_channel_slow(x.data(), 1, slots, 12345, Q_DDC_COS, y.data(), &act) == 0 && x == y && act == 0);
  CHECK(tonegen_channel_slow(nullptr, 1, slots, 0, Q_DDC_COS, y.data(), nullptr) == 0 && y == std::vector<int16_t>(512, 0));
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_queue() || check_slow_loop())
  {
    return 1;
  }
  printf("san_tonegen ok\n");
  return 0;
}
