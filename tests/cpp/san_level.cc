// Sanitizer harness for the HIP-free part of the level bank (hackrfdiags_amd/csrc/hrfd_level.h), CPU only: compiled as plain
// C++ under -fsanitize=address,undefined (tests/test_level_sanitizers.py).  Every check at its limit with its text, the five
// laws on their boundaries (|-32768|, both sides of the two rounding ties, the largest gain, the ramp's ends), the bound
// |y| <= target and the int32 product over random settings through the slow loop, a stream cut into calls against one long
// call, in place against out of place, and n_pcm with other bytes behind it.
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
#include "../../hackrfdiags_amd/csrc/hrfd_level.h"

using namespace hrfd;

#define CHECK(cond)                                                 \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      printf("san_level: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
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
  static_assert(kLevelFrame == HRFD_LEVEL_FRAME && kLevelMaxWeights == HRFD_LEVEL_MAX_WEIGHTS && kLevelMaxBlocks == HRFD_LEVEL_MAX_BLOCKS,
                "the header's limits are the public ones");
  static_assert(sizeof(LevelSetting) == 8, "the kernel reads this layout");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(level_check_create("who", c, &out), "channels"));
  }
  CHECK(refused(level_check_create("who", 1, nullptr), "result pointer") && level_check_create("who", 65536, &out) == HRFD_OK);

  uint16_t w[65];
  for (auto &v : w)
  {
    v = 32768;
  }
  CHECK(refused(level_check_weights("who", w, 0), "1..64 weights") && refused(level_check_weights("who", w, 65), "1..64 weights"));
  CHECK(refused(level_check_weights("who", nullptr, 1), "weights"));
  CHECK(level_check_weights("who", w, 1) == HRFD_OK && level_check_weights("who", w, 64) == HRFD_OK);
  w[0] = 32767;
  CHECK(refused(level_check_weights("who", w, 1), "w[0] must be 32768"));
  w[0] = 32769;
  CHECK(refused(level_check_weights("who", w, 64), "w[0] must be 32768"));
  w[0] = 32768;
  w[63] = 32769;
  CHECK(refused(level_check_weights("who", w, 64), "w[63] = 32769") && level_check_weights("who", w, 63) == HRFD_OK);
  w[63] = 0;
  w[1] = 65535;
  CHECK(refused(level_check_weights("who", w, 2), "w[1] = 65535"));

  CHECK(level_check_set("who", 0, 0, 16, 1) == HRFD_OK && level_check_set("who", HRFD_ALL_CHANNELS, 32767, 32768, 1) == HRFD_OK);
  CHECK(refused(level_check_set("who", 0, 32768, 16, 1), "target 32768") && refused(level_check_set("who", 0, 0xffffffffu, 16, 1), "target"));
  CHECK(refused(level_check_set("who", 0, 0, 15, 1), "floor 15") && refused(level_check_set("who", 0, 0, 32769, 1), "floor 32769"));
  CHECK(refused(level_check_set("who", 0, 0, 0, 1), "floor 0"));
  CHECK(refused(level_check_set("who", 5, 0, 16, 5), "channel 5") && level_check_set("who", 4, 0, 16, 5) == HRFD_OK);

  alignas(16) static char buf[65536];
  const void *in = buf + 16384, *far = buf + 40960, *g = buf + 4096, *p = buf + 8192;
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 0, far, 1024, g, p, 1), "n_blocks"));
  CHECK(refused(level_check_call("who", in, 1 << 21, true, nullptr, 1025, far, 1 << 21, g, p, 1), "n_blocks"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, nullptr, 1024, nullptr, nullptr, 1), "no output"));
  CHECK(level_check_call("who", in, 1024, true, nullptr, 1, nullptr, 0, g, nullptr, 1) == HRFD_OK);      // a meter: out's stride is not looked at
  CHECK(level_check_call("who", in, 1024, true, nullptr, 1, nullptr, 0, nullptr, p, 1) == HRFD_OK);
  CHECK(refused(level_check_call("who", in, 1022, true, nullptr, 1, far, 1024, g, p, 1), "channel_stride_bytes"));
  CHECK(refused(level_check_call("who", in, 1025, true, nullptr, 1, far, 1024, g, p, 1), "channel_stride_bytes"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, far, 1022, g, p, 1), "out_stride_bytes"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, far, 1027, g, p, 1), "out_stride_bytes"));
  CHECK(level_check_call("who", in, 0, false, nullptr, 1, far, 0, g, p, 2) == HRFD_OK);                  // the host entry has no strides
  CHECK(refused(level_check_call("who", buf + 16385, 1024, true, nullptr, 1, far, 1024, g, p, 1), "even addresses"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, buf + 40961, 1024, g, p, 1), "even addresses"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, far, 1024, g, buf + 8193, 1), "even addresses"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, far, 1024, buf + 4098, p, 1), "4-byte aligned"));
  CHECK(refused(level_check_call("who", in, 1024, true, buf + 2, 1, far, 1024, g, p, 1), "4-byte aligned"));
  CHECK(level_check_call("who", in, 1024, true, buf + 4, 1, far, 1024, g, buf + 8194, 1) == HRFD_OK);
  CHECK(refused(level_check_call("who", nullptr, 1024, true, nullptr, 1, far, 1024, g, p, 1), "NULL argument"));
  // in place: the input's own address and stride, and nothing else that overlaps
  CHECK(level_check_call("who", in, 1030, true, nullptr, 1, in, 1030, g, p, 4) == HRFD_OK);
  CHECK(level_check_call("who", in, 0, false, nullptr, 3, in, 0, g, p, 4) == HRFD_OK);
  CHECK(refused(level_check_call("who", in, 1030, true, nullptr, 1, in, 1032, g, p, 4), "overlaps"));
  CHECK(refused(level_check_call("who", in, 1030, true, nullptr, 1, in, 1032, g, p, 1), "in place means"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16386, 1024, g, p, 1), "overlaps"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 - 2, 1024, g, p, 1), "overlaps"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 + 1022, 1024, g, p, 1), "overlaps"));
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 - 1022, 1024, g, p, 1), "overlaps"));
  CHECK(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 + 1024, 1024, g, p, 1) == HRFD_OK);
  CHECK(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 - 1024, 1024, g, p, 1) == HRFD_OK);
  // out one row up: free of channel 0, inside the rows of four
  CHECK(refused(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 + 1024, 1024, g, p, 4), "overlaps"));
  CHECK(level_check_call("who", in, 1024, true, nullptr, 1, buf + 16384 + 4096, 1024, g, p, 4) == HRFD_OK);
  CHECK(refused(level_check_call("who", in, 0, false, nullptr, 1, buf + 16384 + 1022, 0, g, p, 1), "overlaps"));
  return 0;
}

static int check_laws()
{
  // 1. |x| in 32 bits
  CHECK(level_abs(-32768) == 32768 && level_abs(32767) == 32767 && level_abs(0) == 0 && level_abs(-1) == 1);
  // 2. (p w + 2^14) >> 15: identity at w = 32768, 0 at w = 0, the tie p w = 2^14 (mod 2^15) rounds up
  for (uint32_t p : {0u, 1u, 16u, 32767u, 32768u})
  {
    CHECK(level_weighted(p, 32768) == p && level_weighted(p, 0) == 0);
  }
  CHECK(level_weighted(32768, 32768) == 32768);
  CHECK(level_weighted(1, 16384) == 1 && level_weighted(1, 16383) == 0);               // 16384 and 16383 + 2^14
  CHECK(level_weighted(3, 16384) == 2 && level_weighted(16384, 3) == 2 && level_weighted(16383, 3) == 1);      // 1.5 up, 1.49.. down
  uint16_t p3[3] = {200, 100, 10}, w3[3] = {32768, 16384, 32768};
  CHECK(level_envelope(p3 + 2, w3, 3, 16) == 200 && level_envelope(p3 + 2, w3, 2, 16) == 50 && level_envelope(p3 + 2, w3, 1, 16) == 16);
  CHECK(level_envelope(p3 + 2, w3, 1, 10) == 10 && level_envelope(p3 + 2, w3, 1, 9) == 10);
  // 3. the gain: floor division, the largest
  CHECK(level_gain(32767, 16) == 8388352 && level_gain(32767, 32768) == 4095 && level_gain(0, 16) == 0);
  CHECK(level_gain(8192, 8192) == 4096 && level_gain(8192, 8193) == 4095 && level_gain(1, 32768) == 0);
  // 4. attack at once, release ramped: the last sample of the frame is at the new gain
  CHECK(level_sample_gain(5000, 4000, 0) == 4000 && level_sample_gain(5000, 5000, 17) == 5000);
  CHECK(level_sample_gain(4000, 5000, 0) == 4015 && level_sample_gain(4000, 5000, 31) == 4500 && level_sample_gain(4000, 5000, 63) == 5000);
  CHECK(level_sample_gain(0, 8388352, 63) == 8388352 && level_sample_gain(0, 8388352, 0) == 131068);
  CHECK(level_sample_gain(0, 63, 62) == 62 && level_sample_gain(0, 1, 62) == 0 && level_sample_gain(0, 1, 63) == 1);
  // 5. the output: ties of (x gs + 2^11) >> 12 on both signs (the shift is arithmetic), the extremes of the bound
  CHECK(level_output(1, 2048) == 1 && level_output(1, 2047) == 0);
  CHECK(level_output(-1, 2048) == 0 && level_output(-1, 2049) == -1 && level_output(-3, 2048) == -1 && level_output(-3, 2049) == -2);
  CHECK(level_output(-16, 8388352) == -32767 && level_output(16, 8388352) == 32767);
  CHECK(level_output(-32768, 4095) == -32760 && level_output(32767, 4095) == 32759 && level_output(-32768, 4096) == -32768);
  uint16_t w[64];
  level_default_weights(w);
  CHECK(w[0] == 32768 && w[7] == 32768 && w[8] == 32768 && w[9] == 32182 && w[63] == 585 && level_check_weights("who", w, 64) == HRFD_OK);
  return 0;
}

static uint32_t g_seed = 4711u;
static uint32_t next() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

// random settings and amplitudes from 1 to full scale: |y| <= target; the cut into calls, in place, other bytes behind n_pcm
static int check_bound_cutting_and_in_place()
{
  const uint32_t B = 5, n = B * kLevelBlock, F = B * kLevelFramesPerBlock;
  const uint32_t cuts[] = {2, 1, 2};
  for (int round = 0; round < 40; round++)
  {
    const uint32_t Ws[] = {1, 2, 3, 63, 64, 1 + next() % 64};
    const uint32_t W = Ws[next() % 6];
    const uint32_t targets[] = {0, 1, 32767, next() % 32768}, floors[] = {16, 17, 32768, 16 + next() % 32753};
    const uint32_t target = targets[next() % 4], floor = floors[next() % 4];
    std::vector<uint16_t> w(W);
    for (auto &v : w)
    {
      v = (uint16_t)(next() % 32769);
    }
    w[0] = 32768;
    CHECK(level_check_weights("who", w.data(), W) == HRFD_OK && level_check_set("who", 0, target, floor, 1) == HRFD_OK);
    std::vector<int16_t> x(n), other(n);
    uint32_t amp = 1;
    for (uint32_t i = 0; i < n; i++)
    {
      if (i % 192 == 0)
      {
        const uint32_t amps[] = {0, 1, 15, 16, 17, 300, 32767, 32768, 1 + next() % 32768};
        amp = amps[next() % 9];
      }
      const int32_t v = (int32_t)(next() % (2 * amp + 1)) - (int32_t)amp;
      x[i] = (int16_t)(v > 32767 ? 32767 : v);
    }
    x[n / 2] = -32768;
    const uint32_t n_pcm[B] = {512, 0xffffffffu, 300, 0, 511};
    other = x;
    for (uint32_t b = 0; b < B; b++)
    {
      for (uint32_t i = pcm_block_limit(n_pcm, b); i < kLevelBlock; i++)
      {
        other[b * kLevelBlock + i] ^= 0x5a5a;
      }
    }
    std::vector<int16_t> y(n), yc(n), yo(n);
    std::vector<uint32_t> g(F), gc(F), gb(F);
    std::vector<uint16_t> p(F), pc(F), pb(F), hist(kLevelHist, 0), hist_c(kLevelHist, 0), hist_o(kLevelHist, 0), hist_b(kLevelHist, 0);
    level_channel_slow(x.data(), n_pcm, B, w.data(), W, target, floor, false, hist.data(), y.data(), g.data(), p.data());
    for (uint32_t i = 0; i < n; i++)
    {
      CHECK((uint32_t)(y[i] < 0 ? -y[i] : y[i]) <= target);
    }
    for (uint32_t f = 0; f < F; f++)
    {
      CHECK(g[f] <= 8388352u && (uint64_t)g[f] * (p[f] > floor ? p[f] : floor) <= ((uint64_t)target << 12));
    }
    // cut 2 + 1 + 2, in place, with other bytes behind n_pcm
    uint32_t at = 0;
    for (uint32_t k : cuts)
    {
      level_channel_slow(x.data() + at * kLevelBlock, n_pcm + at, k, w.data(), W, target, floor, false, hist_c.data(),
                         yc.data() + at * kLevelBlock, gc.data() + at * kLevelFramesPerBlock, pc.data() + at * kLevelFramesPerBlock);
      int16_t *io = other.data() + at * kLevelBlock;
      level_channel_slow(io, n_pcm + at, k, w.data(), W, target, floor, false, hist_o.data(), io, nullptr, nullptr);
      at += k;
    }
    CHECK(y == yc && g == gc && p == pc && hist == hist_c && y == other && hist == hist_o);
    // bypass: y = x under the limit, the meters as before; a meter call moves the history alike
    level_channel_slow(x.data(), n_pcm, B, w.data(), W, target, floor, true, hist_b.data(), yo.data(), gb.data(), pb.data());
    for (uint32_t i = 0; i < n; i++)
    {
      CHECK(yo[i] == (i % kLevelBlock < pcm_block_limit(n_pcm, i / kLevelBlock) ? x[i] : 0));
    }
    CHECK(g == gb && p == pb && hist == hist_b);
    std::fill(hist_b.begin(), hist_b.end(), (uint16_t)0);
    level_channel_slow(x.data(), n_pcm, B, w.data(), W, target, floor, false, hist_b.data(), nullptr, nullptr, pb.data());
    CHECK(p == pb && hist == hist_b && hist[63] == p[F - 1] && hist[0] == (F >= 64 ? p[F - 64] : 0));
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_bound_cutting_and_in_place())
  {
    return 1;
  }
  printf("san_level ok\n");
  return 0;
}
