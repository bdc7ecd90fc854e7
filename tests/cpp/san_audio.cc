// Sanitizer harness for the HIP-free part of the audio bank (hackrfdiags_amd/csrc/hrfd_audio.h), CPU only: compiled as plain
// C++ under -fsanitize=address,undefined (tests/test_audio_sanitizers.py).  Every check at its limit with its text, the
// three laws on their boundaries, the slow loop at the largest sums the laws allow (sum |h| = 65535 under full-scale input
// of the sign that makes every product positive or negative, T = 512; a bus of 4096 entries of gain +-32767 over
// full-scale z), the history across calls against one long call, and the tone squelch against a loop over the frames.
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
#include "../../hackrfdiags_amd/csrc/hrfd_audio.h"

using namespace hrfd;

#define CHECK(cond)                                                 \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      printf("san_audio: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
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
  static_assert(kAudioMaxTaps == HRFD_AUDIO_MAX_TAPS && kAudioMaxBuses == HRFD_AUDIO_MAX_BUSES && kAudioMaxList == HRFD_AUDIO_MAX_LIST &&
                    kAudioMaxBlocks == HRFD_AUDIO_MAX_BLOCKS && kAudioAnyTone == HRFD_AUDIO_ANY_TONE && kAudioNoTone == HRFD_AUDIO_NO_TONE,
                "the header's limits are the public ones");
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(audio_check_create("who", c, 1, &out), "channels"));
  }
  for (uint32_t m : {0u, 65u, 0xffffffffu})
  {
    CHECK(refused(audio_check_create("who", 1, m, &out), "buses"));
  }
  CHECK(refused(audio_check_create("who", 1, 1, nullptr), "result pointer"));
  CHECK(audio_check_create("who", 1, 1, &out) == HRFD_OK && audio_check_create("who", 65536, 64, &out) == HRFD_OK);

  std::vector<int16_t> h(513, 1);
  CHECK(refused(audio_check_taps("who", h.data(), 0), "taps"));
  CHECK(refused(audio_check_taps("who", h.data(), 513), "taps"));
  CHECK(refused(audio_check_taps("who", nullptr, 1), "taps"));
  CHECK(audio_check_taps("who", h.data(), 512) == HRFD_OK && audio_check_taps("who", h.data(), 1) == HRFD_OK);
  h[0] = -32768;
  h[1] = 32767;
  CHECK(audio_check_taps("who", h.data(), 2) == HRFD_OK);                // 65535
  CHECK(refused(audio_check_taps("who", h.data(), 3), "sum |h| = 65536"));

  std::vector<uint32_t> ch(4097, 7u);
  std::vector<int16_t> g(4097, 32767);
  g[4095] = -32767;
  CHECK(audio_check_bus("who", 63, ch.data(), g.data(), 4096, 8, 64) == HRFD_OK);
  CHECK(audio_check_bus("who", 0, nullptr, nullptr, 0, 1, 1) == HRFD_OK);
  CHECK(refused(audio_check_bus("who", 64, ch.data(), g.data(), 1, 8, 64), "bus 64"));
  CHECK(refused(audio_check_bus("who", 1, ch.data(), g.data(), 1, 8, 1), "bus 1"));
  CHECK(refused(audio_check_bus("who", 0, ch.data(), g.data(), 4097, 8, 64), "4097"));
  CHECK(refused(audio_check_bus("who", 0, nullptr, g.data(), 1, 8, 64), "arrays"));
  CHECK(refused(audio_check_bus("who", 0, ch.data(), nullptr, 1, 8, 64), "arrays"));
  CHECK(refused(audio_check_bus("who", 0, ch.data(), g.data(), 4096, 7, 64), "names channel 7"));
  g[4095] = -32768;
  CHECK(refused(audio_check_bus("who", 0, ch.data(), g.data(), 4096, 8, 64), "entry 4095 has gain -32768"));
  CHECK(audio_check_bus("who", 0, ch.data(), g.data(), 4095, 8, 64) == HRFD_OK);

  for (uint32_t want = 0; want <= 300; want++)
  {
    const bool ok = want < 128 || want == 254 || want == 255;
    CHECK(ok ? audio_check_want("who", 0, want, 1) == HRFD_OK : refused(audio_check_want("who", 0, want, 1), "want"));
  }
  CHECK(refused(audio_check_want("who", 5, 0, 5), "channel 5"));
  CHECK(audio_check_want("who", HRFD_ALL_CHANNELS, 254, 5) == HRFD_OK && audio_check_want("who", 4, 255, 5) == HRFD_OK);
  CHECK(refused(pcm_check_channel("who", 5, 5), "channel 5") && pcm_check_channel("who", 4, 5) == HRFD_OK);
  CHECK(pcm_check_channel("who", HRFD_ALL_CHANNELS, 1) == HRFD_OK);

  alignas(16) static char buf[16384];
  const void *p = buf;
  CHECK(refused(audio_check_gate("who", p, p, 128, 0, 0, p), "n_blocks"));
  CHECK(refused(audio_check_gate("who", p, p, 128, 0, 1025, p), "n_blocks"));
  for (uint32_t L : {0u, 64u, 192u, 16384u, 0x80000000u})
  {
    CHECK(refused(audio_check_gate("who", p, p, L, 0, 16, p), "frame_len"));
  }
  for (uint32_t L = 128; L <= 8192; L *= 2)
  {
    for (uint32_t nb = 1; nb <= 1024; nb++)
    {
      const bool whole = (512 * nb) % L == 0;
      CHECK(whole ? audio_check_gate("who", p, p, L, 3, nb, p) == HRFD_OK : refused(audio_check_gate("who", p, p, L, 3, nb, p), "frames"));
    }
  }
  CHECK(refused(audio_check_gate("who", p, p, 128, 4, 1, p), "group"));
  CHECK(refused(audio_check_gate("who", nullptr, p, 128, 0, 1, p), "NULL argument"));
  CHECK(refused(audio_check_gate("who", p, nullptr, 128, 0, 1, p), "NULL argument"));
  CHECK(refused(audio_check_gate("who", p, p, 128, 0, 1, nullptr), "NULL argument"));

  const void *in = buf + 4096, *mix = buf + 12288;
  CHECK(refused(audio_check_call("who", in, 1024, true, 0, buf, 1024, mix, mix, 1), "n_blocks"));
  CHECK(refused(audio_check_call("who", in, 1 << 21, true, 1025, buf, 1 << 21, mix, mix, 1), "n_blocks"));
  CHECK(refused(audio_check_call("who", in, 1024, true, 1, nullptr, 1024, nullptr, mix, 1), "no output"));
  CHECK(refused(audio_check_call("who", in, 1022, true, 1, buf, 1024, mix, mix, 1), "channel_stride_bytes"));
  CHECK(refused(audio_check_call("who", in, 1025, true, 1, buf, 1024, mix, mix, 1), "channel_stride_bytes"));
  CHECK(refused(audio_check_call("who", in, 1024, true, 1, buf, 1022, mix, mix, 1), "out_stride_bytes"));
  CHECK(refused(audio_check_call("who", in, 1024, true, 1, buf, 1027, mix, mix, 1), "out_stride_bytes"));
  CHECK(audio_check_call("who", in, 1024, true, 1, nullptr, 7, mix, mix, 1) == HRFD_OK);       // no out: its stride is not looked at
  CHECK(audio_check_call("who", in, 0, false, 2, buf, 0, mix, mix, 2) == HRFD_OK);             // the host entry has no strides
  CHECK(refused(audio_check_call("who", buf + 4097, 1024, true, 1, buf, 1024, mix, mix, 1), "even address"));
  CHECK(refused(audio_check_call("who", in, 1024, true, 1, buf + 1, 1024, mix, mix, 1), "even address"));
  CHECK(refused(audio_check_call("who", in, 1024, true, 1, buf, 1024, buf + 12289, mix, 1), "even address"));
  CHECK(refused(audio_check_call("who", in, 1024, true, 1, buf, 1024, mix, buf + 12290, 1), "aligned"));
  CHECK(refused(audio_check_call("who", nullptr, 1024, true, 1, buf, 1024, mix, mix, 1), "NULL argument"));
  // out against the input's rows: [4096, 4096 + 3 x 1030 + 1024) with 4 channels
  CHECK(audio_check_call("who", in, 1030, true, 1, buf + 4096 - 3 * 1024 - 1024, 1024, mix, mix, 4) == HRFD_OK);
  CHECK(refused(audio_check_call("who", in, 1030, true, 1, buf + 4096 - 3 * 1024 - 1022, 1024, mix, mix, 4), "overlaps"));
  CHECK(audio_check_call("who", in, 1030, true, 1, buf + 4096 + 3 * 1030 + 1024, 1024, nullptr, nullptr, 4) == HRFD_OK);
  CHECK(refused(audio_check_call("who", in, 1030, true, 1, buf + 4096 + 3 * 1030 + 1022, 1024, nullptr, nullptr, 4), "overlaps"));
  CHECK(refused(audio_check_call("who", in, 0, false, 2, buf + 4096 + 2046, 0, mix, mix, 1), "overlaps"));
  CHECK(audio_check_call("who", in, 0, false, 2, buf + 4096 + 2048, 0, mix, mix, 1) == HRFD_OK);
  return 0;
}

static int check_laws()
{
  // the filter's rounding and saturation (pcm_fir_round): tests/cpp/san_pcm.cc
  // the envelope: 64 samples, monotonic, exact ends
  for (uint32_t n = 0; n < 512; n++)
  {
    CHECK(audio_envelope(true, true, n) == 32768 && audio_envelope(false, false, n) == 0);
    const int32_t up = audio_envelope(false, true, n), down = audio_envelope(true, false, n);
    CHECK(up + down == 32768 && up == (n < 64 ? 512 * (int32_t)(n + 1) : 32768));
  }
  CHECK(audio_envelope(false, true, 0) == 512 && audio_envelope(false, true, 62) == 32256 && audio_envelope(false, true, 63) == 32768);
  CHECK(audio_envelope(true, false, 0) == 32256 && audio_envelope(true, false, 63) == 0);
  for (int32_t y : {-32768, -32767, -1, 0, 1, 32767})
  {
    CHECK(audio_gate(y, 32768) == y && audio_gate(y, 0) == 0);
  }
  CHECK(audio_gate(32767, 512) == 512 && audio_gate(-32768, 512) == -512 && audio_gate(-32768, 32256) == -32256);
  // bus rounding and clips: (s + 2^11) >> 12 at 32767, 32768, -32768, -32769
  bool clip = true;
  CHECK(audio_mix_round(32767ll * 4096 + 2047, &clip) == 32767 && !clip);
  CHECK(audio_mix_round(32767ll * 4096 + 2048, &clip) == 32767 && clip);
  CHECK(audio_mix_round(-32768ll * 4096 - 2048, &clip) == -32768 && !clip);
  CHECK(audio_mix_round(-32768ll * 4096 - 2049, &clip) == -32768 && clip);
  const int64_t most = 4096ll * 32767 * 32768;
  CHECK(most < (1ll << 42));
  CHECK(audio_mix_round(most, &clip) == 32767 && clip && audio_mix_round(-most, &clip) == -32768 && clip);
  CHECK(audio_mix_round(0, &clip) == 0 && !clip && audio_mix_round(-2048, &clip) == 0 && audio_mix_round(-2049, &clip) == -1 && !clip);
  for (int32_t gain : {-32767, -1, 0, 1, 32767})
  {
    for (uint32_t c : {0u, 1u, 65535u})
    {
      const uint32_t e = audio_pack_entry(c, gain);
      CHECK(audio_entry_channel(e) == c && audio_entry_gain(e) == gain);
    }
  }
  return 0;
}

static int check_extremes()
{
  // T = 512, sum |h| = 65535: 511 taps of 128 and one of 127, signs alternating; the input follows the signs
  const uint32_t T = 512, n_blocks = 3;
  std::vector<int16_t> h(T), hist(T - 1, 0), pcm(512 * n_blocks), z(512 * n_blocks);
  for (uint32_t k = 0; k < T; k++)
  {
    h[k] = (int16_t)((k & 1) ? -128 : 128);
  }
  h[T - 1] = -127;
  CHECK(audio_check_taps("who", h.data(), T) == HRFD_OK);
  for (int sign : {1, -1})
  {
    // x[n] = -32768 where the tap that meets it at the last output is positive (sign = -1 makes every product negative)
    for (uint32_t j = 0; j < 512 * n_blocks; j++)
    {
      const uint32_t k = (512 * n_blocks - 1 - j) % 2;     // parity of the tap index at the last output
      const bool tap_positive = k == 0;
      pcm[j] = (int16_t)((tap_positive == (sign < 0)) ? -32768 : 32767);
    }
    std::fill(hist.begin(), hist.end(), (int16_t)0);
    uint8_t prev = 1;
    audio_channel_slow(pcm.data(), nullptr, nullptr, n_blocks, h.data(), T, hist.data(), &prev, z.data());
    // at the last output 256 taps of 128 meet one value and 255 of 128 plus one of 127 the other
    const int64_t acc_pos = 256ll * 128 * 32767 + (255ll * 128 + 127) * 32768, acc_neg = -(256ll * 128 * 32768) - (255ll * 128 + 127) * 32767;
    CHECK(z[512 * n_blocks - 1] == (sign > 0 ? 32767 : -32768));
    CHECK(acc_pos < (1ll << 31) - (1 << 14) && -acc_neg < (1ll << 31) - (1 << 14));
    CHECK(prev == 1 && hist[T - 2] == pcm[512 * n_blocks - 1] && hist[0] == pcm[512 * n_blocks - (T - 1)]);
  }
  // all taps of one sign against input of one sign: the bound itself, 65535 x 32768
  std::vector<int16_t> two = {-32768, -32767};
  std::vector<int16_t> h1(1);
  std::fill(pcm.begin(), pcm.end(), (int16_t)-32768);
  uint8_t prev = 1;
  audio_channel_slow(pcm.data(), nullptr, nullptr, n_blocks, two.data(), 2, h1.data(), &prev, z.data());
  CHECK(z[0] == 32767 && z[1] == 32767 && z[512 * n_blocks - 1] == 32767);       // acc = 2^30, then 65535 x 32768 from z[1] on
  return 0;
}

static int check_cutting_and_n_pcm()
{
  const uint32_t n_blocks = 6;
  for (uint32_t T : {1u, 2u, 5u, 511u, 512u})
  {
    std::vector<int16_t> h(T), pcm(512 * n_blocks), other(512 * n_blocks), z(512 * n_blocks), zc(512 * n_blocks), zo(512 * n_blocks);
    uint32_t s = 12345u + T;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 16; };
    for (auto &v : h)
    {
      v = (int16_t)((int)(next() % 255) - 127);
    }
    for (auto &v : pcm)
    {
      v = (int16_t)next();
    }
    const uint32_t n_pcm[n_blocks] = {512, 100, 0, 0xffffffffu, 1, 511};
    const uint8_t open[n_blocks] = {1, 0, 0, 9, 255, 0};
    other = pcm;
    for (uint32_t b = 0; b < n_blocks; b++)
    {
      for (uint32_t n = pcm_block_limit(n_pcm, b); n < 512; n++)
      {
        other[512 * b + n] ^= 0x5a5a;
      }
    }
    std::vector<int16_t> hist(T), hist_c(T), hist_o(T);    // T - 1 in use
    uint8_t prev = 0, prev_c = 0, prev_o = 0;
    audio_channel_slow(pcm.data(), n_pcm, open, n_blocks, h.data(), T, hist.data(), &prev, z.data());
    audio_channel_slow(other.data(), n_pcm, open, n_blocks, h.data(), T, hist_o.data(), &prev_o, zo.data());
    uint32_t at = 0;
    for (uint32_t nb : {1u, 2u, 3u})
    {
      audio_channel_slow(pcm.data() + 512 * at, n_pcm + at, open + at, nb, h.data(), T, hist_c.data(), &prev_c, zc.data() + 512 * at);
      at += nb;
    }
    CHECK(z == zc && z == zo && hist == hist_c && hist == hist_o && prev == prev_c && prev == 0);
    // the gate's envelope shows in z: block 1 ramps down from block 0, block 2 is silent, block 3 ramps up
    for (uint32_t n = 64; n < 512; n++)
    {
      CHECK(z[512 + n] == 0 && z[1024 + n] == 0);
    }
  }
  return 0;
}

static int check_squelch()
{
  const uint32_t n_blocks = 16;
  uint32_t s = 99u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 16; };
  for (uint32_t L = 128; L <= 8192; L *= 2)
  {
    const uint32_t F = 512 * n_blocks / L;
    std::vector<uint8_t> best(F * 4), present(F * 4);
    for (uint32_t i = 0; i < F * 4; i++)
    {
      const uint8_t pick[3] = {5, 6, 255};
      best[i] = pick[next() % 3];
      present[i] = (uint8_t)(next() % 3);
    }
    for (uint32_t want : {5u, 6u, 127u, 254u, 255u})
    {
      for (uint32_t g = 0; g < 4; g++)
      {
        for (uint32_t b = 0; b < n_blocks; b++)
        {
          bool hit = want == 255;
          for (uint32_t f = 0; f < F; f++)
          {
            // frame f overlaps block b
            const bool overlaps = f * L < (b + 1) * 512 && b * 512 < (f + 1) * L;
            hit = hit || (overlaps && present[f * 4 + g] != 0 && (want == 254 || best[f * 4 + g] == want));
          }
          CHECK(audio_block_open(best.data(), present.data(), L, g, want, b) == hit);
        }
      }
    }
  }
  return 0;
}

int main()
{
  if (check_the_checks() || check_laws() || check_extremes() || check_cutting_and_n_pcm() || check_squelch())
  {
    return 1;
  }
  printf("san_audio ok\n");
  return 0;
}
