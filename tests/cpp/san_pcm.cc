// Sanitizer harness for the PCM contract the tone, audio and resampler banks share (hackrfdiags_amd/csrc/hrfd_pcm.h), CPU
// only: compiled as plain C++ under -fsanitize=address,undefined (tests/test_sanitizers.py).  The block limit at its edges
// and with other bytes behind the row, the FIR rounding at the largest sums the tap check allows, around both saturation
// points and at its ties, every shared check on both sides of its limit with its text, and the overlap check with ranges
// that touch, ranges that share one byte, 1 and 65536 channels and strides larger than a row.
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
#include "../../hackrfdiags_amd/csrc/hrfd_pcm.h"

using namespace hrfd;

#define CHECK(cond)                                               \
  do                                                              \
  {                                                               \
    if (!(cond))                                                  \
    {                                                             \
      printf("san_pcm: line %d: %s (%s)\n", __LINE__, #cond, g_err); \
      return 1;                                                   \
    }                                                             \
  } while (0)

// refused with HRFD_EINVAL, a text that starts with the function's name and holds `word`
static bool refused(int rc, const char *word)
{
  return rc == HRFD_EINVAL && strncmp(g_err, "who: ", 5) == 0 && strstr(g_err, word) != nullptr;
}

static int check_block_limit()
{
  static_assert(kPcmBlock == 512, "a block row is 512 samples");
  CHECK(pcm_block_limit(nullptr, 0) == 512 && pcm_block_limit(nullptr, 0xffffffffu) == 512);
  // a row of exactly seven entries on the heap: a read past it is the sanitizer's to find
  const std::vector<uint32_t> row = {0u, 511u, 512u, 513u, 0xffffffffu, 1u, 0x80000000u};
  const uint32_t want[7] = {0, 511, 512, 512, 512, 1, 512};
  for (uint32_t b = 0; b < 7; b++)
  {
    CHECK(pcm_block_limit(row.data(), b) == want[b]);
  }
  // a channel's row inside [C][n_blocks] with other bytes behind it: block b of channel 1 is entry n_blocks + b
  const uint32_t n_pcm[2][3] = {{7u, 8u, 9u}, {100u, 0u, 600u}};
  CHECK(pcm_block_limit(n_pcm[1], 0) == 100 && pcm_block_limit(n_pcm[1], 1) == 0 && pcm_block_limit(n_pcm[1], 2) == 512);
  CHECK(pcm_block_limit(n_pcm[0], 2) == 9);
  return 0;
}

static int check_rounding()
{
  CHECK(pcm_sat16(32767) == 32767 && pcm_sat16(32768) == 32767 && pcm_sat16(-32768) == -32768 && pcm_sat16(-32769) == -32768);
  CHECK(pcm_sat16(INT64_MAX) == 32767 && pcm_sat16(INT64_MIN) == -32768 && pcm_sat16(0) == 0 && pcm_sat16(-1) == -1);
  // rounding and saturation of the filter: (acc + 2^13) >> 14 at 32767, 32768, -32768, -32769
  CHECK(pcm_fir_round(32767 * 16384 + 8191) == 32767 && pcm_fir_round(32767 * 16384 + 8192) == 32767);
  CHECK(pcm_fir_round(32766 * 16384 + 8192) == 32767 && pcm_fir_round(32766 * 16384 + 8191) == 32766);
  CHECK(pcm_fir_round(-32768 * 16384 - 8192) == -32768 && pcm_fir_round(-32768 * 16384 - 8193) == -32768);
  CHECK(pcm_fir_round(-32767 * 16384 - 8193) == -32768 && pcm_fir_round(-32767 * 16384 - 8192) == -32767);
  // the ties: half an output step rounds towards plus infinity
  CHECK(pcm_fir_round(-1) == 0 && pcm_fir_round(-8192) == 0 && pcm_fir_round(-8193) == -1 && pcm_fir_round(8191) == 0);
  CHECK(pcm_fir_round(8192) == 1 && pcm_fir_round(0) == 0 && pcm_fir_round(16384 + 8192) == 2 && pcm_fir_round(-16384 - 8192) == -1);
  // the largest accumulators the tap check allows: acc + 2^13 stays inside int32 (the sanitizer would say otherwise)
  const int64_t top = 65535ll * 32768;
  CHECK(top < (1ll << 31) - (1 << 14));
  CHECK(top < (1ll << 31) - (1 << 13));
  CHECK(pcm_fir_round((int32_t)top) == 32767 && pcm_fir_round((int32_t)-top) == -32768);
  return 0;
}

static int check_the_checks()
{
  int out = 0;
  for (uint32_t c : {0u, 65537u, 0xffffffffu})
  {
    CHECK(refused(pcm_check_channels("who", c, &out), "channels"));
  }
  CHECK(refused(pcm_check_channels("who", 1, nullptr), "result pointer") && refused(pcm_check_channels("who", 65536, nullptr), "got 65536"));
  CHECK(pcm_check_channels("who", 1, &out) == HRFD_OK && pcm_check_channels("who", 65536, &out) == HRFD_OK);

  CHECK(refused(pcm_check_channel("who", 5, 5), "channel 5 (0..4 or HRFD_ALL_CHANNELS)") && pcm_check_channel("who", 4, 5) == HRFD_OK);
  CHECK(refused(pcm_check_channel("who", 1, 1), "channel 1") && pcm_check_channel("who", 0, 1) == HRFD_OK);
  CHECK(refused(pcm_check_channel("who", 65536, 65536), "channel 65536") && pcm_check_channel("who", 65535, 65536) == HRFD_OK);
  CHECK(refused(pcm_check_channel("who", 0xfffffffeu, 65536), "channel"));
  CHECK(pcm_check_channel("who", HRFD_ALL_CHANNELS, 1) == HRFD_OK && pcm_check_channel("who", HRFD_ALL_CHANNELS, 65536) == HRFD_OK);

  for (uint32_t L : {0u, 1u, 64u, 127u, 129u, 192u, 255u, 8191u, 8193u, 16384u, 0x80000000u, 0xffffffffu})
  {
    CHECK(refused(pcm_check_frame_len("who", L), "frame_len"));
  }
  for (uint32_t L = 128; L <= 8192; L *= 2)
  {
    CHECK(pcm_check_frame_len("who", L) == HRFD_OK);
    for (uint32_t nb = 1; nb <= 1024; nb++)
    {
      const bool whole = (512 * nb) % L == 0;
      CHECK(whole ? pcm_check_frames("who", nb, L) == HRFD_OK : refused(pcm_check_frames("who", nb, L), "frames"));
    }
  }
  CHECK(refused(pcm_check_frames("who", 15, 8192), "15 blocks of 512 samples are no whole number of frames of 8192"));

  // a stride: even, and at least a row
  CHECK(pcm_check_stride("who", "channel_stride_bytes", 1024, 1024) == HRFD_OK && pcm_check_stride("who", "x", 1026, 1024) == HRFD_OK);
  CHECK(refused(pcm_check_stride("who", "channel_stride_bytes", 1022, 1024), "channel_stride_bytes 1022 must be even and >= 1024"));
  CHECK(refused(pcm_check_stride("who", "out_stride_bytes", 1025, 1024), "out_stride_bytes 1025"));
  CHECK(refused(pcm_check_stride("who", "out_stride_bytes", 14, 16, " (2 x out_capacity)"), ">= 16 (2 x out_capacity)"));
  CHECK(pcm_check_stride("who", "x", 0, 0) == HRFD_OK && refused(pcm_check_stride("who", "x", 1, 0), "x 1"));
  CHECK(pcm_check_stride("who", "x", 1ull << 40, (1ull << 40)) == HRFD_OK);
  CHECK(refused(pcm_check_stride("who", "x", (1ull << 40) - 2, 1ull << 40), "1099511627774 must be even and >= 1099511627776"));
  CHECK(refused(pcm_check_stride("who", "x", 0xffffffffffffffffull, 2), "x 18446744073709551615"));

  // alignment: NULL is aligned to everything
  alignas(16) static char buf[32];
  CHECK(pcm_aligned(nullptr, 2) && pcm_aligned(nullptr, 4) && pcm_aligned(nullptr, 8));
  for (int o = 0; o < 17; o++)
  {
    CHECK(pcm_aligned(buf + o, 2) == (o % 2 == 0) && pcm_aligned(buf + o, 4) == (o % 4 == 0) && pcm_aligned(buf + o, 8) == (o % 8 == 0));
  }
  return 0;
}

// addresses only: nothing is read through them
static const void *at(uint64_t a) { return (const void *)(uintptr_t)a; }

static int check_overlap()
{
  const char *why = "the reason";
  const uint64_t in = 1ull << 32;
  struct Shape
  {
    uint32_t C;
    uint64_t in_stride, in_row, out_stride, out_row;
  };
  // dense rows, strides larger than a row on either side, one channel and the most
  const Shape shapes[] = {{1, 1024, 1024, 1024, 1024}, {1, 4096, 1024, 8192, 200},   {4, 1030, 1024, 1024, 1024},
                          {4, 206, 200, 1204, 1200},   {65536, 1024, 1024, 2048, 2048}, {65536, 1030, 1024, 1204, 1200}};
  for (const Shape &s : shapes)
  {
    const uint64_t in_span = (s.C - 1) * s.in_stride + s.in_row, out_span = (s.C - 1) * s.out_stride + s.out_row;
    auto check = [&](uint64_t out) { return pcm_check_no_overlap("who", at(in), s.in_stride, s.in_row, at(out), s.out_stride, s.out_row, s.C, why); };
    // the output ends where the input begins, or begins where it ends: they touch
    CHECK(check(in - out_span) == HRFD_OK && check(in + in_span) == HRFD_OK);
    CHECK(check(in - out_span - 2) == HRFD_OK && check(in + in_span + 2) == HRFD_OK && check(0) == HRFD_OK);
    // one byte in common at either end
    CHECK(refused(check(in - out_span + 1), "out overlaps the input (the reason)"));
    CHECK(refused(check(in + in_span - 1), "overlaps"));
    // in place, and one range inside the other
    CHECK(refused(check(in), "overlaps") && refused(check(in + in_span / 2), "overlaps") && refused(check(in - out_span / 2), "overlaps"));
  }
  // the gaps between strided rows are part of the range: an output that sits in one is refused as well
  CHECK(refused(pcm_check_no_overlap("who", at(in), 4096, 1024, at(in + 2048), 4096, 1024, 2, why), "overlaps"));
  // with one channel the strides do not count
  CHECK(pcm_check_no_overlap("who", at(in), 1ull << 40, 1024, at(in + 1024), 1ull << 40, 1024, 1, why) == HRFD_OK);
  CHECK(pcm_check_no_overlap("who", at(in), 206, 200, at(in + 3 * 206 + 198), 1204, 1200, 1, why) == HRFD_OK);
  CHECK(refused(pcm_check_no_overlap("who", at(in), 206, 200, at(in + 3 * 206 + 198), 1204, 1200, 4, why), "overlaps"));
  return 0;
}

int main()
{
  if (check_block_limit() || check_rounding() || check_the_checks() || check_overlap())
  {
    return 1;
  }
  printf("san_pcm ok\n");
  return 0;
}
