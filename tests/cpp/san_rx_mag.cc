// Sanitizer harness for rx_magnitude_unobservable (hackrfdiags_amd/csrc/hrfd_rx_plan.h), CPU only: compiled as plain C++
// under -fsanitize=address,undefined (tests/test_rx_mag_predicate.py) and run.  The predicate says when a WBFM batch may
// leave the squelch magnitude out; here it is held against the detector itself, by brute force over every block mean the
// kernels can look up (0 .. 127), with the kernels' own arithmetic: dbfs8[m] - 42, then the gain taken off in 32 bits
// (finish_block, hrfd_rx_flow.hip).
//   * a gain at which that subtraction does not wrap for any mean (gain_db <= 2^31 - 42): the predicate is true EXACTLY
//     when every mean passes the threshold;
//   * a gain at which it wraps for some mean: the predicate says "observable" whatever the threshold is (the comparison
//     is rx_plan's, in 64 bits; the wrapped levels are not something to build on);
//   * everywhere: true only where every mean passes (what the kernel relies on); never true when a buffer was given.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/hrfd.h"
static int fail(int code, const char *, ...) { return code; }
#include "../../hackrfdiags_amd/csrc/hrfd_rx_plan.h"

using namespace hrfd;

#define CHECK(cond)                                                                                              \
  do                                                                                                             \
  {                                                                                                              \
    if (!(cond))                                                                                                 \
    {                                                                                                            \
      printf("san_rx_mag: line %d: %s (gain_db %llu, threshold %lld)\n", __LINE__, #cond, (unsigned long long)g, \
             (long long)t);                                                                                      \
      return 1;                                                                                                  \
    }                                                                                                            \
  } while (0)

int main()
{
  (void)fail;
  int32_t dbfs[257];
  rx_build_dbfs(dbfs);
  int8_t dbfs8[128];                                       // as setup_lds keeps the reachable part in LDS
  for (int m = 0; m < 128; m++)
  {
    dbfs8[m] = (int8_t)dbfs[m];
  }
  const uint32_t gains[6] = {0u, 1u, 40u, 0x7fffffffu - 42u, 0x80000000u, 0xffffffffu};
  long n_true = 0, n_false = 0, n_wrap = 0;
  for (const uint32_t g : gains)
  {
    const int64_t cand[7] = {INT32_MIN, -200, -43 - (int64_t)g, -42 - (int64_t)g, -41 - (int64_t)g, 0, INT32_MAX};
    std::vector<int32_t> thresholds;
    for (const int64_t v : cand)
    {
      if (v >= INT32_MIN && v <= INT32_MAX)                 // where representable
      {
        thresholds.push_back((int32_t)v);
      }
    }
    for (const int32_t t : thresholds)
    {
      bool all_pass = true, wraps = false;
      for (int m = 0; m < 128; m++)
      {
        int32_t level = (int32_t)dbfs8[m] - 42;
        const int64_t exact = (int64_t)level - (int64_t)g;
        level = (int32_t)((uint32_t)level - g);
        wraps = wraps || (int64_t)level != exact;
        all_pass = all_pass && level >= t;
      }
      const bool p = rx_magnitude_unobservable(t, g, false);
      CHECK(!rx_magnitude_unobservable(t, g, true));        // a caller who passed a buffer gets its magnitudes
      CHECK(!p || all_pass);
      if (wraps)
      {
        CHECK(!p);
        n_wrap++;
      }
      else
      {
        CHECK(p == all_pass);
      }
      (p ? n_true : n_false)++;
    }
  }
  // the sweep saw both answers, and the wrap
  const uint32_t g = 0;
  const int32_t t = 0;
  CHECK(n_true >= 6 && n_false >= 6 && n_wrap >= 4);
  // the reference's defaults: threshold -200 (IqDataProcessor.cc:121), gain 0 .. 40 dB
  CHECK(rx_magnitude_unobservable(-200, 0, false) && rx_magnitude_unobservable(-200, 40, false));
  CHECK(rx_magnitude_unobservable(-42, 0, false) && !rx_magnitude_unobservable(-41, 0, false));
  printf("san_rx_mag ok: %ld unobservable, %ld observable (%ld at a wrapping gain)\n", n_true, n_false, n_wrap);
  return 0;
}
