/* glibc 2.35 sinf / cosf (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, sincosf.h, s_sincosf_data.c: the ARM
 * optimized-routines algorithm: double-precision range reduction by pi/2 and two degree-7/8 polynomials), restated, and
 * checked against THIS host's libm over EVERY float of the argument range the device code uses (|x| < 120, the
 * reduce_fast branch: Nco::run passes phases in (-pi, pi], signals/fm.cc phases up to 2 pi).
 *
 * Why: Nco::run and the pm / fm generators call cos(float) / sin(float), which C++ overload resolution turns into
 * cosf / sinf.  libhrfd computed those in double and rounded (<= 1 ulp off: the last non-zero tolerance of
 * the repository).  With the algorithm restated the device produces libm's floats bit for bit.
 *
 * The x86-64 build of glibc dispatches between a plain and an -mfma -mavx2 build of the same source (ifunc): the
 * two can differ where a product-sum is contracted.  Both variants are evaluated here (FMA = 0 / 1) and the program
 * says which one -- or both -- equals the host's sinf / cosf everywhere.
 *
 * The restatement itself lives in oracle/sincosf_model.h: the CPU checker evaluates the same text
 * (orc_sincosf_eval / orc_sincosf_digest), tests/test_sincos_model.py makes this program's statement a test and
 * tests/test_gpu_sincos.py holds the DEVICE's restatement to it on every float of the range.
 *
 * build: gcc -O2 -ffp-contract=off -fopenmp -o sincosf_glibc sincosf_glibc.c -lm      run: ./sincosf_glibc
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../oracle/sincosf_model.h"                    /* the restatement: hrfd_sinf / hrfd_cosf (FMA, x) */

static inline uint32_t asuint(float f) { return scm_asuint(f); }

int main(void)
{
  /* every float with |x| < 120: bit patterns 0 .. bits(120.0f) - 1, both signs */
  const uint32_t top = asuint(120.0f);
  unsigned long long bad[2][2] = {{0, 0}, {0, 0}};
#pragma omp parallel for schedule(static) reduction(+ : bad)
  for (uint32_t b = 0; b < top; b++)
  {
    for (int sg = 0; sg < 2; sg++)
    {
      const uint32_t u = b | ((uint32_t)sg << 31);
      float x;
      memcpy(&x, &u, 4);
      const uint32_t ws = asuint(sinf(x)), wc = asuint(cosf(x));
      for (int f = 0; f < 2; f++)
      {
        bad[f][0] += asuint(hrfd_sinf(f, x)) != ws;
        bad[f][1] += asuint(hrfd_cosf(f, x)) != wc;
      }
    }
  }
  printf("floats checked: %llu (|x| < 120, both signs)\n", 2ull * top);
  for (int f = 0; f < 2; f++)
  {
    printf("variant %s: sinf mismatches %llu, cosf mismatches %llu\n", f ? "with fused multiply-adds (the -mfma build)" : "without contraction (plain build)   ",
           bad[f][0], bad[f][1]);
  }
  return (bad[0][0] + bad[0][1] == 0 || bad[1][0] + bad[1][1] == 0) ? 0 : 1;
}
