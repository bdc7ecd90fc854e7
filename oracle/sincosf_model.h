/* oracle/sincosf_model.h -- glibc 2.35 sinf / cosf (sysdeps/ieee754/flt-32/s_sinf.c, s_cosf.c, sincosf.h,
 * s_sincosf_data.c: the ARM optimized-routines algorithm: double-precision range reduction by pi/2 and two degree-7/8
 * polynomials), restated in plain C.  This project's own restatement, shared by the CPU checker (hrfd_oracle.c:
 * orc_sincosf_eval / orc_sincosf_digest) and the proof program tools/proofs/sincosf_glibc.c.
 *
 * The x86-64 build of glibc dispatches between a plain and an -mfma -mavx2 build of the same source (ifunc): the two
 * can differ where a product-sum is contracted.  FMA = 0 / 1 selects the variant; compile with -ffp-contract=off so
 * that variant 0 really rounds twice.
 *
 * Range: the restatement covers the reduce_fast branch, |x| < 120 (Nco::run passes phases in (-pi, pi], signals/fm.cc
 * phases up to 2 pi).  Outside it (|x| >= 120, infinity, NaN) the double sin / cos rounded to float stand in, as on the
 * device (glibc_sincosf_v, hrfd_tx_kernels.hip): no bit equality with libm is claimed there.
 */
#ifndef HRFD_SINCOSF_MODEL_H
#define HRFD_SINCOSF_MODEL_H

#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct
{
  double sign[4];
  double hpi_inv, hpi, c0, c1, c2, c3, c4, s1, s2, s3;
} scm_sincos_t;

static const scm_sincos_t scm_T[2] = {
    {{1.0, -1.0, -1.0, 1.0},
     0x1.45F306DC9C883p+23,
     0x1.921FB54442D18p0,
     0x1p0,
     -0x1.ffffffd0c621cp-2,
     0x1.55553e1068f19p-5,
     -0x1.6c087e89a359dp-10,
     0x1.99343027bf8c3p-16,
     -0x1.555545995a603p-3,
     0x1.1107605230bc4p-7,
     -0x1.994eb3774cf24p-13},
    {{1.0, -1.0, -1.0, 1.0},
     0x1.45F306DC9C883p+23,
     0x1.921FB54442D18p0,
     -0x1p0,
     0x1.ffffffd0c621cp-2,
     -0x1.55553e1068f19p-5,
     0x1.6c087e89a359dp-10,
     -0x1.99343027bf8c3p-16,
     -0x1.555545995a603p-3,
     0x1.1107605230bc4p-7,
     -0x1.994eb3774cf24p-13}};

static inline uint32_t scm_asuint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline uint32_t scm_abstop12(float x) { return (scm_asuint(x) >> 20) & 0x7ff; }

#define SCM_MA(FMA, a, b, c) ((FMA) ? fma((a), (b), (c)) : ((a) * (b) + (c)))

/* sinf_poly: n even -> sine polynomial of x, odd -> cosine polynomial */
static inline float scm_poly(int FMA, double x, double x2, const scm_sincos_t *p, int n)
{
  if ((n & 1) == 0)
  {
    const double x3 = x * x2;
    const double s1 = SCM_MA(FMA, x2, p->s3, p->s2);
    const double x7 = x3 * x2;
    const double s = SCM_MA(FMA, x3, p->s1, x);
    return (float)SCM_MA(FMA, x7, s1, s);
  }
  const double x4 = x2 * x2;
  const double c2 = SCM_MA(FMA, x2, p->c4, p->c3);
  const double c1 = SCM_MA(FMA, x2, p->c1, p->c0);
  const double x6 = x4 * x2;
  const double c = SCM_MA(FMA, x4, p->c2, c1);
  return (float)SCM_MA(FMA, x6, c2, c);
}

static inline double scm_reduce_fast(int FMA, double x, const scm_sincos_t *p, int *np)
{
  const double r = x * p->hpi_inv;
  const int n = ((int32_t)r + 0x800000) >> 24;
  *np = n;
  return FMA ? fma(-(double)n, p->hpi, x) : x - n * p->hpi;
}

static inline float hrfd_sinf(int FMA, float y)
{
  double x = y;
  const scm_sincos_t *p = &scm_T[0];
  if (scm_abstop12(y) >= scm_abstop12(120.0f))             /* outside the restated range */
  {
    return (float)sin(x);
  }
  if (scm_abstop12(y) < scm_abstop12(0x1.921FB6p-1f))      /* |y| < pi/4 */
  {
    const double s = x * x;
    if (scm_abstop12(y) < scm_abstop12(0x1p-12f))
    {
      return y;
    }
    return scm_poly(FMA, x, s, p, 0);
  }
  int n;
  x = scm_reduce_fast(FMA, x, p, &n);
  const double s = p->sign[n & 3];
  if (n & 2)
  {
    p = &scm_T[1];
  }
  return scm_poly(FMA, x * s, x * x, p, n);
}

static inline float hrfd_cosf(int FMA, float y)
{
  double x = y;
  const scm_sincos_t *p = &scm_T[0];
  if (scm_abstop12(y) >= scm_abstop12(120.0f))
  {
    return (float)cos(x);
  }
  if (scm_abstop12(y) < scm_abstop12(0x1.921FB6p-1f))
  {
    const double x2 = x * x;
    if (scm_abstop12(y) < scm_abstop12(0x1p-12f))
    {
      return 1.0f;
    }
    return scm_poly(FMA, x, x2, p, 1);
  }
  int n;
  x = scm_reduce_fast(FMA, x, p, &n);
  const double s = p->sign[n & 3];
  if (n & 2)
  {
    p = &scm_T[1];
  }
  return scm_poly(FMA, x * s, x * x, p, n ^ 1);
}

#endif /* HRFD_SINCOSF_MODEL_H */
