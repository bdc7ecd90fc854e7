// hackrfdiags_amd/csrc/hrfd_cal.hip -- hrfd_cal_*: a bank of capture conditioners (DC offset and IQ imbalance).
//
// W int8 IQ captures in, the same captures through one 2 x 2 Q14 matrix and one Q8 offset per capture out, and / or the
// moments of the raw input a correction is solved from.  Exact integer arithmetic, contract in include/hrfd.h;
// tests/cal_model.py restates it in numpy.  hrfd_cal_solve is host only.
//
// k_cal<APPLY, MEASURE>: one workgroup of 256 threads per (capture, contiguous share of the row's 16-byte groups).  Only
// whole samples are handled anywhere.  A row at an even address peels to the first 16-byte boundary: the head before it
// and the tail behind the last whole group (at most 7 samples each) go sample by sample in the capture's first
// workgroup, the groups between as one 16-byte load per lane, four of them in flight.  A row at an odd address has no
// aligned group of whole samples: its groups start at the row's start and are read byte by byte.  A group is stored
// 16 bytes wide where its output address is 16-byte aligned (for even rows: where the residues of input and output
// agree), else as dwords, halfwords or bytes, whatever the output's residue allows.  Every sample is read and written by
// one lane only, so d_out == d_in is safe.
// Moments: byte dot products (v_dot4c_i32_i8 in the gfx950 disassembly) into per-lane 32-bit partial sums, widened to 64
// bits every kCalWiden steps (a step of 32 samples adds at most 2^19 to a partial), then wave -> workgroup -> one 64-bit atomic add per word
// into the zeroed row (integer sums: the order does not matter), or a plain store when the capture has one workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace hrfd {

constexpr int kCalThreads = 256;
constexpr int kCalDepth = 4;               // 16-byte groups a lane has in flight
constexpr uint32_t kCalWiden = 2048;       // steps between two widenings: 2048 x 2^19 = 2^30 stays inside int32
constexpr int kCalWords = 7;               // n, S_I, S_Q, S_II, S_QQ, S_IQ, clips (word 7 is 0)

// signed byte dot product of two dwords plus acc, without clamping; device code only
#define CAL_DOT4(a, b, acc) __builtin_amdgcn_sdot4((int)(a), (int)(b), (acc), false)
#define CAL_MUL24(a, b) __mul24((a), (b))

// one capture's correction as the kernel reads it (16 bytes)
struct CalRecord
{
  int32_t dc_i, dc_q;                      // Q8
  int16_t m_ii, m_iq, m_qi, m_qq;          // Q14
};
static_assert(sizeof(CalRecord) == 16, "the kernel reads this layout");

struct CalParams
{
  const int8_t *in;                        // [W] rows of n_bytes, in_stride apart, any byte address
  uint64_t in_stride;
  int8_t *out;                             // APPLY: [W] rows, out_stride apart; may be `in`
  uint64_t out_stride;
  const CalRecord *rec;                    // [W]
  unsigned long long *moments;             // MEASURE: [W][8]
  uint32_t n_bytes;
  uint32_t groups_per_wg;                  // a multiple of kCalThreads * kCalDepth
  uint32_t wg_per_capture;
};

// a lane's partial sums between two widenings
struct CalPart
{
  uint32_t n, sII, sQQ, clips;
  int sI, sQ, sIQ;
};

// y = (m (x << 8 - dc) + 2^21) >> 22 per rail, before sat8: |x| <= 65280 and |m| <= 32768 fit the 24-bit multiplier, and
// the row rule keeps the sums inside int32
__device__ __forceinline__ void cal_apply(int I, int Q, const CalRecord &r, int &yi, int &yq)
{
  const int xi = (I << 8) - r.dc_i, xq = (Q << 8) - r.dc_q;
  yi = (CAL_MUL24((int)r.m_ii, xi) + CAL_MUL24((int)r.m_iq, xq) + (1 << 21)) >> 22;
  yq = (CAL_MUL24((int)r.m_qi, xi) + CAL_MUL24((int)r.m_qq, xq) + (1 << 21)) >> 22;
}

__device__ __forceinline__ int cal_sat8(int y) { return min(max(y, -128), 127); }

// 8 samples: x = 4 dwords of (I0, Q0, I1, Q1) bytes
template <bool APPLY, bool MEASURE>
__device__ __forceinline__ void cal_group(const uint32_t x[4], const CalRecord &r, uint32_t y[4], CalPart &p)
{
#pragma unroll
  for (int k = 0; k < 4; k++)
  {
    const uint32_t d = x[k];
    if (MEASURE)
    {
      p.sI = CAL_DOT4(0x00010001u, d, p.sI);
      p.sQ = CAL_DOT4(0x01000100u, d, p.sQ);
      p.sII = (uint32_t)CAL_DOT4(d & 0x00ff00ffu, d, (int)p.sII);
      p.sQQ = (uint32_t)CAL_DOT4(d & 0xff00ff00u, d, (int)p.sQQ);
      p.sIQ = CAL_DOT4((d >> 8) & 0x00ff00ffu, d, p.sIQ);              // (Q0, 0, Q1, 0) . (I0, Q0, I1, Q1)
    }
    if (APPLY)
    {
      uint32_t o = 0;
#pragma unroll
      for (int j = 0; j < 2; j++)
      {
        int yi, yq;
        cal_apply((int)(int8_t)(d >> (16 * j)), (int)(int8_t)(d >> (16 * j + 8)), r, yi, yq);
        const int ci = cal_sat8(yi), cq = cal_sat8(yq);
        if (MEASURE)
        {
          p.clips += (uint32_t)(ci != yi) + (uint32_t)(cq != yq);
        }
        o |= (((uint32_t)ci & 0xffu) | (((uint32_t)cq & 0xffu) << 8)) << (16 * j);
      }
      y[k] = o;
    }
  }
  if (MEASURE)
  {
    p.n += 8;
  }
}

// one sample of a row's head or tail, byte by byte
template <bool APPLY, bool MEASURE>
__device__ __forceinline__ void cal_edge(const int8_t *src, int8_t *dst, const CalRecord &r, CalPart &p)
{
  const int I = src[0], Q = src[1];
  if (MEASURE)
  {
    p.n += 1;
    p.sI += I;
    p.sQ += Q;
    p.sII += (uint32_t)(I * I);
    p.sQQ += (uint32_t)(Q * Q);
    p.sIQ += I * Q;
  }
  if (APPLY)
  {
    int yi, yq;
    cal_apply(I, Q, r, yi, yq);
    const int ci = cal_sat8(yi), cq = cal_sat8(yq);
    if (MEASURE)
    {
      p.clips += (uint32_t)(ci != yi) + (uint32_t)(cq != yq);
    }
    dst[0] = (int8_t)ci;
    dst[1] = (int8_t)cq;
  }
}

__device__ __forceinline__ void cal_load16(const int8_t *src, bool aligned, uint32_t x[4])
{
  if (aligned)
  {
    const uint4 v = *(const uint4 *)src;
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  }
  else
  {
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
      const uint8_t *b = (const uint8_t *)src + 4 * k;
      x[k] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
    }
  }
}

// width: the largest of 16, 4, 2, 1 bytes that dst's address allows (the same for every group of a row)
__device__ __forceinline__ void cal_store16(int8_t *dst, uint32_t width, const uint32_t y[4])
{
  if (width == 16)
  {
    *(uint4 *)dst = make_uint4(y[0], y[1], y[2], y[3]);
  }
  else if (width == 4)
  {
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
      ((uint32_t *)dst)[k] = y[k];
    }
  }
  else if (width == 2)
  {
#pragma unroll
    for (int k = 0; k < 8; k++)
    {
      ((uint16_t *)dst)[k] = (uint16_t)(y[k >> 1] >> (16 * (k & 1)));
    }
  }
  else
  {
#pragma unroll
    for (int k = 0; k < 16; k++)
    {
      ((uint8_t *)dst)[k] = (uint8_t)(y[k >> 2] >> (8 * (k & 3)));
    }
  }
}

// a lane's sums: 64-bit totals and the 32-bit partials since the last widening
struct CalAcc
{
  unsigned long long t[kCalWords];
  CalPart p;
  __device__ __forceinline__ void widen()
  {
    t[0] += p.n;
    t[1] += (unsigned long long)(long long)p.sI;
    t[2] += (unsigned long long)(long long)p.sQ;
    t[3] += p.sII;
    t[4] += p.sQQ;
    t[5] += (unsigned long long)(long long)p.sIQ;
    t[6] += p.clips;
    p = CalPart{0u, 0u, 0u, 0u, 0, 0, 0};
  }
};

// the lane's groups g, g + 256, .. below g1 of a row whose groups start at src (dst: where they go), kCalDepth loads ahead
template <bool APPLY, bool MEASURE, bool ALIGNED>
__device__ __forceinline__ void cal_groups(const int8_t *src, int8_t *dst, uint32_t width, uint32_t g, uint32_t g1,
                                           const CalRecord &r, CalAcc &acc)
{
  uint32_t steps = 0;
  for (; g < g1; g += kCalThreads * kCalDepth)
  {
    uint32_t x[kCalDepth][4];
#pragma unroll
    for (int d = 0; d < kCalDepth; d++)
    {
      const uint32_t gd = g + d * kCalThreads;
      if (gd < g1)
      {
        cal_load16(src + 16 * gd, ALIGNED, x[d]);
      }
    }
#pragma unroll
    for (int d = 0; d < kCalDepth; d++)
    {
      const uint32_t gd = g + d * kCalThreads;
      if (gd < g1)
      {
        uint32_t y[4];
        cal_group<APPLY, MEASURE>(x[d], r, y, acc.p);
        if (APPLY)
        {
          cal_store16(dst + 16 * gd, width, y);
        }
      }
    }
    if (MEASURE && ++steps == kCalWiden)
    {
      acc.widen();
      steps = 0;
    }
  }
}

template <bool APPLY, bool MEASURE>
__global__ __launch_bounds__(kCalThreads) void k_cal(const CalParams P)
{
  __shared__ unsigned long long part[kCalThreads / 64][kCalWords];
  const uint32_t tid = threadIdx.x;
  const uint32_t w = blockIdx.x / P.wg_per_capture, j = blockIdx.x - w * P.wg_per_capture;
  const CalRecord r = P.rec[w];
  const int8_t *in = P.in + (uint64_t)w * P.in_stride;
  int8_t *out = APPLY ? P.out + (uint64_t)w * P.out_stride : nullptr;
  const uint32_t n = P.n_bytes;
  const bool aligned = ((uintptr_t)in & 1u) == 0;
  const uint32_t head = aligned ? min(n, (uint32_t)((0 - (uintptr_t)in) & 15u)) : 0u;      // even: whole samples
  const uint32_t groups = (n - head) >> 4, tail = head + 16 * groups;
  uint32_t width = 0;
  if (APPLY)
  {
    const uintptr_t a = (uintptr_t)(out + head);
    width = (a & 15u) == 0 ? 16 : (a & 3u) == 0 ? 4 : (a & 1u) == 0 ? 2 : 1;
  }
  CalAcc acc = {{0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}, {0u, 0u, 0u, 0u, 0, 0, 0}};
  if (j == 0 && tid < 16)
  {
    // lanes 0..7 the head's samples, lanes 8..15 the tail's: at most 7 each
    const uint32_t o = tid < 8 ? 2 * tid : tail + 2 * (tid - 8), end = tid < 8 ? head : n;
    if (o < end)
    {
      cal_edge<APPLY, MEASURE>(in + o, APPLY ? out + o : nullptr, r, acc.p);
    }
  }
  const uint32_t g0 = j * P.groups_per_wg, g1 = min(groups, g0 + P.groups_per_wg);
  if (aligned)
  {
    cal_groups<APPLY, MEASURE, true>(in + head, APPLY ? out + head : nullptr, width, g0 + tid, g1, r, acc);
  }
  else
  {
    cal_groups<APPLY, MEASURE, false>(in + head, APPLY ? out + head : nullptr, width, g0 + tid, g1, r, acc);
  }
  if (MEASURE)
  {
    acc.widen();
#pragma unroll
    for (int i = 0; i < kCalWords; i++)
    {
      unsigned long long v = acc.t[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1)
      {
        v += __shfl_xor(v, o);
      }
      if ((tid & 63u) == 0)
      {
        part[tid >> 6][i] = v;
      }
    }
    __syncthreads();
    unsigned long long *row = P.moments + 8 * (uint64_t)w;
    if (tid < kCalWords)
    {
      unsigned long long total = 0ull;
      for (int i = 0; i < kCalThreads / 64; i++)
      {
        total += part[i][tid];
      }
      if (P.wg_per_capture == 1)
      {
        row[tid] = total;
      }
      else
      {
        atomicAdd(row + tid, total);
      }
    }
    else if (tid == kCalWords && P.wg_per_capture == 1)
    {
      row[kCalWords] = 0ull;
    }
  }
}

template __global__ void k_cal<true, false>(const CalParams);
template __global__ void k_cal<false, true>(const CalParams);
template __global__ void k_cal<true, true>(const CalParams);

} // namespace hrfd

#ifndef HRFD_CAL_KERNEL_ONLY
// ------------------------------------------------------------------ host side
struct hrfd_cal
{
  hrfd::BankCore core;
  uint32_t n_captures = 0;
  uint32_t target_wgs = 2048;              // workgroups a launch aims for (eight per CU fit beside each other); under core.mu
  hrfd::PinnedBuf<hrfd::CalRecord> h_stage;   // [W]

  // host records, under core.mu
  std::vector<hrfd::CalRecord> rec;
  bool dirty = true;

  hrfd::DevBuf<hrfd::CalRecord> d_rec;
  hrfd::DevBuf<int8_t> d_io;               // host-path staging, corrected in place
  hrfd::DevBuf<unsigned long long> d_moments;
};

static const hrfd::CalRecord kCalIdentity = {0, 0, 16384, 0, 0, 16384};

extern "C" int hrfd_cal_create(uint32_t n_captures, int device, hrfd_cal **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  if (out == nullptr || n_captures == 0 || n_captures > 65536)
  {
    return fail(HRFD_EINVAL, "hrfd_cal_create: need 1..65536 captures and a result pointer (got %u)", n_captures);
  }
  hrfd_cal *c = nullptr;
  BANK_TRY(bank_new("hrfd_cal_create", device, &c));
  c->n_captures = n_captures;
  c->rec.assign(n_captures, kCalIdentity);
  if (!(c->d_rec.alloc(n_captures) && c->h_stage.alloc(n_captures)))
  {
    (void)hipGetLastError();
    bank_free(c);
    return fail(HRFD_ENOMEM, "hrfd_cal_create: device allocation failed");
  }
  *out = c;
  return HRFD_OK;
}

extern "C" int hrfd_cal_destroy(hrfd_cal *c)
{
  if (c != nullptr)
  {
    hrfd::bank_free(c);
  }
  return HRFD_OK;
}

static int64_t cal_abs(int64_t v) { return v < 0 ? -v : v; }

extern "C" int hrfd_cal_set_correction(hrfd_cal *c, uint32_t capture, const int32_t dc[2], const int16_t m[4])
{
  hrfd::CalRecord r = kCalIdentity;
  if (dc != nullptr)
  {
    if (cal_abs(dc[0]) > HRFD_CAL_MAX_DC || cal_abs(dc[1]) > HRFD_CAL_MAX_DC)
    {
      return fail(HRFD_EINVAL, "hrfd_cal_set_correction: dc (%d, %d) outside +-%d (Q8)", dc[0], dc[1], HRFD_CAL_MAX_DC);
    }
    r.dc_i = dc[0];
    r.dc_q = dc[1];
  }
  if (m != nullptr)
  {
    // |m_a| + |m_b| <= 32768 over both rows: with |x| <= 65280 the int32 sums of the apply step then cannot overflow
    for (int row = 0; row < 2; row++)
    {
      const int64_t sum = cal_abs(m[2 * row]) + cal_abs(m[2 * row + 1]);
      if (sum > HRFD_CAL_MAX_ROW)
      {
        return fail(HRFD_EINVAL, "hrfd_cal_set_correction: row %d has |m_a| + |m_b| = %lld > %d (the int32 sum could overflow)",
                    row, (long long)sum, HRFD_CAL_MAX_ROW);
      }
    }
    r.m_ii = m[0];
    r.m_iq = m[1];
    r.m_qi = m[2];
    r.m_qq = m[3];
  }
  if (c == nullptr || (capture >= c->n_captures && capture != HRFD_ALL_CHANNELS))
  {
    return fail(HRFD_EINVAL, "hrfd_cal_set_correction: bad handle or capture");
  }
  std::lock_guard<std::mutex> g(c->core.mu);
  for (uint32_t w = 0; w < c->n_captures; w++)
  {
    if (capture == HRFD_ALL_CHANNELS || w == capture)
    {
      c->rec[w] = r;
    }
  }
  c->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_cal_get_correction(hrfd_cal *c, uint32_t capture, int32_t dc[2], int16_t m[4])
{
  if (c == nullptr || capture >= c->n_captures || dc == nullptr || m == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_cal_get_correction: bad handle, capture or NULL result");
  }
  std::lock_guard<std::mutex> g(c->core.mu);
  const hrfd::CalRecord &r = c->rec[capture];
  dc[0] = r.dc_i;
  dc[1] = r.dc_q;
  m[0] = r.m_ii;
  m[1] = r.m_iq;
  m[2] = r.m_qi;
  m[3] = r.m_qq;
  return HRFD_OK;
}

// test hook: with few workgroups one of them takes many steps, so its sums pass 32 bits before the atomics see them
extern "C" int hrfd_cal_debug_set_workgroups(hrfd_cal *c, int wgs)
{
  HRFD_HOOK_GATE("hrfd_cal_debug_set_workgroups");
  if (c == nullptr || wgs < 1 || wgs > 65536)
  {
    return fail(HRFD_EINVAL, "hrfd_cal_debug_set_workgroups: need a handle and 1..65536 workgroups");
  }
  std::lock_guard<std::mutex> g(c->core.mu);
  c->target_wgs = (uint32_t)wgs;
  return HRFD_OK;
}

static int cal_check_call(hrfd_cal *c, const void *in, uint64_t in_stride, uint32_t n_bytes, const void *out,
                          uint64_t out_stride, const void *moments, const char *who)
{
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text
  if (n_bytes < 2 || (n_bytes & 1u) != 0 || n_bytes > HRFD_CAL_MAX_BYTES)
  {
    return fail(HRFD_EINVAL, "%s: n_bytes must be even, >= 2 and <= 2^30 (got %u)", who, n_bytes);
  }
  if (out == nullptr && moments == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: neither an output nor moments asked for", who);
  }
  if (in_stride < n_bytes || (out != nullptr && out_stride < n_bytes))
  {
    return fail(HRFD_EINVAL, "%s: strides %llu / %llu are shorter than a row of %u bytes", who,
                (unsigned long long)in_stride, (unsigned long long)out_stride, n_bytes);
  }
  if (((uintptr_t)moments & 7u) != 0)
  {
    return fail(HRFD_EINVAL, "%s: moments must be 8-byte aligned", who);
  }
  if (out != nullptr && out == in && out_stride != in_stride)
  {
    return fail(HRFD_EINVAL, "%s: in place needs equal strides (got %llu in, %llu out)", who, (unsigned long long)in_stride,
                (unsigned long long)out_stride);
  }
  if (c == nullptr || in == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  if (out != nullptr && out != in)
  {
    const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (uintptr_t)(in_stride * (c->n_captures - 1)) + n_bytes;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(out_stride * (c->n_captures - 1)) + n_bytes;
    if (i0 < o1 && o0 < i1)
    {
      return fail(HRFD_EINVAL, "%s: the output overlaps the input without being in place", who);
    }
  }
  return HRFD_OK;
}

// one call on `st`: the record upload, then k_cal over every capture
static int cal_launch(hrfd_cal *c, const int8_t *d_in, uint64_t in_stride, uint32_t n_bytes, int8_t *d_out, uint64_t out_stride,
                      unsigned long long *d_moments, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(c->core.order_behind_last(st));
  uint32_t target_wgs;
  {
    std::lock_guard<std::mutex> g(c->core.mu);
    target_wgs = c->target_wgs;
    if (c->dirty)
    {
      BANK_TRY(c->core.staging_wait());
      memcpy(c->h_stage, c->rec.data(), sizeof(CalRecord) * c->n_captures);
      HIP_TRY(hipMemcpyAsync(c->d_rec, c->h_stage, sizeof(CalRecord) * c->n_captures, hipMemcpyHostToDevice, st));
      c->dirty = false;
      BANK_TRY(c->core.staging_sent(st));
    }
  }
  CalParams P;
  P.in = d_in;
  P.in_stride = in_stride;
  P.out = d_out;
  P.out_stride = out_stride;
  P.rec = c->d_rec;
  P.moments = d_moments;
  P.n_bytes = n_bytes;
  // rounds of 256 groups: a workgroup takes at least kCalDepth of them (16 KiB), more when the launch would pass target_wgs
  const uint32_t groups = n_bytes / 16u, rounds = (groups + kCalThreads - 1) / kCalThreads;
  const uint32_t want = std::max(1u, target_wgs / c->n_captures);
  uint32_t per = std::max((uint32_t)kCalDepth, (rounds + want - 1) / want);
  per = (per + kCalDepth - 1) / kCalDepth * kCalDepth;
  P.groups_per_wg = per * kCalThreads;
  P.wg_per_capture = std::max(1u, (groups + P.groups_per_wg - 1) / P.groups_per_wg);
  if (d_moments != nullptr && P.wg_per_capture > 1)
  {
    HIP_TRY(hipMemsetAsync(d_moments, 0, sizeof(unsigned long long) * 8 * (size_t)c->n_captures, st));
  }
  const dim3 grid(c->n_captures * P.wg_per_capture), block(kCalThreads);
  if (d_out != nullptr && d_moments != nullptr)
  {
    hipLaunchKernelGGL((k_cal<true, true>), grid, block, 0, st, P);
  }
  else if (d_out != nullptr)
  {
    hipLaunchKernelGGL((k_cal<true, false>), grid, block, 0, st, P);
  }
  else
  {
    hipLaunchKernelGGL((k_cal<false, true>), grid, block, 0, st, P);
  }
  BANK_TRY(bank_launch_ok("k_cal"));
  c->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_cal_process_device(hrfd_cal *c, const int8_t *d_in, uint64_t in_stride, uint32_t n_bytes, int8_t *d_out,
                                       uint64_t out_stride, int64_t *d_moments, void *stream)
{
  BANK_TRY(cal_check_call(c, d_in, in_stride, n_bytes, d_out, out_stride, d_moments, "hrfd_cal_process_device"));
  HIP_TRY(hipSetDevice(c->core.device));
  return cal_launch(c, d_in, in_stride, n_bytes, d_out, out_stride, (unsigned long long *)d_moments, c->core.stream_or_own(stream));
}

extern "C" int hrfd_cal_process(hrfd_cal *c, const int8_t *captures, uint32_t n_bytes, int8_t *out, int64_t *moments)
{
  BANK_TRY(cal_check_call(c, captures, n_bytes, n_bytes, out, n_bytes, moments, "hrfd_cal_process"));
  hrfd::BankHostCall call(c->core);
  const size_t total = (size_t)n_bytes * c->n_captures, m_total = sizeof(int64_t) * 8 * (size_t)c->n_captures;
  int8_t *d_io = call.up(c->d_io, captures, total);        // corrected in place when out is asked for
  unsigned long long *d_moments = call.room(c->d_moments, moments, m_total);
  BANK_TRY(call.rc);
  BANK_TRY(cal_launch(c, d_io, n_bytes, n_bytes, out != nullptr ? d_io : nullptr, n_bytes, d_moments, call.st));
  call.down(out, d_io, total);
  call.down(moments, d_moments, m_total);
  return call.finish();
}

// The operation order is the header's; the library is built without contraction, so no line fuses a multiply and an add.
extern "C" int hrfd_cal_solve(const int64_t moments[8], int32_t dc[2], int16_t m[4])
{
  if (moments == nullptr || dc == nullptr || m == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_cal_solve: NULL argument");
  }
  dc[0] = dc[1] = 0;
  m[0] = m[3] = 16384;
  m[1] = m[2] = 0;
  if (moments[0] <= 0)
  {
    return HRFD_CAL_DEGENERATE;
  }
  const double n = (double)moments[0];
  const double mi = (double)moments[1] / n, mq = (double)moments[2] / n;
  const double vii = (double)moments[3] / n - mi * mi;
  const double vqq = (double)moments[4] / n - mq * mq;
  const double viq = (double)moments[5] / n - mi * mq;
  const double D = vii * vqq - viq * viq;
  const double mean[2] = {mi, mq};
  for (int k = 0; k < 2; k++)
  {
    double v = floor(mean[k] * 256.0 + 0.5);
    v = v > (double)HRFD_CAL_MAX_DC ? (double)HRFD_CAL_MAX_DC : v < -(double)HRFD_CAL_MAX_DC ? -(double)HRFD_CAL_MAX_DC : v;
    dc[k] = (int32_t)v;
  }
  if (!(vii > 0.0) || !(D > 0.0))
  {
    return HRFD_CAL_DEGENERATE;
  }
  const double r = sqrt(D);
  const double qi = floor(((-viq) / r) * 16384.0 + 0.5), qq = floor((vii / r) * 16384.0 + 0.5);
  if (!(fabs(qi) + fabs(qq) <= (double)HRFD_CAL_MAX_ROW) || qi > 32767.0 || qq > 32767.0)
  {
    return HRFD_CAL_DEGENERATE;
  }
  m[2] = (int16_t)qi;
  m[3] = (int16_t)qq;
  return HRFD_OK;
}
#endif /* HRFD_CAL_KERNEL_ONLY */
