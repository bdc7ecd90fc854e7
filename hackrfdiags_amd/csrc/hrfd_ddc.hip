// hackrfdiags_amd/csrc/hrfd_ddc.hip -- hrfd_ddc_*: a bank of digital down-converters in front of hrfd_rx.
//
// W wideband int8 IQ captures at R x 2.048 MS/s in, C channel streams of int8 IQ at 2.048 MS/s out: per channel a
// mixer (e^{-j theta(n)} from a 4096-entry Q15 cosine table), stage A (FIR, decimation by R) and stage B (channel FIR
// at 2.048 MS/s), then a gain shift to int8.  Exact integer arithmetic, contract in include/hrfd.h; tests/ddc_model.py
// restates it in numpy.
//
// One workgroup (256 threads) per (channel, tile of kDdcTile outputs); no recurrence in time, so tiles are independent:
//   1. the tile's input samples plus the halo of both filters are mixed into LDS as two int16 rails (I, Q); the phase
//      of every sample is theta_call + j * step (no phase carried between lanes or calls)
//   2. stage A writes a16 for the tile plus stage B's look-back into two more int16 rails
//   3. stage B, 4 consecutive outputs per lane, int8 IQ straight to the output row (8 bytes per lane)
// Both FIRs run on v_dot2_i32_i16 over packed rail dwords with a register-blocked window; a window that starts on an
// odd sample uses the taps shifted by one (a leading zero), so every read is a whole dword.  Taps sit in LDS as
// (even, odd) pairs and are read as broadcasts.  W extra workgroups per launch copy the last H input samples of every
// capture into the other history buffer (ping-pong: the tiles of the same launch read the current one).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "hrfd_ddc_tables.h"

namespace hrfd {

constexpr int kDdcTile = 1024;             // outputs per workgroup
constexpr int kDdcThreads = 256;
constexpr int kDdcMaxTA = 64;
constexpr int kDdcMaxTB = 256;
constexpr int kDdcJA = kDdcMaxTA / 2 + 1;  // packed tap dwords per variant
constexpr int kDdcJB = kDdcMaxTB / 2 + 1;
constexpr int kDdcPad = 40;                // dwords behind every rail: windows of the last lane's outputs overrun by < 32

// y rail: (kDdcTile + 256) R + 64 + 2 samples at most (tile, stage B look-back in a16 samples, stage A look-back).
// For R >= 4 a rail is stored in kH2 = R / 2 polyphase parts: dword D at (D mod kH2) * kYS + D / kH2.  Stage A's lanes
// take neighbouring outputs, whose windows start kH2 dwords apart: in this layout they read neighbouring dwords of one
// part (no bank conflict), where the linear layout put a 32-lane group on 64 / R banks.  kYS is 32 / kH2 modulo 32, so
// that the mixer's stores (consecutive dwords to the kH2 parts in turn) spread over the banks as well.
template <int R>
struct DdcLds
{
  static constexpr int kH2 = R >= 2 ? R / 2 : 1;
  static constexpr int kYLin = ((kDdcTile + kDdcMaxTB) * R + kDdcMaxTA + 2) / 2 + kDdcPad;
  static constexpr int kYBase = (kYLin + kH2 - 1) / kH2;
  static constexpr int kYS = kH2 == 1 ? kYLin : kYBase + ((32 / kH2 - kYBase % 32) % 32 + 32) % 32;
  static constexpr int kYDw = kH2 * kYS;
  static constexpr int kADw = (kDdcTile + kDdcMaxTB) / 2 + kDdcPad;
  static_assert(kH2 == 1 || kYS % 32 == 32 / kH2, "part stride");
  static __device__ __forceinline__ int dw(int D) { return kH2 == 1 ? D : (D % kH2) * kYS + D / kH2; }
};

struct DdcChanDev
{
  uint32_t capture;
  uint32_t step;
  uint32_t theta_ref;
  uint32_t g;
  uint64_t n_ref;
};

struct DdcParams
{
  const int8_t *cap;           // [W] rows of R * 2M bytes, cap_stride apart
  uint64_t cap_stride;
  const int8_t *hist_in;       // [W][H] IQ samples: the H samples in front of this call
  int8_t *hist_out;            // [W][H]: the H samples in front of the next call
  int8_t *out;                 // [C] rows of 2M bytes, out_stride apart
  uint64_t out_stride;
  const DdcChanDev *chan;
  const uint2 *taps;           // [kDdcJA] stage A (even, odd) pairs, then [kDdcJB] stage B
  const uint32_t *cs;          // [4096] (COS[k], COS[(k - 1024) & 4095]) as packed int16
  uint64_t n0;                 // absolute index of the call's first input sample
  uint32_t M;                  // outputs per channel
  uint32_t n_tiles;
  uint32_t n_channels;
  uint32_t n_captures;
  uint32_t H;
  int TA, TB;                  // 0 = bypass
  int JA, JB;                  // packed tap dwords in use
};

__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// P outputs of a FIR over two int16 rails: output i starts its window at sample 2 b + PAR0 + i STEP and sums
// J packed tap dwords: even start -> taps.x (pairs of the time-reversed taps), odd start -> taps.y (the same, one
// leading zero) from the dword below.
template <int P, int STEP, int PAR0>
__device__ __forceinline__ void ddc_fir(const uint32_t *xI, const uint32_t *xQ, int b, int J, const uint2 *taps,
                                        int (&accI)[P], int (&accQ)[P])
{
  constexpr int K = 8;
  constexpr int DL = (PAR0 + (P - 1) * STEP) >> 1;
  int jb = 0;
  for (; jb + K <= J; jb += K)
  {
    uint32_t wI[DL + K], wQ[DL + K];
#pragma unroll
    for (int d = 0; d < DL + K; d++)
    {
      wI[d] = xI[b + jb + d];
      wQ[d] = xQ[b + jb + d];
    }
#pragma unroll
    for (int k = 0; k < K; k++)
    {
      const uint2 t = taps[jb + k];
#pragma unroll
      for (int i = 0; i < P; i++)
      {
        const int d = ((PAR0 + i * STEP) >> 1) + k;
        const uint32_t tt = ((PAR0 + i * STEP) & 1) ? t.y : t.x;
        accI[i] = dot2(wI[d], tt, accI[i]);
        accQ[i] = dot2(wQ[d], tt, accQ[i]);
      }
    }
  }
  for (; jb < J; jb++)
  {
    const uint2 t = taps[jb];
#pragma unroll
    for (int i = 0; i < P; i++)
    {
      const int d = ((PAR0 + i * STEP) >> 1);
      const uint32_t tt = ((PAR0 + i * STEP) & 1) ? t.y : t.x;
      accI[i] = dot2(xI[b + jb + d], tt, accI[i]);
      accQ[i] = dot2(xQ[b + jb + d], tt, accQ[i]);
    }
  }
}

template <int P, int STEP>
__device__ __forceinline__ void ddc_fir_any(int par, const uint32_t *xI, const uint32_t *xQ, int b, int J,
                                            const uint2 *taps, int (&accI)[P], int (&accQ)[P])
{
  if (par)
  {
    ddc_fir<P, STEP, 1>(xI, xQ, b, J, taps, accI, accQ);
  }
  else
  {
    ddc_fir<P, STEP, 0>(xI, xQ, b, J, taps, accI, accQ);
  }
}

__device__ __forceinline__ uint32_t ddc_load_sample(const DdcParams &P, uint32_t w, int64_t j, int64_t n_in)
{
  if (j >= 0 && j < n_in)
  {
    return *(const uint16_t *)(P.cap + (uint64_t)w * P.cap_stride + 2 * (uint64_t)j);
  }
  if (j < 0 && j >= -(int64_t)P.H)
  {
    return *(const uint16_t *)(P.hist_in + ((uint64_t)w * P.H + (uint64_t)(P.H + j)) * 2);
  }
  return 0u;                               // never under a non-zero tap (the halo is rounded up to whole dwords)
}

template <int R>
__global__ __launch_bounds__(kDdcThreads) void k_ddc(const DdcParams P)
{
  using L = DdcLds<R>;
  __shared__ uint32_t cs[4096];
  __shared__ uint32_t yI[L::kYDw], yQ[L::kYDw];
  __shared__ uint32_t aI[L::kADw], aQ[L::kADw];
  __shared__ uint2 taps[kDdcJA + kDdcJB];
  const int tid = threadIdx.x;
  const int64_t n_in = (int64_t)R * P.M;                  // input samples of the call per capture
  const uint32_t n_units = P.n_tiles * P.n_channels;
  if (blockIdx.x >= n_units)
  {
    // history: the last H samples of (history, this call's input) of capture w, for the next call
    const uint32_t w = blockIdx.x - n_units;
    for (uint32_t i = tid; i < P.H; i += kDdcThreads)
    {
      const uint32_t v = ddc_load_sample(P, w, n_in - (int64_t)P.H + i, n_in);
      *(uint16_t *)(P.hist_out + ((uint64_t)w * P.H + i) * 2) = (uint16_t)v;
    }
    return;
  }
  const uint32_t c = blockIdx.x / P.n_tiles;
  const int m_t = (int)(blockIdx.x - c * P.n_tiles) * kDdcTile;
  const int cnt = min(kDdcTile, (int)P.M - m_t);
  const DdcChanDev ch = P.chan[c];

  for (int i = tid; i < 4096; i += kDdcThreads)
  {
    cs[i] = P.cs[i];
  }
  for (int i = tid; i < kDdcJA + kDdcJB; i += kDdcThreads)
  {
    taps[i] = P.taps[i];
  }
  const int TA = P.TA, TB = P.TB;
  const int LB = (TB > 0) ? ((TB - 1 + 1) & ~1) : 0;       // stage B look-back in a16 samples, rounded up to even
  const int jy0 = ((m_t - LB) * R + R - max(TA, 1)) & ~1;  // first y sample in LDS (local index), even
  const int ny = (m_t + cnt) * R - jy0;
  const int nyd = (ny + 1) >> 1;
  __syncthreads();

  // 1. mix: pair p holds samples jy0 + 2p, jy0 + 2p + 1
  {
    const uint32_t theta_call = ch.theta_ref + (uint32_t)(P.n0 - ch.n_ref) * ch.step;
    uint32_t th = theta_call + (uint32_t)(jy0 + 2 * tid) * ch.step;
    const uint32_t dth = (uint32_t)(2 * kDdcThreads) * ch.step;
    for (int p = tid; p < nyd; p += kDdcThreads, th += dth)
    {
      const int64_t j = (int64_t)jy0 + 2 * p;
      uint32_t ri = 0, rq = 0;
#pragma unroll
      for (int e = 0; e < 2; e++)
      {
        const uint32_t v = ddc_load_sample(P, ch.capture, j + e, n_in);
        const int si = (int8_t)(v & 0xffu), sq = (int8_t)(v >> 8);
        const uint32_t t = th + (e ? ch.step : 0u);
        const uint32_t k = ((t + (1u << 19)) >> 20) & 4095u;
        const uint32_t csk = cs[k];
        const uint32_t iq = ((uint32_t)si & 0xffffu) | ((uint32_t)sq << 16);
        const uint32_t qn = ((uint32_t)sq & 0xffffu) | ((uint32_t)(-si) << 16);
        const int vi = dot2(iq, csk, 128) >> 8;          // I c + Q s
        const int vq = dot2(qn, csk, 128) >> 8;          // Q c - I s
        ri |= ((uint32_t)vi & 0xffffu) << (16 * e);
        rq |= ((uint32_t)vq & 0xffffu) << (16 * e);
      }
      yI[L::dw(p)] = ri;
      yQ[L::dw(p)] = rq;
    }
  }
  __syncthreads();

  // 2. stage A: a16[u] for u = 0 .. LB + cnt - 1 (a16 index m_t - LB + u); its window ends at y sample e_u
  const int na = LB + cnt;
  const int e0 = (m_t - LB) * R + R - 1 - jy0;
  if constexpr (R == 1)
  {
  // full rate: four consecutive outputs per lane on a register-blocked window (lanes two dwords apart)
  {
    const int16_t *y16I = (const int16_t *)yI, *y16Q = (const int16_t *)yQ;
    for (int q = tid; 4 * q < na; q += kDdcThreads)
    {
      const int u0 = 4 * q;
      int accI[4], accQ[4];
      if (TA == 0)
      {
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
          accI[i] = y16I[e0 + (u0 + i) * R];
          accQ[i] = y16Q[e0 + (u0 + i) * R];
        }
      }
      else
      {
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
          accI[i] = 1 << 14;
          accQ[i] = 1 << 14;
        }
        const int s0 = e0 + u0 * R - (TA - 1);               // >= 0
        ddc_fir_any<4, R>(s0 & 1, yI, yQ, s0 >> 1, P.JA, taps, accI, accQ);
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
          accI[i] = sat16(accI[i] >> 15);
          accQ[i] = sat16(accQ[i] >> 15);
        }
      }
      // four samples = two dwords per rail (the rails have room behind na)
      aI[2 * q] = ((uint32_t)accI[0] & 0xffffu) | ((uint32_t)accI[1] << 16);
      aI[2 * q + 1] = ((uint32_t)accI[2] & 0xffffu) | ((uint32_t)accI[3] << 16);
      aQ[2 * q] = ((uint32_t)accQ[0] & 0xffffu) | ((uint32_t)accQ[1] << 16);
      aQ[2 * q + 1] = ((uint32_t)accQ[2] & 0xffffu) | ((uint32_t)accQ[3] << 16);
    }
  }
  }
  else
  {
    // one output per lane and pass, neighbouring lanes on neighbouring outputs: for every tap pair j the lanes read
    // consecutive dwords of one polyphase part.  s_u = s0 + u R has the parity of s0 for every u.
    constexpr int H2 = L::kH2;
    const int s0 = e0 - (TA - 1);                            // >= 0
    const int b0 = s0 >> 1;
    const uint32_t *tsel = (const uint32_t *)taps + (s0 & 1);  // .x (even start) or .y (odd start)
    int16_t *a16I = (int16_t *)aI, *a16Q = (int16_t *)aQ;
    for (int u = tid; u < na; u += kDdcThreads)
    {
      int accI, accQ;
      if (TA == 0)
      {
        const int e = e0 + u * R;
        const int sh = 16 * (e & 1);
        accI = (int)(int16_t)(yI[L::dw(e >> 1)] >> sh);
        accQ = (int)(int16_t)(yQ[L::dw(e >> 1)] >> sh);
      }
      else
      {
        accI = 1 << 14;
        accQ = 1 << 14;
#pragma unroll
        for (int ph = 0; ph < H2; ph++)
        {
          const int j0 = ((ph - b0) % H2 + H2) % H2;         // first tap pair whose dword lies in part ph
          const uint32_t *rI = yI + ph * L::kYS + (b0 + j0) / H2 + u;
          const uint32_t *rQ = yQ + ph * L::kYS + (b0 + j0) / H2 + u;
          const int nt = (P.JA - j0 + H2 - 1) / H2;
#pragma unroll 4
          for (int t = 0; t < nt; t++)
          {
            const uint32_t tt = tsel[2 * (j0 + H2 * t)];
            accI = dot2(rI[t], tt, accI);
            accQ = dot2(rQ[t], tt, accQ);
          }
        }
        accI = sat16(accI >> 15);
        accQ = sat16(accQ >> 15);
      }
      a16I[u] = (int16_t)accI;
      a16Q[u] = (int16_t)accQ;
    }
  }
  __syncthreads();

  // 3. stage B: outputs m_t + 4 tid + i; a16 index u = LB + 4 tid + i, window from u - TB + 1
  const int o0 = 4 * tid;
  if (o0 >= cnt)
  {
    return;
  }
  int bI[4], bQ[4];
  if (TB == 0)
  {
    const int16_t *a16I = (const int16_t *)aI, *a16Q = (const int16_t *)aQ;
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
      bI[i] = a16I[o0 + i];
      bQ[i] = a16Q[o0 + i];
    }
  }
  else
  {
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
      bI[i] = 1 << 14;
      bQ[i] = 1 << 14;
    }
    const int s0 = LB + o0 - (TB - 1);                      // >= 0
    ddc_fir_any<4, 1>(s0 & 1, aI, aQ, s0 >> 1, P.JB, taps + kDdcJA, bI, bQ);
#pragma unroll
    for (int i = 0; i < 4; i++)
    {
      bI[i] = sat16(bI[i] >> 15);
      bQ[i] = sat16(bQ[i] >> 15);
    }
  }
  const int g = (int)ch.g;
  const int r = (g < 7) ? (1 << (6 - g)) : 0;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < 4; i++)
  {
    const uint32_t vi = (uint32_t)min(max((bI[i] + r) >> (7 - g), -128), 127) & 0xffu;
    const uint32_t vq = (uint32_t)min(max((bQ[i] + r) >> (7 - g), -128), 127) & 0xffu;
    const uint32_t pair = vi | (vq << 8);
    if (i < 2)
    {
      lo |= pair << (16 * i);
    }
    else
    {
      hi |= pair << (16 * (i - 2));
    }
  }
  int8_t *dst = P.out + (uint64_t)c * P.out_stride + 2 * (uint64_t)(m_t + o0);
  if (o0 + 4 <= cnt && ((uintptr_t)dst & 7u) == 0)
  {
    *(uint2 *)dst = make_uint2(lo, hi);
  }
  else
  {
    const uint64_t v = (uint64_t)lo | ((uint64_t)hi << 32);
    const int nb = 2 * min(4, cnt - o0);
    for (int k = 0; k < nb; k++)
    {
      dst[k] = (int8_t)(v >> (8 * k));
    }
  }
}

template __global__ void k_ddc<1>(const DdcParams);
template __global__ void k_ddc<2>(const DdcParams);
template __global__ void k_ddc<4>(const DdcParams);
template __global__ void k_ddc<8>(const DdcParams);

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_ddc
{
  int device = 0;
  uint32_t n_captures = 0, n_channels = 0, R = 1, H = 0;
  hipStream_t stream = nullptr;
  hipStream_t last_stream = nullptr;       // the stream of the last launch: the next one is ordered behind it
  hipEvent_t ev_last = nullptr;            // recorded on last_stream when the next launch runs on another stream
  hipEvent_t ev_upload = nullptr;          // the last upload from the pinned staging buffer has been read
  hrfd::DdcChanDev *h_stage_chan = nullptr;   // pinned staging of the records and packed taps (uploads in stream order)
  uint2 *h_stage_taps = nullptr;

  std::mutex mu;                           // guards the host records (setters may come from another thread)
  std::vector<hrfd::DdcChanDev> h_chan;
  std::vector<int16_t> tapsA, tapsB;
  bool dirty = true;
  uint64_t N = 0;                          // absolute input-sample counter
  bool clear_history = true;

  hrfd::DdcChanDev *d_chan = nullptr;
  uint2 *d_taps = nullptr;
  uint32_t *d_cs = nullptr;
  int8_t *d_hist[2] = {nullptr, nullptr};
  int cur = 0;
  int8_t *d_in = nullptr, *d_out = nullptr, *d_rx = nullptr;   // host-path staging and hrfd_ddc_receive's buffer
  size_t cap_in = 0, cap_out = 0, cap_rx = 0;
  uint8_t *d_scratch_mag = nullptr;
  size_t cap_scratch = 0;
};

static int ddc_taps_ok(const char *who, const int16_t *taps, uint32_t n, uint32_t max_n)
{
  if (n > max_n || (n > 0 && taps == nullptr))
  {
    return fail(HRFD_EINVAL, "%s: %u taps (at most %u, and a tap array when n > 0)", who, n, max_n);
  }
  int64_t sum = 0;
  for (uint32_t k = 0; k < n; k++)
  {
    sum += taps[k] < 0 ? -(int64_t)taps[k] : (int64_t)taps[k];
  }
  if (sum > 65535)
  {
    return fail(HRFD_EINVAL, "%s: sum |h| = %lld exceeds 65535 (the int32 accumulator could overflow)", who, (long long)sum);
  }
  return HRFD_OK;
}

// (even, odd) packed pairs of the time-reversed taps: x = (g[2j], g[2j+1]), y = (g'[2j], g'[2j+1]) with g' = 0, g
static void ddc_pack_taps(const std::vector<int16_t> &h, uint2 *out, int J)
{
  const int T = (int)h.size();
  auto g = [&](int i) -> uint32_t { return (i >= 0 && i < T) ? (uint16_t)h[T - 1 - i] : 0u; };
  for (int j = 0; j < J; j++)
  {
    out[j].x = g(2 * j) | (g(2 * j + 1) << 16);
    out[j].y = g(2 * j - 1) | (g(2 * j) << 16);
  }
}

static int ddc_packed_len(int T) { return T > 0 ? T / 2 + 1 : 0; }

extern "C" int hrfd_ddc_create(uint32_t n_captures, uint32_t n_channels, uint32_t decimation, int device, hrfd_ddc **out)
{
  if (out == nullptr || n_captures == 0 || n_channels == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_create: need n_captures > 0, n_channels > 0 and a result pointer");
  }
  *out = nullptr;
  if (decimation != 1 && decimation != 2 && decimation != 4 && decimation != 8)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_create: decimation must be 1, 2, 4 or 8 (got %u)", decimation);
  }
  if (hrfd_device_count() <= 0)
  {
    return fail(HRFD_ENODEV, "hrfd_ddc_create: no HIP device visible (this library has no CPU path)");
  }
  if (device < 0)
  {
    HIP_TRY(hipGetDevice(&device));
  }
  HIP_TRY(hipSetDevice(device));
  hrfd_ddc *d = new hrfd_ddc;
  d->device = device;
  d->n_captures = n_captures;
  d->n_channels = n_channels;
  d->R = decimation;
  d->H = 255u * decimation + 63u;
  d->h_chan.assign(n_channels, hrfd::DdcChanDev{0u, 0u, 0u, 0u, 0ull});
  switch (decimation)
  {
  case 2: d->tapsA.assign(hrfd::Q_DDC_A2, hrfd::Q_DDC_A2 + hrfd::N_DDC_A2); break;
  case 4: d->tapsA.assign(hrfd::Q_DDC_A4, hrfd::Q_DDC_A4 + hrfd::N_DDC_A4); break;
  case 8: d->tapsA.assign(hrfd::Q_DDC_A8, hrfd::Q_DDC_A8 + hrfd::N_DDC_A8); break;
  default: break;                          // R = 1: stage A in bypass
  }
  d->tapsB.assign(hrfd::Q_DDC_B, hrfd::Q_DDC_B + hrfd::N_DDC_B);
  std::vector<uint32_t> cs(4096);
  for (int k = 0; k < 4096; k++)
  {
    cs[k] = (uint16_t)hrfd::Q_DDC_COS[k] | ((uint32_t)(uint16_t)hrfd::Q_DDC_COS[(k - 1024) & 4095] << 16);
  }
  const size_t hist_bytes = (size_t)n_captures * d->H * 2;
  bool ok = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipMalloc((void **)&d->d_chan, sizeof(hrfd::DdcChanDev) * n_channels) == hipSuccess;
  ok = ok && hipMalloc((void **)&d->d_taps, sizeof(uint2) * (hrfd::kDdcJA + hrfd::kDdcJB)) == hipSuccess;
  ok = ok && hipMalloc((void **)&d->d_cs, sizeof(uint32_t) * 4096) == hipSuccess;
  ok = ok && hipMalloc((void **)&d->d_hist[0], hist_bytes) == hipSuccess;
  ok = ok && hipMalloc((void **)&d->d_hist[1], hist_bytes) == hipSuccess;
  ok = ok && hipMemcpy(d->d_cs, cs.data(), sizeof(uint32_t) * 4096, hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&d->ev_last, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&d->ev_upload, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipHostMalloc((void **)&d->h_stage_chan, sizeof(hrfd::DdcChanDev) * n_channels, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void **)&d->h_stage_taps, sizeof(uint2) * (hrfd::kDdcJA + hrfd::kDdcJB), hipHostMallocDefault) == hipSuccess;
  if (!ok)
  {
    (void)hipGetLastError();
    hrfd_ddc_destroy(d);
    return fail(HRFD_ENOMEM, "hrfd_ddc_create: device allocation failed");
  }
  d->last_stream = d->stream;
  *out = d;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_destroy(hrfd_ddc *d)
{
  if (d == nullptr)
  {
    return HRFD_OK;
  }
  (void)hipSetDevice(d->device);
  if (d->stream)
  {
    (void)hipStreamSynchronize(d->stream);
  }
  if (d->last_stream && d->last_stream != d->stream)
  {
    (void)hipStreamSynchronize(d->last_stream);
  }
  void *ptrs[] = {d->d_chan, d->d_taps, d->d_cs, d->d_hist[0], d->d_hist[1], d->d_in, d->d_out, d->d_rx, d->d_scratch_mag};
  for (void *p : ptrs)
  {
    if (p) (void)hipFree(p);
  }
  if (d->h_stage_chan) (void)hipHostFree(d->h_stage_chan);
  if (d->h_stage_taps) (void)hipHostFree(d->h_stage_taps);
  if (d->ev_last) (void)hipEventDestroy(d->ev_last);
  if (d->ev_upload) (void)hipEventDestroy(d->ev_upload);
  if (d->stream)
  {
    (void)hipStreamDestroy(d->stream);
  }
  delete d;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_reset(hrfd_ddc *d)
{
  if (d == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_reset: NULL handle");
  }
  std::lock_guard<std::mutex> g(d->mu);
  d->N = 0;
  for (hrfd::DdcChanDev &c : d->h_chan)
  {
    c.theta_ref = 0u;
    c.n_ref = 0ull;
  }
  d->clear_history = true;
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_set_tuning(hrfd_ddc *d, uint32_t channel, uint32_t capture, uint32_t step)
{
  if (d == nullptr || channel >= d->n_channels || capture >= d->n_captures)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_tuning: bad handle, channel or capture");
  }
  std::lock_guard<std::mutex> g(d->mu);
  hrfd::DdcChanDev &c = d->h_chan[channel];
  // phase-continuous at the change point: theta_ref = theta(N) under the old tuning
  c.theta_ref = c.theta_ref + (uint32_t)(d->N - c.n_ref) * c.step;
  c.n_ref = d->N;
  c.step = step;
  c.capture = capture;
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_set_gain_shift(hrfd_ddc *d, uint32_t channel, uint32_t gshift)
{
  if (gshift > 7)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_gain_shift: g must be 0..7 (got %u)", gshift);
  }
  if (d == nullptr || (channel >= d->n_channels && channel != HRFD_ALL_CHANNELS))
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_gain_shift: bad handle or channel");
  }
  std::lock_guard<std::mutex> g(d->mu);
  for (uint32_t c = 0; c < d->n_channels; c++)
  {
    if (channel == HRFD_ALL_CHANNELS || c == channel)
    {
      d->h_chan[c].g = gshift;
    }
  }
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_set_filter(hrfd_ddc *d, int stage, const int16_t *taps, uint32_t n)
{
  if (stage != 0 && stage != 1)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_filter: stage must be 0 (A) or 1 (B) (got %d)", stage);
  }
  const int rc = ddc_taps_ok("hrfd_ddc_set_filter", taps, n, stage == 0 ? hrfd::kDdcMaxTA : hrfd::kDdcMaxTB);
  if (rc != HRFD_OK)
  {
    return rc;
  }
  if (d == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_filter: NULL handle");
  }
  std::lock_guard<std::mutex> g(d->mu);
  (stage == 0 ? d->tapsA : d->tapsB).assign(taps, taps + n);
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_get_phase(hrfd_ddc *d, uint32_t channel, uint32_t *theta)
{
  if (d == nullptr || channel >= d->n_channels || theta == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_get_phase: bad handle, channel or NULL result");
  }
  std::lock_guard<std::mutex> g(d->mu);
  const hrfd::DdcChanDev &c = d->h_chan[channel];
  *theta = c.theta_ref + (uint32_t)(d->N - c.n_ref) * c.step;
  return HRFD_OK;
}

// one launch over every channel on `s`: out_bytes per channel from R * out_bytes per capture
static int ddc_launch(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes, int8_t *d_out,
                      uint64_t out_stride, hipStream_t s)
{
  using namespace hrfd;
  // The history ping-pong and the records are the handle's: a launch on another stream than the last one waits for it
  // on the device (without it, this launch would read the history the last one is still writing).
  if (s != d->last_stream)
  {
    HIP_TRY(hipEventRecord(d->ev_last, d->last_stream));
    HIP_TRY(hipStreamWaitEvent(s, d->ev_last, 0));
  }
  DdcParams P;
  {
    std::lock_guard<std::mutex> g(d->mu);
    if (d->dirty || d->clear_history)
    {
      // records, taps and a cleared history go to the device on `s`, ahead of this launch; the pinned staging buffer
      // is rewritten only once the device has read the previous upload out of it
      HIP_TRY(hipEventSynchronize(d->ev_upload));
      memcpy(d->h_stage_chan, d->h_chan.data(), sizeof(DdcChanDev) * d->n_channels);
      memset(d->h_stage_taps, 0, sizeof(uint2) * (kDdcJA + kDdcJB));
      ddc_pack_taps(d->tapsA, d->h_stage_taps, ddc_packed_len((int)d->tapsA.size()));
      ddc_pack_taps(d->tapsB, d->h_stage_taps + kDdcJA, ddc_packed_len((int)d->tapsB.size()));
      HIP_TRY(hipMemcpyAsync(d->d_chan, d->h_stage_chan, sizeof(DdcChanDev) * d->n_channels, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d->d_taps, d->h_stage_taps, sizeof(uint2) * (kDdcJA + kDdcJB), hipMemcpyHostToDevice, s));
      HIP_TRY(hipEventRecord(d->ev_upload, s));
      if (d->clear_history)
      {
        HIP_TRY(hipMemsetAsync(d->d_hist[d->cur], 0, (size_t)d->n_captures * d->H * 2, s));
        d->clear_history = false;
      }
      d->dirty = false;
    }
    P.TA = (int)d->tapsA.size();
    P.TB = (int)d->tapsB.size();
    P.n0 = d->N;
    d->N += (uint64_t)d->R * (out_bytes / 2u);   // under the same lock as the read: a setter sees N before or after
  }
  P.cap = d_captures;
  P.cap_stride = capture_stride;
  P.hist_in = d->d_hist[d->cur];
  P.hist_out = d->d_hist[d->cur ^ 1];
  P.out = d_out;
  P.out_stride = out_stride;
  P.chan = d->d_chan;
  P.taps = d->d_taps;
  P.cs = d->d_cs;
  P.M = out_bytes / 2u;
  P.n_tiles = (P.M + kDdcTile - 1) / kDdcTile;
  P.n_channels = d->n_channels;
  P.n_captures = d->n_captures;
  P.H = d->H;
  P.JA = ddc_packed_len(P.TA);
  P.JB = ddc_packed_len(P.TB);
  const dim3 grid(P.n_tiles * d->n_channels + d->n_captures);
  switch (d->R)
  {
  case 1: hipLaunchKernelGGL(k_ddc<1>, grid, dim3(kDdcThreads), 0, s, P); break;
  case 2: hipLaunchKernelGGL(k_ddc<2>, grid, dim3(kDdcThreads), 0, s, P); break;
  case 4: hipLaunchKernelGGL(k_ddc<4>, grid, dim3(kDdcThreads), 0, s, P); break;
  default: hipLaunchKernelGGL(k_ddc<8>, grid, dim3(kDdcThreads), 0, s, P); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess)
  {
    // the counter and the history advance only with a launch that was accepted
    std::lock_guard<std::mutex> g(d->mu);
    d->N = P.n0;
    return fail(HRFD_ENODEV, "k_ddc launch failed: %s", hipGetErrorString(e));
  }
  d->cur ^= 1;
  d->last_stream = s;
  return HRFD_OK;
}

static int ddc_check_call(hrfd_ddc *d, const void *captures, uint64_t capture_stride, uint32_t out_bytes, const void *out,
                          uint64_t out_stride, const char *who)
{
  if (d == nullptr || captures == nullptr || out == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  if (out_bytes < 2 || (out_bytes & 1u) != 0 || out_bytes > (1u << 25))
  {
    return fail(HRFD_EINVAL, "%s: out_bytes must be even, >= 2 and <= 2^25 (got %u)", who, out_bytes);
  }
  // one launch: gridDim.x * blockDim.x work-items must fit in 32 bits
  if ((uint64_t)d->n_channels * ((out_bytes / 2u + hrfd::kDdcTile - 1) / hrfd::kDdcTile) + d->n_captures >
      0xffffffffull / hrfd::kDdcThreads)
  {
    return fail(HRFD_EINVAL, "%s: %u channels x %u bytes need more workgroups than one launch takes", who, d->n_channels,
                out_bytes);
  }
  if (capture_stride < (uint64_t)d->R * out_bytes || out_stride < out_bytes || (capture_stride & 1u) != 0 ||
      ((uintptr_t)captures & 1u) != 0)
  {
    return fail(HRFD_EINVAL, "%s: strides shorter than a row, or an odd capture stride / address", who);
  }
  return HRFD_OK;
}

extern "C" int hrfd_ddc_process_device(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes,
                                       int8_t *d_out, uint64_t out_stride, void *stream)
{
  int rc = ddc_check_call(d, d_captures, capture_stride, out_bytes, d_out, out_stride, "hrfd_ddc_process_device");
  if (rc != HRFD_OK)
  {
    return rc;
  }
  HIP_TRY(hipSetDevice(d->device));
  return ddc_launch(d, d_captures, capture_stride, out_bytes, d_out, out_stride,
                    stream ? (hipStream_t)stream : d->stream);
}

extern "C" int hrfd_ddc_process(hrfd_ddc *d, const int8_t *captures, uint32_t out_bytes, int8_t *out)
{
  int rc = ddc_check_call(d, captures, d ? (uint64_t)d->R * out_bytes : 0, out_bytes, out, out_bytes, "hrfd_ddc_process");
  if (rc != HRFD_OK)
  {
    return rc;
  }
  HIP_TRY(hipSetDevice(d->device));
  hipStream_t s = d->stream;
  HIP_TRY(hipStreamSynchronize(s));
  const size_t in_bytes = (size_t)d->n_captures * d->R * out_bytes, out_total = (size_t)d->n_channels * out_bytes;
  if ((rc = grow((void **)&d->d_in, &d->cap_in, in_bytes)) != HRFD_OK) return rc;
  if ((rc = grow((void **)&d->d_out, &d->cap_out, out_total)) != HRFD_OK) return rc;
  HIP_TRY(hipMemcpyAsync(d->d_in, captures, in_bytes, hipMemcpyHostToDevice, s));
  if ((rc = ddc_launch(d, d->d_in, (uint64_t)d->R * out_bytes, out_bytes, d->d_out, out_bytes, s)) != HRFD_OK)
  {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(out, d->d_out, out_total, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return HRFD_OK;
}

extern "C" int hrfd_ddc_receive(hrfd_ddc *d, hrfd_rx *rx, const int8_t *d_captures, uint64_t capture_stride,
                                uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db, int16_t *d_pcm, uint32_t *d_n_pcm,
                                uint32_t *d_magnitude, uint8_t *d_signal_allowed, uint32_t *n_replayed)
{
  if (rx == nullptr || d_pcm == nullptr || d_n_pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_receive: NULL argument");
  }
  if (d != nullptr && rx->n_channels != d->n_channels)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_receive: the rx handle has %u channels, the DDC %u", rx->n_channels, d->n_channels);
  }
  if (block_bytes == 0 || (block_bytes & 1u) != 0 || block_bytes > HRFD_BLOCK_BYTES || n_blocks == 0 ||
      (uint64_t)block_bytes * n_blocks > (1u << 25))
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_receive: block_bytes must be even, > 0 and <= %u, n_blocks > 0, at most 2^25 "
                "bytes per channel (got %u x %u)", HRFD_BLOCK_BYTES, block_bytes, n_blocks);
  }
  const uint32_t out_bytes = block_bytes * n_blocks;
  int rc = ddc_check_call(d, d_captures, capture_stride, out_bytes, d_pcm, out_bytes, "hrfd_ddc_receive");
  if (rc != HRFD_OK)
  {
    return rc;
  }
  if (rx->device != d->device)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_receive: the rx handle lives on device %d, the DDC on %d", rx->device, d->device);
  }
  HIP_TRY(hipSetDevice(d->device));
  hipStream_t s = rx->stream;
  const uint32_t C = d->n_channels;
  const size_t units = (size_t)C * n_blocks;
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = grow((void **)&d->d_rx, &d->cap_rx, (size_t)C * out_bytes)) != HRFD_OK) return rc;
  if (d_magnitude == nullptr || d_signal_allowed == nullptr)
  {
    // the rx launches always write both: scratch rows for the ones the caller does not want
    if ((rc = grow((void **)&d->d_scratch_mag, &d->cap_scratch, units * 5)) != HRFD_OK) return rc;
  }
  uint32_t *mag = d_magnitude ? d_magnitude : (uint32_t *)d->d_scratch_mag;
  uint8_t *allowed = d_signal_allowed ? d_signal_allowed : (uint8_t *)d->d_scratch_mag + units * 4;
  if ((rc = ddc_launch(d, d_captures, capture_stride, out_bytes, d->d_rx, out_bytes, s)) != HRFD_OK)
  {
    return rc;
  }
  // mode NONE / squelched units produce no PCM: zeros, as hrfd_rx_process_block hands back
  HIP_TRY(hipMemsetAsync(d_pcm, 0, units * ((block_bytes + 511u) / 512u) * sizeof(int16_t), s));
  uint32_t replayed = 0;
  if ((rc = rx_run_batch(rx, d->d_rx, block_bytes, n_blocks, gain_db, d_pcm, d_n_pcm, mag, allowed, nullptr, s,
                         &replayed)) != HRFD_OK)
  {
    return rc;
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (n_replayed != nullptr)
  {
    *n_replayed = replayed;
  }
  return HRFD_OK;
}
