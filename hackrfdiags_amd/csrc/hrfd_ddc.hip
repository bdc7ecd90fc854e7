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
//
// The receive key (k_ddc<R, true>; hrfd_ddc_key.h): a key byte per (channel, block of 2^k outputs).  A
// workgroup owns one (channel, tile) and nothing of a channel is carried through time, so a unit whose key block is off
// stores its zeros, counts itself on its channel's meter and returns, ahead of every table, capture and history load.  The
// history workgroups know no key.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrfd_ddc_key.h"
#include "hrfd_ddc_tables.h"

namespace hrfd {

constexpr int kDdcTile = kBankTile;        // outputs per workgroup
constexpr int kDdcThreads = kBankThreads;
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

struct DdcParams
{
  const int8_t *cap;           // [W] rows of R * 2M bytes, cap_stride apart
  uint64_t cap_stride;
  const int8_t *hist_in;       // [W][H] IQ samples: the H samples in front of this call
  int8_t *hist_out;            // [W][H]: the H samples in front of the next call
  int8_t *out;                 // [C] rows of 2M bytes, out_stride apart
  uint64_t out_stride;
  const BankTuning *chan;        // word: the gain shift g
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
  // the receive key (k_ddc<R, true> only)
  const uint8_t *key;          // [C] rows of ceil(M / 2^key_log2) bytes, key_stride apart
  uint64_t key_stride;
  uint32_t key_log2;
  unsigned long long *skips;   // [C] the units of every channel skipped since create / reset
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

// n zero bytes at dst, any address: whole 16-byte stores over the aligned middle, bytes at the two ends, nothing past n
__device__ __forceinline__ void ddc_store_zeros(int8_t *dst, int n, int tid)
{
  const int head = min((int)(-(uintptr_t)dst & 15u), n);
  const int n16 = (n - head) >> 4;
  const int tail = n - head - 16 * n16;
  for (int i = tid; i < n16; i += kDdcThreads)
  {
    *(uint4 *)(dst + head + 16 * i) = make_uint4(0u, 0u, 0u, 0u);
  }
  if (tid < head)
  {
    dst[tid] = 0;
  }
  if (tid < tail)
  {
    dst[head + 16 * n16 + tid] = 0;
  }
}

template <int R, bool KEYED>
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
  if constexpr (KEYED)
  {
    // one byte, the same for the whole workgroup, ahead of the tables and their barrier
    if (ddc_key_skip(P.key + (uint64_t)c * P.key_stride, (uint32_t)m_t / kDdcTile, P.key_log2))
    {
      ddc_store_zeros(P.out + (uint64_t)c * P.out_stride + 2 * (uint64_t)m_t, 2 * cnt, tid);
      if (tid == 0)
      {
        atomicAdd(P.skips + c, 1ull);
      }
      return;
    }
  }
  const BankTuning ch = P.chan[c];

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
    const uint32_t theta_call = bank_phase_at(ch, P.n0);
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
  const int g = (int)ch.word;
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

template __global__ void k_ddc<1, false>(const DdcParams);
template __global__ void k_ddc<2, false>(const DdcParams);
template __global__ void k_ddc<4, false>(const DdcParams);
template __global__ void k_ddc<8, false>(const DdcParams);
template __global__ void k_ddc<1, true>(const DdcParams);
template __global__ void k_ddc<2, true>(const DdcParams);
template __global__ void k_ddc<4, true>(const DdcParams);
template __global__ void k_ddc<8, true>(const DdcParams);

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_ddc
{
  hrfd::BankCore core;
  uint32_t n_captures = 0, n_channels = 0, R = 1, H = 0;
  // pinned staging of the records and packed taps (uploads in stream order)
  hrfd::PinnedBuf<hrfd::BankTuning> h_stage_chan;
  hrfd::PinnedBuf<uint2> h_stage_taps;

  // host records, under core.mu
  std::vector<hrfd::BankTuning> h_chan;
  std::vector<int16_t> tapsA, tapsB;
  bool dirty = true;
  uint64_t N = 0;                          // absolute input-sample counter
  bool clear_history = true;               // also clears the skip meters
  uint32_t key_log2 = hrfd::kDdcKeyDefaultLog2;   // the key block of the next keyed call

  hrfd::DevBuf<unsigned long long> d_skips;       // [C] units the keyed kernel skipped, per channel
  hrfd::DevBuf<uint8_t> d_key;                    // host-path staging of the key rows
  hrfd::DevBuf<hrfd::BankTuning> d_chan;
  hrfd::DevBuf<uint2> d_taps;
  hrfd::DevBuf<uint32_t> d_cs;
  hrfd::DevBuf<int8_t> d_hist[2];
  int cur = 0;
  hrfd::DevBuf<int8_t> d_in, d_out, d_rx;  // host-path staging and hrfd_ddc_receive's buffer
  hrfd::DevBuf<uint8_t> d_scratch_mag;
};

extern "C" int hrfd_ddc_create(uint32_t n_captures, uint32_t n_channels, uint32_t decimation, int device, hrfd_ddc **out)
{
  using namespace hrfd;
  if (out == nullptr || n_captures == 0 || n_channels == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_create: need n_captures > 0, n_channels > 0 and a result pointer");
  }
  *out = nullptr;
  BANK_TRY(bank_rate_ok("hrfd_ddc_create", "decimation", decimation));
  hrfd_ddc *d = nullptr;
  BANK_TRY(bank_new("hrfd_ddc_create", device, &d));
  d->n_captures = n_captures;
  d->n_channels = n_channels;
  d->R = decimation;
  d->H = 255u * decimation + 63u;
  d->h_chan.assign(n_channels, BankTuning{0u, 0u, 0u, 0u, 0ull});
  switch (decimation)
  {
  case 2: d->tapsA.assign(Q_DDC_A2, Q_DDC_A2 + N_DDC_A2); break;
  case 4: d->tapsA.assign(Q_DDC_A4, Q_DDC_A4 + N_DDC_A4); break;
  case 8: d->tapsA.assign(Q_DDC_A8, Q_DDC_A8 + N_DDC_A8); break;
  default: break;                          // R = 1: stage A in bypass
  }
  d->tapsB.assign(Q_DDC_B, Q_DDC_B + N_DDC_B);
  const size_t hist_bytes = (size_t)n_captures * d->H * 2;
  const bool ok = d->d_chan.alloc(n_channels) && d->d_taps.alloc(kDdcJA + kDdcJB) && bank_upload_cos(d->d_cs) &&
                  d->d_skips.alloc(n_channels) && d->d_hist[0].alloc(hist_bytes) && d->d_hist[1].alloc(hist_bytes) && d->h_stage_chan.alloc(n_channels) &&
                  d->h_stage_taps.alloc(kDdcJA + kDdcJB);
  if (!ok)
  {
    (void)hipGetLastError();
    bank_free(d);
    return fail(HRFD_ENOMEM, "hrfd_ddc_create: device allocation failed");
  }
  *out = d;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_destroy(hrfd_ddc *d)
{
  if (d != nullptr)
  {
    hrfd::bank_free(d);
  }
  return HRFD_OK;
}

extern "C" int hrfd_ddc_reset(hrfd_ddc *d) { return hrfd::tuned_reset(d, "hrfd_ddc_reset"); }

extern "C" int hrfd_ddc_set_tuning(hrfd_ddc *d, uint32_t channel, uint32_t capture, uint32_t step)
{
  return hrfd::tuned_set_tuning(d, "hrfd_ddc_set_tuning", channel, capture, step);
}

extern "C" int hrfd_ddc_set_gain_shift(hrfd_ddc *d, uint32_t channel, uint32_t gshift)
{
  if (gshift > 7)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_gain_shift: g must be 0..7 (got %u)", gshift);
  }
  return hrfd::tuned_set_word(d, "hrfd_ddc_set_gain_shift", channel, gshift);
}

extern "C" int hrfd_ddc_set_filter(hrfd_ddc *d, int stage, const int16_t *taps, uint32_t n)
{
  if (stage != 0 && stage != 1)
  {
    return fail(HRFD_EINVAL, "hrfd_ddc_set_filter: stage must be 0 (A) or 1 (B) (got %d)", stage);
  }
  BANK_TRY(hrfd::bank_tap_count_ok("hrfd_ddc_set_filter", taps, n, stage == 0 ? hrfd::kDdcMaxTA : hrfd::kDdcMaxTB));
  BANK_TRY(hrfd::bank_tap_sums_ok("hrfd_ddc_set_filter", taps, n, 1u));
  BANK_TRY(hrfd::bank_need_handle("hrfd_ddc_set_filter", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  (stage == 0 ? d->tapsA : d->tapsB).assign(taps, taps + n);
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_get_phase(hrfd_ddc *d, uint32_t channel, uint32_t *theta)
{
  return hrfd::tuned_get_phase(d, "hrfd_ddc_get_phase", channel, theta);
}

extern "C" int hrfd_ddc_set_key_block(hrfd_ddc *d, uint32_t log2_samples)
{
  BANK_TRY(hrfd::ddc_key_check_block("hrfd_ddc_set_key_block", log2_samples));
  BANK_TRY(hrfd::bank_need_handle("hrfd_ddc_set_key_block", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  d->key_log2 = log2_samples;              // a launch takes its own copy; the key touches no state of the handle
  return HRFD_OK;
}

extern "C" int hrfd_ddc_n_keys(hrfd_ddc *d, uint32_t out_bytes, uint32_t *n)
{
  BANK_TRY(hrfd::ddc_key_check_result("hrfd_ddc_n_keys", n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_ddc_n_keys", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  *n = hrfd::ddc_key_n(out_bytes / 2u, d->key_log2);
  return HRFD_OK;
}

extern "C" int hrfd_ddc_get_key_skips(hrfd_ddc *d, uint32_t channel, uint64_t *n)
{
  BANK_TRY(hrfd::ddc_key_check_result("hrfd_ddc_get_key_skips", n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_ddc_get_key_skips", d));
  BANK_TRY(hrfd::ddc_key_check_channel("hrfd_ddc_get_key_skips", channel, d->n_channels));
  HIP_TRY(hipSetDevice(d->core.device));
  {
    std::lock_guard<std::mutex> g(d->core.mu);
    if (d->clear_history)
    {
      *n = 0;                              // no launch since create or reset
      return HRFD_OK;
    }
  }
  HIP_TRY(hipStreamSynchronize(d->core.last_stream));
  const bool all = channel == HRFD_ALL_CHANNELS;
  std::vector<unsigned long long> v(all ? d->n_channels : 1u);
  HIP_TRY(hipMemcpy(v.data(), d->d_skips + (all ? 0u : channel), sizeof(unsigned long long) * v.size(), hipMemcpyDeviceToHost));
  uint64_t sum = 0;
  for (unsigned long long x : v)
  {
    sum += x;
  }
  *n = sum;
  return HRFD_OK;
}

extern "C" int hrfd_ddc_count_key_skips(const uint8_t *key, uint64_t key_stride, uint32_t n_channels, uint32_t out_bytes,
                                        uint32_t log2_samples, uint64_t *per_channel, uint64_t *sum)
{
  const char *who = "hrfd_ddc_count_key_skips";
  BANK_TRY(hrfd::ddc_key_check_block(who, log2_samples));
  if (key == nullptr || n_channels == 0 || out_bytes < 2u)
  {
    return fail(HRFD_EINVAL, "%s: need key rows, n_channels > 0 and out_bytes >= 2", who);
  }
  BANK_TRY(hrfd::ddc_key_check_result(who, sum));
  BANK_TRY(hrfd::ddc_key_check_stride(who, key, key_stride, out_bytes, log2_samples));
  *sum = hrfd::ddc_key_count_skips(key, key_stride, n_channels, out_bytes / 2u, log2_samples, per_channel);
  return HRFD_OK;
}

// the key block of a call that starts now: a setter on another thread lands before or behind it
static uint32_t ddc_key_log2(hrfd_ddc *d)
{
  std::lock_guard<std::mutex> g(d->core.mu);
  return d->key_log2;
}

// one launch over every channel on `s`: out_bytes per channel from R * out_bytes per capture; d_key NULL: the unkeyed kernel
static int ddc_launch(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes, int8_t *d_out,
                      uint64_t out_stride, hipStream_t s, const uint8_t *d_key = nullptr, uint64_t key_stride = 0,
                      uint32_t key_log2 = hrfd::kDdcKeyDefaultLog2)
{
  using namespace hrfd;
  // without this wait, the launch would read the history the last one is still writing
  BANK_TRY(d->core.order_behind_last(s));
  DdcParams P;
  {
    std::lock_guard<std::mutex> g(d->core.mu);
    if (d->dirty || d->clear_history)
    {
      // records, taps and a cleared history go to the device on `s`, ahead of this launch
      BANK_TRY(d->core.staging_wait());
      memcpy(d->h_stage_chan, d->h_chan.data(), sizeof(BankTuning) * d->n_channels);
      memset(d->h_stage_taps, 0, sizeof(uint2) * (kDdcJA + kDdcJB));
      bank_pack_taps(d->tapsA.data(), (int)d->tapsA.size(), d->h_stage_taps.p, bank_packed_len((int)d->tapsA.size()));
      bank_pack_taps(d->tapsB.data(), (int)d->tapsB.size(), d->h_stage_taps + kDdcJA, bank_packed_len((int)d->tapsB.size()));
      HIP_TRY(hipMemcpyAsync(d->d_chan, d->h_stage_chan, sizeof(BankTuning) * d->n_channels, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d->d_taps, d->h_stage_taps, sizeof(uint2) * (kDdcJA + kDdcJB), hipMemcpyHostToDevice, s));
      BANK_TRY(d->core.staging_sent(s));
      if (d->clear_history)
      {
        HIP_TRY(hipMemsetAsync(d->d_hist[d->cur], 0, (size_t)d->n_captures * d->H * 2, s));
        HIP_TRY(hipMemsetAsync(d->d_skips, 0, sizeof(unsigned long long) * d->n_channels, s));
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
  P.JA = bank_packed_len(P.TA);
  P.JB = bank_packed_len(P.TB);
  P.key = d_key;
  P.key_stride = key_stride;
  P.key_log2 = key_log2;
  P.skips = d->d_skips;
  const dim3 grid(P.n_tiles * d->n_channels + d->n_captures);
  if (d_key == nullptr)
  {
    switch (d->R)
    {
    case 1: hipLaunchKernelGGL((k_ddc<1, false>), grid, dim3(kDdcThreads), 0, s, P); break;
    case 2: hipLaunchKernelGGL((k_ddc<2, false>), grid, dim3(kDdcThreads), 0, s, P); break;
    case 4: hipLaunchKernelGGL((k_ddc<4, false>), grid, dim3(kDdcThreads), 0, s, P); break;
    default: hipLaunchKernelGGL((k_ddc<8, false>), grid, dim3(kDdcThreads), 0, s, P); break;
    }
  }
  else
  {
    switch (d->R)
    {
    case 1: hipLaunchKernelGGL((k_ddc<1, true>), grid, dim3(kDdcThreads), 0, s, P); break;
    case 2: hipLaunchKernelGGL((k_ddc<2, true>), grid, dim3(kDdcThreads), 0, s, P); break;
    case 4: hipLaunchKernelGGL((k_ddc<4, true>), grid, dim3(kDdcThreads), 0, s, P); break;
    default: hipLaunchKernelGGL((k_ddc<8, true>), grid, dim3(kDdcThreads), 0, s, P); break;
    }
  }
  const int rc = bank_launch_ok("k_ddc");
  if (rc != HRFD_OK)
  {
    // the counter and the history advance only with a launch that was accepted
    std::lock_guard<std::mutex> g(d->core.mu);
    d->N = P.n0;
    return rc;
  }
  d->cur ^= 1;
  d->core.launched_on(s);
  return HRFD_OK;
}

static int ddc_check_call(hrfd_ddc *d, const void *captures, uint64_t capture_stride, uint32_t out_bytes, const void *out,
                          uint64_t out_stride, const char *who)
{
  if (d == nullptr || captures == nullptr || out == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return hrfd::bank_check_call(who, "out_bytes", out_bytes, captures, capture_stride, d->R, out_stride, 1u, d->n_channels,
                               d->n_captures);
}

// The three entries, with and without a key (key NULL: the unkeyed call), under `who`.  The key's stride is checked against
// the largest key block first, which needs no handle, then against the handle's; *k is the block the launch uses
static int ddc_check_keyed(hrfd_ddc *d, const void *captures, uint64_t capture_stride, uint32_t out_bytes, const void *out,
                           uint64_t out_stride, const void *key, uint64_t key_stride, const char *who, uint32_t *k)
{
  BANK_TRY(hrfd::ddc_key_check_stride(who, key, key_stride, out_bytes, hrfd::kDdcKeyMaxLog2));
  BANK_TRY(ddc_check_call(d, captures, capture_stride, out_bytes, out, out_stride, who));
  *k = ddc_key_log2(d);
  return hrfd::ddc_key_check_stride(who, key, key_stride, out_bytes, *k);
}

static int ddc_process_device(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes,
                              const uint8_t *d_key, uint64_t key_stride, int8_t *d_out, uint64_t out_stride, void *stream,
                              const char *who)
{
  uint32_t k = 0;
  BANK_TRY(ddc_check_keyed(d, d_captures, capture_stride, out_bytes, d_out, out_stride, d_key, key_stride, who, &k));
  HIP_TRY(hipSetDevice(d->core.device));
  return ddc_launch(d, d_captures, capture_stride, out_bytes, d_out, out_stride, d->core.stream_or_own(stream), d_key,
                    key_stride, k);
}

static int ddc_process(hrfd_ddc *d, const int8_t *captures, uint32_t out_bytes, const uint8_t *key, int8_t *out, const char *who)
{
  uint32_t k = 0;
  // the host entry's key is dense: rows of n_keys bytes
  BANK_TRY(ddc_check_keyed(d, captures, d ? (uint64_t)d->R * out_bytes : 0, out_bytes, out, out_bytes, nullptr, 0, who, &k));
  const uint32_t n_keys = hrfd::ddc_key_n(out_bytes / 2u, k);
  hrfd::BankHostCall call(d->core);
  const size_t in_bytes = (size_t)d->n_captures * d->R * out_bytes, out_total = (size_t)d->n_channels * out_bytes;
  const int8_t *d_in = call.up(d->d_in, captures, in_bytes);
  const uint8_t *d_key = call.up(d->d_key, key, (size_t)d->n_channels * n_keys);
  int8_t *d_out = call.room(d->d_out, out, out_total);
  BANK_TRY(call.rc);
  BANK_TRY(ddc_launch(d, d_in, (uint64_t)d->R * out_bytes, out_bytes, d_out, out_bytes, call.st, d_key, n_keys, k));
  call.down(out, d_out, out_total);
  return call.finish();
}

static int ddc_receive(hrfd_ddc *d, hrfd_rx *rx, const int8_t *d_captures, uint64_t capture_stride, uint32_t block_bytes,
                       uint32_t n_blocks, const uint8_t *d_key, uint64_t key_stride, uint32_t gain_db, int16_t *d_pcm,
                       uint32_t *d_n_pcm, uint32_t *d_magnitude, uint8_t *d_signal_allowed, uint32_t *n_replayed, const char *who)
{
  if (rx == nullptr || d_pcm == nullptr || d_n_pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  if (d != nullptr && rx->n_channels != d->n_channels)
  {
    return fail(HRFD_EINVAL, "%s: the rx handle has %u channels, the DDC %u", who, rx->n_channels, d->n_channels);
  }
  if (block_bytes == 0 || (block_bytes & 1u) != 0 || block_bytes > HRFD_BLOCK_BYTES || n_blocks == 0 ||
      (uint64_t)block_bytes * n_blocks > (1u << 25))
  {
    return fail(HRFD_EINVAL, "%s: block_bytes must be even, > 0 and <= %u, n_blocks > 0, at most 2^25 "
                "bytes per channel (got %u x %u)", who, HRFD_BLOCK_BYTES, block_bytes, n_blocks);
  }
  const uint32_t out_bytes = block_bytes * n_blocks;
  uint32_t k = 0;
  BANK_TRY(ddc_check_keyed(d, d_captures, capture_stride, out_bytes, d_pcm, out_bytes, d_key, key_stride, who, &k));
  if (rx->device != d->core.device)
  {
    return fail(HRFD_EINVAL, "%s: the rx handle lives on device %d, the DDC on %d", who, rx->device, d->core.device);
  }
  HIP_TRY(hipSetDevice(d->core.device));
  hipStream_t s = rx->stream;
  const uint32_t C = d->n_channels;
  const size_t units = (size_t)C * n_blocks;
  HIP_TRY(hipStreamSynchronize(s));
  BANK_TRY(d->d_rx.grow_bytes((size_t)C * out_bytes));
  if (d_magnitude == nullptr || d_signal_allowed == nullptr)
  {
    // the rx launches always write both: scratch rows for the ones the caller does not want
    BANK_TRY(d->d_scratch_mag.grow_bytes(units * 5));
  }
  uint32_t *mag = d_magnitude ? d_magnitude : (uint32_t *)d->d_scratch_mag.p;
  uint8_t *allowed = d_signal_allowed ? d_signal_allowed : d->d_scratch_mag + units * 4;
  // the rx bank runs over every channel, keyed or not: its state moves on over a keyed-off block's zeros
  BANK_TRY(ddc_launch(d, d_captures, capture_stride, out_bytes, d->d_rx, out_bytes, s, d_key, key_stride, k));
  // mode NONE / squelched units produce no PCM: zeros, as hrfd_rx_process_block hands back
  HIP_TRY(hipMemsetAsync(d_pcm, 0, units * ((block_bytes + 511u) / 512u) * sizeof(int16_t), s));
  uint32_t replayed = 0;
  BANK_TRY(rx_run_batch(rx, d->d_rx, block_bytes, n_blocks, gain_db, d_pcm, d_n_pcm, mag, allowed, nullptr, s,
                         &replayed));
  HIP_TRY(hipStreamSynchronize(s));
  if (n_replayed != nullptr)
  {
    *n_replayed = replayed;
  }
  return HRFD_OK;
}

extern "C" int hrfd_ddc_process_device(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes,
                                       int8_t *d_out, uint64_t out_stride, void *stream)
{
  return ddc_process_device(d, d_captures, capture_stride, out_bytes, nullptr, 0, d_out, out_stride, stream,
                            "hrfd_ddc_process_device");
}

extern "C" int hrfd_ddc_process_device_keyed(hrfd_ddc *d, const int8_t *d_captures, uint64_t capture_stride, uint32_t out_bytes,
                                             const uint8_t *d_key, uint64_t key_stride, int8_t *d_out, uint64_t out_stride,
                                             void *stream)
{
  return ddc_process_device(d, d_captures, capture_stride, out_bytes, d_key, key_stride, d_out, out_stride, stream,
                            "hrfd_ddc_process_device_keyed");
}

extern "C" int hrfd_ddc_process(hrfd_ddc *d, const int8_t *captures, uint32_t out_bytes, int8_t *out)
{
  return ddc_process(d, captures, out_bytes, nullptr, out, "hrfd_ddc_process");
}

extern "C" int hrfd_ddc_process_keyed(hrfd_ddc *d, const int8_t *captures, uint32_t out_bytes, const uint8_t *key, int8_t *out)
{
  return ddc_process(d, captures, out_bytes, key, out, "hrfd_ddc_process_keyed");
}

extern "C" int hrfd_ddc_receive(hrfd_ddc *d, hrfd_rx *rx, const int8_t *d_captures, uint64_t capture_stride,
                                uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db, int16_t *d_pcm, uint32_t *d_n_pcm,
                                uint32_t *d_magnitude, uint8_t *d_signal_allowed, uint32_t *n_replayed)
{
  return ddc_receive(d, rx, d_captures, capture_stride, block_bytes, n_blocks, nullptr, 0, gain_db, d_pcm, d_n_pcm, d_magnitude,
                     d_signal_allowed, n_replayed, "hrfd_ddc_receive");
}

extern "C" int hrfd_ddc_receive_keyed(hrfd_ddc *d, hrfd_rx *rx, const int8_t *d_captures, uint64_t capture_stride,
                                      uint32_t block_bytes, uint32_t n_blocks, const uint8_t *d_key, uint64_t key_stride,
                                      uint32_t gain_db, int16_t *d_pcm, uint32_t *d_n_pcm, uint32_t *d_magnitude,
                                      uint8_t *d_signal_allowed, uint32_t *n_replayed)
{
  return ddc_receive(d, rx, d_captures, capture_stride, block_bytes, n_blocks, d_key, key_stride, gain_db, d_pcm, d_n_pcm,
                     d_magnitude, d_signal_allowed, n_replayed, "hrfd_ddc_receive_keyed");
}
