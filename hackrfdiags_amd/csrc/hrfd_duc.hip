// hackrfdiags_amd/csrc/hrfd_duc.hip -- hrfd_duc_*: a bank of digital up-converters behind hrfd_mod.
//
// C channel streams of int8 IQ at 2.048 MS/s in, W wideband int8 IQ captures at R x 2.048 MS/s out: per channel stage B
// (channel FIR at 2.048 MS/s), an amplitude, stage A (zero-stuffed interpolation by R) and a mixer (e^{+j theta(n)} from
// the DDC's 4096-entry Q15 cosine table); the channels of a capture are summed in int32 and shifted to int8.  Exact
// integer arithmetic, contract in include/hrfd.h; tests/duc_model.py restates it in numpy.
//
// One workgroup (256 threads) per (capture, tile of kDucTile channel samples = R kDucTile wideband outputs); it loops over
// the channels mapped to its capture (a per-capture list on the device) and keeps the sums in registers:
//   1. the tile's channel samples plus the look-back of both filters are read as dwords into two int16 rails u = x << 8
//   2. stage B (4 consecutive outputs per lane, ddc_fir's register-blocked v_dot2_i32_i16) and the amplitude write v
//   3. every lane owns two pairs of neighbouring channel positions (2 tid, 2 tid + 1 and 512 more): one window of v per
//      pair gives both positions' R polyphase outputs (taps.x for the even position, taps.y -- one leading zero -- for the
//      odd one), so no multiply touches a stuffed zero; neighbouring lanes read neighbouring dwords.  The 2 R wideband
//      outputs of a pair are mixed and added to the lane's int32 sums.
// After the last channel: one rounded, saturated int8 store per output and one clip count per workgroup (a wave
// reduction, an LDS counter, one global atomicAdd).  C extra workgroups per launch copy the last H samples of every
// channel into the other history buffer (ping-pong: the tiles of the same launch read the current one).
//
// The transmit key (k_duc<R, true>; hrfd_duc_key.h): a key byte per (channel, block of 2^k samples).  A
// keyed-off sample is read as zero, by the history workgroups as well, and a unit (channel, tile) whose own key block and
// the one in front of it are off is skipped ahead of every load: zeros through every stage are zeros.  The decision is
// uniform over the workgroup, which counts its skipped units and adds them to the handle's meter once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrfd_duc_key.h"
#include "hrfd_duc_tables.h"

namespace hrfd {

constexpr int kDucTile = kBankTile;        // channel samples per workgroup
constexpr int kDucThreads = kBankThreads;
constexpr int kDucMaxTA = 64;
constexpr int kDucMaxTB = 256;
constexpr int kDucH = 318;                 // history: stage B's 255 samples behind stage A's 63 (R = 1)
constexpr int kDucJB = kDucMaxTB / 2 + 1;  // packed tap dwords of stage B
constexpr int kDucJA = 40;                 // R branches x ((63 / R + 1) / 2 + 1) packed tap dwords at most (R = 8: 8 x 5)
constexpr uint32_t kDucMaxChannels = 32768;
constexpr uint32_t kDucMaxShift = 24;
// u rails: local samples [0, OFF + kDucTile + 16), OFF <= 318 (look-back of both stages, even)
constexpr int kDucUDw = (kDucH + kDucTile + 16) / 2 + 8;
// v rails: kDucTile + LA (<= 63) samples rounded up to quads, plus the last window's overrun
constexpr int kDucVDw = (kDucTile + 64 + 8) / 2 + 8;

struct DucParams
{
  const int8_t *in;            // [C] rows of 2M bytes, in_stride apart
  uint64_t in_stride;
  const int8_t *hist_in;       // [C][kDucH] IQ samples: the samples in front of this call
  int8_t *hist_out;            // [C][kDucH]: the samples in front of the next call
  int8_t *cap;                 // [W] rows of 2 R M bytes, cap_stride apart
  uint64_t cap_stride;
  const BankTuning *chan;        // word: the amplitude A
  const uint32_t *list_off;    // [W + 1]: the channels of capture w are list[list_off[w] .. list_off[w + 1])
  const uint32_t *list;        // [C]
  const uint32_t *shift;       // [W] output shifts
  const uint2 *taps;           // [kDucJA] stage A: branch p at p * JA, then [kDucJB] stage B
  const uint32_t *cs;          // [4096] (COS[k], COS[(k - 1024) & 4095]) as packed int16
  unsigned long long *clips;   // [W]
  uint64_t n0;                 // absolute index of the call's first wideband output
  uint32_t M;                  // channel samples per channel
  uint32_t n_tiles;
  uint32_t n_channels;
  uint32_t n_captures;
  int TA, TB;                  // 0 = bypass
  int LA;                      // stage A look-back in channel samples: (TA - 1) / R
  int JA, JB;                  // packed tap dwords in use (JA per branch)
  // the transmit key (k_duc<R, true> only)
  const uint8_t *key;          // [C] rows of ceil(M / 2^key_log2) bytes, key_stride apart
  uint64_t key_stride;
  uint32_t key_log2;
  unsigned long long *skips;   // the units skipped since create / reset
};

// one IQ sample of channel c at call-local index j (history in front of the call, zeros beyond it) as (I, Q) bytes
__device__ __forceinline__ uint32_t duc_load_sample(const DucParams &P, uint32_t c, int64_t j)
{
  if (j >= 0 && j < (int64_t)P.M)
  {
    return *(const uint16_t *)(P.in + (uint64_t)c * P.in_stride + 2 * (uint64_t)j);
  }
  if (j < 0 && j >= -(int64_t)kDucH)
  {
    return *(const uint16_t *)(P.hist_in + ((uint64_t)c * kDucH + (uint64_t)(kDucH + j)) * 2);
  }
  return 0u;
}

// samples j, j + 1 (j even) as (I0, Q0, I1, Q1) bytes: one dword load where both lie in one aligned source dword
__device__ __forceinline__ uint32_t duc_load_pair(const DucParams &P, uint32_t c, int64_t j)
{
  if (j >= 0 && j + 1 < (int64_t)P.M)
  {
    const int8_t *p = P.in + (uint64_t)c * P.in_stride + 2 * (uint64_t)j;
    if (((uintptr_t)p & 3u) == 0)
    {
      return *(const uint32_t *)p;
    }
  }
  else if (j < 0 && j >= -(int64_t)kDucH)
  {
    // a history row is kDucH = 318 samples = 636 bytes (4-byte aligned) and j is even
    return *(const uint32_t *)(P.hist_in + ((uint64_t)c * kDucH + (uint64_t)(kDucH + j)) * 2);
  }
  return duc_load_sample(P, c, j) | (duc_load_sample(P, c, j + 1) << 16);
}

__device__ __forceinline__ uint32_t pack16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }

template <int R, bool KEYED>
__global__ __launch_bounds__(kDucThreads) void k_duc(const DucParams P)
{
  __shared__ uint32_t cs[4096];
  __shared__ uint32_t uI[kDucUDw], uQ[kDucUDw];
  __shared__ uint32_t vI[kDucVDw], vQ[kDucVDw];
  __shared__ uint2 taps[kDucJA + kDucJB];
  __shared__ uint32_t clip_sum;
  __shared__ uint32_t skip_sum;                         // keyed: this workgroup's skipped units, thread 0's alone
  const int tid = threadIdx.x;
  const uint32_t n_units = P.n_tiles * P.n_captures;
  if (blockIdx.x >= n_units)
  {
    // history: the last kDucH samples of (history, this call's input) of channel c, for the next call
    const uint32_t c = blockIdx.x - n_units;
    for (int i = tid; i < kDucH; i += kDucThreads)
    {
      const int64_t j = (int64_t)P.M - kDucH + i;
      uint32_t v = 0u;
      if (!KEYED || duc_key_on(P.key + (uint64_t)c * P.key_stride, j, P.M, P.key_log2))
      {
        v = duc_load_sample(P, c, j);
      }
      *(uint16_t *)(P.hist_out + ((uint64_t)c * kDucH + i) * 2) = (uint16_t)v;
    }
    return;
  }
  const uint32_t w = blockIdx.x / P.n_tiles;
  const int m_t = (int)(blockIdx.x - w * P.n_tiles) * kDucTile;
  const int cnt = min(kDucTile, (int)P.M - m_t);

  for (int i = tid; i < 4096; i += kDucThreads)
  {
    cs[i] = P.cs[i];
  }
  for (int i = tid; i < kDucJA + kDucJB; i += kDucThreads)
  {
    taps[i] = P.taps[i];
  }
  if (tid == 0)
  {
    clip_sum = 0u;
    if (KEYED)
    {
      skip_sum = 0u;
    }
  }
  const int TA = P.TA, TB = P.TB, LA = P.LA;
  const int LB = TB > 0 ? TB - 1 : 0;
  const int OFF = (LA + LB + 1) & ~1;                   // u local index 0 = channel position m_t - OFF (even)
  const int delta = OFF - LA - LB;                      // stage B window of v index k starts at u index k + delta
  const int nud = (OFF + kDucTile + 16) / 2;            // u dwords filled
  const int nq = (kDucTile + LA + 3) / 4;               // v quads: v index k = channel position m_t - LA + k

  int sI[2][2 * R], sQ[2][2 * R];
#pragma unroll
  for (int h = 0; h < 2; h++)
  {
#pragma unroll
    for (int i = 0; i < 2 * R; i++)
    {
      sI[h][i] = 0;
      sQ[h][i] = 0;
    }
  }

  const uint32_t c_end = P.list_off[w + 1];
  for (uint32_t ci = P.list_off[w]; ci < c_end; ci++)
  {
    const uint32_t c = P.list[ci];
    // keyed: the u dwords [p_lo, p_hi) are read, the others are zeros.  The look-back lies in the tile in front and so in
    // one key block, the tile in another or the same; tile 0 looks back into the history, which holds masked samples
    // already.  The rails' last 16 samples lie behind the tile, where the row may end: no output of the tile needs them
    // (their stage B outputs meet stage A's zero taps only), so the keyed kernel reads neither them nor their key
    int p_lo = 0, p_hi = nud;
    if (KEYED)
    {
      const uint8_t *row = P.key + (uint64_t)c * P.key_stride;
      const uint32_t t = (uint32_t)m_t / kDucTile;
      if (duc_key_skip(row, t, P.key_log2))
      {
        if (tid == 0)
        {
          skip_sum++;
        }
        continue;                                         // uniform over the workgroup, ahead of the amplitude's mute
      }
      const bool on_prev = t == 0u || row[duc_key_block_of((uint32_t)m_t - kDucTile, P.key_log2)] != 0;
      const bool on_cur = row[duc_key_block_of((uint32_t)m_t, P.key_log2)] != 0;
      p_lo = on_prev ? 0 : OFF / 2;
      p_hi = on_cur ? (OFF + kDucTile) / 2 : OFF / 2;
    }
    const BankTuning ch = P.chan[c];
    if (ch.word == 0u)
    {
      continue;                                         // muted: every y is 0 (uniform over the workgroup)
    }
    // 1. u rails: dword p holds samples m_t - OFF + 2p, + 1 (x << 8 in every half)
    for (int p = tid; p < nud; p += kDucThreads)
    {
      uint32_t d = 0u;
      // both samples of a dword lie in one tile (OFF and the tile are even), so in one key block
      if (!KEYED || (p >= p_lo && p < p_hi))
      {
        d = duc_load_pair(P, c, (int64_t)m_t - OFF + 2 * p);
      }
      uI[p] = (d & 0x00ff00ffu) << 8;
      uQ[p] = d & 0xff00ff00u;
    }
    __syncthreads();

    // 2. stage B and the amplitude: v index 4q + i
    const int amp = (int)ch.word;
    for (int q = tid; q < nq; q += kDucThreads)
    {
      int bI[4], bQ[4];
      const int s0 = 4 * q + delta;
      if (TB == 0)
      {
        const int16_t *u16I = (const int16_t *)uI, *u16Q = (const int16_t *)uQ;
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
          bI[i] = u16I[s0 + i];
          bQ[i] = u16Q[s0 + i];
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
        ddc_fir_any<4, 1>(s0 & 1, uI, uQ, s0 >> 1, P.JB, taps + kDucJA, bI, bQ);
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
          bI[i] = sat16(bI[i] >> 15);
          bQ[i] = sat16(bQ[i] >> 15);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; i++)
      {
        bI[i] = (bI[i] * amp + (1 << 14)) >> 15;
        bQ[i] = (bQ[i] * amp + (1 << 14)) >> 15;
      }
      vI[2 * q] = pack16(bI[0], bI[1]);
      vI[2 * q + 1] = pack16(bI[2], bI[3]);
      vQ[2 * q] = pack16(bQ[0], bQ[1]);
      vQ[2 * q + 1] = pack16(bQ[2], bQ[3]);
    }
    __syncthreads();

    // 3. stage A, mixer, sum: positions m, m + 1 of pair h (v indices m + LA, m + 1 + LA), outputs (m_t + m) R + i
    const uint32_t theta_call = bank_phase_at(ch, P.n0);
#pragma unroll
    for (int h = 0; h < 2; h++)
    {
      const int m = 2 * tid + (kDucTile / 2) * h;
      if (m >= cnt)
      {
        continue;
      }
      int aI[2 * R], aQ[2 * R];
      if (TA == 0)
      {
        const uint32_t dI = vI[(m + LA) >> 1], dQ = vQ[(m + LA) >> 1];   // LA = 0: m even, one dword
#pragma unroll
        for (int i = 0; i < 2 * R; i++)
        {
          aI[i] = (int)(int16_t)(i < R ? dI : dI >> 16);
          aQ[i] = (int)(int16_t)(i < R ? dQ : dQ >> 16);
        }
      }
      else
      {
#pragma unroll
        for (int i = 0; i < 2 * R; i++)
        {
          aI[i] = 1 << 14;
          aQ[i] = 1 << 14;
        }
        const uint32_t *rI = vI + (m >> 1), *rQ = vQ + (m >> 1);
        for (int t = 0; t < P.JA; t++)
        {
          const uint32_t wI = rI[t], wQ = rQ[t];
#pragma unroll
          for (int p = 0; p < R; p++)
          {
            const uint2 tt = taps[p * P.JA + t];
            aI[p] = dot2(wI, tt.x, aI[p]);
            aQ[p] = dot2(wQ, tt.x, aQ[p]);
            aI[R + p] = dot2(wI, tt.y, aI[R + p]);
            aQ[R + p] = dot2(wQ, tt.y, aQ[R + p]);
          }
        }
#pragma unroll
        for (int i = 0; i < 2 * R; i++)
        {
          aI[i] = sat16(aI[i] >> 15);
          aQ[i] = sat16(aQ[i] >> 15);
        }
      }
      uint32_t th = theta_call + (uint32_t)((m_t + m) * R) * ch.step;
#pragma unroll
      for (int i = 0; i < 2 * R; i++, th += ch.step)
      {
        const uint32_t k = ((th + (1u << 19)) >> 20) & 4095u;
        const uint32_t t = cs[k];                                        // (c, s)
        const uint32_t cns = (t & 0xffffu) | ((uint32_t)(-(int)(int16_t)(t >> 16)) << 16);   // (c, -s)
        const uint32_t sc = (t >> 16) | (t << 16);                       // (s, c)
        const uint32_t a = pack16(aI[i], aQ[i]);
        sI[h][i] += dot2(a, cns, 1 << 14) >> 15;                         // aI c - aQ s
        sQ[h][i] += dot2(a, sc, 1 << 14) >> 15;                          // aI s + aQ c
      }
    }
  }

  // output: sat8((S + r) >> s), 2 R samples (4 R bytes) per pair
  const int sh = (int)P.shift[w];
  const int r = sh ? 1 << (sh - 1) : 0;
  uint32_t clipped = 0;
#pragma unroll
  for (int h = 0; h < 2; h++)
  {
    const int m = 2 * tid + (kDucTile / 2) * h;
    if (m >= cnt)
    {
      continue;
    }
    const int n_out = R * min(2, cnt - m);                // outputs of the pair inside the call: 2 R, or R at its end
    uint32_t word[R];
#pragma unroll
    for (int i = 0; i < R; i++)
    {
      word[i] = 0u;
    }
#pragma unroll
    for (int i = 0; i < 2 * R; i++)
    {
      const int yi = (sI[h][i] + r) >> sh, yq = (sQ[h][i] + r) >> sh;
      const int oi = min(max(yi, -128), 127), oq = min(max(yq, -128), 127);
      clipped += (i < n_out) ? (uint32_t)(oi != yi) + (uint32_t)(oq != yq) : 0u;
      word[i >> 1] |= (((uint32_t)oi & 0xffu) | (((uint32_t)oq & 0xffu) << 8)) << (16 * (i & 1));
    }
    int8_t *dst = P.cap + (uint64_t)w * P.cap_stride + 2 * (uint64_t)(m_t + m) * R;
    const int nb = 2 * n_out;
    if (nb == 4 * R && ((uintptr_t)dst & 3u) == 0)
    {
#pragma unroll
      for (int i = 0; i < R; i++)
      {
        ((uint32_t *)dst)[i] = word[i];
      }
    }
    else
    {
      for (int k = 0; k < nb; k++)
      {
        dst[k] = (int8_t)(word[k >> 2] >> (8 * (k & 3)));
      }
    }
  }
  // clip count: a wave reduction, one LDS atomic per wave, one global atomic per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    clipped += __shfl_xor(clipped, o);
  }
  if ((tid & 63) == 0 && clipped != 0u)
  {
    atomicAdd(&clip_sum, clipped);
  }
  __syncthreads();
  if (tid == 0 && clip_sum != 0u)
  {
    atomicAdd(P.clips + w, (unsigned long long)clip_sum);
  }
  if (KEYED && tid == 0 && skip_sum != 0u)
  {
    atomicAdd(P.skips, (unsigned long long)skip_sum);
  }
}

template __global__ void k_duc<1, false>(const DucParams);
template __global__ void k_duc<2, false>(const DucParams);
template __global__ void k_duc<4, false>(const DucParams);
template __global__ void k_duc<8, false>(const DucParams);
template __global__ void k_duc<1, true>(const DucParams);
template __global__ void k_duc<2, true>(const DucParams);
template __global__ void k_duc<4, true>(const DucParams);
template __global__ void k_duc<8, true>(const DucParams);

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_duc
{
  hrfd::BankCore core;
  uint32_t n_captures = 0, n_channels = 0, R = 1;
  // pinned staging of the records, the channel lists, the shifts and the packed taps (uploads in stream order)
  hrfd::PinnedBuf<hrfd::BankTuning> h_stage_chan;
  hrfd::PinnedBuf<uint32_t> h_stage_u32;   // [W + 1] list offsets, [C] list, [W] shifts
  hrfd::PinnedBuf<uint2> h_stage_taps;

  // host records, under core.mu
  std::vector<hrfd::BankTuning> h_chan;
  std::vector<uint32_t> h_shift;
  std::vector<int16_t> tapsA, tapsB;
  bool dirty = true;
  uint64_t N = 0;                          // absolute wideband output-sample counter
  bool clear_history = true;               // also clears the clip counters and the count of skipped units
  uint32_t key_log2 = hrfd::kDucKeyDefaultLog2;   // the key block of the next keyed call

  hrfd::DevBuf<unsigned long long> d_skips;       // [1] units the keyed kernel skipped
  hrfd::DevBuf<uint8_t> d_key;                    // host-path staging of the key rows
  hrfd::DevBuf<hrfd::BankTuning> d_chan;
  hrfd::DevBuf<uint32_t> d_u32;
  hrfd::DevBuf<uint2> d_taps;
  hrfd::DevBuf<uint32_t> d_cs;
  hrfd::DevBuf<unsigned long long> d_clips;
  hrfd::DevBuf<int8_t> d_hist[2];
  int cur = 0;
  hrfd::DevBuf<int8_t> d_in, d_out, d_tx;  // host-path staging and hrfd_duc_transmit's buffer
};

extern "C" int hrfd_duc_create(uint32_t n_captures, uint32_t n_channels, uint32_t interpolation, int device, hrfd_duc **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  if (out == nullptr || n_captures == 0 || n_channels == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_create: need n_captures > 0, n_channels > 0 and a result pointer");
  }
  if (n_channels > kDucMaxChannels)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_create: at most %u channels (the int32 sums), got %u", kDucMaxChannels, n_channels);
  }
  BANK_TRY(bank_rate_ok("hrfd_duc_create", "interpolation", interpolation));
  if (n_captures > 65536)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_create: at most 65536 captures (got %u)", n_captures);
  }
  hrfd_duc *d = nullptr;
  BANK_TRY(bank_new("hrfd_duc_create", device, &d));
  d->n_captures = n_captures;
  d->n_channels = n_channels;
  d->R = interpolation;
  d->h_chan.assign(n_channels, BankTuning{0u, 0u, 0u, 32768u, 0ull});
  d->h_shift.assign(n_captures, 8u);
  switch (interpolation)
  {
  case 2: d->tapsA.assign(Q_DUC_A2, Q_DUC_A2 + N_DUC_A2); break;
  case 4: d->tapsA.assign(Q_DUC_A4, Q_DUC_A4 + N_DUC_A4); break;
  case 8: d->tapsA.assign(Q_DUC_A8, Q_DUC_A8 + N_DUC_A8); break;
  default: break;                          // R = 1: stage A holds
  }
  d->tapsB.assign(Q_DDC_B, Q_DDC_B + N_DDC_B);
  const size_t hist_bytes = (size_t)n_channels * kDucH * 2;
  const size_t n_u32 = 2 * (size_t)n_captures + 1 + n_channels;
  const size_t n_taps = kDucJA + kDucJB;
  const bool ok = d->d_chan.alloc(n_channels) && d->d_u32.alloc(n_u32) && d->d_taps.alloc(n_taps) &&
                  bank_upload_cos(d->d_cs) && d->d_clips.alloc(n_captures) && d->d_skips.alloc(1) && d->d_hist[0].alloc(hist_bytes) &&
                  d->d_hist[1].alloc(hist_bytes) && d->h_stage_chan.alloc(n_channels) && d->h_stage_u32.alloc(n_u32) &&
                  d->h_stage_taps.alloc(n_taps);
  if (!ok)
  {
    (void)hipGetLastError();
    bank_free(d);
    return fail(HRFD_ENOMEM, "hrfd_duc_create: device allocation failed");
  }
  *out = d;
  return HRFD_OK;
}

extern "C" int hrfd_duc_destroy(hrfd_duc *d)
{
  if (d != nullptr)
  {
    hrfd::bank_free(d);
  }
  return HRFD_OK;
}

extern "C" int hrfd_duc_reset(hrfd_duc *d) { return hrfd::tuned_reset(d, "hrfd_duc_reset"); }

extern "C" int hrfd_duc_set_tuning(hrfd_duc *d, uint32_t channel, uint32_t capture, uint32_t step)
{
  return hrfd::tuned_set_tuning(d, "hrfd_duc_set_tuning", channel, capture, step);
}

extern "C" int hrfd_duc_set_amplitude(hrfd_duc *d, uint32_t channel, uint32_t amplitude)
{
  if (amplitude > 32768u)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_set_amplitude: A must be 0..32768 (got %u)", amplitude);
  }
  return hrfd::tuned_set_word(d, "hrfd_duc_set_amplitude", channel, amplitude);
}

extern "C" int hrfd_duc_set_output_shift(hrfd_duc *d, uint32_t capture, uint32_t s)
{
  if (s > hrfd::kDucMaxShift)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_set_output_shift: s must be 0..%u (got %u)", hrfd::kDucMaxShift, s);
  }
  if (d == nullptr || (capture >= d->n_captures && capture != HRFD_ALL_CHANNELS))
  {
    return fail(HRFD_EINVAL, "hrfd_duc_set_output_shift: bad handle or capture");
  }
  std::lock_guard<std::mutex> g(d->core.mu);
  for (uint32_t w = 0; w < d->n_captures; w++)
  {
    if (capture == HRFD_ALL_CHANNELS || w == capture)
    {
      d->h_shift[w] = s;
    }
  }
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_duc_set_filter(hrfd_duc *d, int stage, const int16_t *taps, uint32_t n)
{
  if (stage != 0 && stage != 1)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_set_filter: stage must be 0 (A) or 1 (B) (got %d)", stage);
  }
  // the tap count, and stage B's sum, need no handle; stage A's bound is per polyphase branch of the handle's R
  BANK_TRY(hrfd::bank_tap_count_ok("hrfd_duc_set_filter", taps, n, stage == 0 ? hrfd::kDucMaxTA : hrfd::kDucMaxTB));
  if (stage == 1)
  {
    BANK_TRY(hrfd::bank_tap_sums_ok("hrfd_duc_set_filter", taps, n, 1u));
  }
  BANK_TRY(hrfd::bank_need_handle("hrfd_duc_set_filter", d));
  if (stage == 0)
  {
    BANK_TRY(hrfd::bank_tap_sums_ok("hrfd_duc_set_filter", taps, n, d->R));
  }
  std::lock_guard<std::mutex> g(d->core.mu);
  (stage == 0 ? d->tapsA : d->tapsB).assign(taps, taps + n);
  d->dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_duc_get_phase(hrfd_duc *d, uint32_t channel, uint32_t *theta)
{
  return hrfd::tuned_get_phase(d, "hrfd_duc_get_phase", channel, theta);
}

extern "C" int hrfd_duc_get_clips(hrfd_duc *d, uint32_t capture, uint64_t *n)
{
  if (d == nullptr || capture >= d->n_captures || n == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_duc_get_clips: bad handle, capture or NULL result");
  }
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
  unsigned long long v = 0;
  HIP_TRY(hipMemcpy(&v, d->d_clips + capture, sizeof(v), hipMemcpyDeviceToHost));
  *n = (uint64_t)v;
  return HRFD_OK;
}

extern "C" int hrfd_duc_set_key_block(hrfd_duc *d, uint32_t log2_samples)
{
  BANK_TRY(hrfd::duc_key_check_block("hrfd_duc_set_key_block", log2_samples));
  BANK_TRY(hrfd::bank_need_handle("hrfd_duc_set_key_block", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  d->key_log2 = log2_samples;              // a launch takes its own copy: the history is untouched
  return HRFD_OK;
}

extern "C" int hrfd_duc_n_keys(hrfd_duc *d, uint32_t in_bytes, uint32_t *n)
{
  BANK_TRY(hrfd::duc_key_check_result("hrfd_duc_n_keys", n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_duc_n_keys", d));
  std::lock_guard<std::mutex> g(d->core.mu);
  *n = hrfd::duc_key_n(in_bytes / 2u, d->key_log2);
  return HRFD_OK;
}

extern "C" int hrfd_duc_get_key_skips(hrfd_duc *d, uint64_t *n)
{
  BANK_TRY(hrfd::duc_key_check_result("hrfd_duc_get_key_skips", n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_duc_get_key_skips", d));
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
  unsigned long long v = 0;
  HIP_TRY(hipMemcpy(&v, d->d_skips, sizeof(v), hipMemcpyDeviceToHost));
  *n = (uint64_t)v;
  return HRFD_OK;
}

// the key block of a call that starts now: a setter on another thread lands before or behind it
static uint32_t duc_key_log2(hrfd_duc *d)
{
  std::lock_guard<std::mutex> g(d->core.mu);
  return d->key_log2;
}

// one launch over every capture on `s`: R * in_bytes per capture from in_bytes per channel; d_key NULL: the unkeyed kernel
static int duc_launch(hrfd_duc *d, const int8_t *d_channels, uint64_t channel_stride, uint32_t in_bytes, int8_t *d_captures,
                      uint64_t capture_stride, hipStream_t s, const uint8_t *d_key = nullptr, uint64_t key_stride = 0,
                      uint32_t key_log2 = hrfd::kDucKeyDefaultLog2)
{
  using namespace hrfd;
  BANK_TRY(d->core.order_behind_last(s));
  const uint32_t W = d->n_captures, C = d->n_channels;
  DucParams P;
  {
    std::lock_guard<std::mutex> g(d->core.mu);
    P.TA = (int)d->tapsA.size();
    P.TB = (int)d->tapsB.size();
    P.LA = bank_branch_lookback(P.TA, (int)d->R);
    P.JA = P.TA > 0 ? bank_packed_len(P.LA + 1) : 0;
    P.JB = bank_packed_len(P.TB);
    if (d->dirty || d->clear_history)
    {
      // records, channel lists, shifts, taps, a cleared history and cleared clip counters go to the device on `s`,
      // ahead of this launch
      BANK_TRY(d->core.staging_wait());
      memcpy(d->h_stage_chan, d->h_chan.data(), sizeof(BankTuning) * C);
      uint32_t *off = d->h_stage_u32, *list = off + W + 1, *shift = list + C;
      bank_channel_lists(d->h_chan.data(), C, W, off, list);
      memcpy(shift, d->h_shift.data(), sizeof(uint32_t) * W);
      memset(d->h_stage_taps, 0, sizeof(uint2) * (kDucJA + kDucJB));
      if (P.TA > 0)
      {
        bank_pack_branch_taps(d->tapsA.data(), P.TA, (int)d->R, d->h_stage_taps.p, P.JA);
      }
      bank_pack_taps(d->tapsB.data(), P.TB, d->h_stage_taps + kDucJA, P.JB);
      HIP_TRY(hipMemcpyAsync(d->d_chan, d->h_stage_chan, sizeof(BankTuning) * C, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d->d_u32, d->h_stage_u32, sizeof(uint32_t) * (2 * (size_t)W + 1 + C), hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d->d_taps, d->h_stage_taps, sizeof(uint2) * (kDucJA + kDucJB), hipMemcpyHostToDevice, s));
      BANK_TRY(d->core.staging_sent(s));
      if (d->clear_history)
      {
        HIP_TRY(hipMemsetAsync(d->d_hist[d->cur], 0, (size_t)C * kDucH * 2, s));
        HIP_TRY(hipMemsetAsync(d->d_clips, 0, sizeof(unsigned long long) * W, s));
        HIP_TRY(hipMemsetAsync(d->d_skips, 0, sizeof(unsigned long long), s));
        d->clear_history = false;
      }
      d->dirty = false;
    }
    P.n0 = d->N;
    d->N += (uint64_t)d->R * (in_bytes / 2u);   // under the same lock as the read: a setter sees N before or after
  }
  P.in = d_channels;
  P.in_stride = channel_stride;
  P.hist_in = d->d_hist[d->cur];
  P.hist_out = d->d_hist[d->cur ^ 1];
  P.cap = d_captures;
  P.cap_stride = capture_stride;
  P.chan = d->d_chan;
  P.list_off = d->d_u32;
  P.list = d->d_u32 + W + 1;
  P.shift = d->d_u32 + W + 1 + C;
  P.taps = d->d_taps;
  P.cs = d->d_cs;
  P.clips = d->d_clips;
  P.M = in_bytes / 2u;
  P.n_tiles = (P.M + kDucTile - 1) / kDucTile;
  P.n_channels = C;
  P.n_captures = W;
  P.key = d_key;
  P.key_stride = key_stride;
  P.key_log2 = key_log2;
  P.skips = d->d_skips;
  const dim3 grid(P.n_tiles * W + C);
  if (d_key == nullptr)
  {
    switch (d->R)
    {
    case 1: hipLaunchKernelGGL((k_duc<1, false>), grid, dim3(kDucThreads), 0, s, P); break;
    case 2: hipLaunchKernelGGL((k_duc<2, false>), grid, dim3(kDucThreads), 0, s, P); break;
    case 4: hipLaunchKernelGGL((k_duc<4, false>), grid, dim3(kDucThreads), 0, s, P); break;
    default: hipLaunchKernelGGL((k_duc<8, false>), grid, dim3(kDucThreads), 0, s, P); break;
    }
  }
  else
  {
    switch (d->R)
    {
    case 1: hipLaunchKernelGGL((k_duc<1, true>), grid, dim3(kDucThreads), 0, s, P); break;
    case 2: hipLaunchKernelGGL((k_duc<2, true>), grid, dim3(kDucThreads), 0, s, P); break;
    case 4: hipLaunchKernelGGL((k_duc<4, true>), grid, dim3(kDucThreads), 0, s, P); break;
    default: hipLaunchKernelGGL((k_duc<8, true>), grid, dim3(kDucThreads), 0, s, P); break;
    }
  }
  const int rc = bank_launch_ok("k_duc");
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

static int duc_check_call(hrfd_duc *d, const void *channels, uint64_t channel_stride, uint32_t in_bytes, const void *captures,
                          uint64_t capture_stride, const char *who)
{
  if (d == nullptr || channels == nullptr || captures == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return hrfd::bank_check_call(who, "in_bytes", in_bytes, channels, channel_stride, 1u, capture_stride, d->R, d->n_captures,
                               d->n_channels);
}

// The three entries, with and without a key (key NULL: the unkeyed call), under `who`.  The key's stride is checked against
// the largest key block first, which needs no handle, then against the handle's; *k is the block the launch uses
static int duc_check_keyed(hrfd_duc *d, const void *channels, uint64_t channel_stride, uint32_t in_bytes, const void *captures,
                           uint64_t capture_stride, const void *key, uint64_t key_stride, const char *who, uint32_t *k)
{
  BANK_TRY(hrfd::duc_key_check_stride(who, key, key_stride, in_bytes, hrfd::kDucKeyMaxLog2));
  BANK_TRY(duc_check_call(d, channels, channel_stride, in_bytes, captures, capture_stride, who));
  *k = duc_key_log2(d);
  return hrfd::duc_key_check_stride(who, key, key_stride, in_bytes, *k);
}

static int duc_process_device(hrfd_duc *d, const int8_t *d_channels, uint64_t channel_stride, uint32_t in_bytes,
                              const uint8_t *d_key, uint64_t key_stride, int8_t *d_captures, uint64_t capture_stride, void *stream,
                              const char *who)
{
  uint32_t k = 0;
  BANK_TRY(duc_check_keyed(d, d_channels, channel_stride, in_bytes, d_captures, capture_stride, d_key, key_stride, who, &k));
  HIP_TRY(hipSetDevice(d->core.device));
  return duc_launch(d, d_channels, channel_stride, in_bytes, d_captures, capture_stride, d->core.stream_or_own(stream), d_key,
                    key_stride, k);
}

static int duc_process(hrfd_duc *d, const int8_t *channels, uint32_t in_bytes, const uint8_t *key, int8_t *captures, const char *who)
{
  uint32_t k = 0;
  // the host entry's key is dense: rows of n_keys bytes
  BANK_TRY(duc_check_keyed(d, channels, in_bytes, in_bytes, captures, d ? (uint64_t)d->R * in_bytes : 0, nullptr, 0, who, &k));
  const uint32_t n_keys = hrfd::duc_key_n(in_bytes / 2u, k);
  hrfd::BankHostCall call(d->core);
  const size_t in_total = (size_t)d->n_channels * in_bytes, out_total = (size_t)d->n_captures * d->R * in_bytes;
  const int8_t *d_in = call.up(d->d_in, channels, in_total);
  const uint8_t *d_key = call.up(d->d_key, key, (size_t)d->n_channels * n_keys);
  int8_t *d_out = call.room(d->d_out, captures, out_total);
  BANK_TRY(call.rc);
  BANK_TRY(duc_launch(d, d_in, in_bytes, in_bytes, d_out, (uint64_t)d->R * in_bytes, call.st, d_key, n_keys, k));
  call.down(captures, d_out, out_total);
  return call.finish();
}

static int duc_transmit(hrfd_duc *d, hrfd_mod *mod, const int16_t *d_pcm, uint32_t n_per_channel, const uint8_t *d_key,
                        uint64_t key_stride, int8_t *d_captures, uint64_t capture_stride, void *stream, const char *who)
{
  if (mod == nullptr || d_pcm == nullptr || n_per_channel == 0 || n_per_channel > (1u << 16))
  {
    return fail(HRFD_EINVAL, "%s: NULL argument, or n_per_channel not in 1..65536 (got %u)", who, n_per_channel);
  }
  if (d != nullptr && mod->n_channels != d->n_channels)
  {
    return fail(HRFD_EINVAL, "%s: the modulator has %u channels, the DUC %u", who, mod->n_channels, d->n_channels);
  }
  const uint32_t in_bytes = 512u * n_per_channel;
  uint32_t k = 0;
  BANK_TRY(duc_check_keyed(d, d_pcm, in_bytes, in_bytes, d_captures, capture_stride, d_key, key_stride, who, &k));
  if (mod->core.device != d->core.device)
  {
    return fail(HRFD_EINVAL, "%s: the modulator lives on device %d, the DUC on %d", who, mod->core.device, d->core.device);
  }
  HIP_TRY(hipSetDevice(d->core.device));
  hipStream_t s = d->core.stream_or_own(stream);
  const size_t need = (size_t)d->n_channels * in_bytes;
  if (need > d->d_tx.cap)
  {
    HIP_TRY(hipStreamSynchronize(d->core.last_stream));  // the last launch may still read the old buffer
    BANK_TRY(d->d_tx.grow_bytes(need));
  }
  // the modulator overwrites the buffer the handle's last launch reads: behind it on the device.  It runs over every
  // channel, keyed or not: its state (FM phase, interpolator history) moves on under the key
  BANK_TRY(d->core.order_behind_last(s));
  BANK_TRY(hrfd_mod_process_device(mod, d_pcm, n_per_channel, d->d_tx, s));
  return duc_launch(d, d->d_tx, in_bytes, in_bytes, d_captures, capture_stride, s, d_key, key_stride, k);
}

extern "C" int hrfd_duc_process_device(hrfd_duc *d, const int8_t *d_channels, uint64_t channel_stride, uint32_t in_bytes,
                                       int8_t *d_captures, uint64_t capture_stride, void *stream)
{
  return duc_process_device(d, d_channels, channel_stride, in_bytes, nullptr, 0, d_captures, capture_stride, stream,
                            "hrfd_duc_process_device");
}

extern "C" int hrfd_duc_process_device_keyed(hrfd_duc *d, const int8_t *d_channels, uint64_t channel_stride, uint32_t in_bytes,
                                             const uint8_t *d_key, uint64_t key_stride, int8_t *d_captures,
                                             uint64_t capture_stride, void *stream)
{
  return duc_process_device(d, d_channels, channel_stride, in_bytes, d_key, key_stride, d_captures, capture_stride, stream,
                            "hrfd_duc_process_device_keyed");
}

extern "C" int hrfd_duc_process(hrfd_duc *d, const int8_t *channels, uint32_t in_bytes, int8_t *captures)
{
  return duc_process(d, channels, in_bytes, nullptr, captures, "hrfd_duc_process");
}

extern "C" int hrfd_duc_process_keyed(hrfd_duc *d, const int8_t *channels, uint32_t in_bytes, const uint8_t *key, int8_t *captures)
{
  return duc_process(d, channels, in_bytes, key, captures, "hrfd_duc_process_keyed");
}

extern "C" int hrfd_duc_transmit(hrfd_duc *d, hrfd_mod *mod, const int16_t *d_pcm, uint32_t n_per_channel,
                                 int8_t *d_captures, uint64_t capture_stride, void *stream)
{
  return duc_transmit(d, mod, d_pcm, n_per_channel, nullptr, 0, d_captures, capture_stride, stream, "hrfd_duc_transmit");
}

extern "C" int hrfd_duc_transmit_keyed(hrfd_duc *d, hrfd_mod *mod, const int16_t *d_pcm, uint32_t n_per_channel,
                                       const uint8_t *d_key, uint64_t key_stride, int8_t *d_captures, uint64_t capture_stride,
                                       void *stream)
{
  return duc_transmit(d, mod, d_pcm, n_per_channel, d_key, key_stride, d_captures, capture_stride, stream,
                      "hrfd_duc_transmit_keyed");
}

