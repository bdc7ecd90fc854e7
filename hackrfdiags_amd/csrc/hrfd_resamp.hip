// hackrfdiags_amd/csrc/hrfd_resamp.hip -- hrfd_resamp_*: a rational polyphase resampler by L / M over the PCM of C channels,
// between the library's 8 kS/s and the rates of sound cards, recorders and codecs.
//
// Rows of n_in int16 (and n_pcm) in, rows of n_out int16 out.  Exact integer arithmetic, contract in include/hrfd.h;
// tests/resamp_model.py restates it in numpy, hrfd_resamp.h holds the laws both sides of this file share.
//
// k_resamp: one workgroup of 256 threads per (channel, tile of kResampTile = 1024 consecutive outputs), 4 consecutive
// outputs per lane.
//   1. output j has q = d + j M, i = q div L, p = q mod L and sums the K taps of branch p over x[i - K + 1 .. i].  The
//      tile's inputs, from the first output's i - (K - 1) rounded down to an even sample up to the last output's i, go into
//      LDS as packed int16 pairs, zero behind each block's n_pcm and behind n_in; samples below 0 come from the handle's
//      history (the side of the ping-pong this call reads).  M <= 8 L bounds the span: at most 8184 + K samples, 4352 dwords
//   2. a lane takes (i, p) of its first output from one division and steps them by (M div L, M mod L) with a conditional
//      subtract.  A window that starts on an odd sample reads from the dword below it against the branch's taps packed one
//      sample up (bank_pack_branch_taps gives both packings): no LDS read is 2-byte aligned.  The taps lie in global memory
//      as [L][2][J4] dwords, J4 = the K / 2 + 1 pairs of a branch rounded up to whole 16 bytes, so a step is one
//      global_load_dwordx4 and four LDS dwords for four v_dot2_i32_i16; the rows stay in L2 (84 KB at most).
//      |acc| <= sum |h| x 32768 <= 65535 x 32768 < 2^31 - 2^13: int32 is exact at every partial sum, and for the rounding
//      constant on top
//   3. y = sat16((acc + 2^13) >> 14); 8 bytes per lane go out as dwords where they are 4-byte aligned, as halfwords where
//      they are not or the row ends inside them
//   4. the workgroup of the row's last tile writes the next history to the other side: the last 512 values of x, from the
//      row and, where n_in < 512, from the old history.  A call without outputs has one workgroup per channel that does
//      only this.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hrfd_resamp.h"

namespace hrfd {

constexpr int kResampThreads = 256;
constexpr int kResampPer = 4;                              // consecutive outputs of one lane
constexpr int kResampTile = kResampThreads * kResampPer;   // outputs of one workgroup
constexpr int kResampHistDw = kResampHist / 2;             // 256 dwords of history
constexpr int kResampMaxJ4 = (kResampMaxBranch / 2 + 1 + 3) / 4 * 4;      // 260
// the last window starts at most (kResampTile - 1) * 8 + 1 samples behind the first dword, and reads J4 dwords
constexpr int kResampXsDw = ((kResampTile - 1) * (int)kResampMaxDown + 1) / 2 + kResampMaxJ4;      // 4352
static_assert(kResampHistDw == kResampThreads, "one dword of the next history per thread");
static_assert(kResampXsDw * 4 < 18 * 1024, "the tile stays under 18 KB of LDS");

struct ResampParams
{
  const int16_t *pcm;                      // [C] rows of n_in samples, stride bytes apart, even address
  uint64_t stride;
  const uint32_t *n_pcm;                   // [C][n_in / 512] or NULL
  const uint32_t *hist_in;                 // [C][256] packed pairs
  uint32_t *hist_out;
  const uint8_t *reset;                    // [C]: non-zero = this channel starts from zeros; or NULL
  int16_t *out;                            // [C] rows, out_stride bytes apart, even address
  uint64_t out_stride;
  uint64_t first_wg;
  uint32_t n_in, n_out, tiles;             // tiles per channel, at least one
  uint32_t L, M, Mq, Mr;                   // M = Mq L + Mr
  uint32_t K, J4, d;
};

// samples s and s + 1 of one channel's x as a packed pair; s even, -512 <= s
__device__ __forceinline__ uint32_t resamp_pair(const ResampParams &P, const int16_t *row, const uint32_t *n_row, const uint32_t *hist,
                                                bool fresh, int32_t s)
{
  if (s < 0)
  {
    return fresh ? 0u : hist[(s + (int32_t)kResampHist) >> 1];
  }
  if ((uint32_t)s >= P.n_in)
  {
    return 0u;
  }
  const uint32_t pos = (uint32_t)s % kResampBlock, lim = pcm_block_limit(n_row, (uint32_t)s / kResampBlock);
  if (pos >= lim)
  {
    return 0u;
  }
  const bool two = pos + 1 < lim && (uint32_t)s + 1 < P.n_in;
  const int16_t *src = row + s;
  if (two && ((uintptr_t)src & 3u) == 0)
  {
    return *(const uint32_t *)src;
  }
  uint32_t v = (uint16_t)src[0];
  if (two)
  {
    v |= (uint32_t)(uint16_t)src[1] << 16;
  }
  return v;
}

// taps: [L][2][J4] dwords; a parameter of its own so that it can be __restrict__
__global__ __launch_bounds__(kResampThreads) void k_resamp(const ResampParams P, const uint32_t *__restrict__ taps)
{
  __shared__ uint32_t xs[kResampXsDw];
  const uint32_t tid = threadIdx.x;
  const uint64_t wg = P.first_wg + blockIdx.x;
  const uint32_t c = (uint32_t)(wg / P.tiles), tile = (uint32_t)(wg - (uint64_t)c * P.tiles);
  const uint32_t j0 = tile * kResampTile;
  const uint32_t nj = min((uint32_t)kResampTile, P.n_out - j0);       // 0 in the one tile of a call without outputs
  const int16_t *row = (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride);
  const uint32_t *n_row = P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * (P.n_in / kResampBlock) : nullptr;
  const uint32_t *hist = P.hist_in + (uint64_t)c * kResampHistDw;
  const bool fresh = P.reset != nullptr && P.reset[c] != 0;

  // 4. the row's last tile leaves the handle's next history: samples n_in - 512 .. n_in - 1
  if (tile + 1 == P.tiles)
  {
    const int32_t s = (int32_t)P.n_in - (int32_t)kResampHist + 2 * (int32_t)tid, even = s & ~1;
    uint32_t v = resamp_pair(P, row, n_row, hist, fresh, even);
    if (s & 1)
    {
      v = (v >> 16) | (resamp_pair(P, row, n_row, hist, fresh, even + 2) << 16);
    }
    P.hist_out[(uint64_t)c * kResampHistDw + tid] = v;
  }
  if (nj == 0)
  {
    return;
  }

  // 1. the samples: dword idx holds samples base + 2 idx and base + 2 idx + 1
  const uint32_t q0 = P.d + j0 * P.M, i0 = q0 / P.L, ie = (q0 + (nj - 1) * P.M) / P.L;
  const int32_t base = ((int32_t)i0 - (int32_t)(P.K - 1)) & ~1;
  const uint32_t nd = min((uint32_t)kResampXsDw, (uint32_t)(((int32_t)ie - (int32_t)(P.K - 1) - base) >> 1) + P.J4);
  for (uint32_t idx = tid; idx < nd; idx += kResampThreads)
  {
    xs[idx] = resamp_pair(P, row, n_row, hist, fresh, base + 2 * (int32_t)idx);
  }
  __syncthreads();

  // 2. the filter
  const uint32_t o = tid * kResampPer;                     // the lane's first output, counted from the tile's start
  if (o >= nj)
  {
    return;
  }
  const uint32_t q = q0 + o * P.M;
  uint32_t i = q / P.L, p = q - i * P.L;
  int32_t y[kResampPer];
#pragma unroll
  for (int t = 0; t < kResampPer; t++)
  {
    y[t] = 0;
    if (o + t < nj)
    {
      const uint32_t w = (uint32_t)((int32_t)i - (int32_t)(P.K - 1) - base);       // >= 0: i >= i0
      const uint32_t *win = xs + (w >> 1);
      const uint32_t *tp = taps + (uint64_t)(2u * p + (w & 1u)) * P.J4;
      int acc = 0;
      for (uint32_t jb = 0; jb < P.J4; jb += 4)
      {
        const uint4 tv = *(const uint4 *)(tp + jb);
        acc = dot2(win[jb], tv.x, acc);
        acc = dot2(win[jb + 1], tv.y, acc);
        acc = dot2(win[jb + 2], tv.z, acc);
        acc = dot2(win[jb + 3], tv.w, acc);
      }
      y[t] = pcm_fir_round(acc);
      i += P.Mq;
      p += P.Mr;
      if (p >= P.L)
      {
        p -= P.L;
        i++;
      }
    }
  }

  // 3. store
  int16_t *dst = (int16_t *)((char *)P.out + (uint64_t)c * P.out_stride) + j0 + o;
  if (o + kResampPer <= nj && ((uintptr_t)dst & 3u) == 0)
  {
    ((uint32_t *)dst)[0] = ((uint32_t)y[0] & 0xffffu) | ((uint32_t)y[1] << 16);
    ((uint32_t *)dst)[1] = ((uint32_t)y[2] & 0xffffu) | ((uint32_t)y[3] << 16);
  }
  else
  {
#pragma unroll
    for (int t = 0; t < kResampPer; t++)
    {
      if (o + t < nj)
      {
        dst[t] = (int16_t)y[t];
      }
    }
  }
}

// the pairs of one branch, in whole 16 bytes
static inline uint32_t resamp_j4(uint32_t K) { return ((uint32_t)bank_packed_len((int)K) + 3u) / 4u * 4u; }

// the most dwords the taps of a handle with L branches can take: K <= 512 and K <= ceil(16384 / L)
static inline size_t resamp_taps_dw(uint32_t L)
{
  return (size_t)L * 2 * resamp_j4(std::min(kResampMaxBranch, resamp_branch_taps(kResampMaxTaps, L)));
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
static_assert(hrfd::kResampHistDw == hrfd::BankHistory::kDw, "k_resamp reads and writes the core's history rows");

struct hrfd_resamp
{
  hrfd::BankCore core;
  uint32_t n_channels = 0, L = 1, M = 1;

  // host settings, under core.mu
  std::vector<int16_t> taps;               // empty = none set yet
  bool taps_dirty = true;
  uint32_t d = 0;                          // the phase of the next call's first output, 0..M-1
  hrfd::BankHistory hist;

  // pinned staging: the packed taps, then the fresh flags
  hrfd::PinnedBuf<uint8_t> h_stage;
  size_t off_fresh = 0;
  hrfd::DevBuf<uint32_t> d_taps;           // [L][2][J4]

  // host-path staging
  hrfd::DevBuf<int16_t> d_pcm, d_out;
  hrfd::DevBuf<uint32_t> d_n_pcm;
};

extern "C" int hrfd_resamp_create(uint32_t n_channels, uint32_t up, uint32_t down, int device, hrfd_resamp **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(resamp_check_create("hrfd_resamp_create", n_channels, up, down, out));
  hrfd_resamp *r = nullptr;
  BANK_TRY(bank_new("hrfd_resamp_create", device, &r));
  const size_t C = n_channels;
  r->n_channels = n_channels;
  r->L = up;
  r->M = down;
  if (up == 1 && down == 1)
  {
    r->taps.assign(1, (int16_t)16384);
  }
  r->off_fresh = 4 * resamp_taps_dw(up);
  if (!(r->d_taps.alloc(resamp_taps_dw(up)) && r->hist.alloc(C) && r->h_stage.alloc(r->off_fresh + C)))
  {
    (void)hipGetLastError();
    bank_free(r);
    return fail(HRFD_ENOMEM, "hrfd_resamp_create: device allocation failed");
  }
  *out = r;
  return HRFD_OK;
}

extern "C" int hrfd_resamp_destroy(hrfd_resamp *r)
{
  if (r != nullptr)
  {
    hrfd::bank_free(r);
  }
  return HRFD_OK;
}

// under core.mu: a reset of all channels also takes the phase back to 0
static void resamp_mark_fresh(hrfd_resamp *r, uint32_t channel)
{
  r->hist.mark(channel);
  if (channel == HRFD_ALL_CHANNELS)
  {
    r->d = 0;
  }
}

extern "C" int hrfd_resamp_set_taps(hrfd_resamp *r, const int16_t *taps, uint32_t n)
{
  BANK_TRY(hrfd::resamp_check_tap_list("hrfd_resamp_set_taps", taps, n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_resamp_set_taps", r));
  BANK_TRY(hrfd::resamp_check_taps("hrfd_resamp_set_taps", taps, n, r->L));
  std::lock_guard<std::mutex> g(r->core.mu);
  r->taps.assign(taps, taps + n);
  r->taps_dirty = true;
  resamp_mark_fresh(r, HRFD_ALL_CHANNELS);
  return HRFD_OK;
}

extern "C" int hrfd_resamp_reset(hrfd_resamp *r, uint32_t channel)
{
  BANK_TRY(hrfd::pcm_check_channel("hrfd_resamp_reset", channel, 65536));
  BANK_TRY(hrfd::bank_need_handle("hrfd_resamp_reset", r));
  BANK_TRY(hrfd::pcm_check_channel("hrfd_resamp_reset", channel, r->n_channels));
  std::lock_guard<std::mutex> g(r->core.mu);
  resamp_mark_fresh(r, channel);
  return HRFD_OK;
}

// test hook: the workgroups of one launch of k_resamp, 1 .. 2^22 (2^22 unless set)
extern "C" int hrfd_resamp_debug_set_max_wgs(hrfd_resamp *r, uint32_t n)
{
  HRFD_HOOK_GATE("hrfd_resamp_debug_set_max_wgs");
  return hrfd::bank_set_max_wgs("hrfd_resamp_debug_set_max_wgs", r, n);
}

extern "C" int hrfd_resamp_out_count(hrfd_resamp *r, uint32_t n_in, uint32_t *n_out)
{
  using namespace hrfd;
  BANK_TRY(resamp_check_n_in("hrfd_resamp_out_count", n_in));
  if (n_out == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_resamp_out_count: NULL argument");
  }
  BANK_TRY(hrfd::bank_need_handle("hrfd_resamp_out_count", r));
  BANK_TRY(resamp_check_span("hrfd_resamp_out_count", n_in, r->L));
  std::lock_guard<std::mutex> g(r->core.mu);
  *n_out = resamp_out_count(n_in, r->L, r->M, r->d);
  return HRFD_OK;
}

static int resamp_check_process(hrfd_resamp *r, const char *who, const void *pcm, uint64_t stride, bool device_entry, const void *n_pcm,
                                uint32_t n_in, const void *out, uint64_t out_stride, uint32_t out_capacity, const void *n_out)
{
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text
  BANK_TRY(hrfd::resamp_check_call(who, pcm, stride, device_entry, n_pcm, n_in, out, out_stride, out_capacity, n_out, 1));
  BANK_TRY(hrfd::bank_need_handle(who, r));
  BANK_TRY(hrfd::resamp_check_call(who, pcm, stride, device_entry, n_pcm, n_in, out, out_stride, out_capacity, n_out, r->n_channels));
  BANK_TRY(hrfd::resamp_check_span(who, n_in, r->L));
  // before a buffer grows or a copy starts; resamp_launch looks again under the lock that moves d
  std::lock_guard<std::mutex> g(r->core.mu);
  if (r->taps.empty())
  {
    return fail(HRFD_ESTATE, "%s: no taps yet: a handle with up x down > 1 has no default, call hrfd_resamp_set_taps first", who);
  }
  return hrfd::resamp_check_capacity(who, hrfd::resamp_out_count(n_in, r->L, r->M, r->d), out_capacity);
}

// under core.mu, between staging_wait and staging_sent: branch p's K taps packed for both parities, [L][2][J4]
static void resamp_stage_taps(hrfd_resamp *r, uint32_t K, uint32_t J4)
{
  using namespace hrfd;
  const int J = bank_packed_len((int)K);
  std::vector<uint2> pairs((size_t)r->L * J);
  bank_pack_branch_taps(r->taps.data(), (int)r->taps.size(), (int)r->L, pairs.data(), J);
  uint32_t *dst = (uint32_t *)r->h_stage.p;
  memset(dst, 0, 4 * (size_t)r->L * 2 * J4);
  for (uint32_t p = 0; p < r->L; p++)
  {
    for (int j = 0; j < J; j++)
    {
      dst[(size_t)(2 * p) * J4 + j] = pairs[(size_t)p * J + j].x;
      dst[(size_t)(2 * p + 1) * J4 + j] = pairs[(size_t)p * J + j].y;
    }
  }
}

// one call on `st`: what the setters changed, then k_resamp over every tile; *n_out and the handle's d move only once
// nothing can be refused any more
static int resamp_launch(hrfd_resamp *r, const char *who, const int16_t *d_pcm, uint64_t stride, const uint32_t *d_n_pcm, uint32_t n_in,
                         int16_t *d_out, uint64_t out_stride, uint32_t out_capacity, bool dense_out, uint32_t *n_out, hipStream_t st)
{
  using namespace hrfd;
  ResampParams P;
  {
    std::lock_guard<std::mutex> g(r->core.mu);
    if (r->taps.empty())
    {
      return fail(HRFD_ESTATE, "%s: no taps yet: a handle with up x down > 1 has no default, call hrfd_resamp_set_taps first", who);
    }
    P.n_out = resamp_out_count(n_in, r->L, r->M, r->d);
    BANK_TRY(resamp_check_capacity(who, P.n_out, out_capacity));
    BANK_TRY(r->core.order_behind_last(st));
    P.K = resamp_branch_taps((uint32_t)r->taps.size(), r->L);
    P.J4 = resamp_j4(P.K);
    P.reset = r->hist.reset();
    P.hist_in = r->hist.in();
    P.hist_out = r->hist.out();
    if (r->taps_dirty || r->hist.any_fresh)
    {
      BANK_TRY(r->core.staging_wait());
      if (r->taps_dirty)
      {
        resamp_stage_taps(r, P.K, P.J4);
        HIP_TRY(hipMemcpyAsync(r->d_taps, r->h_stage, 4 * (size_t)r->L * 2 * P.J4, hipMemcpyHostToDevice, st));
      }
      BANK_TRY(r->hist.upload(r->h_stage + r->off_fresh, st));
      r->taps_dirty = false;
      BANK_TRY(r->core.staging_sent(st));
    }
    P.d = r->d;
    r->d = resamp_advance(r->d, n_in, P.n_out, r->L, r->M);
    r->hist.flip();
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.n_pcm = d_n_pcm;
  P.out = d_out;
  P.out_stride = dense_out ? 2ull * P.n_out : out_stride;
  P.n_in = n_in;
  P.tiles = std::max(1u, (P.n_out + kResampTile - 1) / kResampTile);
  P.L = r->L;
  P.M = r->M;
  P.Mq = r->M / r->L;
  P.Mr = r->M % r->L;
  BANK_TRY(bank_launch_chunked("k_resamp", r->core, (uint64_t)r->n_channels * P.tiles, P, [&](dim3 grid) {
    hipLaunchKernelGGL(k_resamp, grid, dim3(kResampThreads), 0, st, P, (const uint32_t *)r->d_taps.p);
  }));
  r->core.launched_on(st);
  *n_out = P.n_out;
  return HRFD_OK;
}

extern "C" int hrfd_resamp_process_device(hrfd_resamp *r, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                                          uint32_t n_in, int16_t *d_out, uint64_t out_stride_bytes, uint32_t out_capacity,
                                          uint32_t *n_out, void *stream)
{
  const char *who = "hrfd_resamp_process_device";
  BANK_TRY(resamp_check_process(r, who, d_pcm, channel_stride_bytes, true, d_n_pcm, n_in, d_out, out_stride_bytes, out_capacity, n_out));
  HIP_TRY(hipSetDevice(r->core.device));
  return resamp_launch(r, who, d_pcm, channel_stride_bytes, d_n_pcm, n_in, d_out, out_stride_bytes, out_capacity, false, n_out,
                       r->core.stream_or_own(stream));
}

extern "C" int hrfd_resamp_process(hrfd_resamp *r, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_in, int16_t *out,
                                   uint32_t out_capacity, uint32_t *n_out)
{
  using namespace hrfd;
  const char *who = "hrfd_resamp_process";
  BANK_TRY(resamp_check_process(r, who, pcm, 0, false, n_pcm, n_in, out, 0, out_capacity, n_out));
  BankHostCall call(r->core);
  const size_t C = r->n_channels, row = 2 * (size_t)n_in;
  const int16_t *d_pcm = call.up(r->d_pcm, pcm, row * C);
  const uint32_t *d_n_pcm = call.up(r->d_n_pcm, n_pcm, 4 * C * (n_in / kResampBlock));
  int16_t *d_out = call.room(r->d_out, out, std::max<size_t>(16, 2 * (size_t)out_capacity * C));
  BANK_TRY(call.rc);
  uint32_t n = 0;
  // the device rows are dense at n_out, the caller's out_capacity samples apart: a strided copy of its own brings them back
  BANK_TRY(resamp_launch(r, who, d_pcm, row, d_n_pcm, n_in, d_out, 0, out_capacity, true, &n, call.st));
  if (n != 0)
  {
    HIP_TRY(hipMemcpy2DAsync(out, 2 * (size_t)out_capacity, d_out, 2 * (size_t)n, 2 * (size_t)n, C, hipMemcpyDeviceToHost, call.st));
  }
  BANK_TRY(call.finish());
  *n_out = n;
  return HRFD_OK;
}
