// hackrfdiags_amd/csrc/hrfd_dcsgen.hip -- hrfd_dcsgen_*: digital coded squelch keyed onto the transmit chain's PCM: the 23-bit
// word of a code sent cyclically at 134.4 bit/s, the 134.4 Hz turn-off code behind it, both through one shaping filter, queued
// per channel as segments and added to the PCM rows the modulators and the DUC read.  The mirror of the DCS bank.
//
// PCM rows [C][n_blocks][512] int16 in (or none: generate only), the same rows with the code added out, clips per channel
// and, optionally, whether anything sounds in every block.  Exact integer arithmetic, contract in include/hrfd.h;
// tests/dcsgen_model.py restates it in numpy, hrfd_gen.h and hrfd_dcsgen.h hold the laws and the queue rules both sides of
// this file share.  The clock, the clip counters and the process entries are GenCore's (hrfd_bank.hip); the queues, their
// copy on the device, the taps and the launch are this file's.
//
// The handle keeps the queues on the host (at most 8 segments per channel, absolute stream times) and a copy on the device:
// 8 slots of 32 bytes per channel, the unused ones empty.  The kernel is given the stream time N of the call's first sample
// and N mod 28750 as parameters, so the copy changes only where a setter changed a queue or a call dropped segments that
// have ended; only those channels are staged again.  The raw level r[n] is computed from n and the slots, never carried: the
// output at stream time n is a pure function of n, the slots, the taps and x, and tiles are independent.
//
// k_dcsgen: k_tonegen's shape: 256 threads, 8 consecutive samples (16 bytes) per lane, tiles of 2048 samples (4 blocks); grid
// (C, gy), the workgroups of a row stride over its tiles.
//   1. lane j < 8 of every wave holds slot j's start and end.  Per tile a ballot against [n0 - 511, n0 + 2048) says whether
//      the tile has anything to do: every wave computes the same mask from its own registers.  If not, the tile is a copy (out
//      of place), zeros (generate only) or nothing at all (in place), and the taps are never loaded
//   2. else the lanes write r for the tile's 2048 samples and the 512 in front of them into LDS as packed int16 pairs in
//      k_audio_fir's layout: a lane has dwords tid, tid + 256, ..: it reduces its first u = n mod 28750 in 32 bits once and
//      steps it by 512 with a conditional subtract; per sample the bit index and the turn-off half are found once, then the
//      hits (usually one) give the level from offsets clamped into 32 bits
//   3. the filter is k_audio_fir's: audio_fir_run, taps through the scalar cache, three ds_read_b128 and 64 v_dot2_i32_i16 a
//      step; g = (acc + 2^13) >> 14
//   4. y = sat16(x + g), 16 bytes per lane out; clipped samples are counted per lane, summed over the wave by shuffles behind
//      the last tile, and added to clips[c] with one vector atomic per wave that has any
//   5. active: wave w of a tile tests the slots against block w of the tile and the filter's reach, lane 0 writes the byte
// Two barriers a busy tile, none an idle one.  In place: every sample is loaded once, by the lane that stores it.  Rows at
// any even address and stride take one path through a vector type of alignment 2 (pcm_load8, pcm_store8).
// The grid is at most 65536 x 64 = 2^22 workgroups = kBankMaxWgs: the launch is never cut (no first_wg, no max_wgs hook).
// No float; every result leaves through a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hrfd_dcsgen.h"

namespace hrfd {

constexpr int kDcsgenThreads = 256;
constexpr int kDcsgenPer = 8;                              // consecutive samples of one lane: 16 bytes
constexpr int kDcsgenTile = kDcsgenThreads * kDcsgenPer;   // 2048 samples
constexpr int kDcsgenTileBlocks = kDcsgenTile / (int)kGenBlock;      // 4: one per wave
constexpr int kDcsgenHistDw = (int)kGenBlock / 2;          // 256 dwords in front of the tile
constexpr int kDcsgenXsDw = 4 + (kDcsgenTileBlocks + 1) * kDcsgenHistDw + 12;     // k_audio_fir's: offset, history, tile, the last step's reach
constexpr int kDcsgenFillDw = (kDcsgenTileBlocks + 1) * kDcsgenHistDw;            // the dwords that hold r; zeros behind them
constexpr uint32_t kDcsgenMaxGridY = 64;
constexpr uint32_t kDcsgenAimWgs = 2048;                   // workgroups a launch aims for before a workgroup takes a second tile
constexpr uint32_t kDcsgenStageChannels = 1024;            // channels of one upload from the pinned staging buffer
constexpr int32_t kDcsgenClamp = 1 << 20;                  // offsets beyond this are as good as infinite: a tile spans 2560
static_assert(kDcsgenTileBlocks == kAudioRun && kDcsgenPer == kAudioPer && kDcsgenThreads == kAudioThreads &&
                  kDcsgenMaxTaps == kAudioMaxTaps && kDcsgenXsDw == kAudioXsDw && kDcsgenHistDw == kAudioHistDw,
              "stage 2 is k_audio_fir's layout and stage 3 audio_fir_run");
static_assert(kDcsgenTileBlocks == kDcsgenThreads / 64, "one wave per block of a tile");
static_assert(kDcsgenMaxSegments <= 64, "one slot per lane of a wave");
static_assert(kDcsgenFillDw % kDcsgenThreads == 0 && kDcsgenXsDw - kDcsgenFillDw <= kDcsgenThreads, "the fill loop's shape");
static_assert(2 * kDcsgenHistDw >= (int)kDcsgenReach + 1 && 2 * kDcsgenHistDw < (int)kDcsgenPeriod, "the samples in front of a tile");
static_assert(16 * ((kDcsgenXsDw + 3) / 4) + 32 * (int)kDcsgenMaxSegments <= 8192, "LDS: under 8 KiB a workgroup");
static_assert(65536ull * kDcsgenMaxGridY <= kBankMaxWgs, "the grid is one launch");

struct DcsgenParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address; or NULL
  uint64_t stride;
  int16_t *out;                            // [C] rows, out_stride bytes apart, even address; may be pcm itself
  uint64_t out_stride;
  const DcsgenSlot *slots;                 // [C][8]
  unsigned long long *clips;               // [C]
  uint8_t *active;                         // [C][n_blocks] or NULL
  uint64_t N;                              // the stream time of the call's first sample
  uint32_t Nu;                             // N mod 28750
  uint32_t n_blocks, T, J;
};

// a stream time as an offset from the first sample in LDS, n0 - 512 (which may lie in front of time 0): t - n0 + 512 where
// that lies within 2^20 of 512, and as good as infinite beyond
__device__ __forceinline__ int32_t dcsgen_offset(uint64_t t, uint64_t n0)
{
  if (t >= n0)
  {
    const uint64_t d = t - n0;             // kDcsgenNoEnd lands here
    return d >= (uint64_t)kDcsgenClamp ? kDcsgenClamp : (int32_t)d + 2 * kDcsgenHistDw;
  }
  const uint64_t d = n0 - t;
  return d >= (uint64_t)kDcsgenClamp ? -kDcsgenClamp : 2 * kDcsgenHistDw - (int32_t)d;
}

// taps: [P.J] (even, odd) pairs, J a multiple of kAudioStep; a parameter of its own so that it can be __restrict__ and come
// through the scalar cache
__global__ __launch_bounds__(kDcsgenThreads) void k_dcsgen(const DcsgenParams P, const uint2 *__restrict__ taps)
{
  __shared__ audio_u4 xs4[(kDcsgenXsDw + 3) / 4];
  __shared__ DcsgenSlot slot[kDcsgenMaxSegments];
  uint32_t *xs = (uint32_t *)xs4;
  const uint32_t tid = threadIdx.x, c = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = P.n_blocks * kGenBlock;
  const uint32_t par = (P.T - 1) & 1u, lead = (kGenBlock + 1 - P.T - par) / 2, pad = (4u - (lead & 3u)) & 3u;
  const int16_t *row = P.pcm != nullptr ? (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride) : nullptr;
  int16_t *orow = (int16_t *)((char *)P.out + (uint64_t)c * P.out_stride);
  const bool in_place = (const int16_t *)orow == row;
  const DcsgenSlot *mine = P.slots + (uint64_t)c * kDcsgenMaxSegments;

  // 1. lane j of every wave: slot j's start and end; the other lanes hold an empty slot
  const uint64_t s_start = lane < kDcsgenMaxSegments ? mine[lane].start : kDcsgenEmptySlot.start;
  const uint64_t s_end = lane < kDcsgenMaxSegments ? mine[lane].end : kDcsgenEmptySlot.end;
  const bool s_open = s_end == kDcsgenNoEnd;
  const bool row_busy = __ballot(s_start < P.N + n && (s_open || s_end + kDcsgenReach > P.N)) != 0ull;      // the same in every wave
  if (row_busy)
  {
    if (tid < kDcsgenMaxSegments)
    {
      slot[tid] = mine[tid];
    }
    __syncthreads();
  }

  uint32_t clipped = 0;
  for (uint32_t t0 = blockIdx.y * kDcsgenTile; t0 < n; t0 += gridDim.y * kDcsgenTile)
  {
    const uint64_t n0 = P.N + t0;                          // the tile's first stream time
    const uint32_t at = t0 + tid * kDcsgenPer;             // the lane's first sample
    const bool live = at < n;                              // n is whole blocks: a lane has all of its samples or none
    // the hit list: the segments that meet [n0 - 511, n0 + 2048)
    uint32_t hits = row_busy ? (uint32_t)__ballot(s_start < n0 + kDcsgenTile && (s_open || s_end + kDcsgenReach > n0)) : 0u;
    if (P.active != nullptr)
    {
      // 5. wave w: block w of the tile against [S, E + T - 1)
      const uint64_t b0 = n0 + wave * kGenBlock;
      const uint64_t m = row_busy ? __ballot(s_start < b0 + kGenBlock && (s_open || s_end + (P.T - 1) > b0)) : 0ull;
      const uint32_t b = t0 / kGenBlock + wave;
      if (lane == 0 && b < P.n_blocks)
      {
        P.active[(uint64_t)c * P.n_blocks + b] = m != 0ull ? 1 : 0;
      }
    }
    if (hits == 0u)
    {
      // an idle tile: a copy, zeros, or nothing at all (no barrier on this path; hits is the same in every wave)
      if (live && !in_place)
      {
        pcm_u4 cur = {0u, 0u, 0u, 0u};
        if (row != nullptr)
        {
          cur = pcm_load8(row + at);
        }
        pcm_store8(orow + at, cur);
      }
      continue;
    }

    // 2. r into LDS: dword idx holds the stream times n0 - 512 + 2 idx and the one behind it
    uint32_t u = (P.Nu + t0 + (kDcsgenPeriod - 2 * kDcsgenHistDw) + 2 * tid) % kDcsgenPeriod;      // below 2^20 in front of the division
    uint32_t code[2 * kDcsgenFillDw / kDcsgenThreads];     // per sample: the bit index, and 32 for the turn-off code's low half
    int32_t r[2 * kDcsgenFillDw / kDcsgenThreads];
#pragma unroll
    for (int k = 0; k < kDcsgenFillDw / kDcsgenThreads; k++)
    {
      const uint32_t u1 = u + 1 == kDcsgenPeriod ? 0u : u + 1;
      code[2 * k] = dcsgen_bit_index(u) | (dcsgen_sq_low(u) ? 32u : 0u);
      code[2 * k + 1] = dcsgen_bit_index(u1) | (dcsgen_sq_low(u1) ? 32u : 0u);
      r[2 * k] = r[2 * k + 1] = 0;
      u += 2 * kDcsgenThreads;
      u = u >= kDcsgenPeriod ? u - kDcsgenPeriod : u;
    }
    while (hits != 0u)
    {
      const uint32_t j = (uint32_t)__builtin_ctz(hits);
      hits &= hits - 1u;
      const DcsgenSlot s = slot[j];
      const int32_t o_start = dcsgen_offset(s.start, n0), o_mid = dcsgen_offset(s.mid, n0), o_end = dcsgen_offset(s.end, n0);
      const int32_t a = (int32_t)s.amp;
#pragma unroll
      for (int k = 0; k < kDcsgenFillDw / kDcsgenThreads; k++)
      {
#pragma unroll
        for (int h = 0; h < 2; h++)
        {
          const int32_t p = 2 * (int32_t)(tid + k * kDcsgenThreads) + h;
          const uint32_t cd = code[2 * k + h];
          const bool high = p < o_mid ? ((s.word >> (cd & 31u)) & 1u) != 0 : (cd & 32u) == 0;
          r[2 * k + h] += p >= o_start && p < o_end ? (high ? a : -a) : 0;      // segments never overlap: at most one adds
        }
      }
    }
    __syncthreads();                                       // the tile before has been read
#pragma unroll
    for (int k = 0; k < kDcsgenFillDw / kDcsgenThreads; k++)
    {
      xs[pad + tid + k * kDcsgenThreads] = ((uint32_t)r[2 * k] & 0xffffu) | ((uint32_t)r[2 * k + 1] << 16);
    }
    if (tid < (uint32_t)(kDcsgenXsDw - kDcsgenFillDw) - pad)
    {
      xs[pad + kDcsgenFillDw + tid] = 0u;                  // what the last step reads over
    }
    __syncthreads();
    if (!live)
    {
      continue;                                            // (the barriers above are behind every lane)
    }

    // 3. the filter
    int acc[kDcsgenPer];
#pragma unroll
    for (int i = 0; i < kDcsgenPer; i++)
    {
      acc[i] = 0;
    }
    const audio_u4 *win = xs4 + (pad + lead + tid * kDcsgenPer / 2) / 4;      // 16-byte aligned by the choice of pad
    if (par)
    {
      audio_fir_run<1>(win, taps, P.J, acc);
    }
    else
    {
      audio_fir_run<0>(win, taps, P.J, acc);
    }

    // 4. the output
    pcm_u4 cur = {0u, 0u, 0u, 0u};
    if (row != nullptr)
    {
      cur = pcm_load8(row + at);
    }
    const uint32_t d[4] = {cur.x, cur.y, cur.z, cur.w};
    uint32_t y[kDcsgenPer];
#pragma unroll
    for (int i = 0; i < kDcsgenPer; i++)
    {
      const int32_t x = (i & 1) ? (int32_t)d[i / 2] >> 16 : (int32_t)(int16_t)d[i / 2];
      bool clip;
      y[i] = (uint32_t)gen_output(x, dcsgen_round(acc[i]), &clip);
      clipped += clip ? 1u : 0u;
    }
    pcm_u4 v;
    v.x = (y[0] & 0xffffu) | (y[1] << 16);
    v.y = (y[2] & 0xffffu) | (y[3] << 16);
    v.z = (y[4] & 0xffffu) | (y[5] << 16);
    v.w = (y[6] & 0xffffu) | (y[7] << 16);
    pcm_store8(orow + at, v);
  }

  if (__ballot(clipped != 0u) != 0ull)
  {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
    {
      clipped += (uint32_t)__shfl_xor((int)clipped, m);
    }
    if (lane == 0)
    {
      atomicAdd(P.clips + c, (unsigned long long)clipped);
    }
  }
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_dcsgen
{
  hrfd::BankCore core;
  hrfd::GenCore gen;                       // the clock, the clips, the host path's staging
  uint32_t n_channels = 0;

  // host records, under core.mu
  std::vector<hrfd::DcsgenQueue> queue;    // [C]
  std::vector<int16_t> taps;
  bool taps_dirty = true;
  uint32_t dirty_lo = 0, dirty_hi = 0;     // channels dirty_lo .. dirty_hi - 1 differ from the device's copy

  hrfd::PinnedBuf<hrfd::DcsgenSlot> h_stage;       // [min(C, 1024)][8]
  hrfd::PinnedBuf<uint2> h_taps;           // [kAudioMaxJ]
  hrfd::DevBuf<hrfd::DcsgenSlot> d_slots;  // [C][8]
  hrfd::DevBuf<uint2> d_taps;              // [kAudioMaxJ]

  void touch(uint32_t c)
  {
    if (dirty_lo == dirty_hi)
    {
      dirty_lo = c;
      dirty_hi = c + 1;
    }
    dirty_lo = std::min(dirty_lo, c);
    dirty_hi = std::max(dirty_hi, c + 1);
  }

  // the watermark GenCore keeps: nothing leaves a queue before it
  void watch(const hrfd::DcsgenQueue &q) { gen.next_end = std::min(gen.next_end, hrfd::dcsgen_next_end(q)); }
};

extern "C" int hrfd_dcsgen_create(uint32_t n_channels, int device, hrfd_dcsgen **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(dcsgen_check_create("hrfd_dcsgen_create", n_channels, out));
  hrfd_dcsgen *t = nullptr;
  BANK_TRY(bank_new("hrfd_dcsgen_create", device, &t));
  const size_t C = n_channels;
  t->n_channels = n_channels;
  t->queue.resize(C);
  t->taps.assign(1, (int16_t)16384);
  t->dirty_lo = 0;
  t->dirty_hi = n_channels;                // the device's copy starts as empty slots, through the first call's staging
  if (!(t->d_slots.alloc(C * kDcsgenMaxSegments) && t->h_stage.alloc(std::min<size_t>(C, kDcsgenStageChannels) * kDcsgenMaxSegments) &&
        t->d_taps.alloc(kAudioMaxJ) && t->h_taps.alloc(kAudioMaxJ) && t->gen.alloc(C)))
  {
    (void)hipGetLastError();
    bank_free(t);
    return fail(HRFD_ENOMEM, "hrfd_dcsgen_create: device allocation failed");
  }
  *out = t;
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_destroy(hrfd_dcsgen *t)
{
  if (t != nullptr)
  {
    hrfd::bank_free(t);
  }
  return HRFD_OK;
}

// the queue and the clock stay: r is a function of the stream time alone, and the filter has no state to lose
extern "C" int hrfd_dcsgen_set_taps(hrfd_dcsgen *t, const int16_t *taps, uint32_t n)
{
  BANK_TRY(hrfd::dcsgen_check_taps("hrfd_dcsgen_set_taps", taps, n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_dcsgen_set_taps", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  t->taps.assign(taps, taps + n);
  t->taps_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_queue(hrfd_dcsgen *t, uint32_t channel, const hrfd_dcsgen_segment *segs, uint32_t n, uint64_t start)
{
  using namespace hrfd;
  const char *who = "hrfd_dcsgen_queue";
  BANK_TRY(dcsgen_check_segments(who, segs, n));
  BANK_TRY(pcm_check_channel(who, channel, 65536));
  if (start != kGenAppend)
  {
    BANK_TRY(gen_check_time(who, start));
  }
  BANK_TRY(bank_need_handle(who, t));
  BANK_TRY(pcm_check_channel(who, channel, t->n_channels));
  std::lock_guard<std::mutex> g(t->core.mu);
  // refused whole: every selected channel is laid out before one is changed
  const uint32_t first = channel == HRFD_ALL_CHANNELS ? 0 : channel, last = channel == HRFD_ALL_CHANNELS ? t->n_channels : channel + 1;
  std::vector<DcsgenQueue> merged(last - first);
  for (uint32_t c = first; c < last; c++)
  {
    BANK_TRY(dcsgen_lay_out(who, t->queue[c], t->gen.N, segs, n, start, merged[c - first]));
  }
  for (uint32_t c = first; c < last; c++)
  {
    t->queue[c].swap(merged[c - first]);
    t->watch(t->queue[c]);
    t->touch(c);
  }
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_cut(hrfd_dcsgen *t, uint32_t channel, int with_tail)
{
  using namespace hrfd;
  BANK_TRY(pcm_check_channel("hrfd_dcsgen_cut", channel, 65536));
  BANK_TRY(bank_need_handle("hrfd_dcsgen_cut", t));
  BANK_TRY(pcm_check_channel("hrfd_dcsgen_cut", channel, t->n_channels));
  std::lock_guard<std::mutex> g(t->core.mu);
  bank_each_selected(t->n_channels, channel, [&](uint32_t c) {
    DcsgenQueue &q = t->queue[c];
    if (!q.empty())
    {
      dcsgen_cut(q, t->gen.N, with_tail != 0);
      t->watch(q);
      t->touch(c);
    }
  });
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_reset(hrfd_dcsgen *t)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_dcsgen_reset", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  for (hrfd::DcsgenQueue &q : t->queue)
  {
    q.clear();
  }
  t->gen.reset();
  t->dirty_lo = 0;
  t->dirty_hi = t->n_channels;
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_set_time(hrfd_dcsgen *t, uint64_t N)
{
  BANK_TRY(hrfd::gen_check_time("hrfd_dcsgen_set_time", N));
  BANK_TRY(hrfd::bank_need_handle("hrfd_dcsgen_set_time", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  t->gen.N = N;
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_time(hrfd_dcsgen *t, uint64_t *N) { return hrfd::gen_time(t, "hrfd_dcsgen_time", N); }

extern "C" int hrfd_dcsgen_pending(hrfd_dcsgen *t, uint32_t channel, uint32_t *n_segments, uint64_t *end)
{
  using namespace hrfd;
  const char *who = "hrfd_dcsgen_pending";
  if (channel >= 65536)
  {
    return fail(HRFD_EINVAL, "%s: channel %u (one channel)", who, channel);
  }
  if (n_segments == nullptr && end == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL results", who);
  }
  BANK_TRY(gen_check_getter(t, who, channel));
  std::lock_guard<std::mutex> g(t->core.mu);
  // counted without dropping: what has ended leaves the queue with the next call
  uint32_t count = 0;
  uint64_t last = t->gen.N;
  for (const DcsgenSeg &s : t->queue[channel])
  {
    if (!dcsgen_ended(s.s, t->gen.N))
    {
      count++;
      last = s.s.end;
    }
  }
  if (n_segments != nullptr)
  {
    *n_segments = count;
  }
  if (end != nullptr)
  {
    *end = last;
  }
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_get_clips(hrfd_dcsgen *t, uint32_t channel, uint64_t *n)
{
  return hrfd::gen_get_clips(t, "hrfd_dcsgen_get_clips", channel, n);
}

// the channels lo .. hi - 1 from the host's queues to the device's slots, through the pinned staging buffer in uploads of
// at most kDcsgenStageChannels channels (rule 2 of BankCore around each)
static int dcsgen_stage(hrfd_dcsgen *t, uint32_t lo, uint32_t hi, hipStream_t st)
{
  using namespace hrfd;
  for (uint32_t c0 = lo; c0 < hi; c0 += kDcsgenStageChannels)
  {
    const uint32_t count = std::min(hi - c0, kDcsgenStageChannels);
    BANK_TRY(t->core.staging_wait());
    for (uint32_t i = 0; i < count; i++)
    {
      dcsgen_fill_slots(t->queue[c0 + i], t->h_stage + (size_t)i * kDcsgenMaxSegments);
    }
    HIP_TRY(hipMemcpyAsync(t->d_slots + (size_t)c0 * kDcsgenMaxSegments, t->h_stage, sizeof(DcsgenSlot) * kDcsgenMaxSegments * count,
                           hipMemcpyHostToDevice, st));
    BANK_TRY(t->core.staging_sent(st));
  }
  return HRFD_OK;
}

// one call on `st`: what the setters and the clock changed, then k_dcsgen; the clock moves on, on the host
static int dcsgen_launch(hrfd_dcsgen *t, const int16_t *d_pcm, uint64_t stride, uint32_t n_blocks, int16_t *d_out,
                         uint64_t out_stride, uint8_t *d_active, hipStream_t st)
{
  using namespace hrfd;
  const uint64_t n = (uint64_t)kGenBlock * n_blocks;
  DcsgenParams P;
  BANK_TRY(t->core.order_behind_last(st));
  {
    std::lock_guard<std::mutex> g(t->core.mu);
    P.N = t->gen.N;
    P.Nu = dcsgen_u(P.N);
    P.T = (uint32_t)t->taps.size();
    P.J = ((uint32_t)bank_packed_len((int)P.T) + kAudioStep - 1) / kAudioStep * kAudioStep;
    if (t->gen.next_end <= t->gen.N)
    {
      // segments have ended: they leave the queues, and the device's copy of their channels with them
      t->gen.next_end = kDcsgenNoEnd;
      for (uint32_t c = 0; c < t->n_channels; c++)
      {
        DcsgenQueue &q = t->queue[c];
        const size_t before = q.size();
        dcsgen_drop_ended(q, t->gen.N);
        if (q.size() != before)
        {
          t->touch(c);
        }
        t->watch(q);
      }
    }
    if (t->taps_dirty)
    {
      BANK_TRY(t->core.staging_wait());
      bank_pack_taps(t->taps.data(), (int)P.T, t->h_taps.p, (int)P.J);
      HIP_TRY(hipMemcpyAsync(t->d_taps, t->h_taps, sizeof(uint2) * P.J, hipMemcpyHostToDevice, st));
      BANK_TRY(t->core.staging_sent(st));
      t->taps_dirty = false;
    }
    if (t->dirty_lo != t->dirty_hi)
    {
      BANK_TRY(dcsgen_stage(t, t->dirty_lo, t->dirty_hi, st));
      t->dirty_lo = t->dirty_hi = 0;
    }
    BANK_TRY(t->gen.advance(t->n_channels, n, st));
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.out = d_out;
  P.out_stride = out_stride;
  P.slots = t->d_slots;
  P.clips = t->gen.d_clips;
  P.active = d_active;
  P.n_blocks = n_blocks;
  const uint32_t tiles = (uint32_t)((n + kDcsgenTile - 1) / kDcsgenTile);
  const uint32_t want = (kDcsgenAimWgs + t->n_channels - 1) / t->n_channels;
  const uint32_t gy = std::min(std::min(tiles, kDcsgenMaxGridY), std::max(want, 1u));
  hipLaunchKernelGGL(k_dcsgen, dim3(t->n_channels, gy), dim3(kDcsgenThreads), 0, st, P, (const uint2 *)t->d_taps.p);
  BANK_TRY(bank_launch_ok("k_dcsgen"));
  t->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_process_device(hrfd_dcsgen *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, uint32_t n_blocks,
                                          int16_t *d_out, uint64_t out_stride_bytes, uint8_t *d_active, void *stream)
{
  return hrfd::gen_process_device(t, "hrfd_dcsgen_process_device", dcsgen_launch, d_pcm, channel_stride_bytes, n_blocks, d_out,
                                  out_stride_bytes, d_active, stream);
}

extern "C" int hrfd_dcsgen_process(hrfd_dcsgen *t, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active)
{
  return hrfd::gen_process(t, "hrfd_dcsgen_process", dcsgen_launch, pcm, n_blocks, out, active);
}

// ---- the contract on the host, no device needed (include/hrfd_debug.h).  queue6: rows of {start, mid, end, word, amp, tail}
static int dcsgen_debug_queue(const char *who, const uint64_t *queue6, uint32_t n_queue, hrfd::DcsgenQueue &q)
{
  using namespace hrfd;
  if (n_queue > kDcsgenMaxSegments || (n_queue > 0 && queue6 == nullptr))
  {
    return fail(HRFD_EINVAL, "%s: a queue of %u segments (at most %u, and their array)", who, n_queue, kDcsgenMaxSegments);
  }
  q.clear();
  for (uint32_t i = 0; i < n_queue; i++)
  {
    const uint64_t *v = queue6 + 6 * (size_t)i;
    if (v[0] > v[1] || v[1] > v[2] || v[3] > kDcsgenWordMask || v[4] > kGenMaxAmp || v[5] > 0xfffffffeull ||
        (i > 0 && queue6[6 * (size_t)(i - 1) + 2] > v[0]))
    {
      return fail(HRFD_EINVAL, "%s: segment %u of the queue is out of order", who, i);
    }
    q.push_back(DcsgenSeg{DcsgenSlot{v[0], v[1], v[2], (uint32_t)v[3], (uint32_t)v[4]}, (uint32_t)v[5]});
  }
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_debug_edit(uint64_t *queue6, uint32_t *n_queue, uint64_t N, int op, const hrfd_dcsgen_segment *segs,
                                      uint32_t n, uint64_t arg)
{
  using namespace hrfd;
  const char *who = "hrfd_dcsgen_debug_edit";
  if (n_queue == nullptr || op < 0 || op > 2)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument, or op %d (0 queue, 1 cut, 2 drop)", who, op);
  }
  BANK_TRY(gen_check_time(who, N));
  DcsgenQueue q;
  BANK_TRY(dcsgen_debug_queue(who, queue6, *n_queue, q));
  if (op == 0)
  {
    BANK_TRY(dcsgen_check_segments(who, segs, n));
    if (arg != kGenAppend)
    {
      BANK_TRY(gen_check_time(who, arg));
    }
    DcsgenQueue merged;
    BANK_TRY(dcsgen_lay_out(who, q, N, segs, n, arg, merged));
    q.swap(merged);
  }
  else if (op == 1)
  {
    dcsgen_cut(q, N, arg != 0);
  }
  else
  {
    dcsgen_drop_ended(q, N);
  }
  for (size_t i = 0; i < q.size(); i++)
  {
    const uint64_t v[6] = {q[i].s.start, q[i].s.mid, q[i].s.end, q[i].s.word, q[i].s.amp, q[i].tail};
    memcpy(queue6 + 6 * i, v, sizeof(v));
  }
  *n_queue = (uint32_t)q.size();
  return HRFD_OK;
}

extern "C" int hrfd_dcsgen_debug_slow(const int16_t *taps, uint32_t n_taps, const uint64_t *queue6, uint32_t n_queue, uint64_t N,
                                      const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active, uint64_t *clips)
{
  using namespace hrfd;
  const char *who = "hrfd_dcsgen_debug_slow";
  BANK_TRY(dcsgen_check_taps(who, taps, n_taps));
  DcsgenQueue q;
  BANK_TRY(dcsgen_debug_queue(who, queue6, n_queue, q));
  BANK_TRY(gen_check_call(who, pcm, 0, false, n_blocks, out, 0, 1));
  BANK_TRY(gen_check_time(who, N));
  BANK_TRY(gen_check_time(who, N + (uint64_t)kGenBlock * n_blocks - 1));
  DcsgenSlot slots[kDcsgenMaxSegments];
  dcsgen_fill_slots(q, slots);
  const uint64_t v = dcsgen_channel_slow(pcm, n_blocks, slots, taps, n_taps, N, out, active);
  if (clips != nullptr)
  {
    *clips = v;
  }
  return HRFD_OK;
}
