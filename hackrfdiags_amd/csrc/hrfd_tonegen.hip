// hackrfdiags_amd/csrc/hrfd_tonegen.hip -- hrfd_tonegen_*: signalling tones on the transmit chain's PCM: CTCSS sub-tones,
// DTMF digits, tone bursts and paging sequences, queued per channel as segments on two tracks and added to the PCM rows the
// modulators and the DUC read.
//
// PCM rows [C][n_blocks][512] int16 in (or none: generate only), the same rows with the tones added out, clips per channel
// and, optionally, which tracks sound in every block.  Exact integer arithmetic on the tone bank's phase grid, contract in
// include/hrfd.h; tests/tonegen_model.py restates it in numpy, hrfd_gen.h and hrfd_tonegen.h hold the laws and the queue
// rules both sides of this file share.  The clock, the clip counters, the sine table and the process entries are GenCore's
// (hrfd_bank.hip); the queues, their copy on the device and the launch are this file's.
//
// The handle keeps the queues on the host (two tracks of at most 32 segments per channel, absolute stream times) and a copy
// on the device: 64 slots of 32 bytes per channel, the unused ones empty.  The kernel is given the stream time N of the
// call's first sample as a parameter, so the copy changes only where a setter changed a queue or a call dropped segments
// that have ended; only those channels are staged again.  The output at stream time n is a pure function of n, the slots and
// x: however a stream is cut into calls, it comes out the same.
//
// k_tonegen: 256 threads, 8 consecutive samples (16 bytes) per lane, tiles of 2048 samples (4 blocks); grid (C, gy), the
// workgroups of a row stride over its tiles.
//   1. lane j of every wave holds slot j's start and end.  One ballot against the call's range says whether the row has
//      anything to do at all; if not, its workgroups copy (out of place), write zeros (generate only) or touch nothing (in
//      place), and never load the sine table
//   2. else the sine table (COS rotated by a quarter turn, 8 KiB) and the 64 slots (2 KiB) go to LDS once per workgroup
//   3. per tile a ballot against the tile's range is the hit list: every wave computes the same 64-bit mask from its own
//      registers, so no barrier stands in the tile loop.  Lanes walk the set bits (usually none to three) and add each hit's
//      g to their 8 sums: the ramp terms k + 1 and end - n are clamped into 32 bits once per hit, the phase advances by the
//      step per sample
//   4. y = sat16(x + sum), 16 bytes per lane out; clipped samples are counted per lane, summed over the wave by shuffles
//      behind the last tile, and added to clips[c] with one vector atomic per wave that has any
//   5. active: wave w of a tile tests the slots against block w of the tile, lane 0 writes the two track bits
// In place: every sample is loaded once, by the lane that stores it.  Rows at any even address and stride take one path
// through a vector type of alignment 2 (pcm_load8, pcm_store8).
// The grid is at most 65536 x 64 = 2^22 workgroups = kBankMaxWgs: the launch is never cut (no first_wg, no max_wgs hook).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hrfd_tonegen.h"

namespace hrfd {

constexpr int kTonegenThreads = 256;
constexpr int kTonegenPer = 8;                             // consecutive samples of one lane: 16 bytes
constexpr int kTonegenTile = kTonegenThreads * kTonegenPer;      // 2048 samples
constexpr int kTonegenTileBlocks = kTonegenTile / (int)kGenBlock;  // 4: one per wave
constexpr uint32_t kTonegenMaxGridY = 64;
constexpr uint32_t kTonegenAimWgs = 2048;                  // workgroups a launch aims for before a workgroup takes a second tile
constexpr uint32_t kTonegenStageChannels = 1024;           // channels of one upload from the pinned staging buffer
constexpr int32_t kTonegenClamp = 1 << 20;                 // |k + 1| and |end - n| beyond this are as good as infinite
static_assert(kTonegenTileBlocks == kTonegenThreads / 64, "one wave per block of a tile");
static_assert(kTonegenSlots == 64, "one slot per lane of a wave");
static_assert(65536ull * kTonegenMaxGridY <= kBankMaxWgs, "the grid is one launch");

struct TonegenParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address; or NULL
  uint64_t stride;
  int16_t *out;                            // [C] rows, out_stride bytes apart, even address; may be pcm itself
  uint64_t out_stride;
  const TonegenSlot *slots;                // [C][64]
  unsigned long long *clips;               // [C]
  uint8_t *active;                         // [C][n_blocks] or NULL
  uint64_t N;                              // the stream time of the call's first sample
  uint32_t n_blocks;
};

__device__ __forceinline__ int32_t tonegen_clamp(int64_t v)
{
  return (int32_t)(v < -(int64_t)kTonegenClamp ? -(int64_t)kTonegenClamp : (v > (int64_t)kTonegenClamp ? (int64_t)kTonegenClamp : v));
}

// sine: [4096] int16, sine[i] = COS[(i - 1024) & 4095]; a parameter of its own so that it can be __restrict__
__global__ __launch_bounds__(kTonegenThreads) void k_tonegen(const TonegenParams P, const int16_t *__restrict__ sine)
{
  __shared__ int16_t sl[4096];
  __shared__ TonegenSlot slot[kTonegenSlots];
  const uint32_t tid = threadIdx.x, c = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = P.n_blocks * kGenBlock;
  const int16_t *row = P.pcm != nullptr ? (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride) : nullptr;
  int16_t *orow = (int16_t *)((char *)P.out + (uint64_t)c * P.out_stride);
  const bool in_place = (const int16_t *)orow == row;
  const TonegenSlot *mine = P.slots + (uint64_t)c * kTonegenSlots;

  // 1. lane j of every wave: slot j's start and end
  const uint64_t s_start = mine[lane].start, s_end = mine[lane].end;
  const bool row_busy = __ballot(s_start < P.N + n && s_end > P.N) != 0ull;        // the same in every wave
  if (row_busy)
  {
    // 2. the table and the slots
    const pcm_u4 *src = (const pcm_u4 *)sine;
    pcm_u4 *dst = (pcm_u4 *)sl;
    dst[tid] = src[tid];
    dst[tid + kTonegenThreads] = src[tid + kTonegenThreads];
    if (tid < kTonegenSlots)
    {
      slot[tid] = mine[tid];
    }
    __syncthreads();
  }

  uint32_t clipped = 0;
  for (uint32_t t0 = blockIdx.y * kTonegenTile; t0 < n; t0 += gridDim.y * kTonegenTile)
  {
    const uint64_t n0 = P.N + t0;                          // the tile's first stream time
    const uint32_t at = t0 + tid * kTonegenPer;            // the lane's first sample
    const bool live = at < n;                              // n is whole blocks: a lane has all of its samples or none
    // 3. the hit list
    uint64_t hits = row_busy ? __ballot(s_start < n0 + kTonegenTile && s_end > n0) : 0ull;
    if (P.active != nullptr)
    {
      // 5. wave w: block w of the tile
      const uint64_t b0 = n0 + wave * kGenBlock;
      const uint64_t m = row_busy ? __ballot(s_start < b0 + kGenBlock && s_end > b0) : 0ull;
      const uint32_t b = t0 / kGenBlock + wave;
      if (lane == 0 && b < P.n_blocks)
      {
        P.active[(uint64_t)c * P.n_blocks + b] = (uint8_t)(((uint32_t)m != 0u ? 1u : 0u) | ((uint32_t)(m >> 32) != 0u ? 2u : 0u));
      }
    }
    if (!live || (hits == 0ull && in_place))
    {
      continue;                                            // (no barrier in this loop)
    }
    pcm_u4 cur = {0u, 0u, 0u, 0u};
    if (row != nullptr)
    {
      cur = pcm_load8(row + at);
    }
    if (hits == 0ull)
    {
      pcm_store8(orow + at, cur);                          // a copy, or zeros
      continue;
    }
    int32_t sum[kTonegenPer];
#pragma unroll
    for (int i = 0; i < kTonegenPer; i++)
    {
      sum[i] = 0;
    }
    const uint64_t nl = P.N + at;                          // the lane's first stream time
    while (hits != 0ull)
    {
      const uint32_t j = (uint32_t)__builtin_ctzll(hits);
      hits &= hits - 1ull;
      const TonegenSlot s = slot[j];
      // k + 1 and end - n of the lane's first sample, clamped into 32 bits: below 1 = outside, 64 and more = no ramp, and
      // the clamp (2^20) keeps both orders for the 8 samples of a lane
      const int32_t up0 = tonegen_clamp((int64_t)(nl - s.start) + 1);
      const int32_t down0 = s.end == kTonegenNoEnd ? kTonegenClamp : tonegen_clamp((int64_t)(s.end - nl));
      if (up0 + (kTonegenPer - 1) < 1 || down0 < 1)
      {
        continue;                                          // the lane's samples lie in front of the segment or behind it
      }
      const uint32_t amp_a = s.amps & 0xffffu, amp_b = s.amps >> 16;
      uint32_t th_a = s.step_a * (uint32_t)(nl - s.start), th_b = s.step_b * (uint32_t)(nl - s.start);
#pragma unroll
      for (int i = 0; i < kTonegenPer; i++)
      {
        const int32_t up = up0 + i, down = down0 - i;
        if (up >= 1 && down >= 1)
        {
          const int32_t v = gen_mix(amp_a, sl[gen_cos_index(th_a)], amp_b, sl[gen_cos_index(th_b)]);
          sum[i] += gen_ramp(v, (uint32_t)up, (uint32_t)down);
        }
        th_a += s.step_a;
        th_b += s.step_b;
      }
    }
    // 4. the output
    const uint32_t d[4] = {cur.x, cur.y, cur.z, cur.w};
    uint32_t y[kTonegenPer];
#pragma unroll
    for (int i = 0; i < kTonegenPer; i++)
    {
      const int32_t x = (i & 1) ? (int32_t)d[i / 2] >> 16 : (int32_t)(int16_t)d[i / 2];
      bool clip;
      y[i] = (uint32_t)gen_output(x, sum[i], &clip);
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
struct hrfd_tonegen
{
  hrfd::BankCore core;
  hrfd::GenCore gen;                       // the clock, the clips, the sine table, the host path's staging
  uint32_t n_channels = 0;

  // host records, under core.mu
  std::vector<hrfd::TonegenTrack> track;   // [C][2]
  uint32_t dirty_lo = 0, dirty_hi = 0;     // channels dirty_lo .. dirty_hi - 1 differ from the device's copy

  hrfd::PinnedBuf<hrfd::TonegenSlot> h_stage;      // [min(C, 1024)][64]
  hrfd::DevBuf<hrfd::TonegenSlot> d_slots; // [C][64]

  hrfd::TonegenTrack &q(uint32_t c, uint32_t t) { return track[(size_t)c * hrfd::kTonegenTracks + t]; }

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
};

extern "C" int hrfd_tonegen_create(uint32_t n_channels, int device, hrfd_tonegen **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(tonegen_check_create("hrfd_tonegen_create", n_channels, out));
  hrfd_tonegen *t = nullptr;
  BANK_TRY(bank_new("hrfd_tonegen_create", device, &t));
  const size_t C = n_channels;
  t->n_channels = n_channels;
  t->track.resize(C * kTonegenTracks);
  t->dirty_lo = 0;
  t->dirty_hi = n_channels;                // the device's copy starts as empty slots, through the first call's staging
  if (!(t->d_slots.alloc(C * kTonegenSlots) && t->h_stage.alloc(std::min<size_t>(C, kTonegenStageChannels) * kTonegenSlots) &&
        t->gen.alloc(C)))
  {
    (void)hipGetLastError();
    bank_free(t);
    return fail(HRFD_ENOMEM, "hrfd_tonegen_create: device allocation failed");
  }
  *out = t;
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_destroy(hrfd_tonegen *t)
{
  if (t != nullptr)
  {
    hrfd::bank_free(t);
  }
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_queue(hrfd_tonegen *t, uint32_t channel, uint32_t track, const hrfd_tonegen_segment *segs, uint32_t n,
                                  uint64_t start)
{
  using namespace hrfd;
  const char *who = "hrfd_tonegen_queue";
  BANK_TRY(tonegen_check_segments(who, segs, n, track));
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
  std::vector<TonegenTrack> merged(last - first);
  for (uint32_t c = first; c < last; c++)
  {
    BANK_TRY(tonegen_lay_out(who, t->q(c, track), t->gen.N, segs, n, start, merged[c - first]));
  }
  for (uint32_t c = first; c < last; c++)
  {
    t->q(c, track).swap(merged[c - first]);
    for (const TonegenSlot &s : t->q(c, track))
    {
      t->gen.next_end = std::min(t->gen.next_end, s.end);
    }
    t->touch(c);
  }
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_cut(hrfd_tonegen *t, uint32_t channel, uint32_t track)
{
  using namespace hrfd;
  BANK_TRY(tonegen_check_track("hrfd_tonegen_cut", channel, track, 65536));
  BANK_TRY(bank_need_handle("hrfd_tonegen_cut", t));
  BANK_TRY(tonegen_check_track("hrfd_tonegen_cut", channel, track, t->n_channels));
  std::lock_guard<std::mutex> g(t->core.mu);
  bank_each_selected(t->n_channels, channel, [&](uint32_t c) {
    TonegenTrack &q = t->q(c, track);
    if (!q.empty())
    {
      tonegen_cut(q, t->gen.N);
      for (const TonegenSlot &s : q)
      {
        t->gen.next_end = std::min(t->gen.next_end, s.end);
      }
      t->touch(c);
    }
  });
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_reset(hrfd_tonegen *t)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_tonegen_reset", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  for (hrfd::TonegenTrack &q : t->track)
  {
    q.clear();
  }
  t->gen.reset();
  t->dirty_lo = 0;
  t->dirty_hi = t->n_channels;
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_set_time(hrfd_tonegen *t, uint64_t N)
{
  BANK_TRY(hrfd::gen_check_time("hrfd_tonegen_set_time", N));
  BANK_TRY(hrfd::bank_need_handle("hrfd_tonegen_set_time", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  t->gen.N = N;
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_time(hrfd_tonegen *t, uint64_t *N) { return hrfd::gen_time(t, "hrfd_tonegen_time", N); }

extern "C" int hrfd_tonegen_pending(hrfd_tonegen *t, uint32_t channel, uint32_t track, uint32_t *n_segments, uint64_t *end)
{
  using namespace hrfd;
  const char *who = "hrfd_tonegen_pending";
  if (track >= kTonegenTracks || channel >= 65536)
  {
    return fail(HRFD_EINVAL, "%s: channel %u, track %u (one channel, track 0..%u)", who, channel, track, kTonegenTracks - 1);
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
  for (const TonegenSlot &s : t->q(channel, track))
  {
    if (s.end > t->gen.N)
    {
      count++;
      last = s.end;
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

extern "C" int hrfd_tonegen_get_clips(hrfd_tonegen *t, uint32_t channel, uint64_t *n)
{
  return hrfd::gen_get_clips(t, "hrfd_tonegen_get_clips", channel, n);
}

// the channels lo .. hi - 1 from the host's queues to the device's slots, through the pinned staging buffer in uploads of
// at most kTonegenStageChannels channels (rule 2 of BankCore around each)
static int tonegen_stage(hrfd_tonegen *t, uint32_t lo, uint32_t hi, hipStream_t st)
{
  using namespace hrfd;
  for (uint32_t c0 = lo; c0 < hi; c0 += kTonegenStageChannels)
  {
    const uint32_t count = std::min(hi - c0, kTonegenStageChannels);
    BANK_TRY(t->core.staging_wait());
    for (uint32_t i = 0; i < count; i++)
    {
      tonegen_fill_slots(&t->q(c0 + i, 0), t->h_stage + (size_t)i * kTonegenSlots);
    }
    HIP_TRY(hipMemcpyAsync(t->d_slots + (size_t)c0 * kTonegenSlots, t->h_stage, sizeof(TonegenSlot) * kTonegenSlots * count,
                           hipMemcpyHostToDevice, st));
    BANK_TRY(t->core.staging_sent(st));
  }
  return HRFD_OK;
}

// one call on `st`: what the setters and the clock changed, then k_tonegen; the clock moves on, on the host
static int tonegen_launch(hrfd_tonegen *t, const int16_t *d_pcm, uint64_t stride, uint32_t n_blocks, int16_t *d_out,
                          uint64_t out_stride, uint8_t *d_active, hipStream_t st)
{
  using namespace hrfd;
  const uint64_t n = (uint64_t)kGenBlock * n_blocks;
  TonegenParams P;
  BANK_TRY(t->core.order_behind_last(st));
  {
    std::lock_guard<std::mutex> g(t->core.mu);
    P.N = t->gen.N;
    if (t->gen.next_end <= t->gen.N)
    {
      // segments have ended: they leave the queues, and the device's copy of their channels with them
      t->gen.next_end = kTonegenNoEnd;
      for (uint32_t c = 0; c < t->n_channels; c++)
      {
        for (uint32_t k = 0; k < kTonegenTracks; k++)
        {
          TonegenTrack &q = t->q(c, k);
          const size_t before = q.size();
          tonegen_drop_ended(q, t->gen.N);
          if (q.size() != before)
          {
            t->touch(c);
          }
          for (const TonegenSlot &s : q)
          {
            t->gen.next_end = std::min(t->gen.next_end, s.end);
          }
        }
      }
    }
    if (t->dirty_lo != t->dirty_hi)
    {
      BANK_TRY(tonegen_stage(t, t->dirty_lo, t->dirty_hi, st));
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
  const uint32_t tiles = (uint32_t)((n + kTonegenTile - 1) / kTonegenTile);
  const uint32_t want = (kTonegenAimWgs + t->n_channels - 1) / t->n_channels;
  const uint32_t gy = std::min(std::min(tiles, kTonegenMaxGridY), std::max(want, 1u));
  hipLaunchKernelGGL(k_tonegen, dim3(t->n_channels, gy), dim3(kTonegenThreads), 0, st, P, (const int16_t *)t->gen.d_sine.p);
  BANK_TRY(bank_launch_ok("k_tonegen"));
  t->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_tonegen_process_device(hrfd_tonegen *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, uint32_t n_blocks,
                                           int16_t *d_out, uint64_t out_stride_bytes, uint8_t *d_active, void *stream)
{
  return hrfd::gen_process_device(t, "hrfd_tonegen_process_device", tonegen_launch, d_pcm, channel_stride_bytes, n_blocks, d_out,
                                  out_stride_bytes, d_active, stream);
}

extern "C" int hrfd_tonegen_process(hrfd_tonegen *t, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active)
{
  return hrfd::gen_process(t, "hrfd_tonegen_process", tonegen_launch, pcm, n_blocks, out, active);
}
