// hackrfdiags_amd/csrc/hrfd_afskgen.hip -- hrfd_afskgen_*: packet data keyed onto the transmit chain's PCM: continuous-phase
// audio frequency-shift keying (Bell 202, Bell 103 and any other pair of tones and baud rate), queued per channel as messages
// of bits and added to the PCM rows the modulators and the DUC read.  The mirror of hrfd_afsk.hip, which decodes it.
//
// PCM rows [C][n_blocks][512] int16 in (or none: generate only), the same rows with the messages added out, clips per
// channel and, optionally, in which blocks a message sounds.  Exact integer arithmetic on the tone generator's phase grid,
// contract in include/hrfd.h; tests/afskgen_model.py restates it in numpy, hrfd_gen.h and hrfd_afskgen.h hold the laws and
// the queue rules both sides of this file share.  The clock, the clip counters, the sine table and the process entries are
// GenCore's (hrfd_bank.hip); the queues, their copy on the device and the launch are this file's.
//
// The handle keeps the queues on the host (at most 4 messages per channel that have not ended, absolute stream times) and a
// copy on the device: per channel 4 slots of 32 bytes and 4 x 256 dwords of levels, 4 KiB of levels a channel, 256 MiB at
// 65536 channels (264 MiB with the slots).  Both arrays are [slot][channel], so that a message queued on every channel is one run of memory.  Only
// the (channel, slot) pairs a setter changed are staged again; a slot's levels only when a message was queued on it.
//
// k_afskgen: ONE launch, one workgroup of 256 threads per channel, which walks its row in tiles of 2048 samples, 8
// consecutive samples (16 bytes) per lane.  The phase of a message is the running sum of a step that changes with every
// bit, so per tile and message that hits it (a uniform loop over the 4 slots, usually one pass):
//   1. every lane forms st(k) of its 8 samples: the bit by v_mul_hi_u32, a bit test on the two level words the 8 samples
//      can lie in (at most 5 bits: they come through the vector cache, 33 dwords a tile at the most), a select; samples
//      outside the message or behind the call's end add 0
//   2. the lane sums its 8
//   3. the exclusive scan of the 256 sums: shuffles inside a wave, the four wave totals through LDS behind ONE barrier (the
//      totals alternate between two rows, so that no second barrier is needed)
//   4. the lane adds the anchor and steps through its 8 samples on the rotated sine table in LDS (8 KiB)
// The anchor is 0 for a message that starts inside the tile, the running sum of the tile before otherwise, and for the
// message in progress at the call's first sample one dword per channel in device memory, which the workgroup writes at the
// end of every call that ends inside a message.  The calls of a handle are ordered by BankCore, and a message that starts at
// or behind N never reads the dword, so reset clears nothing.
// Everything that decides whether a pass runs is uniform over the workgroup: the slots, N and the tile.
// A row no message touches in the call takes k_tonegen's path: nothing in place, a copy out of place, zeros for generate
// only, and the table is never loaded.  Rows at any even address and stride go through a vector type of alignment 2.
// The grid is the channel count, at most 65536 < kBankMaxWgs: no chunked launch, no max_wgs hook.  The price, as for k_level
// and k_afsk: a call of few channels and many blocks does not fill the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "hrfd_afskgen.h"

namespace hrfd {

constexpr int kAfskgenThreads = 256;
constexpr int kAfskgenPer = 8;                             // consecutive samples of one lane: 16 bytes
constexpr int kAfskgenTile = kAfskgenThreads * kAfskgenPer;        // 2048 samples
constexpr int kAfskgenWaves = kAfskgenThreads / 64;
constexpr uint32_t kAfskgenStageSlots = 256;               // (channel, slot) pairs of one upload from the pinned staging
static_assert(kAfskgenTile / (int)kGenBlock == kAfskgenWaves, "one wave per block of a tile");
static_assert(65536u <= kBankMaxWgs, "the grid is one launch");
static_assert(kAfskgenPer * 1ull * kAfskgenMaxStep / (1ull << 32) + 1 < 32, "the bits of a lane's samples lie in two level words");

struct AfskgenParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address; or NULL
  uint64_t stride;
  int16_t *out;                            // [C] rows, out_stride bytes apart, even address; may be pcm itself
  uint64_t out_stride;
  const AfskgenSlot *slots;                // [4][C]
  const uint32_t *levels;                  // [4][C][256]
  uint32_t *anchor;                        // [C]: theta of the message in progress where the last call ended
  unsigned long long *clips;               // [C]
  uint8_t *active;                         // [C][n_blocks] or NULL
  uint64_t N;                              // the stream time of the call's first sample
  uint32_t n_blocks;
  uint32_t n_channels;
};

__device__ __forceinline__ int32_t afskgen_clamp(int64_t v)
{
  constexpr int64_t far = 1 << 20;         // |k + 1| and |end - n| beyond this are as good as infinite
  return (int32_t)(v < -far ? -far : (v > far ? far : v));
}

// sine: [4096] int16, sine[i] = COS[(i - 1024) & 4095]
__global__ __launch_bounds__(kAfskgenThreads) void k_afskgen(const AfskgenParams P, const int16_t *__restrict__ sine)
{
  __shared__ int16_t sl[4096];
  __shared__ uint32_t totals[2][kAfskgenWaves];
  const uint32_t tid = threadIdx.x, c = blockIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t n = P.n_blocks * kGenBlock;
  const uint64_t call_end = P.N + n;
  const int16_t *row = P.pcm != nullptr ? (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride) : nullptr;
  int16_t *orow = (int16_t *)((char *)P.out + (uint64_t)c * P.out_stride);
  const bool in_place = (const int16_t *)orow == row;

  // the channel's four slots: the same for every lane
  AfskgenSlot slot[kAfskgenMaxMessages];
  bool row_busy = false;
#pragma unroll
  for (uint32_t j = 0; j < kAfskgenMaxMessages; j++)
  {
    slot[j] = P.slots[(uint64_t)j * P.n_channels + c];
    row_busy = row_busy || (slot[j].start < call_end && slot[j].end > P.N);
  }
  uint32_t carry = 0;                      // theta of the message in progress at the tile's first sample
  if (row_busy)
  {
    const pcm_u4 *src = (const pcm_u4 *)sine;
    pcm_u4 *dst = (pcm_u4 *)sl;
    dst[tid] = src[tid];
    dst[tid + kAfskgenThreads] = src[tid + kAfskgenThreads];
    carry = P.anchor[c];
    __syncthreads();
  }

  uint32_t clipped = 0, pass = 0;
  bool carry_live = false;                 // a message goes on behind the tile: carry is its theta there
  for (uint32_t t0 = 0; t0 < n; t0 += kAfskgenTile)
  {
    const uint64_t n0 = P.N + t0;                          // the tile's first stream time
    const uint64_t n1 = n0 + kAfskgenTile < call_end ? n0 + kAfskgenTile : call_end;       // behind its last
    const uint32_t at = t0 + tid * kAfskgenPer;            // the lane's first sample
    const bool live = at < n;                              // n is whole blocks: a lane has all of its samples or none
    const uint64_t nl = P.N + at;                          // the lane's first stream time
    if (P.active != nullptr)
    {
      // wave w: block w of the tile
      const uint64_t b0 = n0 + wave * kGenBlock;
      const uint32_t b = t0 / kGenBlock + wave;
      bool sounds = false;
#pragma unroll
      for (uint32_t j = 0; j < kAfskgenMaxMessages; j++)
      {
        sounds = sounds || (slot[j].start < b0 + kGenBlock && slot[j].end > b0);
      }
      if (lane == 0 && b < P.n_blocks)
      {
        P.active[(uint64_t)c * P.n_blocks + b] = sounds ? 1 : 0;
      }
    }
    int32_t g[kAfskgenPer];
#pragma unroll
    for (int i = 0; i < kAfskgenPer; i++)
    {
      g[i] = 0;
    }
    bool tile_hit = false;
    uint32_t carry_next = 0;
    carry_live = false;
#pragma unroll
    for (uint32_t j = 0; j < kAfskgenMaxMessages; j++)
    {
      const AfskgenSlot s = slot[j];
      if (!(s.start < n1 && s.end > n0))
      {
        continue;                                          // uniform: the barrier below is met by all or by none
      }
      tile_hit = true;
      const uint32_t *lv = P.levels + ((uint64_t)j * P.n_channels + c) * kAfskgenLevelWords;
      // k + 1 and end - n of the lane's first sample, clamped into 32 bits: below 1 = outside, 64 and more = no ramp, and the
      // clamp keeps both orders for the 8 samples of a lane.  last - n: the same against the call's end, for the sums
      const int32_t up0 = afskgen_clamp((int64_t)(nl - s.start) + 1);
      const int32_t down0 = afskgen_clamp((int64_t)(s.end - nl));
      const int32_t left0 = afskgen_clamp((int64_t)((s.end < n1 ? s.end : n1) - nl));
      const uint32_t k0 = (uint32_t)(nl - s.start);        // k of the lane's first sample; wraps in front of the message
      // 1. the steps of the lane's samples: the two level words its bits can lie in
      const bool any = up0 + (kAfskgenPer - 1) >= 1 && left0 >= 1;
      const uint32_t k_first = up0 >= 1 ? k0 : 0u;         // the first of the lane's samples inside the message
      const uint32_t w = any ? __umulhi(k_first, s.baud_step) >> 5 : 0u;       // < 256: the bit lies below n_bits <= 8192
      const uint32_t w_hi = w + 1 < kAfskgenLevelWords ? w + 1 : w;
      const uint64_t two = any ? (uint64_t)lv[w] | ((uint64_t)lv[w_hi] << 32) : 0ull;
      uint32_t st[kAfskgenPer], mine = 0;
#pragma unroll
      for (int i = 0; i < kAfskgenPer; i++)
      {
        const uint32_t bit = __umulhi(k0 + i, s.baud_step);
        const uint32_t level = (uint32_t)(two >> ((bit - 32u * w) & 63u)) & 1u;
        const bool inside = up0 + i >= 1 && left0 - i >= 1;
        st[i] = inside ? (level != 0u ? s.mark_step : s.space_step) : 0u;
        mine += st[i];                                     // 2.
      }
      // 3. the exclusive scan over the workgroup
      uint32_t inc = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1)
      {
        const uint32_t below = (uint32_t)__shfl_up((int)inc, d);
        inc += lane >= (uint32_t)d ? below : 0u;
      }
      if (lane == 63)
      {
        totals[pass & 1u][wave] = inc;
      }
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (uint32_t v = 0; v < (uint32_t)kAfskgenWaves; v++)
      {
        const uint32_t t = totals[pass & 1u][v];
        before += v < wave ? t : 0u;
        total += t;
      }
      pass++;
      const uint32_t base = s.start < n0 ? carry : 0u;     // the anchor
      if (s.end > n1)
      {
        carry_next = base + total;
        carry_live = true;
      }
      // 4. the lane's samples
      if (any)
      {
        uint32_t theta = base + before + (inc - mine);
#pragma unroll
        for (int i = 0; i < kAfskgenPer; i++)
        {
          const int32_t up = up0 + i, down = down0 - i;
          if (up >= 1 && left0 - i >= 1)
          {
            const int32_t v = gen_mix(s.amp, sl[gen_cos_index(theta)], 0u, 0);
            g[i] += gen_ramp(v, (uint32_t)up, (uint32_t)down);
          }
          theta += st[i];
        }
      }
    }
    carry = carry_next;
    if (!live || (in_place && !tile_hit))
    {
      continue;                                            // (behind the passes: every lane has met their barriers)
    }
    pcm_u4 cur = {0u, 0u, 0u, 0u};
    if (row != nullptr)
    {
      cur = pcm_load8(row + at);
    }
    if (!tile_hit)
    {
      pcm_store8(orow + at, cur);                          // a copy, or zeros
      continue;
    }
    const uint32_t d[4] = {cur.x, cur.y, cur.z, cur.w};
    uint32_t y[kAfskgenPer];
#pragma unroll
    for (int i = 0; i < kAfskgenPer; i++)
    {
      const int32_t x = (i & 1) ? (int32_t)d[i / 2] >> 16 : (int32_t)(int16_t)d[i / 2];
      bool clip;
      y[i] = (uint32_t)gen_output(x, g[i], &clip);
      clipped += clip ? 1u : 0u;
    }
    pcm_u4 v;
    v.x = (y[0] & 0xffffu) | (y[1] << 16);
    v.y = (y[2] & 0xffffu) | (y[3] << 16);
    v.z = (y[4] & 0xffffu) | (y[5] << 16);
    v.w = (y[6] & 0xffffu) | (y[7] << 16);
    pcm_store8(orow + at, v);
  }

  // the message in progress where the call ends: its theta there, for the next call
  if (carry_live && tid == 0)
  {
    P.anchor[c] = carry;
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
struct hrfd_afskgen
{
  hrfd::BankCore core;
  hrfd::GenCore gen;                       // the clock, the clips, the sine table, the host path's staging
  uint32_t n_channels = 0;

  // host records, under core.mu
  std::vector<hrfd::AfskgenQueue> queue;   // [C]
  std::vector<uint8_t> dirty;              // [4][C]: 0 = as on the device, 1 = the slot differs, 2 = the slot and its levels
  std::vector<uint32_t> dirty_ids;         // the indices of the entries above that are not 0
  bool clear_slots = false;                // reset: the device's slots are zeroed ahead of the next launch

  hrfd::PinnedBuf<hrfd::AfskgenSlot> h_slots;      // [256]
  hrfd::PinnedBuf<uint32_t> h_levels;      // [256][256]
  hrfd::DevBuf<hrfd::AfskgenSlot> d_slots; // [4][C]
  hrfd::DevBuf<uint32_t> d_levels;         // [4][C][256]
  hrfd::DevBuf<uint32_t> d_anchor;         // [C]

  void touch(uint32_t c, uint32_t slot, uint8_t what)
  {
    const uint32_t id = slot * n_channels + c;
    if (dirty[id] == 0)
    {
      dirty_ids.push_back(id);
    }
    dirty[id] = std::max(dirty[id], what);
  }

  // the message on the (channel, slot) of `id`, or NULL: the slot is empty
  const hrfd::AfskgenMsg *find(uint32_t id) const
  {
    for (const hrfd::AfskgenMsg &m : queue[id % n_channels])
    {
      if (m.slot == id / n_channels)
      {
        return &m;
      }
    }
    return nullptr;
  }

  // what has ended at N leaves the queues; its slots are emptied on the device, so that a clock set back finds nothing
  void drop_ended()
  {
    if (gen.next_end > gen.N)
    {
      return;
    }
    gen.next_end = ~0ull;
    for (uint32_t c = 0; c < n_channels; c++)
    {
      for (const hrfd::AfskgenMsg &m : queue[c])
      {
        if (m.s.end <= gen.N)
        {
          touch(c, m.slot, 1);
        }
      }
      hrfd::afskgen_drop_ended(queue[c], gen.N);
      for (const hrfd::AfskgenMsg &m : queue[c])
      {
        gen.next_end = std::min(gen.next_end, m.s.end);
      }
    }
  }
};

extern "C" int hrfd_afskgen_create(uint32_t n_channels, int device, hrfd_afskgen **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(afskgen_check_create("hrfd_afskgen_create", n_channels, out));
  hrfd_afskgen *t = nullptr;
  BANK_TRY(bank_new("hrfd_afskgen_create", device, &t));
  const size_t C = n_channels, S = kAfskgenMaxMessages;
  t->n_channels = n_channels;
  t->queue.resize(C);
  t->dirty.assign(S * C, 0);
  if (!(t->d_slots.alloc(S * C) && t->d_levels.alloc(S * C * kAfskgenLevelWords) && t->d_anchor.alloc(C) &&
        t->h_slots.alloc(kAfskgenStageSlots) && t->h_levels.alloc((size_t)kAfskgenStageSlots * kAfskgenLevelWords) && t->gen.alloc(C) &&
        hipMemset(t->d_slots, 0, sizeof(AfskgenSlot) * S * C) == hipSuccess &&
        hipMemset(t->d_levels, 0, sizeof(uint32_t) * S * C * kAfskgenLevelWords) == hipSuccess &&
        hipMemset(t->d_anchor, 0, sizeof(uint32_t) * C) == hipSuccess))
  {
    (void)hipGetLastError();
    bank_free(t);
    return fail(HRFD_ENOMEM, "hrfd_afskgen_create: device allocation failed");
  }
  *out = t;
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_destroy(hrfd_afskgen *t)
{
  if (t != nullptr)
  {
    hrfd::bank_free(t);
  }
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_queue(hrfd_afskgen *t, uint32_t channel, const hrfd_afskgen_message *msg, const uint8_t *bits, uint64_t start)
{
  using namespace hrfd;
  const char *who = "hrfd_afskgen_queue";
  uint64_t L = 0;
  BANK_TRY(afskgen_check_message(who, msg, bits, &L));
  BANK_TRY(pcm_check_channel(who, channel, 65536));
  if (start != kGenAppend)
  {
    BANK_TRY(gen_check_time(who, start));
  }
  BANK_TRY(bank_need_handle(who, t));
  BANK_TRY(pcm_check_channel(who, channel, t->n_channels));
  std::vector<uint32_t> levels((msg->n_bits + 31) / 32);
  afskgen_levels(bits, msg->n_bits, (msg->flags & kAfskgenNrzi) != 0, levels.data());
  std::lock_guard<std::mutex> g(t->core.mu);
  // refused whole: every selected channel is laid out before one is changed
  const uint32_t first = channel == HRFD_ALL_CHANNELS ? 0 : channel, last = channel == HRFD_ALL_CHANNELS ? t->n_channels : channel + 1;
  std::vector<AfskgenSlot> laid(last - first);
  for (uint32_t c = first; c < last; c++)
  {
    BANK_TRY(afskgen_lay_out(who, t->queue[c], t->gen.N, msg, L, start, &laid[c - first]));
  }
  t->drop_ended();
  for (uint32_t c = first; c < last; c++)
  {
    afskgen_drop_ended(t->queue[c], t->gen.N);                 // (drop_ended has, unless nothing was due)
    const uint32_t slot = afskgen_insert(t->queue[c], laid[c - first], std::vector<uint32_t>(levels));
    t->gen.next_end = std::min(t->gen.next_end, laid[c - first].end);
    t->touch(c, slot, 2);
  }
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_cut(hrfd_afskgen *t, uint32_t channel)
{
  using namespace hrfd;
  BANK_TRY(pcm_check_channel("hrfd_afskgen_cut", channel, 65536));
  BANK_TRY(bank_need_handle("hrfd_afskgen_cut", t));
  BANK_TRY(pcm_check_channel("hrfd_afskgen_cut", channel, t->n_channels));
  std::lock_guard<std::mutex> g(t->core.mu);
  t->drop_ended();
  bank_each_selected(t->n_channels, channel, [&](uint32_t c) {
    AfskgenQueue &q = t->queue[c];
    for (const AfskgenMsg &m : q)
    {
      t->touch(c, m.slot, 1);
    }
    afskgen_cut(q, t->gen.N);
    for (const AfskgenMsg &m : q)
    {
      t->gen.next_end = std::min(t->gen.next_end, m.s.end);
    }
  });
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_reset(hrfd_afskgen *t)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_afskgen_reset", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  for (hrfd::AfskgenQueue &q : t->queue)
  {
    q.clear();
  }
  t->gen.reset();
  for (uint32_t id : t->dirty_ids)
  {
    t->dirty[id] = 0;
  }
  t->dirty_ids.clear();
  t->clear_slots = true;
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_set_time(hrfd_afskgen *t, uint64_t N)
{
  using namespace hrfd;
  BANK_TRY(gen_check_time("hrfd_afskgen_set_time", N));
  BANK_TRY(bank_need_handle("hrfd_afskgen_set_time", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  for (uint32_t c = 0; c < t->n_channels; c++)
  {
    if (afskgen_count_pending(t->queue[c], t->gen.N, nullptr) != 0)
    {
      return fail(HRFD_EINVAL, "hrfd_afskgen_set_time: channel %u holds a message that has not ended (a clock that jumps into a "
                               "message would need its phase there)", c);
    }
  }
  t->drop_ended();
  t->gen.N = N;
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_time(hrfd_afskgen *t, uint64_t *N) { return hrfd::gen_time(t, "hrfd_afskgen_time", N); }

extern "C" int hrfd_afskgen_pending(hrfd_afskgen *t, uint32_t channel, uint32_t *n_messages, uint64_t *end)
{
  using namespace hrfd;
  const char *who = "hrfd_afskgen_pending";
  if (channel >= 65536)
  {
    return fail(HRFD_EINVAL, "%s: channel %u (one channel)", who, channel);
  }
  if (n_messages == nullptr && end == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL results", who);
  }
  BANK_TRY(gen_check_getter(t, who, channel));
  std::lock_guard<std::mutex> g(t->core.mu);
  // counted without dropping: what has ended leaves the queue with the next call
  uint64_t last = 0;
  const uint32_t count = afskgen_count_pending(t->queue[channel], t->gen.N, &last);
  if (n_messages != nullptr)
  {
    *n_messages = count;
  }
  if (end != nullptr)
  {
    *end = last;
  }
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_get_clips(hrfd_afskgen *t, uint32_t channel, uint64_t *n)
{
  return hrfd::gen_get_clips(t, "hrfd_afskgen_get_clips", channel, n);
}

// the dirty (channel, slot) pairs from the host's queues to the device's copy, in runs of neighbouring entries that need the
// same, through the pinned staging buffers in uploads of at most kAfskgenStageSlots entries (rule 2 of BankCore around each)
static int afskgen_stage(hrfd_afskgen *t, hipStream_t st)
{
  using namespace hrfd;
  std::vector<uint32_t> &ids = t->dirty_ids;
  std::sort(ids.begin(), ids.end());
  for (size_t i = 0; i < ids.size();)
  {
    const uint8_t what = t->dirty[ids[i]];
    size_t j = i + 1;
    while (j < ids.size() && j - i < kAfskgenStageSlots && ids[j] == ids[j - 1] + 1 && t->dirty[ids[j]] == what)
    {
      j++;
    }
    const size_t count = j - i;
    BANK_TRY(t->core.staging_wait());
    for (size_t k = 0; k < count; k++)
    {
      const AfskgenMsg *m = t->find(ids[i + k]);
      t->h_slots.p[k] = m != nullptr ? m->s : AfskgenSlot{0ull, 0ull, 0u, 0u, 0u, 0u};
      if (what == 2)
      {
        uint32_t *lv = t->h_levels.p + k * kAfskgenLevelWords;
        const size_t have = m != nullptr ? m->levels.size() : 0;
        if (have != 0)
        {
          memcpy(lv, m->levels.data(), sizeof(uint32_t) * have);
        }
        memset(lv + have, 0, sizeof(uint32_t) * (kAfskgenLevelWords - have));
      }
    }
    HIP_TRY(hipMemcpyAsync(t->d_slots + ids[i], t->h_slots, sizeof(AfskgenSlot) * count, hipMemcpyHostToDevice, st));
    if (what == 2)
    {
      HIP_TRY(hipMemcpyAsync(t->d_levels + (size_t)ids[i] * kAfskgenLevelWords, t->h_levels, sizeof(uint32_t) * kAfskgenLevelWords * count,
                             hipMemcpyHostToDevice, st));
    }
    BANK_TRY(t->core.staging_sent(st));
    for (size_t k = 0; k < count; k++)
    {
      t->dirty[ids[i + k]] = 0;
    }
    i = j;
  }
  ids.clear();
  return HRFD_OK;
}

// one call on `st`: what the setters and the clock changed, then k_afskgen; the clock moves on, on the host
static int afskgen_launch(hrfd_afskgen *t, const int16_t *d_pcm, uint64_t stride, uint32_t n_blocks, int16_t *d_out,
                          uint64_t out_stride, uint8_t *d_active, hipStream_t st)
{
  using namespace hrfd;
  const uint64_t n = (uint64_t)kGenBlock * n_blocks;
  AfskgenParams P;
  BANK_TRY(t->core.order_behind_last(st));
  {
    std::lock_guard<std::mutex> g(t->core.mu);
    P.N = t->gen.N;
    if (t->clear_slots)
    {
      // behind a reset: empty slots, then what has been queued since
      HIP_TRY(hipMemsetAsync(t->d_slots, 0, sizeof(AfskgenSlot) * kAfskgenMaxMessages * t->n_channels, st));
      t->clear_slots = false;
    }
    t->drop_ended();
    if (!t->dirty_ids.empty())
    {
      BANK_TRY(afskgen_stage(t, st));
    }
    BANK_TRY(t->gen.advance(t->n_channels, n, st));
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.out = d_out;
  P.out_stride = out_stride;
  P.slots = t->d_slots;
  P.levels = t->d_levels;
  P.anchor = t->d_anchor;
  P.clips = t->gen.d_clips;
  P.active = d_active;
  P.n_blocks = n_blocks;
  P.n_channels = t->n_channels;
  hipLaunchKernelGGL(k_afskgen, dim3(t->n_channels), dim3(kAfskgenThreads), 0, st, P, (const int16_t *)t->gen.d_sine.p);
  BANK_TRY(bank_launch_ok("k_afskgen"));
  t->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_process_device(hrfd_afskgen *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, uint32_t n_blocks,
                                           int16_t *d_out, uint64_t out_stride_bytes, uint8_t *d_active, void *stream)
{
  return hrfd::gen_process_device(t, "hrfd_afskgen_process_device", afskgen_launch, d_pcm, channel_stride_bytes, n_blocks, d_out,
                                  out_stride_bytes, d_active, stream);
}

extern "C" int hrfd_afskgen_process(hrfd_afskgen *t, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active)
{
  return hrfd::gen_process(t, "hrfd_afskgen_process", afskgen_launch, pcm, n_blocks, out, active);
}

// ---- host-only debug entries (include/hrfd_debug.h): the laws of hrfd_afskgen.h, no device
extern "C" int hrfd_afskgen_debug_levels(const uint8_t *bits, uint32_t n_bits, int nrzi, uint32_t *words)
{
  using namespace hrfd;
  if (bits == nullptr || words == nullptr || n_bits == 0 || n_bits > kAfskgenMaxBits)
  {
    return fail(HRFD_EINVAL, "hrfd_afskgen_debug_levels: need 1..%u bits and both arrays (got %u)", kAfskgenMaxBits, n_bits);
  }
  afskgen_levels(bits, n_bits, nrzi != 0, words);
  return HRFD_OK;
}

extern "C" int hrfd_afskgen_debug_length(uint32_t n_bits, uint32_t baud_step, uint64_t *length)
{
  if (length == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_afskgen_debug_length: NULL result");
  }
  return hrfd::afskgen_length("hrfd_afskgen_debug_length", n_bits, baud_step, length);
}

extern "C" int hrfd_afskgen_debug_slow(const hrfd_afskgen_message *msgs, const uint8_t *bits, const uint64_t *starts, const uint64_t *ends,
                                       uint32_t n_msgs, uint64_t N, const int16_t *pcm, uint32_t n_blocks, int16_t *out,
                                       uint8_t *active, uint64_t *clips)
{
  using namespace hrfd;
  const char *who = "hrfd_afskgen_debug_slow";
  BANK_TRY(gen_check_call(who, pcm, 0, false, n_blocks, out, 0, 1));
  BANK_TRY(gen_check_time(who, N));
  BANK_TRY(gen_check_time(who, N + (uint64_t)kGenBlock * n_blocks - 1));
  if (n_msgs > kAfskgenMaxMessages || (n_msgs != 0 && (msgs == nullptr || bits == nullptr || starts == nullptr)))
  {
    return fail(HRFD_EINVAL, "%s: at most %u messages, with their bits and starts (got %u)", who, kAfskgenMaxMessages, n_msgs);
  }
  AfskgenSlot slots[kAfskgenMaxMessages];
  std::vector<uint32_t> levels[kAfskgenMaxMessages];
  const uint32_t *lv[kAfskgenMaxMessages];
  for (uint32_t j = 0; j < n_msgs; j++)
  {
    uint64_t L = 0;
    BANK_TRY(afskgen_check_message(who, msgs + j, bits, &L));
    BANK_TRY(gen_check_time(who, starts[j]));
    const AfskgenQueue none;
    BANK_TRY(afskgen_lay_out(who, none, 0, msgs + j, L, starts[j], &slots[j]));
    if (ends != nullptr && ends[j] < slots[j].end)
    {
      slots[j].end = std::max(ends[j], slots[j].start);    // a cut message
    }
    for (uint32_t i = 0; i < j; i++)
    {
      if (slots[i].start < slots[j].end && slots[j].start < slots[i].end)
      {
        return fail(HRFD_EINVAL, "%s: messages %u and %u overlap", who, i, j);
      }
    }
    levels[j].resize((msgs[j].n_bits + 31) / 32);
    afskgen_levels(bits, msgs[j].n_bits, (msgs[j].flags & kAfskgenNrzi) != 0, levels[j].data());
    lv[j] = levels[j].data();
    bits += msgs[j].n_bits;
  }
  const uint64_t clipped = afskgen_channel_slow(pcm, n_blocks, slots, lv, n_msgs, N, Q_DDC_COS, out, active);
  if (clips != nullptr)
  {
    *clips = clipped;
  }
  return HRFD_OK;
}
