// hackrfdiags_amd/csrc/hrfd_tonegen.h -- what the tone generator bank (hrfd_tonegen_*) needs no HIP for: the limits, the law
// of one segment (phase, sine index, mix, ramp), the output with its saturation, the rules of a track's queue (laying out a
// run of segments, the merge with what is queued, the cut, dropping what has ended), the argument checks, and a slow loop over
// one channel that restates the contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_level.h
// (tests/cpp/san_tonegen.cc compiles it on the CPU; hrfd_tonegen.hip includes it for the host side and the kernel); the
// includer declares `int fail(int code, const char *fmt, ...)`, the HRFD_* codes and hrfd_tonegen_segment first.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hrfd_pcm.h"

namespace hrfd {

constexpr uint32_t kTonegenBlock = kPcmBlock;
constexpr uint32_t kTonegenTracks = 2;
constexpr uint32_t kTonegenMaxSegments = 32;   // per track and channel, those that have not ended
constexpr uint32_t kTonegenSlots = kTonegenTracks * kTonegenMaxSegments;      // 64: one per lane of a wave
constexpr uint32_t kTonegenMaxBlocks = 1024;
constexpr uint32_t kTonegenMaxAmp = 32767;
constexpr uint32_t kTonegenRamp = 64;          // samples of the ramp at either end of a segment
constexpr uint32_t kTonegenForever = 0xffffffffu;
constexpr uint64_t kTonegenAppend = ~0ull;
constexpr uint64_t kTonegenNoEnd = ~0ull;      // the end of a FOREVER segment
constexpr uint64_t kTonegenMaxTime = 1ull << 63;       // every stream time the bank computes with stays below this

// one segment as the handle keeps it and the kernel reads it (32 bytes): it sounds at stream times start <= n < end.  A cut
// can leave a FOREVER segment with an end further than 2^32 from its start, so the end is kept, not the length
struct TonegenSlot
{
  uint64_t start;
  uint64_t end;                            // kTonegenNoEnd: none
  uint32_t step_a, step_b;
  uint32_t amps;                           // amp_a below, amp_b << 16
  uint32_t pad;
};
static_assert(sizeof(TonegenSlot) == 32, "the kernel reads this layout");
constexpr TonegenSlot kTonegenEmptySlot = {~0ull, 0ull, 0u, 0u, 0u, 0u};      // start above every time, end below: no hit

// ---- 1. phase and sine: theta = step k mod 2^32 (the low 32 bits of k), i = ((theta + 2^19) >> 20) & 4095 is the tone
// bank's cosine index, and the sine is COS[(i - 1024) & 4095]: k = 0 gives COS[3072] = 0, a zero crossing
HRFD_PCM_HD uint32_t tonegen_cos_index(uint32_t theta) { return ((theta + (1u << 19)) >> 20) & 4095u; }
HRFD_PCM_HD uint32_t tonegen_sin_index(uint32_t theta) { return (tonegen_cos_index(theta) - 1024u) & 4095u; }

// ---- 2. mix: v = (amp_a S_a + amp_b S_b + 2^14) >> 15, the shift arithmetic.  |S| <= 32767 and amp <= 32767:
// 2 * 32767^2 + 2^14 < 2^31
HRFD_PCM_HD int32_t tonegen_mix(uint32_t amp_a, int32_t S_a, uint32_t amp_b, int32_t S_b)
{
  return ((int32_t)amp_a * S_a + (int32_t)amp_b * S_b + (1 << 14)) >> 15;
}

// ---- 3. ramp: e = min(k + 1, end - n, 64) and g = (v e + 32) >> 6: e = 64 gives g = v.  up = k + 1 and down = end - n,
// each already clamped to 1..64 or more by the caller (|v| <= 65534: v e < 2^23)
HRFD_PCM_HD int32_t tonegen_ramp(int32_t v, uint32_t up, uint32_t down)
{
  uint32_t e = up < down ? up : down;
  e = e < kTonegenRamp ? e : kTonegenRamp;
  return (v * (int32_t)e + 32) >> 6;
}

// one slot's g at stream time n, 0 outside the segment.  cos_table: DDC_COS
HRFD_PCM_HD int32_t tonegen_slot_at(const TonegenSlot &s, uint64_t n, const int16_t *cos_table)
{
  if (n < s.start || n >= s.end)
  {
    return 0;
  }
  const uint64_t k = n - s.start, left = s.end - n;
  const uint32_t k32 = (uint32_t)k;
  const int32_t v = tonegen_mix(s.amps & 0xffffu, cos_table[tonegen_sin_index(s.step_a * k32)], s.amps >> 16,
                                cos_table[tonegen_sin_index(s.step_b * k32)]);
  return tonegen_ramp(v, (uint32_t)(k < kTonegenRamp ? k + 1 : kTonegenRamp), (uint32_t)(left < kTonegenRamp ? left : kTonegenRamp));
}

// ---- 4. output: y = sat16(x + g0 + g1); |g| <= 65534 each.  *clipped: the saturation changed the value
HRFD_PCM_HD int32_t tonegen_output(int32_t x, int32_t g, bool *clipped)
{
  const int32_t sum = x + g, y = pcm_sat16(sum);
  *clipped = y != sum;
  return y;
}

// ---- the queue of one track: slots in order of their starts, none overlapping, only the last without an end
typedef std::vector<TonegenSlot> TonegenTrack;

inline void tonegen_drop_ended(TonegenTrack &q, uint64_t N)
{
  q.erase(std::remove_if(q.begin(), q.end(), [N](const TonegenSlot &s) { return s.end <= N; }), q.end());
}

inline uint64_t tonegen_track_end(const TonegenTrack &q) { return q.empty() ? 0 : q.back().end; }

// what one segment decides on its own
inline int tonegen_check_segments(const char *who, const hrfd_tonegen_segment *segs, uint32_t n, uint32_t track)
{
  if (track >= kTonegenTracks)
  {
    return fail(HRFD_EINVAL, "%s: track %u (0..%u)", who, track, kTonegenTracks - 1);
  }
  if (segs == nullptr || n == 0 || n > kTonegenMaxSegments)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u segments and their array (got %u)", who, kTonegenMaxSegments, n);
  }
  for (uint32_t i = 0; i < n; i++)
  {
    if (segs[i].amp_a > kTonegenMaxAmp || segs[i].amp_b > kTonegenMaxAmp)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has an amp above %u (%u, %u)", who, i, kTonegenMaxAmp, segs[i].amp_a, segs[i].amp_b);
    }
    if (segs[i].length == 0)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has length 0 (1..2^32-2, or HRFD_TONEGEN_FOREVER)", who, i);
    }
    if (segs[i].length == kTonegenForever && i + 1 < n)
    {
      return fail(HRFD_EINVAL, "%s: segment %u lies behind a FOREVER segment", who, i + 1);
    }
  }
  return HRFD_OK;
}

inline int tonegen_check_time(const char *who, uint64_t N)
{
  if (N >= kTonegenMaxTime)
  {
    return fail(HRFD_EINVAL, "%s: stream time %llu (below 2^63)", who, (unsigned long long)N);
  }
  return HRFD_OK;
}

// The run segs[0..n) laid out from `start` (kTonegenAppend: max(N, the track's end)) and merged into what `q` holds that has
// not ended at N: `merged` is the track as it would be.  Refused whole, with `q` as it was: a start before N, an overlap, a
// segment behind a FOREVER one, more than 32 that have not ended, a time at or above 2^63.  segs has passed
// tonegen_check_segments
inline int tonegen_lay_out(const char *who, const TonegenTrack &q, uint64_t N, const hrfd_tonegen_segment *segs, uint32_t n,
                           uint64_t start, TonegenTrack &merged)
{
  merged = q;
  tonegen_drop_ended(merged, N);
  uint64_t at;
  if (start == kTonegenAppend)
  {
    const uint64_t end = tonegen_track_end(merged);
    if (end == kTonegenNoEnd)
    {
      return fail(HRFD_EINVAL, "%s: nothing can be appended behind a FOREVER segment", who);
    }
    at = end > N ? end : N;
  }
  else
  {
    if (start < N)
    {
      return fail(HRFD_EINVAL, "%s: start %llu lies before the stream time %llu", who, (unsigned long long)start,
                  (unsigned long long)N);
    }
    at = start;
  }
  for (uint32_t i = 0; i < n; i++)
  {
    // at < 2^63 and gap, length < 2^32: no sum wraps
    TonegenSlot s;
    s.start = at + segs[i].gap;
    s.end = segs[i].length == kTonegenForever ? kTonegenNoEnd : s.start + segs[i].length;
    s.step_a = segs[i].step_a;
    s.step_b = segs[i].step_b;
    s.amps = segs[i].amp_a | (segs[i].amp_b << 16);
    s.pad = 0;
    if (at >= kTonegenMaxTime || s.start >= kTonegenMaxTime || (s.end != kTonegenNoEnd && s.end >= kTonegenMaxTime))
    {
      return fail(HRFD_EINVAL, "%s: segment %u would lie at or above stream time 2^63", who, i);
    }
    merged.push_back(s);
    at = s.end;                            // (behind a FOREVER segment there is no next one)
  }
  std::stable_sort(merged.begin(), merged.end(), [](const TonegenSlot &a, const TonegenSlot &b) { return a.start < b.start; });
  for (size_t i = 0; i + 1 < merged.size(); i++)
  {
    if (merged[i].end == kTonegenNoEnd)
    {
      return fail(HRFD_EINVAL, "%s: a segment at %llu would lie behind the FOREVER segment at %llu", who,
                  (unsigned long long)merged[i + 1].start, (unsigned long long)merged[i].start);
    }
    if (merged[i].end > merged[i + 1].start)
    {
      return fail(HRFD_EINVAL, "%s: the segments at %llu and %llu would overlap on the track", who,
                  (unsigned long long)merged[i].start, (unsigned long long)merged[i + 1].start);
    }
  }
  if (merged.size() > kTonegenMaxSegments)
  {
    return fail(HRFD_EINVAL, "%s: %zu segments that have not ended on one track (at most %u)", who, merged.size(),
                kTonegenMaxSegments);
  }
  return HRFD_OK;
}

// the segment in progress at N ends at min(its end, N + 64): under the law a ramp down; those not yet begun are dropped
inline void tonegen_cut(TonegenTrack &q, uint64_t N)
{
  tonegen_drop_ended(q, N);
  q.erase(std::remove_if(q.begin(), q.end(), [N](const TonegenSlot &s) { return s.start > N; }), q.end());
  for (TonegenSlot &s : q)
  {
    s.end = std::min(s.end, N + kTonegenRamp);
  }
}

// the 64 slots of a channel as the kernel reads them: track t in slots 32 t .. 32 t + 31, the unused ones empty
inline void tonegen_fill_slots(const TonegenTrack *tracks, TonegenSlot *slots)
{
  for (uint32_t t = 0; t < kTonegenTracks; t++)
  {
    for (uint32_t i = 0; i < kTonegenMaxSegments; i++)
    {
      slots[t * kTonegenMaxSegments + i] = i < tracks[t].size() ? tracks[t][i] : kTonegenEmptySlot;
    }
  }
}

// ---- one channel, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512] or NULL (generate only); slots: its 64; N: the stream time of the first sample;
// cos_table: DDC_COS; out [n_blocks][512], may be pcm_row itself; active [n_blocks] or NULL.  Returns the clipped samples
inline uint64_t tonegen_channel_slow(const int16_t *pcm_row, uint32_t n_blocks, const TonegenSlot *slots, uint64_t N,
                                     const int16_t *cos_table, int16_t *out, uint8_t *active)
{
  uint64_t clips = 0;
  for (uint32_t b = 0; b < n_blocks; b++)
  {
    const uint64_t b0 = N + (uint64_t)b * kTonegenBlock, b1 = b0 + kTonegenBlock;
    if (active != nullptr)
    {
      uint8_t bits = 0;
      for (uint32_t j = 0; j < kTonegenSlots; j++)
      {
        if (slots[j].start < b1 && slots[j].end > b0)
        {
          bits |= (uint8_t)(1u << (j / kTonegenMaxSegments));
        }
      }
      active[b] = bits;
    }
    for (uint32_t i = 0; i < kTonegenBlock; i++)
    {
      const size_t at = (size_t)b * kTonegenBlock + i;
      int32_t g = 0;
      for (uint32_t j = 0; j < kTonegenSlots; j++)
      {
        g += tonegen_slot_at(slots[j], b0 + i, cos_table);
      }
      bool clipped;
      out[at] = (int16_t)tonegen_output(pcm_row != nullptr ? pcm_row[at] : 0, g, &clipped);
      clips += clipped ? 1 : 0;
    }
  }
  return clips;
}

// ---- the checks, each under `who`, the public function's name
inline int tonegen_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

inline int tonegen_check_track(const char *who, uint32_t channel, uint32_t track, uint32_t n_channels)
{
  if (track >= kTonegenTracks)
  {
    return fail(HRFD_EINVAL, "%s: track %u (0..%u)", who, track, kTonegenTracks - 1);
  }
  return pcm_check_channel(who, channel, n_channels);
}

// what a process call's sizes and addresses decide without a handle; n_channels: the handle's, or 1 where there is none
// yet (the ranges that must not overlap grow with it).  The dense host entry has no strides.  pcm may be NULL: generate only
inline int tonegen_check_call(const char *who, const void *pcm, uint64_t in_stride, bool device_entry, uint32_t n_blocks,
                              const void *out, uint64_t out_stride, uint32_t n_channels)
{
  if (n_blocks == 0 || n_blocks > kTonegenMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kTonegenMaxBlocks, n_blocks);
  }
  if (out == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument (out)", who);
  }
  const uint64_t row = 2ull * kTonegenBlock * n_blocks;
  if (device_entry)
  {
    if (pcm != nullptr)
    {
      BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", in_stride, row));
    }
    BANK_TRY(pcm_check_stride(who, "out_stride_bytes", out_stride, row));
  }
  if (!pcm_aligned(pcm, 2) || !pcm_aligned(out, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM and out must sit at even addresses", who);
  }
  const uint64_t si = device_entry ? in_stride : row, so = device_entry ? out_stride : row;
  if (pcm != nullptr && !(out == pcm && si == so))
  {
    return pcm_check_no_overlap(who, pcm, si, row, out, so, row, n_channels,
                                "in place means out at the input's own address and stride, where every sample is read by the "
                                "lane that overwrites it; anywhere else a workgroup would overwrite what another still reads");
  }
  return HRFD_OK;
}

} // namespace hrfd
