// hackrfdiags_amd/csrc/hrfd_tonegen.h -- what the tone generator bank (hrfd_tonegen_*) needs no HIP for, on top of what it
// shares with the AFSK generator (hrfd_gen.h: the limits of a call, sine index, mix, ramp, output, the checks of a time and
// of a process call): the limits of its queues, the law of one segment, the rules of a track's queue (laying out a run of
// segments, the merge with what is queued, the cut, dropping what has ended), its own argument checks, and a slow loop over
// one channel that restates the contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_level.h
// (tests/cpp/san_tonegen.cc compiles it on the CPU; hrfd_tonegen.hip includes it for the host side and the kernel); the
// includer declares `int fail(int code, const char *fmt, ...)`, the HRFD_* codes and hrfd_tonegen_segment first.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hrfd_gen.h"

namespace hrfd {

constexpr uint32_t kTonegenTracks = 2;
constexpr uint32_t kTonegenMaxSegments = 32;   // per track and channel, those that have not ended
constexpr uint32_t kTonegenSlots = kTonegenTracks * kTonegenMaxSegments;      // 64: one per lane of a wave
constexpr uint32_t kTonegenForever = 0xffffffffu;
constexpr uint64_t kTonegenNoEnd = ~0ull;      // the end of a FOREVER segment

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

// one slot's g at stream time n, 0 outside the segment.  cos_table: DDC_COS
HRFD_PCM_HD int32_t tonegen_slot_at(const TonegenSlot &s, uint64_t n, const int16_t *cos_table)
{
  if (n < s.start || n >= s.end)
  {
    return 0;
  }
  const uint64_t k = n - s.start, left = s.end - n;
  const uint32_t k32 = (uint32_t)k;
  const int32_t v = gen_mix(s.amps & 0xffffu, cos_table[gen_sin_index(s.step_a * k32)], s.amps >> 16,
                            cos_table[gen_sin_index(s.step_b * k32)]);
  return gen_ramp(v, (uint32_t)(k < kGenRamp ? k + 1 : kGenRamp), (uint32_t)(left < kGenRamp ? left : kGenRamp));
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
    if (segs[i].amp_a > kGenMaxAmp || segs[i].amp_b > kGenMaxAmp)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has an amp above %u (%u, %u)", who, i, kGenMaxAmp, segs[i].amp_a, segs[i].amp_b);
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

// The run segs[0..n) laid out from `start` (kGenAppend: max(N, the track's end)) and merged into what `q` holds that has
// not ended at N: `merged` is the track as it would be.  Refused whole, with `q` as it was: a start before N, an overlap, a
// segment behind a FOREVER one, more than 32 that have not ended, a time at or above 2^63.  segs has passed
// tonegen_check_segments
inline int tonegen_lay_out(const char *who, const TonegenTrack &q, uint64_t N, const hrfd_tonegen_segment *segs, uint32_t n,
                           uint64_t start, TonegenTrack &merged)
{
  merged = q;
  tonegen_drop_ended(merged, N);
  uint64_t at;
  if (start == kGenAppend)
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
    if (at >= kGenMaxTime || s.start >= kGenMaxTime || (s.end != kTonegenNoEnd && s.end >= kGenMaxTime))
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
    s.end = std::min(s.end, N + kGenRamp);
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
    const uint64_t b0 = N + (uint64_t)b * kGenBlock, b1 = b0 + kGenBlock;
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
    for (uint32_t i = 0; i < kGenBlock; i++)
    {
      const size_t at = (size_t)b * kGenBlock + i;
      int32_t g = 0;
      for (uint32_t j = 0; j < kTonegenSlots; j++)
      {
        g += tonegen_slot_at(slots[j], b0 + i, cos_table);
      }
      bool clipped;
      out[at] = (int16_t)gen_output(pcm_row != nullptr ? pcm_row[at] : 0, g, &clipped);
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

} // namespace hrfd
