// hackrfdiags_amd/csrc/hrfd_dcsgen.h -- what the DCS generator bank (hrfd_dcsgen_*) needs no HIP for, on top of what it shares
// with the tone and AFSK generators (hrfd_gen.h: the limits of a call, the output with its saturation, the checks of a time
// and of a process call): its limits, the laws (the bit grid and the turn-off grid, periodic in 28750 samples; the raw level of
// one segment), the rules of a channel's queue (laying out a run of segments, the merge with what is queued, the cut with and
// without the turn-off tail, dropping what has ended), its own argument checks, and a slow loop over one channel that
// restates the contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_dcs.h (tests/cpp/san_dcsgen.cc compiles it
// on the CPU; hrfd_dcsgen.hip includes it for the host side and the kernel); the includer declares
// `int fail(int code, const char *fmt, ...)`, the HRFD_* codes and hrfd_dcsgen_segment first.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hrfd_gen.h"

namespace hrfd {

constexpr uint32_t kDcsgenMaxSegments = 8;     // per channel, those that have not ended: one slot each
constexpr uint32_t kDcsgenMaxTaps = 512;
constexpr uint32_t kDcsgenForever = 0xffffffffu;
constexpr uint32_t kDcsgenDefaultTail = 1440;  // 180 ms of turn-off code
constexpr uint64_t kDcsgenNoEnd = ~0ull;       // the code part's end and the end of a FOREVER segment
constexpr uint32_t kDcsgenWordMask = 0x7fffffu;
constexpr uint32_t kDcsgenPeriod = 28750;      // 23 * 1250 samples = 483 = 21 * 23 bit times: both grids repeat
constexpr uint32_t kDcsgenReach = 511;         // a segment has ended when E + 511 <= N, whatever T is: T - 1 <= 511
static_assert(kDcsgenMaxTaps - 1 <= kDcsgenReach, "no filter reaches a segment that has ended");
static_assert(21ull * (kDcsgenPeriod - 1) / 1250 == 482 && 42ull * (kDcsgenPeriod - 1) < (1ull << 32), "the grids in 32 bits");

// ---- 1. and 2. the grids, over u = n mod 28750
HRFD_PCM_HD uint32_t dcsgen_u(uint64_t n) { return (uint32_t)(n % kDcsgenPeriod); }
HRFD_PCM_HD uint32_t dcsgen_bit_index(uint32_t u) { return (21u * u / 1250u) % 23u; }
HRFD_PCM_HD bool dcsgen_sq_low(uint32_t u) { return ((42u * u / 1250u) & 1u) != 0; }      // the turn-off code's second half bit

// one segment as the handle keeps it and the kernel reads it (32 bytes): the code at start <= n < mid, the turn-off code at
// mid <= n < end.  A cut can leave a FOREVER segment with times further than 2^32 from its start, so times are kept
struct DcsgenSlot
{
  uint64_t start;
  uint64_t mid;                            // start + L; kDcsgenNoEnd: FOREVER
  uint64_t end;                            // mid + Q; kDcsgenNoEnd: FOREVER
  uint32_t word, amp;
};
static_assert(sizeof(DcsgenSlot) == 32, "the kernel reads this layout");
constexpr DcsgenSlot kDcsgenEmptySlot = {~0ull, ~0ull, 0ull, 0u, 0u};      // start above every time, end below: no hit

// ---- 3. the raw level of one slot at stream time n with u = n mod 28750; 0 outside the segment
HRFD_PCM_HD int32_t dcsgen_slot_at(const DcsgenSlot &s, uint64_t n, uint32_t u)
{
  if (n < s.start || n >= s.end)
  {
    return 0;
  }
  const int32_t a = (int32_t)s.amp;
  if (n < s.mid)
  {
    return ((s.word >> dcsgen_bit_index(u)) & 1u) ? a : -a;
  }
  return dcsgen_sq_low(u) ? -a : a;
}

// ---- 4. g = (acc + 2^13) >> 14, not saturated: |acc| <= 65535 * 32767, so acc + 2^13 < 2^31 and |g| <= 131066
HRFD_PCM_HD int32_t dcsgen_round(int32_t acc) { return (acc + (1 << 13)) >> 14; }

// ---- 7. the queue of one channel: segments in order of their starts, none overlapping, only the last without an end.  The
// host keeps the tail a FOREVER segment was queued with beside the slot: a cut needs it
struct DcsgenSeg
{
  DcsgenSlot s;
  uint32_t tail;
};
typedef std::vector<DcsgenSeg> DcsgenQueue;

HRFD_PCM_HD bool dcsgen_ended(const DcsgenSlot &s, uint64_t N) { return s.end != kDcsgenNoEnd && s.end + kDcsgenReach <= N; }

inline void dcsgen_drop_ended(DcsgenQueue &q, uint64_t N)
{
  q.erase(std::remove_if(q.begin(), q.end(), [N](const DcsgenSeg &g) { return dcsgen_ended(g.s, N); }), q.end());
}

// the time below which nothing of the queue leaves it: min(E + 511), kDcsgenNoEnd for none
inline uint64_t dcsgen_next_end(const DcsgenQueue &q)
{
  uint64_t v = kDcsgenNoEnd;
  for (const DcsgenSeg &g : q)
  {
    v = std::min(v, g.s.end == kDcsgenNoEnd ? kDcsgenNoEnd : g.s.end + kDcsgenReach);
  }
  return v;
}

// what one segment decides on its own
inline int dcsgen_check_segments(const char *who, const hrfd_dcsgen_segment *segs, uint32_t n)
{
  if (segs == nullptr || n == 0 || n > kDcsgenMaxSegments)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u segments and their array (got %u)", who, kDcsgenMaxSegments, n);
  }
  for (uint32_t i = 0; i < n; i++)
  {
    if (segs[i].amp > kGenMaxAmp)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has an amp above %u (%u)", who, i, kGenMaxAmp, segs[i].amp);
    }
    if (segs[i].word > kDcsgenWordMask)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has the word 0x%x (23 bits: at most 0x7fffff)", who, i, segs[i].word);
    }
    if (segs[i].length == 0)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has length 0 (1..2^32-2, or HRFD_DCSGEN_FOREVER)", who, i);
    }
    if (segs[i].tail == 0xffffffffu)
    {
      return fail(HRFD_EINVAL, "%s: segment %u has a tail of 2^32-1 samples (0..2^32-2)", who, i);
    }
    if (segs[i].length == kDcsgenForever && i + 1 < n)
    {
      return fail(HRFD_EINVAL, "%s: segment %u lies behind a FOREVER segment", who, i + 1);
    }
  }
  return HRFD_OK;
}

// The run segs[0..n) laid out from `start` (kGenAppend: max(N, the last E)) and merged into what `q` holds that has not ended
// at N: `merged` is the queue as it would be.  Refused whole, with `q` as it was: a start before N, an overlap, a segment
// behind a FOREVER one, more than 8 that have not ended, a time at or above 2^63.  segs has passed dcsgen_check_segments
inline int dcsgen_lay_out(const char *who, const DcsgenQueue &q, uint64_t N, const hrfd_dcsgen_segment *segs, uint32_t n,
                          uint64_t start, DcsgenQueue &merged)
{
  merged = q;
  dcsgen_drop_ended(merged, N);
  uint64_t at;
  if (start == kGenAppend)
  {
    const uint64_t end = merged.empty() ? 0 : merged.back().s.end;
    if (end == kDcsgenNoEnd)
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
    // at < 2^63 and gap, length, tail < 2^32: no sum wraps
    DcsgenSeg g;
    const bool forever = segs[i].length == kDcsgenForever;
    g.s.start = at + segs[i].gap;
    g.s.mid = forever ? kDcsgenNoEnd : g.s.start + segs[i].length;
    g.s.end = forever ? kDcsgenNoEnd : g.s.mid + segs[i].tail;
    g.s.word = segs[i].word;
    g.s.amp = segs[i].amp;
    g.tail = segs[i].tail;
    if (at >= kGenMaxTime || g.s.start >= kGenMaxTime || (!forever && g.s.end >= kGenMaxTime))
    {
      return fail(HRFD_EINVAL, "%s: segment %u would lie at or above stream time 2^63", who, i);
    }
    merged.push_back(g);
    at = g.s.end;                          // (behind a FOREVER segment there is no next one)
  }
  std::stable_sort(merged.begin(), merged.end(), [](const DcsgenSeg &a, const DcsgenSeg &b) { return a.s.start < b.s.start; });
  for (size_t i = 0; i + 1 < merged.size(); i++)
  {
    if (merged[i].s.end == kDcsgenNoEnd)
    {
      return fail(HRFD_EINVAL, "%s: a segment at %llu would lie behind the FOREVER segment at %llu", who,
                  (unsigned long long)merged[i + 1].s.start, (unsigned long long)merged[i].s.start);
    }
    if (merged[i].s.end > merged[i + 1].s.start)
    {
      return fail(HRFD_EINVAL, "%s: the segments at %llu and %llu would overlap", who, (unsigned long long)merged[i].s.start,
                  (unsigned long long)merged[i + 1].s.start);
    }
  }
  if (merged.size() > kDcsgenMaxSegments)
  {
    return fail(HRFD_EINVAL, "%s: %zu segments that have not ended on one channel (at most %u)", who, merged.size(),
                kDcsgenMaxSegments);
  }
  return HRFD_OK;
}

// the cut at N.  In its code part (S <= N < S + L): the code part ends now and the tail, if asked for, follows (E stays
// below 2^63); S = N: dropped.  In its tail: unchanged with the tail, E = N without.  Not yet begun: dropped.  E <= N:
// untouched.  No sample before N changes
inline void dcsgen_cut(DcsgenQueue &q, uint64_t N, bool with_tail)
{
  dcsgen_drop_ended(q, N);
  q.erase(std::remove_if(q.begin(), q.end(), [N](const DcsgenSeg &g) { return g.s.start >= N; }), q.end());
  for (DcsgenSeg &g : q)
  {
    if (N < g.s.mid)
    {
      g.s.mid = N;
      g.s.end = std::min(N + (with_tail ? g.tail : 0u), kGenMaxTime - 1);
    }
    else if (N < g.s.end && !with_tail)
    {
      g.s.end = N;
    }
  }
}

// the 8 slots of a channel as the kernel reads them, the unused ones empty
inline void dcsgen_fill_slots(const DcsgenQueue &q, DcsgenSlot *slots)
{
  for (uint32_t i = 0; i < kDcsgenMaxSegments; i++)
  {
    slots[i] = i < q.size() ? q[i].s : kDcsgenEmptySlot;
  }
}

// ---- one channel, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512] or NULL (generate only); slots: its 8; taps: T of them; N: the stream time of the
// first sample; out [n_blocks][512], may be pcm_row itself; active [n_blocks] or NULL.  Returns the clipped samples
inline uint64_t dcsgen_channel_slow(const int16_t *pcm_row, uint32_t n_blocks, const DcsgenSlot *slots, const int16_t *taps,
                                    uint32_t T, uint64_t N, int16_t *out, uint8_t *active)
{
  const uint32_t n = n_blocks * kGenBlock;
  // r at the stream times N - 511 .. N + n - 1; 0 in front of the stream's start
  std::vector<int32_t> r(kDcsgenReach + n, 0);
  uint32_t u = (dcsgen_u(N) + kDcsgenPeriod - kDcsgenReach) % kDcsgenPeriod;
  for (uint32_t i = 0; i < kDcsgenReach + n; i++)
  {
    if (N + i >= kDcsgenReach)
    {
      const uint64_t t = N + i - kDcsgenReach;
      for (uint32_t j = 0; j < kDcsgenMaxSegments; j++)
      {
        r[i] += dcsgen_slot_at(slots[j], t, u);
      }
    }
    u = u + 1 == kDcsgenPeriod ? 0 : u + 1;
  }
  uint64_t clips = 0;
  for (uint32_t b = 0; b < n_blocks; b++)
  {
    const uint64_t b0 = N + (uint64_t)b * kGenBlock, b1 = b0 + kGenBlock;
    if (active != nullptr)
    {
      uint8_t on = 0;
      for (uint32_t j = 0; j < kDcsgenMaxSegments; j++)
      {
        if (slots[j].start < b1 && (slots[j].end == kDcsgenNoEnd || slots[j].end + (T - 1) > b0))
        {
          on = 1;
        }
      }
      active[b] = on;
    }
    for (uint32_t i = 0; i < kGenBlock; i++)
    {
      const size_t at = (size_t)b * kGenBlock + i;
      int32_t acc = 0;                         // sum |h| <= 65535 and |r| <= 32767: every partial sum fits
      for (uint32_t j = 0; j < T; j++)
      {
        acc += (int32_t)taps[j] * r[kDcsgenReach + at - j];
      }
      bool clipped;
      out[at] = (int16_t)gen_output(pcm_row != nullptr ? pcm_row[at] : 0, dcsgen_round(acc), &clipped);
      clips += clipped ? 1 : 0;
    }
  }
  return clips;
}

// ---- the checks, each under `who`, the public function's name
inline int dcsgen_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

inline int dcsgen_check_taps(const char *who, const int16_t *taps, uint32_t n)
{
  if (n == 0 || n > kDcsgenMaxTaps || taps == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u taps and their array (got %u)", who, kDcsgenMaxTaps, n);
  }
  return bank_tap_sums_ok(who, taps, n, 1);
}

} // namespace hrfd
