// hackrfdiags_amd/csrc/hrfd_afskgen.h -- what the AFSK generator bank (hrfd_afskgen_*) needs no HIP for: the limits, the law
// of one message (levels, length, the bit of a sample, the phase as a running sum), the rules of a channel's queue (laying a
// message out, the merge with what is queued, the cut, dropping what has ended), the argument checks, and a slow loop over
// one channel that restates the contract of include/hrfd.h sample by sample.  The limits of a call, the sine index, the
// mix, the ramp, the output and the checks of a time and of a process call are the ones it shares with the tone generator
// (hrfd_gen.h).  Plain C++ like hrfd_tonegen.h (tests/cpp/san_afskgen.cc compiles it on the CPU; hrfd_afskgen.hip includes
// it for the host side and the kernel); the includer declares `int fail(int code, const char *fmt, ...)`, the HRFD_* codes
// and hrfd_afskgen_message first.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hrfd_gen.h"

namespace hrfd {

constexpr uint32_t kAfskgenMaxMessages = 4;    // per channel, those that have not ended: the slots of the device's copy
constexpr uint32_t kAfskgenMaxBits = 8192;     // data bits of one message
constexpr uint32_t kAfskgenLevelWords = kAfskgenMaxBits / 32;     // 256 dwords = 1 KiB of levels a slot
constexpr uint32_t kAfskgenMaxStep = 1u << 31;
constexpr uint32_t kAfskgenNrzi = 1u;          // bit 0 of a message's flags
constexpr uint64_t kAfskgenMaxLength = 1ull << 31;     // L stays below this: k fits 31 bits

// one message as the kernel reads it (32 bytes): it sounds at stream times start <= n < end.  A cut moves the end in front
// of start + L; all zeros is an empty slot (no end lies above a stream time)
struct AfskgenSlot
{
  uint64_t start;
  uint64_t end;
  uint32_t mark_step, space_step, baud_step;
  uint32_t amp;
};
static_assert(sizeof(AfskgenSlot) == 32, "the kernel reads this layout");

// one message as the handle keeps it: its slot of the device's copy (0..3, its own until it has ended) and its levels, bit
// i & 31 of word i >> 5 = l[i], whole words, zero behind the last bit
struct AfskgenMsg
{
  AfskgenSlot s;
  uint32_t slot;
  std::vector<uint32_t> levels;
};
typedef std::vector<AfskgenMsg> AfskgenQueue;  // in order of the starts, none overlapping

// ---- 1. levels: l[i] = d[i] & 1, or with NRZI l[-1] = 1 (mark) and a data 1 keeps the level, a 0 turns it over.  words:
// (n_bits + 31) / 32 of them, written whole
inline void afskgen_levels(const uint8_t *bits, uint32_t n_bits, bool nrzi, uint32_t *words)
{
  for (uint32_t w = 0; w < (n_bits + 31) / 32; w++)
  {
    words[w] = 0u;
  }
  uint32_t level = 1u;
  for (uint32_t i = 0; i < n_bits; i++)
  {
    const uint32_t d = bits[i] & 1u;
    level = nrzi ? (d ? level : 1u - level) : d;
    words[i >> 5] |= level << (i & 31u);
  }
}

// ---- 2. length: L = ceil(n_bits 2^32 / baud_step), the least k with (k baud_step) >> 32 >= n_bits.  n_bits < 2^32, so
// n_bits << 32 fits 64 bits.  Refused: L >= 2^31.  (The queue takes n_bits <= 8192 only; the law holds for every n_bits)
inline int afskgen_length(const char *who, uint32_t n_bits, uint32_t baud_step, uint64_t *L)
{
  if (n_bits == 0 || baud_step == 0 || baud_step > kAfskgenMaxStep)
  {
    return fail(HRFD_EINVAL, "%s: n_bits %u, baud_step %u (at least one bit, a step of 1..2^31)", who, n_bits, baud_step);
  }
  const uint64_t v = (uint64_t)n_bits << 32;
  const uint64_t len = v / baud_step + (v % baud_step != 0 ? 1u : 0u);
  if (len >= kAfskgenMaxLength)
  {
    return fail(HRFD_EINVAL, "%s: %u bits at baud_step %u are %llu samples (below 2^31)", who, n_bits, baud_step,
                (unsigned long long)len);
  }
  *L = len;
  return HRFD_OK;
}

// ---- 3. the bit of sample k < 2^31: (k baud_step) >> 32 as a 64-bit product, and its level
HRFD_PCM_HD uint32_t afskgen_bit(uint32_t k, uint32_t baud_step) { return (uint32_t)(((uint64_t)k * baud_step) >> 32); }
HRFD_PCM_HD uint32_t afskgen_level(const uint32_t *levels, uint32_t bit) { return (levels[bit >> 5] >> (bit & 31u)) & 1u; }
HRFD_PCM_HD uint32_t afskgen_step(const AfskgenSlot &s, const uint32_t *levels, uint32_t k)
{
  return afskgen_level(levels, afskgen_bit(k, s.baud_step)) != 0u ? s.mark_step : s.space_step;
}

// the first sample of bit b: ceil(b 2^32 / baud_step)
inline uint64_t afskgen_first_sample(uint64_t b, uint32_t baud_step)
{
  const uint64_t v = b << 32;
  return v / baud_step + (v % baud_step != 0 ? 1u : 0u);
}

// ---- 4. phase: theta(0) = 0, theta(k + 1) = theta(k) + st(k) mod 2^32.  theta(k) for any k <= L without the walk over the
// samples: every bit in front of k adds its step once per sample it holds
inline uint32_t afskgen_theta_at(const AfskgenSlot &s, const uint32_t *levels, uint64_t k)
{
  uint32_t theta = 0;
  uint64_t lo = 0;
  for (uint32_t b = 0; lo < k; b++)
  {
    const uint64_t hi = std::min<uint64_t>(afskgen_first_sample((uint64_t)b + 1, s.baud_step), k);
    theta += (uint32_t)(hi - lo) * (afskgen_level(levels, b) != 0u ? s.mark_step : s.space_step);
    lo = hi;
  }
  return theta;
}

// ---- 5. one sample: g at stream time n inside the message, theta = theta(n - start)
HRFD_PCM_HD int32_t afskgen_sample(const AfskgenSlot &s, uint64_t n, uint32_t theta, const int16_t *cos_table)
{
  const uint64_t k = n - s.start, left = s.end - n;
  const int32_t v = gen_mix(s.amp, cos_table[gen_sin_index(theta)], 0u, 0);
  return gen_ramp(v, (uint32_t)(k < kGenRamp ? k + 1 : kGenRamp), (uint32_t)(left < kGenRamp ? left : kGenRamp));
}

// ---- the queue of one channel
inline void afskgen_drop_ended(AfskgenQueue &q, uint64_t N)
{
  q.erase(std::remove_if(q.begin(), q.end(), [N](const AfskgenMsg &m) { return m.s.end <= N; }), q.end());
}

inline uint32_t afskgen_count_pending(const AfskgenQueue &q, uint64_t N, uint64_t *last_end)
{
  uint32_t count = 0;
  uint64_t last = N;
  for (const AfskgenMsg &m : q)
  {
    if (m.s.end > N)
    {
      count++;
      last = m.s.end;
    }
  }
  if (last_end != nullptr)
  {
    *last_end = last;
  }
  return count;
}

// what a message decides on its own; *L: its length
inline int afskgen_check_message(const char *who, const hrfd_afskgen_message *msg, const uint8_t *bits, uint64_t *L)
{
  if (msg == nullptr || bits == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument (msg, bits)", who);
  }
  if (msg->n_bits == 0 || msg->n_bits > kAfskgenMaxBits)
  {
    return fail(HRFD_EINVAL, "%s: n_bits must be 1..%u (got %u)", who, kAfskgenMaxBits, msg->n_bits);
  }
  const uint32_t steps[3] = {msg->mark_step, msg->space_step, msg->baud_step};
  const char *names[3] = {"mark_step", "space_step", "baud_step"};
  for (int i = 0; i < 3; i++)
  {
    if (steps[i] == 0 || steps[i] > kAfskgenMaxStep)
    {
      return fail(HRFD_EINVAL, "%s: %s must be 1..2^31 (got %u)", who, names[i], steps[i]);
    }
  }
  if (msg->amp > kGenMaxAmp)
  {
    return fail(HRFD_EINVAL, "%s: amp above %u (%u)", who, kGenMaxAmp, msg->amp);
  }
  if ((msg->flags & ~kAfskgenNrzi) != 0 || msg->pad != 0)
  {
    return fail(HRFD_EINVAL, "%s: flags 0x%x, pad %u (only bit 0 of flags, NRZI, and a pad of 0)", who, msg->flags, msg->pad);
  }
  return afskgen_length(who, msg->n_bits, msg->baud_step, L);
}

// The message laid out from `start` (kGenAppend: max(N, the end of the channel's last message)) against what `q` holds
// that has not ended at N: *slot is the message as it would be queued.  Refused, with `q` as it was: a start before N, an
// overlap, a fifth message that has not ended, a time at or above 2^63.  msg has passed afskgen_check_message, which gave L
inline int afskgen_lay_out(const char *who, const AfskgenQueue &q, uint64_t N, const hrfd_afskgen_message *msg, uint64_t L,
                           uint64_t start, AfskgenSlot *slot)
{
  uint64_t at;
  if (start == kGenAppend)
  {
    afskgen_count_pending(q, N, &at);                      // N where nothing is pending
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
  // at < 2^63 is checked first; gap < 2^32 and L < 2^31: no sum wraps
  AfskgenSlot s;
  s.start = at + msg->gap;
  s.end = s.start + L;
  s.mark_step = msg->mark_step;
  s.space_step = msg->space_step;
  s.baud_step = msg->baud_step;
  s.amp = msg->amp;
  if (at >= kGenMaxTime || s.start >= kGenMaxTime || s.end >= kGenMaxTime)
  {
    return fail(HRFD_EINVAL, "%s: the message would lie at or above stream time 2^63", who);
  }
  uint32_t pending = 0;
  for (const AfskgenMsg &m : q)
  {
    if (m.s.end <= N)
    {
      continue;
    }
    pending++;
    if (m.s.start < s.end && s.start < m.s.end)
    {
      return fail(HRFD_EINVAL, "%s: the messages at %llu and %llu would overlap", who, (unsigned long long)std::min(m.s.start, s.start),
                  (unsigned long long)std::max(m.s.start, s.start));
    }
  }
  if (pending >= kAfskgenMaxMessages)
  {
    return fail(HRFD_EINVAL, "%s: %u messages that have not ended on the channel (at most %u)", who, pending + 1, kAfskgenMaxMessages);
  }
  *slot = s;
  return HRFD_OK;
}

// the message that afskgen_lay_out accepted goes into the queue, in the order of the starts, on a slot no pending message
// holds.  Returns the slot.  q holds no ended message (afskgen_drop_ended first)
inline uint32_t afskgen_insert(AfskgenQueue &q, const AfskgenSlot &s, std::vector<uint32_t> &&levels)
{
  uint32_t used = 0;
  for (const AfskgenMsg &m : q)
  {
    used |= 1u << m.slot;
  }
  uint32_t slot = 0;
  while ((used >> slot) & 1u)
  {
    slot++;
  }
  AfskgenMsg m;
  m.s = s;
  m.slot = slot;
  m.levels = std::move(levels);
  q.insert(std::upper_bound(q.begin(), q.end(), m, [](const AfskgenMsg &a, const AfskgenMsg &b) { return a.s.start < b.s.start; }),
           std::move(m));
  return slot;
}

// the message in progress at N ends at min(its end, N + 64): under the law a ramp down; those not yet begun are dropped.
// q holds no ended message
inline void afskgen_cut(AfskgenQueue &q, uint64_t N)
{
  q.erase(std::remove_if(q.begin(), q.end(), [N](const AfskgenMsg &m) { return m.s.start > N; }), q.end());
  for (AfskgenMsg &m : q)
  {
    m.s.end = std::min(m.s.end, N + kGenRamp);
  }
}

// ---- one channel, sample by sample (the contract as a loop; the kernel must agree bit for bit)
// pcm_row: the channel's [n_blocks][512] or NULL (generate only); msgs[0..n_msgs) with their level words: the channel's,
// none overlapping; N: the stream time of the first sample; cos_table: DDC_COS; out [n_blocks][512], may be pcm_row itself;
// active [n_blocks] or NULL.  Returns the clipped samples
inline uint64_t afskgen_channel_slow(const int16_t *pcm_row, uint32_t n_blocks, const AfskgenSlot *msgs, const uint32_t *const *levels,
                                     uint32_t n_msgs, uint64_t N, const int16_t *cos_table, int16_t *out, uint8_t *active)
{
  const uint64_t n = (uint64_t)n_blocks * kGenBlock;
  if (out != pcm_row)
  {
    for (uint64_t i = 0; i < n; i++)
    {
      out[i] = pcm_row != nullptr ? pcm_row[i] : (int16_t)0;
    }
  }
  if (active != nullptr)
  {
    for (uint32_t b = 0; b < n_blocks; b++)
    {
      const uint64_t b0 = N + (uint64_t)b * kGenBlock, b1 = b0 + kGenBlock;
      active[b] = 0;
      for (uint32_t j = 0; j < n_msgs; j++)
      {
        active[b] |= (uint8_t)(msgs[j].start < b1 && msgs[j].end > b0 ? 1 : 0);
      }
    }
  }
  uint64_t clips = 0;
  for (uint32_t j = 0; j < n_msgs; j++)
  {
    const AfskgenSlot &s = msgs[j];
    const uint64_t first = std::max(s.start, N), last = std::min(s.end, N + n);
    if (first >= last)
    {
      continue;
    }
    uint32_t theta = afskgen_theta_at(s, levels[j], first - s.start);
    for (uint64_t t = first; t < last; t++)
    {
      bool clipped;
      out[t - N] = (int16_t)gen_output(out[t - N], afskgen_sample(s, t, theta, cos_table), &clipped);
      clips += clipped ? 1 : 0;
      theta += afskgen_step(s, levels[j], (uint32_t)(t - s.start));
    }
  }
  return clips;
}

// ---- the checks, each under `who`, the public function's name
inline int afskgen_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

} // namespace hrfd
