// hackrfdiags_amd/csrc/hrfd_audio.h -- what the audio bank (hrfd_audio_*) needs no HIP for: the argument checks, the three
// laws (voice filter rounding, gate envelope and product, bus rounding), the tone squelch's block verdict, and a slow loop
// over one channel that restates the contract of include/hrfd.h sample by sample.  Plain C++ like hrfd_tone.h
// (tests/cpp/san_audio.cc compiles it on the CPU; hrfd_audio.hip includes it for the host side and the kernels); the
// includer declares `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>

#include "hrfd_pcm.h"

#define HRFD_AUDIO_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kAudioBlock = kPcmBlock;
constexpr uint32_t kAudioMaxTaps = 512;
constexpr uint32_t kAudioMaxBuses = 64;
constexpr uint32_t kAudioMaxList = 4096;   // entries of one bus
constexpr uint32_t kAudioMaxBlocks = 1024;
constexpr uint32_t kAudioGroups = 4;       // the tone bank's groups
constexpr uint32_t kAudioAnyTone = 254;
constexpr uint32_t kAudioNoTone = 255;
constexpr int32_t kAudioUnity = 32768;     // the envelope of an open gate
constexpr int32_t kAudioRampStep = 512;    // 64 samples from 0 to kAudioUnity

// ---- 1. input (pcm_block_limit) and 2. voice filter (pcm_fir_round): hrfd_pcm.h

// ---- 3. gate: the envelope of sample n (0..511) of a block whose gate is q behind a block whose gate was p
HRFD_AUDIO_HD int32_t audio_envelope(bool p, bool q, uint32_t n)
{
  if (p == q)
  {
    return q ? kAudioUnity : 0;
  }
  const int32_t ramp = kAudioRampStep * (int32_t)(n + 1);
  if (q)
  {
    return ramp < kAudioUnity ? ramp : kAudioUnity;
  }
  return ramp < kAudioUnity ? kAudioUnity - ramp : 0;
}

// z = (y e + 2^14) >> 15: |y e| <= 2^30; y at e = 32768, 0 at e = 0
HRFD_AUDIO_HD int32_t audio_gate(int32_t y, int32_t e) { return (y * e + (1 << 14)) >> 15; }

// ---- 4. tone squelch: is block b open under `want`, from one channel's verdicts best / present [F][4]
HRFD_AUDIO_HD bool audio_frame_match(const uint8_t *best, const uint8_t *present, uint32_t frame, uint32_t group, uint32_t want)
{
  const uint32_t i = frame * kAudioGroups + group;
  return present[i] != 0 && (want == kAudioAnyTone || best[i] == want);
}

HRFD_AUDIO_HD bool audio_block_open(const uint8_t *best, const uint8_t *present, uint32_t L, uint32_t group, uint32_t want, uint32_t b)
{
  if (want == kAudioNoTone)
  {
    return true;
  }
  if (L > kAudioBlock)
  {
    return audio_frame_match(best, present, (uint32_t)((uint64_t)b * kAudioBlock / L), group, want);
  }
  const uint32_t per = kAudioBlock / L;
  for (uint32_t f = b * per; f < (b + 1) * per; f++)
  {
    if (audio_frame_match(best, present, f, group, want))
    {
      return true;
    }
  }
  return false;
}

// ---- 5. buses: s = sum g z, |s| <= 4096 * 32767 * 32768 < 2^42; mix = sat16((s + 2^11) >> 12)
HRFD_AUDIO_HD int32_t audio_mix_round(int64_t s, bool *clipped)
{
  const int64_t r = (s + (1 << 11)) >> 12;
  const int32_t m = pcm_sat16(r);
  *clipped = (int64_t)m != r;
  return m;
}

// a bus entry as the kernel reads it: the channel below, the gain above
HRFD_AUDIO_HD uint32_t audio_pack_entry(uint32_t channel, int32_t gain) { return (channel & 0xffffu) | ((uint32_t)gain << 16); }
HRFD_AUDIO_HD uint32_t audio_entry_channel(uint32_t e) { return e & 0xffffu; }
HRFD_AUDIO_HD int32_t audio_entry_gain(uint32_t e) { return (int32_t)e >> 16; }

// ---- one channel, sample by sample (the contract as a loop; the kernels must agree bit for bit)
// pcm_row: the channel's [n_blocks][512]; n_pcm_row, open_row: its [n_blocks] or NULL; hist: the last T - 1 values of x in
// time order (hist[T - 2] is the newest), read and replaced; prev: the gate of the block before, read and replaced; z:
// [n_blocks][512]
inline void audio_channel_slow(const int16_t *pcm_row, const uint32_t *n_pcm_row, const uint8_t *open_row, uint32_t n_blocks,
                               const int16_t *h, uint32_t T, int16_t *hist, uint8_t *prev, int16_t *z)
{
  const uint32_t H = T - 1;
  for (uint32_t b = 0; b < n_blocks; b++)
  {
    const bool q = open_row == nullptr || open_row[b] != 0, p = *prev != 0;
    const uint32_t lim = pcm_block_limit(n_pcm_row, b);
    int16_t x[kAudioBlock];
    for (uint32_t n = 0; n < kAudioBlock; n++)
    {
      x[n] = n < lim ? pcm_row[b * kAudioBlock + n] : (int16_t)0;
    }
    for (uint32_t n = 0; n < kAudioBlock; n++)
    {
      int32_t acc = 0;
      for (uint32_t k = 0; k < T; k++)
      {
        const int32_t xv = k <= n ? x[n - k] : hist[H + n - k];
        acc += (int32_t)h[k] * xv;
      }
      z[b * kAudioBlock + n] = (int16_t)audio_gate(pcm_fir_round(acc), audio_envelope(p, q, n));
    }
    // H < 512: the new history is the block's own tail
    for (uint32_t i = 0; i < H; i++)
    {
      hist[i] = x[kAudioBlock - H + i];
    }
    *prev = q ? 1 : 0;
  }
}

// ---- the checks, each under `who`, the public function's name
inline int audio_check_create(const char *who, uint32_t n_channels, uint32_t n_buses, const void *out)
{
  BANK_TRY(pcm_check_channels(who, n_channels, out));
  if (n_buses == 0 || n_buses > kAudioMaxBuses)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u buses (got %u)", who, kAudioMaxBuses, n_buses);
  }
  return HRFD_OK;
}

// T = 1..512 and the bank core's tap check over the one branch: sum |h| <= 65535
inline int audio_check_taps(const char *who, const int16_t *taps, uint32_t n)
{
  if (n == 0 || n > kAudioMaxTaps || taps == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: need 1..%u taps and their array (got %u)", who, kAudioMaxTaps, n);
  }
  return bank_tap_sums_ok(who, taps, n, 1);
}

// n_channels, n_buses: the handle's, or the largest any handle has where there is none yet
inline int audio_check_bus(const char *who, uint32_t bus, const uint32_t *channels, const int16_t *gains, uint32_t n,
                           uint32_t n_channels, uint32_t n_buses)
{
  if (bus >= n_buses)
  {
    return fail(HRFD_EINVAL, "%s: bus %u (0..%u)", who, bus, n_buses - 1);
  }
  if (n > kAudioMaxList || (n > 0 && (channels == nullptr || gains == nullptr)))
  {
    return fail(HRFD_EINVAL, "%s: a list of %u entries (at most %u, and both arrays when n > 0)", who, n, kAudioMaxList);
  }
  for (uint32_t j = 0; j < n; j++)
  {
    if (channels[j] >= n_channels)
    {
      return fail(HRFD_EINVAL, "%s: entry %u names channel %u (0..%u)", who, j, channels[j], n_channels - 1);
    }
    if (gains[j] == -32768)
    {
      return fail(HRFD_EINVAL, "%s: entry %u has gain -32768 (-32767..32767)", who, j);
    }
  }
  return HRFD_OK;
}

inline int audio_check_want(const char *who, uint32_t channel, uint32_t want, uint32_t n_channels)
{
  if (want > kAudioNoTone || (want >= 128 && want < kAudioAnyTone))
  {
    return fail(HRFD_EINVAL, "%s: want %u (a tone index 0..127, HRFD_AUDIO_ANY_TONE or HRFD_AUDIO_NO_TONE)", who, want);
  }
  return pcm_check_channel(who, channel, n_channels);
}

inline int audio_check_gate(const char *who, const void *best, const void *present, uint32_t frame_len, uint32_t group,
                            uint32_t n_blocks, const void *open)
{
  if (n_blocks == 0 || n_blocks > kAudioMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kAudioMaxBlocks, n_blocks);
  }
  BANK_TRY(pcm_check_frame_len(who, frame_len));
  BANK_TRY(pcm_check_frames(who, n_blocks, frame_len));
  if (group >= kAudioGroups)
  {
    return fail(HRFD_EINVAL, "%s: group %u (0..%u)", who, group, kAudioGroups - 1);
  }
  if (best == nullptr || present == nullptr || open == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle; n_channels: the handle's, or 1 where there is none
// yet (the ranges that must not overlap grow with it).  The dense host entry has no strides.
inline int audio_check_call(const char *who, const void *pcm, uint64_t in_stride, bool device_entry, uint32_t n_blocks,
                            const void *out, uint64_t out_stride, const void *mix, const void *clips, uint32_t n_channels)
{
  if (n_blocks == 0 || n_blocks > kAudioMaxBlocks)
  {
    return fail(HRFD_EINVAL, "%s: n_blocks must be 1..%u (got %u)", who, kAudioMaxBlocks, n_blocks);
  }
  if (out == nullptr && mix == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: no output asked for (out and mix are both NULL)", who);
  }
  const uint64_t row = 2ull * kAudioBlock * n_blocks;
  if (device_entry)
  {
    BANK_TRY(pcm_check_stride(who, "channel_stride_bytes", in_stride, row));
    if (out != nullptr)
    {
      BANK_TRY(pcm_check_stride(who, "out_stride_bytes", out_stride, row));
    }
  }
  if (!pcm_aligned(pcm, 2) || !pcm_aligned(out, 2) || !pcm_aligned(mix, 2))
  {
    return fail(HRFD_EINVAL, "%s: the PCM, out and mix must sit at even addresses", who);
  }
  if (!pcm_aligned(clips, 4))
  {
    return fail(HRFD_EINVAL, "%s: clips must be 4-byte aligned", who);
  }
  if (pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  if (out != nullptr)
  {
    return pcm_check_no_overlap(who, pcm, device_entry ? in_stride : row, row, out, device_entry ? out_stride : row, row, n_channels,
                                "a block needs the raw tail of the block before it");
  }
  return HRFD_OK;
}

} // namespace hrfd
