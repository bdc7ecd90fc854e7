// hackrfdiags_amd/csrc/hrfd_hdlc.h -- what the HDLC bank (hrfd_hdlc_*) needs no HIP for: the limits, the law bit by bit (the
// run of ones, the class of a zero, the frame check), the record, the bound on a row of records, the argument checks, and a
// slow loop over one channel that restates the contract of include/hrfd.h bit by bit.  Plain C++ like hrfd_afsk.h
// (tests/cpp/san_hdlc.cc compiles it on the CPU; hrfd_hdlc.hip includes it for the host side and the kernel); the includer
// declares `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hrfd_pcm.h"

#define HRFD_HDLC_HD HRFD_PCM_HD

namespace hrfd {

constexpr uint32_t kHdlcMaxBits = 1u << 20;            // bits of one channel in one call
constexpr uint32_t kHdlcMaxPayload = 1021;             // P: with the check sequence and the flag's seven bits 1024 bytes
constexpr uint32_t kHdlcDefaultMin = 1;
constexpr uint32_t kHdlcDefaultMax = 512;
constexpr uint32_t kHdlcBitWords = (kHdlcMaxPayload + 3) / 4;          // 256 dwords hold the longest partial frame
constexpr uint32_t kHdlcStateDw = 4 + kHdlcBitWords;                   // 260
constexpr uint32_t kHdlcMaxOnes = 7;                   // the run of ones saturates here: seven ones abort
constexpr uint32_t kHdlcFlagBits = 7;                  // of a flag, the bits collected before its last: a zero and six ones
constexpr uint32_t kHdlcHeader = 8;                    // bytes of a record in front of its payload
constexpr uint32_t kHdlcResidue = 0xF0B8;              // the CRC register behind a frame with its good check sequence
constexpr uint32_t kHdlcBitValue = 1u;                 // HRFD_AFSK_BIT
constexpr uint32_t kHdlcBitCarrier = 2u;               // HRFD_AFSK_CARRIER

// one channel's state between calls.  Zero is a channel that has seen nothing: no frame is open until the first flag
struct HdlcState
{
  uint32_t ones;                               // the run of ones behind the last bit, 0..7
  uint32_t in_frame;
  uint32_t n;                                  // bits collected since the last flag, 0..cap; 0 where no frame is open
  uint32_t pad;
  uint32_t bits[kHdlcBitWords];                // bit i of the frame: bit i & 31 of word i >> 5 (LSB first, as bytes as well)
};
static_assert(sizeof(HdlcState) == 4 * kHdlcStateDw, "the kernel reads this layout");

struct HdlcLimits
{
  uint32_t min_payload, max_payload, require_carrier;
};

// ---- 1. the sizes the limits give
// the most bits a frame may collect: P + 2 bytes and the seven bits of the closing flag that are in by its last
HRFD_HDLC_HD uint32_t hdlc_cap(uint32_t P) { return 8u * (P + 2u) + kHdlcFlagBits; }
// the fewest a frame of m payload bytes has collected at its closing flag
HRFD_HDLC_HD uint32_t hdlc_least(uint32_t m) { return kHdlcFlagBits + 8u * (m + 2u); }
// a record: the header, the payload, zeros up to a multiple of 4
HRFD_HDLC_HD uint32_t hdlc_record_bytes(uint32_t n_payload) { return kHdlcHeader + ((n_payload + 3u) & ~3u); }

// A row of this many bytes never drops a record of a call of max_bits bits:
//   * a frame of valid length has collected n >= 7 + 8 (m + 2) bits since the flag in front of it, and its own closing bit is
//     one more: the closing bits of two such frames lie at least 8 (m + 3) bits apart, so max_bits bits close at most
//     F = 1 + (max_bits - 1) / (8 (m + 3)) of them
//   * a record is at most 8 + p + 3 = 11 + p bytes for a payload of p
//   * p <= P for every frame; and the 8 p + 23 bits every frame has collected come out of the carried partial frame (at most
//     8 (P + 2) + 7 bits, all in the first frame) or out of this call's bits: sum (8 p_i + 23) <= 8 P + 23 + max_bits, so
//     sum p_i <= P + max_bits / 8 - 23 (F - 1) / 8 <= P + max_bits / 8
// which gives 11 F + min(F P, P + max_bits / 8), rounded up to 4.  At the limits (2^20 bits, m = 1, P = 1021) it is below 2^19
HRFD_HDLC_HD uint32_t hdlc_max_out(uint32_t max_bits, uint32_t m, uint32_t P)
{
  const uint32_t F = 1u + (max_bits - 1u) / (8u * (m + 3u));
  const uint32_t a = F * P, b = P + max_bits / 8u;
  return (11u * F + (a < b ? a : b) + 3u) & ~3u;
}

// ---- 2. the frame check: CRC-16/X.25, reflected 0x1021, the register starts at 0xFFFF; run over a frame's bytes with the
// check sequence behind them it ends at 0xF0B8 exactly when the sequence is the inverted CRC of the rest, low byte first
HRFD_HDLC_HD uint32_t hdlc_crc_byte(uint32_t crc, uint32_t byte)
{
  crc ^= byte;
  for (int i = 0; i < 8; i++)
  {
    crc = (crc >> 1) ^ (0x8408u & (0u - (crc & 1u)));
  }
  return crc;
}

// ---- 3. the class of a bit from its value and the run of ones in front of it (0..7, saturated)
enum
{
  kHdlcKeep = 1,                               // appended to an open frame: every one, and a zero behind fewer than five ones
  kHdlcFlag = 2,                               // a zero behind six ones
  kHdlcAbort = 4                               // a one behind six or more
};
HRFD_HDLC_HD uint32_t hdlc_classify(uint32_t v, uint32_t ones)
{
  if (v != 0)
  {
    return kHdlcKeep | (ones >= 6u ? kHdlcAbort : 0u);
  }
  return ones == 6u ? kHdlcFlag : (ones == 5u ? 0u : kHdlcKeep);
}
HRFD_HDLC_HD uint32_t hdlc_next_ones(uint32_t v, uint32_t ones) { return v != 0 ? (ones < kHdlcMaxOnes ? ones + 1u : kHdlcMaxOnes) : 0u; }

// bits [at, at + 8) of a packed row
HRFD_HDLC_HD uint32_t hdlc_byte_at(const uint32_t *words, uint32_t at)
{
  const uint32_t w = at >> 5, s = at & 31u;
  uint32_t v = words[w] >> s;
  if (s > 24u)
  {
    v |= words[w + 1] << (32u - s);
  }
  return v & 255u;
}

// ---- one channel, bit by bit (the contract as a loop; the kernel must agree bit for bit)
// row: n_bits bytes as hrfd_afsk_process writes them; st: read and replaced; out: out_bytes bytes (a multiple of 4) of
// records; counts: {n_frames, n_bad, dropped}.  Records fill the row in stream order; from the first that does not fit on,
// every good frame of the call is dropped (counted, nothing of it written)
inline void hdlc_channel_slow(const uint8_t *row, uint32_t n_bits, const HdlcLimits &lim, HdlcState *st, uint8_t *out, uint32_t out_bytes,
                              uint32_t *counts)
{
  const uint32_t cap = hdlc_cap(lim.max_payload);
  uint32_t ones = st->ones, in_frame = st->in_frame, n = st->n;
  uint32_t n_frames = 0, n_bad = 0, dropped = 0;
  uint64_t at = 0;                             // bytes of the call's good records, written or not
  for (uint32_t j = 0; j < n_bits; j++)
  {
    const uint32_t v = row[j] & kHdlcBitValue, c = (row[j] >> 1) & 1u;
    if (lim.require_carrier != 0 && c == 0)
    {
      in_frame = 0;
    }
    const uint32_t cls = hdlc_classify(v, ones);
    if ((cls & kHdlcFlag) != 0)
    {
      if (in_frame != 0 && n >= hdlc_least(lim.min_payload) && (n - kHdlcFlagBits) % 8u == 0)
      {
        const uint32_t n_bytes = (n - kHdlcFlagBits) / 8u, p = n_bytes - 2u;
        uint32_t crc = 0xFFFFu;
        for (uint32_t b = 0; b < n_bytes; b++)
        {
          crc = hdlc_crc_byte(crc, hdlc_byte_at(st->bits, 8u * b));
        }
        if (crc != kHdlcResidue)
        {
          n_bad++;
        }
        else
        {
          const uint32_t size = hdlc_record_bytes(p);
          if (at + size <= out_bytes)
          {
            const uint32_t fcs = hdlc_byte_at(st->bits, 8u * p) | (hdlc_byte_at(st->bits, 8u * p + 8u) << 8);
            const uint32_t head[2] = {j, p | (fcs << 16)};
            memcpy(out + at, head, kHdlcHeader);
            memset(out + at + kHdlcHeader, 0, size - kHdlcHeader);
            for (uint32_t b = 0; b < p; b++)
            {
              out[at + kHdlcHeader + b] = (uint8_t)hdlc_byte_at(st->bits, 8u * b);
            }
            n_frames++;
          }
          else
          {
            dropped++;
          }
          at += size;
        }
      }
      in_frame = 1;
      n = 0;
    }
    else if ((cls & kHdlcKeep) != 0 && in_frame != 0)
    {
      if (n == cap)
      {
        in_frame = 0;                          // over-long: dead until the next flag
      }
      else
      {
        if ((n & 31u) == 0)
        {
          st->bits[n >> 5] = 0;
        }
        st->bits[n >> 5] |= v << (n & 31u);
        n++;
      }
    }
    if ((cls & kHdlcAbort) != 0)
    {
      in_frame = 0;
    }
    ones = hdlc_next_ones(v, ones);
  }
  st->ones = ones;
  st->in_frame = in_frame;
  st->n = in_frame != 0 ? n : 0u;
  counts[0] = n_frames;
  counts[1] = n_bad;
  counts[2] = dropped;
}

// ---- the checks, each under `who`, the public function's name
inline int hdlc_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

inline int hdlc_check_limits(const char *who, uint32_t min_payload, uint32_t max_payload)
{
  if (max_payload == 0 || max_payload > kHdlcMaxPayload)
  {
    return fail(HRFD_EINVAL, "%s: max_payload %u (1..%u bytes)", who, max_payload, kHdlcMaxPayload);
  }
  if (min_payload == 0 || min_payload > max_payload)
  {
    return fail(HRFD_EINVAL, "%s: min_payload %u (1..max_payload = %u bytes)", who, min_payload, max_payload);
  }
  return HRFD_OK;
}

inline int hdlc_check_max_bits(const char *who, uint32_t max_bits)
{
  if (max_bits == 0 || max_bits > kHdlcMaxBits)
  {
    return fail(HRFD_EINVAL, "%s: max_bits must be 1..%u (got %u)", who, kHdlcMaxBits, max_bits);
  }
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle.  The dense host entry has no strides
inline int hdlc_check_call(const char *who, const void *bits, uint64_t bits_stride, bool device_entry, const void *n_bits,
                           uint32_t max_bits, const void *out, uint64_t out_stride, uint32_t out_bytes, const void *n_frames,
                           const void *n_bad, const void *dropped)
{
  BANK_TRY(hdlc_check_max_bits(who, max_bits));
  if (device_entry && bits_stride < max_bits)
  {
    return fail(HRFD_EINVAL, "%s: bits_stride_bytes %llu is below max_bits = %u", who, (unsigned long long)bits_stride, max_bits);
  }
  if (out_bytes < 4u || (out_bytes & 3u) != 0)
  {
    return fail(HRFD_EINVAL, "%s: out_bytes %u must be a multiple of 4, at least 4", who, out_bytes);
  }
  if (device_entry && ((out_stride & 3u) != 0 || out_stride < out_bytes))
  {
    return fail(HRFD_EINVAL, "%s: out_stride_bytes %llu must be a multiple of 4 and >= out_bytes = %u", who,
                (unsigned long long)out_stride, out_bytes);
  }
  if (!pcm_aligned(out, 4))
  {
    return fail(HRFD_EINVAL, "%s: the records must sit at a 4-byte aligned address", who);
  }
  if (!pcm_aligned(n_bits, 4) || !pcm_aligned(n_frames, 4) || !pcm_aligned(n_bad, 4) || !pcm_aligned(dropped, 4))
  {
    return fail(HRFD_EINVAL, "%s: n_bits, n_frames, n_bad and dropped must be 4-byte aligned", who);
  }
  if (bits == nullptr || n_bits == nullptr || out == nullptr || n_frames == nullptr || dropped == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument (only n_bad may be NULL)", who);
  }
  return HRFD_OK;
}

} // namespace hrfd
