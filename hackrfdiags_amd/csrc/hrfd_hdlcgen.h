// hackrfdiags_amd/csrc/hrfd_hdlcgen.h -- what the HDLC framer bank (hrfd_hdlcgen_*, hrfd_hdlc_encode) needs no HIP for: the
// limits, the walk of a row of records, the rules bit by bit (a lane's eight data bits behind a run of ones, the run as a scan
// operator, the check sequence as a sum over the bytes), the bound on a row of bits, the argument checks, and a slow loop
// over one row that restates the contract of include/hrfd.h bit by bit.  The record, the CRC step and the limits of a payload
// are the HDLC bank's (hrfd_hdlc.h).  Plain C++ like hrfd_hdlc.h (tests/cpp/san_hdlcgen.cc compiles it on the CPU;
// hrfd_hdlcgen.hip includes it for the host side and the kernel); the includer declares
// `int fail(int code, const char *fmt, ...)` and the HRFD_* codes first.
#pragma once
#include <stdint.h>
#include <string.h>

#include "hrfd_hdlc.h"

#define HRFD_HDLCGEN_HD HRFD_PCM_HD
#if defined(__clang__)
#define HRFD_HDLCGEN_UNROLL _Pragma("unroll")  // the kernel wants the table's entries as immediates
#else
#define HRFD_HDLCGEN_UNROLL
#endif

namespace hrfd {

constexpr uint32_t kHdlcgenMaxBits = 1u << 20;         // bits of one channel in one call
constexpr uint32_t kHdlcgenMaxFlags = 255;             // of each of the three flag counts
constexpr uint32_t kHdlcgenDefaultLead = 12, kHdlcgenDefaultBetween = 2, kHdlcgenDefaultTail = 3;      // api.hdlc_encode's
constexpr uint32_t kHdlcgenFlag = 0x7Eu;
constexpr uint32_t kHdlcgenStuff = 5;                  // a zero goes in behind every fifth one of a run
constexpr uint32_t kHdlcgenMaxData = 8u * (kHdlcMaxPayload + 2u);                  // data bits of the longest frame: 8184
constexpr uint32_t kHdlcgenMaxFrame = kHdlcgenMaxData + kHdlcgenMaxData / kHdlcgenStuff;       // with its stuffed zeros: 9820
constexpr uint32_t kHdlcgenCrcLevels = 10;             // a byte lies at most 1021 < 2^10 bytes in front of the check sequence

struct HdlcgenFlags
{
  uint32_t lead, between, tail;
};

// ---- 1. the walk of a row: the record at byte `at` of a row of in_bytes bytes (at <= in_bytes, both multiples of 4).
// Answers the payload's length, or 0 for a record that ends the walk: a header or a payload past the row, or a length
// outside 1..1021
HRFD_HDLCGEN_HD uint32_t hdlcgen_record_at(const uint8_t *row, uint32_t in_bytes, uint32_t at)
{
  if (in_bytes - at < kHdlcHeader)
  {
    return 0u;
  }
  const uint32_t n = (uint32_t)row[at + 4] | ((uint32_t)row[at + 5] << 8);
  if (n == 0 || n > kHdlcMaxPayload || hdlc_record_bytes(n) > in_bytes - at)
  {
    return 0u;
  }
  return n;
}

// ---- 2. a lane's eight data bits (byte b, LSB first) behind a run of `run` ones: the bits with their stuffed zeros, LSB
// first, in *out, and how many they are (8..10).  Only run % 5 counts: a zero follows every fifth one of a run
HRFD_HDLCGEN_HD uint32_t hdlcgen_stuff_byte(uint32_t b, uint32_t run, uint32_t *out)
{
  uint32_t ones = run % kHdlcgenStuff, v = 0, n = 0;
  for (uint32_t i = 0; i < 8; i++)
  {
    const uint32_t bit = (b >> i) & 1u;
    v |= bit << n;
    n++;
    ones = bit != 0 ? ones + 1u : 0u;
    if (ones == kHdlcgenStuff)
    {
      n++;                                     // the stuffed zero
      ones = 0;
    }
  }
  *out = v;
  return n;
}

// ---- 3. the run of ones as a scan.  An element says what a stretch of data bits does to the run behind it: bit 31 set =
// the stretch is ones throughout and adds its length (the low bits) to the run in front, clear = the run behind it is its
// own trailing ones (the low bits).  The operator is associative, kHdlcgenRunId is its identity; a run in front of a
// frame's first bit is the element 0
constexpr uint32_t kHdlcgenRunAll = 1u << 31;
constexpr uint32_t kHdlcgenRunId = kHdlcgenRunAll;
HRFD_HDLCGEN_HD uint32_t hdlcgen_run_of_byte(uint32_t b)
{
  b &= 255u;
  const uint32_t t = (uint32_t)__builtin_clz(~(b << 24));  // the ones at the byte's top, 8 for 0xFF: the bits below are set
  return b == 255u ? kHdlcgenRunAll | t : t;
}
HRFD_HDLCGEN_HD uint32_t hdlcgen_run_join(uint32_t left, uint32_t right)
{
  return (right & kHdlcgenRunAll) != 0 ? left + (right & ~kHdlcgenRunAll) : right;        // (left keeps its own bit 31)
}

// ---- 4. the check sequence as a sum.  One step of the CRC register over a byte is s -> M (s ^ byte), M linear over GF(2)
// (eight shifts of hdlc_crc_byte), so over n bytes from 0xFFFF the register ends at
//   M^n (0xFFFF ^ b_0) ^ M^(n-1) b_1 ^ .. ^ M b_(n-1):
// byte i, k = n - i bytes in front of the check sequence, adds M^k of itself, every byte on its own.  pow[j][q] = M^(2^j) of
// bit q: M^k is the product of the levels of k's set bits
struct HdlcgenCrcPow
{
  uint16_t pow[kHdlcgenCrcLevels][16];
};
constexpr uint32_t hdlcgen_crc_m(uint32_t s)
{
  for (int i = 0; i < 8; i++)
  {
    s = (s >> 1) ^ (0x8408u & (0u - (s & 1u)));
  }
  return s;
}
constexpr uint32_t hdlcgen_crc_apply(const uint16_t *cols, uint32_t v)
{
  uint32_t r = 0;
  for (uint32_t q = 0; q < 16; q++)
  {
    r ^= (0u - ((v >> q) & 1u)) & cols[q];
  }
  return r;
}
constexpr HdlcgenCrcPow hdlcgen_crc_pow()
{
  HdlcgenCrcPow t = {};
  for (uint32_t q = 0; q < 16; q++)
  {
    t.pow[0][q] = (uint16_t)hdlcgen_crc_m(1u << q);
  }
  for (uint32_t j = 1; j < kHdlcgenCrcLevels; j++)
  {
    for (uint32_t q = 0; q < 16; q++)
    {
      t.pow[j][q] = (uint16_t)hdlcgen_crc_apply(t.pow[j - 1], t.pow[j - 1][q]);
    }
  }
  return t;
}
// what byte i of a payload of n adds to the register: M^(n - i) (byte, ^ 0xFFFF for the first)
HRFD_HDLCGEN_HD uint32_t hdlcgen_crc_term(const HdlcgenCrcPow &t, uint32_t byte, uint32_t i, uint32_t n)
{
  uint32_t v = (byte & 255u) ^ (i == 0 ? 0xFFFFu : 0u);
  const uint32_t k = n - i;
  HRFD_HDLCGEN_UNROLL
  for (uint32_t j = 0; j < kHdlcgenCrcLevels; j++)
  {
    if (((k >> j) & 1u) != 0)
    {
      uint32_t r = 0;
      HRFD_HDLCGEN_UNROLL
      for (uint32_t q = 0; q < 16; q++)
      {
        r ^= (0u - ((v >> q) & 1u)) & t.pow[j][q];
      }
      v = r;
    }
  }
  return v;
}

// ---- 5. the bound: D = 8 (payload_bytes + 2 n_frames) data bits take at most D + D / 5 bits (a frame of D_i takes at most
// D_i + floor(D_i / 5), and the floors' sum is at most the sum's floor), and the flags are lead + (n_frames - 1) between +
// tail.  64 bits: the caller compares with the limit
HRFD_HDLCGEN_HD uint64_t hdlcgen_bound(uint32_t n_frames, uint64_t payload_bytes, const HdlcgenFlags &fl)
{
  const uint64_t D = 8ull * (payload_bytes + 2ull * n_frames);
  return D + D / kHdlcgenStuff + 8ull * (fl.lead + (uint64_t)(n_frames - 1u) * fl.between + fl.tail);
}

// ---- one row, bit by bit (the contract as a loop; the kernel must agree byte for byte)
// row: in_bytes bytes of records, n_frames of which count; bits: max_bits bytes, of which the first *n_bits are written and
// no other; counts: {n_bits, n_sent, dropped}
inline void hdlcgen_row_slow(const uint8_t *row, uint32_t in_bytes, uint32_t n_frames, const HdlcgenFlags &fl, uint8_t *bits,
                             uint32_t max_bits, uint32_t *counts)
{
  uint32_t at = 0, cur = 0, sent = 0;
  auto put_flags = [&](uint32_t n) {
    for (uint32_t i = 0; i < 8u * n; i++)
    {
      bits[cur++] = (uint8_t)((kHdlcgenFlag >> (i & 7u)) & 1u);
    }
  };
  for (uint32_t f = 0; f < n_frames; f++)
  {
    const uint32_t n = hdlcgen_record_at(row, in_bytes, at);
    if (n == 0)
    {
      break;
    }
    const uint8_t *payload = row + at + kHdlcHeader;
    uint32_t crc = 0xFFFFu;
    for (uint32_t i = 0; i < n; i++)
    {
      crc = hdlc_crc_byte(crc, payload[i]);
    }
    crc ^= 0xFFFFu;
    auto data_bit = [&](uint32_t i) -> uint32_t {
      const uint32_t b = i >> 3, byte = b < n ? payload[b] : (b == n ? crc & 255u : crc >> 8);
      return (byte >> (i & 7u)) & 1u;
    };
    // the frame's length first: a frame that does not fit writes nothing
    const uint32_t D = 8u * (n + 2u);
    uint32_t len = 0, ones = 0;
    for (uint32_t i = 0; i < D; i++)
    {
      len++;
      ones = data_bit(i) != 0 ? ones + 1u : 0u;
      if (ones == kHdlcgenStuff)
      {
        len++;
        ones = 0;
      }
    }
    const uint32_t pre = sent == 0 ? fl.lead : fl.between;
    if ((uint64_t)cur + 8u * pre + len + 8u * fl.tail > max_bits)
    {
      break;
    }
    put_flags(pre);
    ones = 0;
    for (uint32_t i = 0; i < D; i++)
    {
      const uint32_t v = data_bit(i);
      bits[cur++] = (uint8_t)v;
      ones = v != 0 ? ones + 1u : 0u;
      if (ones == kHdlcgenStuff)
      {
        bits[cur++] = 0;
        ones = 0;
      }
    }
    sent++;
    at += hdlc_record_bytes(n);
  }
  if (sent != 0)
  {
    put_flags(fl.tail);
  }
  counts[0] = cur;
  counts[1] = sent;
  counts[2] = n_frames - sent;
}

// ---- the checks, each under `who`, the public function's name
inline int hdlcgen_check_create(const char *who, uint32_t n_channels, const void *out) { return pcm_check_channels(who, n_channels, out); }

inline int hdlcgen_check_flags(const char *who, uint32_t lead, uint32_t between, uint32_t tail)
{
  if (lead > kHdlcgenMaxFlags)
  {
    return fail(HRFD_EINVAL, "%s: n_lead_flags %u (0..%u)", who, lead, kHdlcgenMaxFlags);
  }
  if (between == 0 || between > kHdlcgenMaxFlags)
  {
    return fail(HRFD_EINVAL, "%s: n_between %u (1..%u)", who, between, kHdlcgenMaxFlags);
  }
  if (tail == 0 || tail > kHdlcgenMaxFlags)
  {
    return fail(HRFD_EINVAL, "%s: n_tail_flags %u (1..%u)", who, tail, kHdlcgenMaxFlags);
  }
  return HRFD_OK;
}

inline int hdlcgen_check_max_bits(const char *who, uint32_t max_bits)
{
  if (max_bits == 0 || max_bits > kHdlcgenMaxBits)
  {
    return fail(HRFD_EINVAL, "%s: max_bits must be 1..%u (got %u)", who, kHdlcgenMaxBits, max_bits);
  }
  return HRFD_OK;
}

// the arguments of hrfd_hdlcgen_max_bits and the bound itself
inline int hdlcgen_check_bound(const char *who, uint32_t n_frames, uint64_t payload_bytes, const HdlcgenFlags &fl, uint32_t *max_bits)
{
  if (max_bits == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL result pointer", who);
  }
  if (n_frames == 0 || payload_bytes < n_frames || payload_bytes > (uint64_t)kHdlcMaxPayload * n_frames)
  {
    return fail(HRFD_EINVAL, "%s: %u frames of %llu payload bytes together (at least one frame, 1..%u bytes each)", who, n_frames,
                (unsigned long long)payload_bytes, kHdlcMaxPayload);
  }
  const uint64_t need = hdlcgen_bound(n_frames, payload_bytes, fl);
  if (need > kHdlcgenMaxBits)
  {
    return fail(HRFD_EINVAL, "%s: %llu bits are more than one call's %u", who, (unsigned long long)need, kHdlcgenMaxBits);
  }
  *max_bits = (uint32_t)need;
  return HRFD_OK;
}

// what a process call's sizes and addresses decide without a handle.  The dense host entries have no strides, and
// n_channels = 1 where the handle is not known yet
inline int hdlcgen_check_call(const char *who, const void *in, uint64_t in_stride, uint32_t in_bytes, bool device_entry,
                              const void *n_frames, const void *bits, uint64_t bits_stride, uint32_t max_bits, const void *n_bits,
                              const void *n_sent, const void *dropped, uint32_t n_channels)
{
  BANK_TRY(hdlcgen_check_max_bits(who, max_bits));
  if (in_bytes < 4u || (in_bytes & 3u) != 0)
  {
    return fail(HRFD_EINVAL, "%s: in_bytes %u must be a multiple of 4, at least 4", who, in_bytes);
  }
  if (device_entry && ((in_stride & 3u) != 0 || in_stride < in_bytes))
  {
    return fail(HRFD_EINVAL, "%s: in_stride_bytes %llu must be a multiple of 4 and >= in_bytes = %u", who,
                (unsigned long long)in_stride, in_bytes);
  }
  if (device_entry && bits_stride < max_bits)
  {
    return fail(HRFD_EINVAL, "%s: bits_stride_bytes %llu is below max_bits = %u", who, (unsigned long long)bits_stride, max_bits);
  }
  if (!pcm_aligned(in, 4))
  {
    return fail(HRFD_EINVAL, "%s: the records must sit at a 4-byte aligned address", who);
  }
  if (!pcm_aligned(n_frames, 4) || !pcm_aligned(n_bits, 4) || !pcm_aligned(n_sent, 4) || !pcm_aligned(dropped, 4))
  {
    return fail(HRFD_EINVAL, "%s: n_frames, n_bits, n_sent and dropped must be 4-byte aligned", who);
  }
  if (in == nullptr || n_frames == nullptr || bits == nullptr || n_bits == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument (only n_sent and dropped may be NULL)", who);
  }
  if (device_entry)
  {
    BANK_TRY(pcm_check_no_overlap(who, in, in_stride, in_bytes, bits, bits_stride, max_bits, n_channels,
                                  "a row of bits is written while the records are read"));
  }
  return HRFD_OK;
}

} // namespace hrfd
