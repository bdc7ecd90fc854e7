// hackrfdiags_amd/csrc/hrfd_hdlc.hip -- hrfd_hdlc_*: packet frames out of the bits the AFSK bank writes, on the device.
//
// Rows of bits (a byte a bit, hrfd_afsk_process_device's) and their counts in; per channel a row of frame records and three
// counts out.  The law is bit by bit, contract in include/hrfd.h; tests/hdlc_model.py restates it, hrfd_hdlc.h holds the rules
// both sides of this file share and the slow loop.
//
// k_hdlc: one launch, one workgroup of 256 threads per channel, which takes its row in tiles of kHdlcTile = 2048 bits, 8
// consecutive bits per lane as one byte mask.  Nothing walks the row: every step of a tile is the same few instructions for
// every lane, or a scan over the lanes.
//   1. the run of ones in front of a lane's first bit.  The run saturates at 7 and a lane holds 8 bits, so the lane in front
//      decides it alone: min(7, its trailing ones).  (The max-scan of "index of the last zero" collapses to one neighbour:
//      a lane of eight ones already saturates the run.)  Lane 0 takes the carried run.  The lane then classifies its eight
//      bits with hdlc_classify: keep / flag / abort masks.  Under require_carrier a bit without carrier is an abort mark too
//   2. one exclusive scan over the lanes of (kept bits, flags), packed in a dword: shuffles inside a wave, the four totals
//      through LDS.  It gives every kept bit its index among the kept and every flag its ordinal
//   3. the kept bits are compacted into `kb`, a bit row in LDS that starts with the carried partial frame: a lane's bits
//      land in at most two dwords, by LDS vector atomics (ds_or_b32).  Flags cut kb into segments; flag f leaves its position
//      in kb and its bit index in fl[f]; an abort mark sets dead[f] of the segment it lies in (a flag belongs to the segment
//      it closes)
//   4. frame close: flag f's segment is kb[S, E), S the flag before (0 for the first: the carried bits are in front).
//      Thread f checks that it is not dead, its length, runs the CRC over its bytes and, for a good one, takes its place in
//      the row by a second scan (of the record sizes) and writes the record.  Only segments of valid length cost a CRC,
//      at most one per 8 (m + 3) bits
//   5. what lies behind the tile's last flag (or all of kb where there was none) moves to the front of kb for the next tile:
//      a funnel shift, two dwords a lane
// Behind the last tile the open partial frame and the three words of state go to the other side of the state's ping-pong.
// The grid is the channel count, at most 65536 workgroups: below kBankMaxWgs, so the launch is never cut.  The counts are
// read on the device; no call waits for it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hrfd_hdlc.h"

namespace hrfd {

constexpr int kHdlcThreads = 256;
constexpr int kHdlcPer = 8;                                // consecutive bits of one lane
constexpr uint32_t kHdlcTile = kHdlcThreads * kHdlcPer;    // bits of one tile
constexpr uint32_t kHdlcMaxCap = 8u * (kHdlcMaxPayload + 2u) + kHdlcFlagBits;      // 8191
constexpr uint32_t kHdlcKbDw = (kHdlcMaxCap + kHdlcTile + 31u) / 32u + 2u;         // the carried bits, a tile's, a dword to read over
constexpr uint32_t kHdlcMaxFlags = kHdlcTile / 7u + 2u;    // flags that share their zeros lie seven bits apart
static_assert(kHdlcMaxCap <= 32u * kHdlcBitWords, "the state holds the longest partial frame");
static_assert(kHdlcKbDw <= 2 * kHdlcThreads, "step 5 moves two dwords a lane");
static_assert(65536u <= kBankMaxWgs, "one workgroup per channel is one launch");

typedef uint32_t hdlc_u2_any __attribute__((ext_vector_type(2), aligned(1)));      // 8 bytes at any address

struct HdlcParams
{
  const uint8_t *bits;                     // [C] rows, bits_stride bytes apart, any address
  uint64_t bits_stride;
  const uint32_t *n_bits;                  // [C]
  uint32_t max_bits;
  const uint32_t *state_in;                // [C][260]: HdlcState
  uint32_t *state_out;
  const uint8_t *reset;                    // [C]: non-zero = this channel starts from a zero state; or NULL
  uint8_t *out;                            // [C] rows of records, out_stride bytes apart, 4-byte aligned
  uint64_t out_stride;
  uint32_t out_bytes;
  uint32_t *n_frames, *n_bad, *dropped;    // [C]; n_bad may be NULL
  uint32_t least, cap, require_carrier;    // hdlc_least(m), hdlc_cap(P)
};

// exclusive scan of v over the workgroup, and the total; wt: four dwords of LDS.  Every thread calls it
__device__ __forceinline__ uint32_t hdlc_scan(uint32_t v, uint32_t *wt, uint32_t *total)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t o = __shfl_up(inc, d, 64);
    inc += lane >= (uint32_t)d ? o : 0u;
  }
  if (lane == 63u)
  {
    wt[wave] = inc;
  }
  __syncthreads();
  uint32_t pre = 0, sum = 0;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)kHdlcThreads / 64u; w++)
  {
    const uint32_t t = wt[w];
    pre += w < wave ? t : 0u;
    sum += t;
  }
  __syncthreads();                         // the next scan writes wt again
  *total = sum;
  return pre + inc - v;
}

// bits [at, at + 32) of a bit row; reads the dword behind as well
__device__ __forceinline__ uint32_t hdlc_word_at(const uint32_t *words, uint32_t at)
{
  const uint32_t w = at >> 5, s = at & 31u;
  return (uint32_t)((((uint64_t)words[w + 1] << 32) | words[w]) >> s);
}

__global__ __launch_bounds__(kHdlcThreads) void k_hdlc(const HdlcParams P)
{
  __shared__ uint32_t kb[kHdlcKbDw];
  __shared__ uint32_t fl[kHdlcMaxFlags];       // flag f: its position among the tile's kept bits | its bit of the tile << 16
  __shared__ uint32_t dead[kHdlcMaxFlags + 1]; // segment f (the one flag f closes; the last: the open one) holds an abort mark
  __shared__ uint8_t vmb[kHdlcThreads];
  __shared__ uint32_t wt[4];
  __shared__ uint32_t cnt[3];                  // n_frames, n_bad, dropped
  __shared__ uint32_t end_ones;
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  const uint8_t *row = P.bits + (uint64_t)c * P.bits_stride;
  uint8_t *out_row = P.out + (uint64_t)c * P.out_stride;
  const uint32_t *st_in = P.state_in + (uint64_t)c * kHdlcStateDw;
  const bool fresh = P.reset != nullptr && P.reset[c] != 0;
  const uint32_t nb = min(P.n_bits[c], P.max_bits);

  // the carried state, uniform: the run of ones, whether a frame is open, its bits so far (n_c <= cap)
  uint32_t ones_c = 0, alive_c = 0, n_c = 0;
  if (!fresh)
  {
    ones_c = min(st_in[0], kHdlcMaxOnes);
    alive_c = st_in[1] != 0 ? 1u : 0u;
    n_c = alive_c != 0 ? min(st_in[2], P.cap) : 0u;
  }
  for (uint32_t i = tid; i < kHdlcKbDw; i += kHdlcThreads)
  {
    kb[i] = i < (n_c + 31u) / 32u ? st_in[4 + i] : 0u;
  }
  if (tid < 3)
  {
    cnt[tid] = 0;
  }
  uint32_t out_off = 0;                        // bytes of the call's good records, written or not

  for (uint32_t t0 = 0; t0 < nb; t0 += kHdlcTile)
  {
    // 1. the lane's bits
    const uint32_t at = t0 + tid * kHdlcPer;
    const uint32_t k = at < nb ? min((uint32_t)kHdlcPer, nb - at) : 0u;
    uint32_t vm = 0, cm = 0;
    if (k == (uint32_t)kHdlcPer)
    {
      const hdlc_u2_any d = *(const hdlc_u2_any *)(row + at);
      // bit 0 of byte i to bit i, bit 1 of byte i to bit i: a multiply gathers a dword's four
      const uint32_t v0 = d.x & 0x01010101u, v1 = d.y & 0x01010101u;
      const uint32_t c0 = (d.x >> 1) & 0x01010101u, c1 = (d.y >> 1) & 0x01010101u;
      vm = ((v0 * 0x10204080u) >> 28) | (((v1 * 0x10204080u) >> 28) << 4);
      cm = ((c0 * 0x10204080u) >> 28) | (((c1 * 0x10204080u) >> 28) << 4);
    }
    else
    {
      for (uint32_t i = 0; i < k; i++)
      {
        const uint32_t b = row[at + i];
        vm |= (b & kHdlcBitValue) << i;
        cm |= ((b >> 1) & 1u) << i;
      }
    }
    vmb[tid] = (uint8_t)vm;
    for (uint32_t i = tid; i < kHdlcMaxFlags + 1u; i += kHdlcThreads)
    {
      dead[i] = i == 0 && alive_c == 0 ? 1u : 0u;
    }
    __syncthreads();

    // the run in front of the lane (a lane with bits has a whole lane in front of it), then the classes of its bits
    uint32_t ones = ones_c;
    if (tid > 0)
    {
      const uint32_t inv = ~(uint32_t)vmb[tid - 1] & 255u;
      ones = min(kHdlcMaxOnes, (uint32_t)__builtin_clz((inv << 24) | 0x00800000u));
    }
    uint32_t keepm = 0, flagm = 0, abortm = 0;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)kHdlcPer; i++)
    {
      if (i < k)
      {
        const uint32_t v = (vm >> i) & 1u, cls = hdlc_classify(v, ones);
        keepm |= (cls & kHdlcKeep) != 0 ? 1u << i : 0u;
        flagm |= (cls & kHdlcFlag) != 0 ? 1u << i : 0u;
        abortm |= (cls & kHdlcAbort) != 0 ? 1u << i : 0u;
        ones = hdlc_next_ones(v, ones);
      }
    }
    if (P.require_carrier != 0)
    {
      abortm |= ~cm & ((1u << k) - 1u);
    }
    const uint32_t n_tile = min(kHdlcTile, nb - t0);
    if (tid == (n_tile - 1u) / (uint32_t)kHdlcPer)
    {
      end_ones = ones;
    }

    // 2. where the lane's kept bits and flags lie among the tile's
    uint32_t total;
    const uint32_t ex = hdlc_scan((uint32_t)__builtin_popcount(keepm) | ((uint32_t)__builtin_popcount(flagm) << 16), wt, &total);
    const uint32_t K = ex & 0xffffu, F = ex >> 16, Kt = total & 0xffffu, Ft = total >> 16;

    // 3. compaction, the flags' places, the dead segments
    {
      uint32_t cv = 0, nk = 0;
#pragma unroll
      for (uint32_t i = 0; i < (uint32_t)kHdlcPer; i++)
      {
        if ((keepm >> i) & 1u)
        {
          cv |= ((vm >> i) & 1u) << nk;
          nk++;
        }
      }
      const uint32_t pos = n_c + K, s = pos & 31u;
      if (cv != 0)
      {
        atomicOr(&kb[pos >> 5], cv << s);
        if (s + nk > 32u)
        {
          atomicOr(&kb[(pos >> 5) + 1u], cv >> (32u - s));
        }
      }
      uint32_t fm = flagm;
      while (fm != 0)
      {
        const uint32_t i = (uint32_t)__builtin_ctz(fm), below = (1u << i) - 1u;
        fm &= fm - 1u;
        fl[F + (uint32_t)__builtin_popcount(flagm & below)] = (K + (uint32_t)__builtin_popcount(keepm & below)) | ((tid * kHdlcPer + i) << 16);
      }
      uint32_t am = abortm;
      while (am != 0)
      {
        const uint32_t i = (uint32_t)__builtin_ctz(am), below = (1u << i) - 1u;
        am &= am - 1u;
        dead[F + (uint32_t)__builtin_popcount(flagm & below)] = 1u;
      }
    }
    __syncthreads();

    // 4. the frames that close in the tile, 256 flags a round
    for (uint32_t f0 = 0; f0 < Ft; f0 += kHdlcThreads)
    {
      const uint32_t f = f0 + tid;
      uint32_t S = 0, n_bytes = 0, size = 0, end_bit = 0;
      if (f < Ft)
      {
        const uint32_t e = fl[f];
        const uint32_t E = n_c + (e & 0xffffu);
        S = f > 0 ? n_c + (fl[f - 1] & 0xffffu) : 0u;
        end_bit = t0 + (e >> 16);
        const uint32_t n = E - S;
        if (dead[f] == 0 && n <= P.cap && n >= P.least && ((n - kHdlcFlagBits) & 7u) == 0)
        {
          n_bytes = (n - kHdlcFlagBits) >> 3;
          uint32_t crc = 0xFFFFu;
          for (uint32_t b = 0; b < n_bytes; b++)
          {
            crc = hdlc_crc_byte(crc, hdlc_word_at(kb, S + 8u * b) & 255u);
          }
          if (crc == kHdlcResidue)
          {
            size = hdlc_record_bytes(n_bytes - 2u);
          }
          else
          {
            atomicAdd(&cnt[1], 1u);
          }
        }
      }
      uint32_t sizes;
      const uint32_t off = out_off + hdlc_scan(size, wt, &sizes);
      if (size != 0)
      {
        if (off + size <= P.out_bytes)         // (sizes of a call stay far below 2^32: at most 2^15 frames of 1032 bytes)
        {
          const uint32_t p = n_bytes - 2u, fcs = hdlc_word_at(kb, S + 8u * p) & 0xffffu;
          uint32_t *rec = (uint32_t *)(out_row + off);
          rec[0] = end_bit;
          rec[1] = p | (fcs << 16);
          for (uint32_t j = 0; 4u * j < p; j++)
          {
            const uint32_t left = p - 4u * j;  // payload bytes from this dword on
            const uint32_t w = hdlc_word_at(kb, S + 32u * j);
            rec[2 + j] = left >= 4u ? w : w & ((1u << (8u * left)) - 1u);
          }
          atomicAdd(&cnt[0], 1u);
        }
        else
        {
          atomicAdd(&cnt[2], 1u);
        }
      }
      out_off += sizes;
    }

    // 5. the open segment moves to the front of kb
    const uint32_t S_open = Ft > 0 ? n_c + (fl[Ft - 1] & 0xffffu) : 0u;
    uint32_t n_open = n_c + Kt - S_open;
    uint32_t alive = dead[Ft] == 0 && n_open <= P.cap ? 1u : 0u;
    n_open = alive != 0 ? n_open : 0u;
    uint32_t moved[2];
#pragma unroll
    for (uint32_t q = 0; q < 2; q++)
    {
      const uint32_t i = tid + q * kHdlcThreads;
      moved[q] = 0;
      if (32u * i < n_open)                    // then S_open + 32 i lies below the tile's last kept bit, inside kb
      {
        const uint32_t w = hdlc_word_at(kb, S_open + 32u * i), left = n_open - 32u * i;
        moved[q] = left >= 32u ? w : w & ((1u << left) - 1u);
      }
    }
    const uint32_t next_ones = end_ones;
    __syncthreads();
#pragma unroll
    for (uint32_t q = 0; q < 2; q++)
    {
      const uint32_t i = tid + q * kHdlcThreads;
      if (i < kHdlcKbDw)
      {
        kb[i] = moved[q];
      }
    }
    ones_c = next_ones;
    alive_c = alive;
    n_c = n_open;
    __syncthreads();
  }

  // the state and the counts
  __syncthreads();
  uint32_t *st_out = P.state_out + (uint64_t)c * kHdlcStateDw;
  for (uint32_t i = tid; i < (n_c + 31u) / 32u; i += kHdlcThreads)
  {
    st_out[4 + i] = kb[i];
  }
  if (tid == 0)
  {
    st_out[0] = ones_c;
    st_out[1] = alive_c;
    st_out[2] = n_c;
    st_out[3] = 0;
    P.n_frames[c] = cnt[0];
    if (P.n_bad != nullptr)
    {
      P.n_bad[c] = cnt[1];
    }
    P.dropped[c] = cnt[2];
  }
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_hdlc
{
  hrfd::BankCore core;
  uint32_t n_channels = 0;

  // host settings, under core.mu: they travel in the kernel's arguments, so a setter has nothing to upload
  hrfd::HdlcLimits lim{hrfd::kHdlcDefaultMin, hrfd::kHdlcDefaultMax, 0u};
  hrfd::BankHistory hist;                  // HdlcState per channel as 260 dwords

  hrfd::PinnedBuf<uint8_t> h_stage;        // the fresh flags
  // host-path staging
  hrfd::DevBuf<uint8_t> d_bits, d_out;
  hrfd::DevBuf<uint32_t> d_n_bits, d_n_frames, d_n_bad, d_dropped;
};

extern "C" int hrfd_hdlc_create(uint32_t n_channels, int device, hrfd_hdlc **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(hdlc_check_create("hrfd_hdlc_create", n_channels, out));
  hrfd_hdlc *h = nullptr;
  BANK_TRY(bank_new("hrfd_hdlc_create", device, &h));
  const size_t C = n_channels;
  h->n_channels = n_channels;
  if (!(h->hist.alloc(C, kHdlcStateDw) && h->h_stage.alloc(C)))
  {
    (void)hipGetLastError();
    bank_free(h);
    return fail(HRFD_ENOMEM, "hrfd_hdlc_create: device allocation failed");
  }
  *out = h;
  return HRFD_OK;
}

extern "C" int hrfd_hdlc_destroy(hrfd_hdlc *h)
{
  if (h != nullptr)
  {
    hrfd::bank_free(h);
  }
  return HRFD_OK;
}

// every channel starts again: a partial frame collected under another bound means nothing
extern "C" int hrfd_hdlc_set_limits(hrfd_hdlc *h, uint32_t min_payload, uint32_t max_payload)
{
  using namespace hrfd;
  BANK_TRY(hdlc_check_limits("hrfd_hdlc_set_limits", min_payload, max_payload));
  BANK_TRY(bank_need_handle("hrfd_hdlc_set_limits", h));
  std::lock_guard<std::mutex> g(h->core.mu);
  h->lim.min_payload = min_payload;
  h->lim.max_payload = max_payload;
  h->hist.mark(HRFD_ALL_CHANNELS);
  return HRFD_OK;
}

extern "C" int hrfd_hdlc_set_require_carrier(hrfd_hdlc *h, int on)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_hdlc_set_require_carrier", h));
  std::lock_guard<std::mutex> g(h->core.mu);
  h->lim.require_carrier = on != 0 ? 1u : 0u;
  return HRFD_OK;
}

extern "C" int hrfd_hdlc_reset(hrfd_hdlc *h, uint32_t channel) { return hrfd::bank_reset_history(h, "hrfd_hdlc_reset", channel); }

extern "C" int hrfd_hdlc_max_out(hrfd_hdlc *h, uint32_t max_bits, uint32_t *out_bytes)
{
  using namespace hrfd;
  BANK_TRY(hdlc_check_max_bits("hrfd_hdlc_max_out", max_bits));
  if (out_bytes == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_hdlc_max_out: NULL result pointer");
  }
  BANK_TRY(bank_need_handle("hrfd_hdlc_max_out", h));
  std::lock_guard<std::mutex> g(h->core.mu);
  *out_bytes = hdlc_max_out(max_bits, h->lim.min_payload, h->lim.max_payload);
  return HRFD_OK;
}

// one call on `st`: the fresh flags, then k_hdlc, one workgroup per channel
static int hdlc_launch(hrfd_hdlc *h, const uint8_t *d_bits, uint64_t bits_stride, const uint32_t *d_n_bits, uint32_t max_bits,
                       uint8_t *d_out, uint64_t out_stride, uint32_t out_bytes, uint32_t *d_n_frames, uint32_t *d_n_bad,
                       uint32_t *d_dropped, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(h->core.order_behind_last(st));
  HdlcParams P;
  {
    std::lock_guard<std::mutex> g(h->core.mu);
    P.reset = h->hist.reset();
    P.state_in = h->hist.in();
    P.state_out = h->hist.out();
    h->hist.flip();
    if (h->hist.any_fresh)
    {
      BANK_TRY(h->core.staging_wait());
      BANK_TRY(h->hist.upload(h->h_stage, st));
      BANK_TRY(h->core.staging_sent(st));
    }
    P.least = hdlc_least(h->lim.min_payload);
    P.cap = hdlc_cap(h->lim.max_payload);
    P.require_carrier = h->lim.require_carrier;
  }
  P.bits = d_bits;
  P.bits_stride = bits_stride;
  P.n_bits = d_n_bits;
  P.max_bits = max_bits;
  P.out = d_out;
  P.out_stride = out_stride;
  P.out_bytes = out_bytes;
  P.n_frames = d_n_frames;
  P.n_bad = d_n_bad;
  P.dropped = d_dropped;
  hipLaunchKernelGGL(k_hdlc, dim3(h->n_channels), dim3(kHdlcThreads), 0, st, P);
  BANK_TRY(bank_launch_ok("k_hdlc"));
  h->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_hdlc_process_device(hrfd_hdlc *h, const uint8_t *d_bits, uint64_t bits_stride_bytes, const uint32_t *d_n_bits,
                                        uint32_t max_bits, uint8_t *d_out, uint64_t out_stride_bytes, uint32_t out_bytes,
                                        uint32_t *d_n_frames, uint32_t *d_n_bad, uint32_t *d_dropped, void *stream)
{
  using namespace hrfd;
  BANK_TRY(hdlc_check_call("hrfd_hdlc_process_device", d_bits, bits_stride_bytes, true, d_n_bits, max_bits, d_out, out_stride_bytes,
                           out_bytes, d_n_frames, d_n_bad, d_dropped));
  BANK_TRY(bank_need_handle("hrfd_hdlc_process_device", h));
  HIP_TRY(hipSetDevice(h->core.device));
  return hdlc_launch(h, d_bits, bits_stride_bytes, d_n_bits, max_bits, d_out, out_stride_bytes, out_bytes, d_n_frames, d_n_bad,
                     d_dropped, h->core.stream_or_own(stream));
}

// bits: dense rows of max_bits bytes; out: dense rows of out_bytes.  The records go up as well as down, so that the bytes of
// a row behind its last record come back as they were
extern "C" int hrfd_hdlc_process(hrfd_hdlc *h, const uint8_t *bits, const uint32_t *n_bits, uint32_t max_bits, uint8_t *out,
                                 uint32_t out_bytes, uint32_t *n_frames, uint32_t *n_bad, uint32_t *dropped)
{
  using namespace hrfd;
  BANK_TRY(hdlc_check_call("hrfd_hdlc_process", bits, 0, false, n_bits, max_bits, out, 0, out_bytes, n_frames, n_bad, dropped));
  BANK_TRY(bank_need_handle("hrfd_hdlc_process", h));
  BankHostCall call(h->core);
  const size_t C = h->n_channels;
  const uint8_t *d_bits = call.up(h->d_bits, bits, (size_t)max_bits * C);
  const uint32_t *d_n_bits = call.up(h->d_n_bits, n_bits, 4 * C);
  uint8_t *d_out = call.up(h->d_out, out, (size_t)out_bytes * C);
  uint32_t *d_n_frames = call.room(h->d_n_frames, n_frames, 4 * C);
  uint32_t *d_n_bad = call.room(h->d_n_bad, n_bad, 4 * C);
  uint32_t *d_dropped = call.room(h->d_dropped, dropped, 4 * C);
  BANK_TRY(call.rc);
  BANK_TRY(hdlc_launch(h, d_bits, max_bits, d_n_bits, max_bits, d_out, out_bytes, out_bytes, d_n_frames, d_n_bad, d_dropped, call.st));
  call.down(out, d_out, (size_t)out_bytes * C);
  call.down(n_frames, d_n_frames, 4 * C);
  call.down(n_bad, d_n_bad, 4 * C);
  call.down(dropped, d_dropped, 4 * C);
  return call.finish();
}

// ---- read-only introspection (include/hrfd_debug.h): the law of hrfd_hdlc.h on the host, for tests/test_hdlc_model.py
extern "C" int hrfd_hdlc_debug_slow(const uint32_t *limits3, const uint8_t *bits, uint32_t n_bits, uint32_t *state260, uint8_t *out,
                                    uint32_t out_bytes, uint32_t *counts3)
{
  using namespace hrfd;
  if (limits3 == nullptr || state260 == nullptr || counts3 == nullptr || out == nullptr || (bits == nullptr && n_bits != 0))
  {
    return fail(HRFD_EINVAL, "hrfd_hdlc_debug_slow: NULL argument");
  }
  BANK_TRY(hdlc_check_limits("hrfd_hdlc_debug_slow", limits3[0], limits3[1]));
  if (n_bits > kHdlcMaxBits)
  {
    return fail(HRFD_EINVAL, "hrfd_hdlc_debug_slow: n_bits must be 0..%u (got %u)", kHdlcMaxBits, n_bits);
  }
  if (out_bytes < 4u || (out_bytes & 3u) != 0)
  {
    return fail(HRFD_EINVAL, "hrfd_hdlc_debug_slow: out_bytes %u must be a multiple of 4, at least 4", out_bytes);
  }
  HdlcState st;
  memcpy(&st, state260, sizeof(st));
  if (st.ones > kHdlcMaxOnes || st.n > hdlc_cap(limits3[1]))
  {
    return fail(HRFD_EINVAL, "hrfd_hdlc_debug_slow: a state no call leaves (ones %u, n %u)", st.ones, st.n);
  }
  hdlc_channel_slow(bits, n_bits, HdlcLimits{limits3[0], limits3[1], limits3[2] != 0 ? 1u : 0u}, &st, out, out_bytes, counts3);
  memcpy(state260, &st, sizeof(st));
  return HRFD_OK;
}

extern "C" int hrfd_hdlc_debug_max_out(uint32_t max_bits, uint32_t min_payload, uint32_t max_payload, uint32_t *out_bytes)
{
  using namespace hrfd;
  BANK_TRY(hdlc_check_max_bits("hrfd_hdlc_debug_max_out", max_bits));
  BANK_TRY(hdlc_check_limits("hrfd_hdlc_debug_max_out", min_payload, max_payload));
  if (out_bytes == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_hdlc_debug_max_out: NULL result pointer");
  }
  *out_bytes = hdlc_max_out(max_bits, min_payload, max_payload);
  return HRFD_OK;
}
