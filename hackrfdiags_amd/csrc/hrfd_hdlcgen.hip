// hackrfdiags_amd/csrc/hrfd_hdlcgen.hip -- hrfd_hdlcgen_*: packet frames into bits on the device, the mirror of hrfd_hdlc_*,
// and hrfd_hdlc_encode, the same law for one row on the host.
//
// Rows of frame records (hrfd_hdlc_record: what hrfd_hdlc_process_device writes) and their counts in; per channel a row of
// bits, a byte a bit (what hrfd_afskgen_queue takes and hrfd_hdlc_* reads), and three counts out.  The law is bit by bit,
// contract in include/hrfd.h; tests/hdlcgen_model.py restates it, hrfd_hdlcgen.h holds the rules both sides of this file
// share and the slow loop.
//
// k_hdlcgen: one launch, one workgroup of 256 threads per channel, which takes its row frame by frame and a frame in tiles
// of kHdlcgenTile = 2048 data bits, one byte (8 consecutive bits) per lane.  Nothing walks a frame's bits: every step is the
// same few instructions for every lane, or a scan over the lanes.
//   1. the check sequence: byte i of a payload of n adds M^(n - i) of itself to the CRC register (hrfd_hdlcgen.h 4.), every
//      lane for its own bytes from a table of ten levels that are immediates in the code; one XOR reduction over the workgroup
//      gives the register, and the lanes of bytes n and n + 1 take the two bytes of the sequence
//   2. the run of ones in front of a lane's first bit.  A run is unbounded here (a payload of 0xFF is one run), so it is a real
//      scan with the operator hdlcgen_run_join: shuffles inside a wave, the four wave totals through LDS, the run behind a
//      tile carried to the next, zero at a frame's first bit
//   3. the lane stuffs its byte behind that run (hdlcgen_stuff_byte: 8..10 bits), and an exclusive additive scan of the
//      lengths gives the lane's place in the frame
//   4. the bits go into `ob`, a bit row in LDS that starts with the flags in front of the frame (lead or between): a lane's
//      bits land in at most two dwords, by LDS vector atomics (ds_or_b32)
//   5. the frame's length is now known: if it fits with the tail flags still to come, ob goes out as bytes, four bits a
//      dword store wherever the address is a multiple of 4 and single bytes at the two ends; if not, the walk ends
// Behind the last frame sent the tail flags go out the same way.  The grid is the channel count, at most 65536 workgroups:
// below kBankMaxWgs, so the launch is never cut.  The counts are read and written on the device; no call waits for it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "hrfd_hdlcgen.h"

namespace hrfd {

constexpr int kHdlcgenThreads = 256;
constexpr uint32_t kHdlcgenTile = kHdlcgenThreads * 8u;    // data bits of one tile
constexpr uint32_t kHdlcgenTiles = (kHdlcgenMaxData + kHdlcgenTile - 1u) / kHdlcgenTile;       // 4
constexpr uint32_t kHdlcgenObBits = 8u * kHdlcgenMaxFlags + kHdlcgenMaxFrame;      // the flags in front and the longest frame
constexpr uint32_t kHdlcgenObDw = (kHdlcgenObBits + 31u) / 32u + 1u;               // and a dword to read over
static_assert(65536u <= kBankMaxWgs, "one workgroup per channel is one launch");

struct HdlcgenParams
{
  const uint8_t *in;                       // [C] rows of records, in_stride bytes apart, 4-byte aligned
  uint64_t in_stride;
  uint32_t in_bytes;
  const uint32_t *n_frames;                // [C]
  uint8_t *bits;                           // [C] rows, bits_stride bytes apart, any address
  uint64_t bits_stride;
  uint32_t max_bits;
  uint32_t *n_bits, *n_sent, *dropped;     // [C]; n_sent and dropped may be NULL
  HdlcgenFlags fl;
};

// XOR of v over the workgroup; wt: four dwords of LDS.  Every thread calls it
__device__ __forceinline__ uint32_t hdlcgen_xor_all(uint32_t v, uint32_t *wt)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1)
  {
    v ^= __shfl_xor(v, d, 64);
  }
  if ((threadIdx.x & 63u) == 0)
  {
    wt[threadIdx.x >> 6] = v;
  }
  __syncthreads();
  const uint32_t all = wt[0] ^ wt[1] ^ wt[2] ^ wt[3];
  __syncthreads();                         // the next scan writes wt again
  return all;
}

// exclusive scan of the run elements e over the workgroup behind the run `carry` (an element without bit 31), and in *next
// the run behind the last lane
__device__ __forceinline__ uint32_t hdlcgen_run_scan(uint32_t e, uint32_t carry, uint32_t *wt, uint32_t *next)
{
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = e;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t o = __shfl_up(inc, d, 64);
    inc = lane >= (uint32_t)d ? hdlcgen_run_join(o, inc) : inc;
  }
  if (lane == 63u)
  {
    wt[wave] = inc;
  }
  const uint32_t left = __shfl_up(inc, 1, 64);
  __syncthreads();
  uint32_t pre = carry, run = carry;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)kHdlcgenThreads / 64u; w++)
  {
    run = hdlcgen_run_join(run, wt[w]);
    pre = w + 1u == wave ? run : pre;
  }
  __syncthreads();
  *next = run;
  return lane > 0 ? hdlcgen_run_join(pre, left) : pre;
}

// exclusive scan of v over the workgroup, and the total
__device__ __forceinline__ uint32_t hdlcgen_scan(uint32_t v, uint32_t *wt, uint32_t *total)
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
  for (uint32_t w = 0; w < (uint32_t)kHdlcgenThreads / 64u; w++)
  {
    const uint32_t t = wt[w];
    pre += w < wave ? t : 0u;
    sum += t;
  }
  __syncthreads();
  *total = sum;
  return pre + inc - v;
}

// n whole flags from the front of a bit row: dword i of it
__device__ __forceinline__ uint32_t hdlcgen_flag_word(uint32_t i, uint32_t n)
{
  const uint32_t left = 32u * i < 8u * n ? 8u * n - 32u * i : 0u;
  return left >= 32u ? 0x7E7E7E7Eu : 0x7E7E7E7Eu & ((1u << left) - 1u);
}

// the first n bits of the bit row ob, a byte each, to dst (any address): single bytes up to the first multiple of 4, then
// four bits a dword, then the bytes left over.  ob has a dword behind its last bit.  Every thread calls it
__device__ __forceinline__ void hdlcgen_flush(const uint32_t *ob, uint32_t n, uint8_t *dst)
{
  const uint32_t tid = threadIdx.x;
  uint32_t head = (uint32_t)(0u - (uint32_t)(uintptr_t)dst) & 3u;
  head = head < n ? head : n;
  const uint32_t n_dw = (n - head) >> 2, tail_at = head + 4u * n_dw;
  if (tid < head)
  {
    dst[tid] = (uint8_t)((ob[0] >> tid) & 1u);
  }
  uint32_t *body = (uint32_t *)(dst + head);
  for (uint32_t j = tid; j < n_dw; j += kHdlcgenThreads)
  {
    const uint32_t at = head + 4u * j, w = at >> 5, s = at & 31u;
    const uint32_t x = (uint32_t)((((uint64_t)ob[w + 1] << 32) | ob[w]) >> s) & 15u;
    body[j] = (x * 0x00204081u) & 0x01010101u;             // bit i of x to byte i
  }
  if (tid < n - tail_at)
  {
    const uint32_t at = tail_at + tid;
    dst[at] = (uint8_t)((ob[at >> 5] >> (at & 31u)) & 1u);
  }
}

__global__ __launch_bounds__(kHdlcgenThreads) void k_hdlcgen(const HdlcgenParams P)
{
  __shared__ uint32_t ob[kHdlcgenObDw];
  __shared__ uint32_t wt[4];
  constexpr HdlcgenCrcPow kPow = hdlcgen_crc_pow();
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  const uint8_t *row = P.in + (uint64_t)c * P.in_stride;
  uint8_t *out = P.bits + (uint64_t)c * P.bits_stride;
  const uint32_t nf = P.n_frames[c];
  uint32_t at = 0, cur = 0, sent = 0;          // bytes of the row taken, bits of the row written, frames framed: uniform

  for (uint32_t f = 0; f < nf; f++)
  {
    const uint32_t n = hdlcgen_record_at(row, P.in_bytes, at);
    if (n == 0)
    {
      break;
    }
    const uint8_t *payload = row + at + kHdlcHeader;
    const uint32_t n_data = n + 2u, pre = sent == 0 ? P.fl.lead : P.fl.between;

    // ob starts with the flags in front of the frame; the rest of it is zero for the lanes' ORs
    for (uint32_t i = tid; i < kHdlcgenObDw; i += kHdlcgenThreads)
    {
      ob[i] = hdlcgen_flag_word(i, pre);
    }

    // 1. the lane's bytes and the check sequence
    uint32_t b[kHdlcgenTiles], term = 0;
#pragma unroll
    for (uint32_t t = 0; t < kHdlcgenTiles; t++)
    {
      const uint32_t i = t * kHdlcgenThreads + tid;
      b[t] = 0;
      if (i < n)
      {
        b[t] = payload[i];
        term ^= hdlcgen_crc_term(kPow, b[t], i, n);
      }
    }
    const uint32_t fcs = ~hdlcgen_xor_all(term, wt) & 0xFFFFu;         // (its barriers also order ob's fill before the ORs)
#pragma unroll
    for (uint32_t t = 0; t < kHdlcgenTiles; t++)
    {
      const uint32_t i = t * kHdlcgenThreads + tid;
      b[t] = i == n ? fcs & 255u : (i == n + 1u ? fcs >> 8 : b[t]);
    }

    // 2. to 4. tile by tile: the run in front of the lane, its stuffed bits, their place, into ob
    uint32_t run = 0, len = 0;
#pragma unroll
    for (uint32_t t = 0; t < kHdlcgenTiles; t++)
    {
      if (t * kHdlcgenThreads < n_data)        // uniform
      {
        const uint32_t i = t * kHdlcgenThreads + tid;
        const bool live = i < n_data;
        uint32_t next;
        const uint32_t in_front = hdlcgen_run_scan(live ? hdlcgen_run_of_byte(b[t]) : 0u, run, wt, &next);
        uint32_t v = 0, k = 0;
        if (live)
        {
          k = hdlcgen_stuff_byte(b[t], in_front, &v);
        }
        uint32_t tile_len;
        const uint32_t pos = 8u * pre + len + hdlcgen_scan(k, wt, &tile_len), s = pos & 31u;
        if (v != 0)
        {
          atomicOr(&ob[pos >> 5], v << s);
          if (s + k > 32u)
          {
            atomicOr(&ob[(pos >> 5) + 1u], v >> (32u - s));
          }
        }
        run = next;
        len += tile_len;
      }
    }

    // 5. the frame goes out if it fits with the tail flags still to come
    if ((uint64_t)cur + 8u * pre + len + 8u * P.fl.tail > P.max_bits)
    {
      break;
    }
    __syncthreads();
    hdlcgen_flush(ob, 8u * pre + len, out + cur);
    cur += 8u * pre + len;
    sent++;
    at += hdlc_record_bytes(n);
    __syncthreads();                           // ob is filled again
  }

  if (sent != 0)
  {
    __syncthreads();
    for (uint32_t i = tid; i < 8u * kHdlcgenMaxFlags / 32u + 2u; i += kHdlcgenThreads)
    {
      ob[i] = hdlcgen_flag_word(i, P.fl.tail);
    }
    __syncthreads();
    hdlcgen_flush(ob, 8u * P.fl.tail, out + cur);
    cur += 8u * P.fl.tail;
  }
  if (tid == 0)
  {
    P.n_bits[c] = cur;
    if (P.n_sent != nullptr)
    {
      P.n_sent[c] = sent;
    }
    if (P.dropped != nullptr)
    {
      P.dropped[c] = nf - sent;
    }
  }
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_hdlcgen
{
  hrfd::BankCore core;
  uint32_t n_channels = 0;

  // host settings, under core.mu: they travel in the kernel's arguments, so a setter has nothing to upload
  hrfd::HdlcgenFlags fl{hrfd::kHdlcgenDefaultLead, hrfd::kHdlcgenDefaultBetween, hrfd::kHdlcgenDefaultTail};

  // host-path staging
  hrfd::DevBuf<uint8_t> d_in, d_bits;
  hrfd::DevBuf<uint32_t> d_n_frames, d_n_bits, d_n_sent, d_dropped;
};

extern "C" int hrfd_hdlcgen_create(uint32_t n_channels, int device, hrfd_hdlcgen **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(hdlcgen_check_create("hrfd_hdlcgen_create", n_channels, out));
  hrfd_hdlcgen *h = nullptr;
  BANK_TRY(bank_new("hrfd_hdlcgen_create", device, &h));
  h->n_channels = n_channels;
  *out = h;
  return HRFD_OK;
}

extern "C" int hrfd_hdlcgen_destroy(hrfd_hdlcgen *h)
{
  if (h != nullptr)
  {
    hrfd::bank_free(h);
  }
  return HRFD_OK;
}

extern "C" int hrfd_hdlcgen_set_flags(hrfd_hdlcgen *h, uint32_t n_lead_flags, uint32_t n_between, uint32_t n_tail_flags)
{
  using namespace hrfd;
  BANK_TRY(hdlcgen_check_flags("hrfd_hdlcgen_set_flags", n_lead_flags, n_between, n_tail_flags));
  BANK_TRY(bank_need_handle("hrfd_hdlcgen_set_flags", h));
  std::lock_guard<std::mutex> g(h->core.mu);
  h->fl = HdlcgenFlags{n_lead_flags, n_between, n_tail_flags};
  return HRFD_OK;
}

extern "C" int hrfd_hdlcgen_max_bits(hrfd_hdlcgen *h, uint32_t n_frames, uint64_t payload_bytes, uint32_t *max_bits)
{
  using namespace hrfd;
  // what the arguments decide under any flag counts comes first, so that it is refused without a handle as well
  uint32_t least = 0;
  BANK_TRY(hdlcgen_check_bound("hrfd_hdlcgen_max_bits", n_frames, payload_bytes, HdlcgenFlags{0, 1, 1}, max_bits != nullptr ? &least : nullptr));
  BANK_TRY(bank_need_handle("hrfd_hdlcgen_max_bits", h));
  std::lock_guard<std::mutex> g(h->core.mu);
  return hdlcgen_check_bound("hrfd_hdlcgen_max_bits", n_frames, payload_bytes, h->fl, max_bits);
}

// one call on `st`: k_hdlcgen, one workgroup per channel
static int hdlcgen_launch(hrfd_hdlcgen *h, const uint8_t *d_in, uint64_t in_stride, uint32_t in_bytes, const uint32_t *d_n_frames,
                          uint8_t *d_bits, uint64_t bits_stride, uint32_t max_bits, uint32_t *d_n_bits, uint32_t *d_n_sent,
                          uint32_t *d_dropped, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(h->core.order_behind_last(st));
  HdlcgenParams P;
  {
    std::lock_guard<std::mutex> g(h->core.mu);
    P.fl = h->fl;
  }
  P.in = d_in;
  P.in_stride = in_stride;
  P.in_bytes = in_bytes;
  P.n_frames = d_n_frames;
  P.bits = d_bits;
  P.bits_stride = bits_stride;
  P.max_bits = max_bits;
  P.n_bits = d_n_bits;
  P.n_sent = d_n_sent;
  P.dropped = d_dropped;
  hipLaunchKernelGGL(k_hdlcgen, dim3(h->n_channels), dim3(kHdlcgenThreads), 0, st, P);
  BANK_TRY(bank_launch_ok("k_hdlcgen"));
  h->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_hdlcgen_process_device(hrfd_hdlcgen *h, const uint8_t *d_in, uint64_t in_stride_bytes, uint32_t in_bytes,
                                           const uint32_t *d_n_frames, uint8_t *d_bits, uint64_t bits_stride_bytes, uint32_t max_bits,
                                           uint32_t *d_n_bits, uint32_t *d_n_sent, uint32_t *d_dropped, void *stream)
{
  using namespace hrfd;
  const char *who = "hrfd_hdlcgen_process_device";
  BANK_TRY(hdlcgen_check_call(who, d_in, in_stride_bytes, in_bytes, true, d_n_frames, d_bits, bits_stride_bytes, max_bits, d_n_bits,
                              d_n_sent, d_dropped, 1));
  BANK_TRY(bank_need_handle(who, h));
  BANK_TRY(hdlcgen_check_call(who, d_in, in_stride_bytes, in_bytes, true, d_n_frames, d_bits, bits_stride_bytes, max_bits, d_n_bits,
                              d_n_sent, d_dropped, h->n_channels));
  HIP_TRY(hipSetDevice(h->core.device));
  return hdlcgen_launch(h, d_in, in_stride_bytes, in_bytes, d_n_frames, d_bits, bits_stride_bytes, max_bits, d_n_bits, d_n_sent,
                        d_dropped, h->core.stream_or_own(stream));
}

// records: dense rows of in_bytes bytes; bits: dense rows of max_bits.  The bits go up as well as down, so that the bytes of
// a row behind n_bits come back as they were
extern "C" int hrfd_hdlcgen_process(hrfd_hdlcgen *h, const uint8_t *records, uint32_t in_bytes, const uint32_t *n_frames,
                                    uint8_t *bits, uint32_t max_bits, uint32_t *n_bits, uint32_t *n_sent, uint32_t *dropped)
{
  using namespace hrfd;
  BANK_TRY(hdlcgen_check_call("hrfd_hdlcgen_process", records, 0, in_bytes, false, n_frames, bits, 0, max_bits, n_bits, n_sent,
                              dropped, 1));
  BANK_TRY(bank_need_handle("hrfd_hdlcgen_process", h));
  BankHostCall call(h->core);
  const size_t C = h->n_channels;
  const uint8_t *d_in = call.up(h->d_in, records, (size_t)in_bytes * C);
  const uint32_t *d_n_frames = call.up(h->d_n_frames, n_frames, 4 * C);
  uint8_t *d_bits = call.up(h->d_bits, bits, (size_t)max_bits * C);
  uint32_t *d_n_bits = call.room(h->d_n_bits, n_bits, 4 * C);
  uint32_t *d_n_sent = call.room(h->d_n_sent, n_sent, 4 * C);
  uint32_t *d_dropped = call.room(h->d_dropped, dropped, 4 * C);
  BANK_TRY(call.rc);
  BANK_TRY(hdlcgen_launch(h, d_in, in_bytes, in_bytes, d_n_frames, d_bits, max_bits, max_bits, d_n_bits, d_n_sent, d_dropped, call.st));
  call.down(bits, d_bits, (size_t)max_bits * C);
  call.down(n_bits, d_n_bits, 4 * C);
  call.down(n_sent, d_n_sent, 4 * C);
  call.down(dropped, d_dropped, 4 * C);
  return call.finish();
}

// the law of hrfd_hdlcgen.h for one row on the host: no handle, no device
extern "C" int hrfd_hdlc_encode(const uint8_t *records, uint32_t in_bytes, uint32_t n_frames, uint32_t lead, uint32_t between,
                                uint32_t tail, uint8_t *bits, uint32_t max_bits, uint32_t *n_bits, uint32_t *n_sent, uint32_t *dropped)
{
  using namespace hrfd;
  uint32_t dummy = 0;                          // (the check wants the address of a count that is read; here it is a value)
  BANK_TRY(hdlcgen_check_flags("hrfd_hdlc_encode", lead, between, tail));
  BANK_TRY(hdlcgen_check_call("hrfd_hdlc_encode", records, 0, in_bytes, false, &dummy, bits, 0, max_bits, n_bits, n_sent, dropped, 1));
  BANK_TRY(pcm_check_no_overlap("hrfd_hdlc_encode", records, 0, in_bytes, bits, 0, max_bits, 1,
                                "a row of bits is written while the records are read"));
  uint32_t counts[3];
  hdlcgen_row_slow(records, in_bytes, n_frames, HdlcgenFlags{lead, between, tail}, bits, max_bits, counts);
  *n_bits = counts[0];
  if (n_sent != nullptr)
  {
    *n_sent = counts[1];
  }
  if (dropped != nullptr)
  {
    *dropped = counts[2];
  }
  return HRFD_OK;
}
