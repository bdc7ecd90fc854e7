// hackrfdiags_amd/csrc/hrfd_afsk.hip -- hrfd_afsk_*: packet data (audio frequency-shift keying) off the receive chain's PCM.
//
// PCM rows [C][n_blocks][512] int16 (and n_pcm) in; per channel the recovered bits with a carrier flag, their count, and the
// discriminator's decision for every sample out.  Exact integer arithmetic, contract in include/hrfd.h; tests/afsk_model.py
// restates it in numpy, hrfd_afsk.h holds the laws both sides of this file share.
//
// k_afsk: ONE fused pass, one workgroup of 256 threads per channel, which walks its row in steps of kAfskStep = 2048 samples
// (4 blocks), 8 consecutive samples per lane.  A step has a dense stage for every lane and a serial stage for wave 0:
//   1. a lane loads its 16 bytes (the load of the next step is issued in front of the work on this one), zeroes what lies
//      behind the block's n_pcm and lays them into LDS as packed pairs, behind the 32 samples in front of the step: the
//      handle's state in front of the call, the last four lanes' own registers in front of every later step
//   2. behind a barrier a lane sums the four filters (mark and space, cosine and sine) for its 8 outputs with
//      v_dot2_i32_i16.  Every lane's first output is even, so the parity of its window's start is that of W - 1 for the
//      whole launch: the taps are packed for both parities like the bank core's (bank_pack_taps), as k_audio_fir holds them.
//      They lie in the kernel's arguments, J = W / 2 + 1 pairs a filter, and come through the scalar cache; a pair costs one
//      LDS dword (a window of five slides along) and 32 v_dot2.  |I| <= 32 x 32768 x 2047 < 2^31: int32 is exact at every
//      partial sum.  The squares and their sums run in 64 bits (v_mad_i64_i32); h = P_mark > P_space and the carrier flag
//      of the lane's 8 samples are one byte each: byte n >> 3 of the row of `hard`, and of two bit masks of the step in LDS
//      (with eight consecutive samples in a lane the masks need no ballot)
//   3. behind a second barrier wave 0 walks the two masks in uniform code (the phase, the masks' words and the counters
//      live in scalar registers): per sample the phase advances, a wrap samples a bit, a transition pulls the phase towards
//      mid-bit.  The walk of a word of 32 samples is unrolled, and the wrap is a compare against 2^32 - baud_step in front
//      of the add, not the add's carry: the common sample is then five scalar instructions, the two rare paths lie out of
//      line.  Lane 0 stores the bytes.  The other waves go on to stage 1 of the next step and wait at its barrier; what
//      overlaps the walk is the other workgroups of the compute unit.  A call without bits skips the walk
//   4. behind the last step lanes 0..15 write the last 32 samples, lane 0 the phase and the two flags, to the other side of
//      the state's ping-pong.
// Rows at any even address and stride take one path: the 16 bytes of a lane go through a vector type of alignment 2, as in
// k_level.  The grid is the channel count, at most 65536 workgroups: below kBankMaxWgs for every call the checks let
// through, so the launch is never cut.  The price is that a row is walked by one workgroup, and its bits by one wave: a call
// of few channels and many blocks does not fill the device (DESIGN.md 3.15 has the figures).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrfd_afsk.h"

namespace hrfd {

constexpr int kAfskThreads = 256;
constexpr int kAfskPer = 8;                                // consecutive samples of one lane: 16 bytes
constexpr int kAfskStep = kAfskThreads * kAfskPer;         // samples of one step
constexpr int kAfskStepDw = kAfskStep / 2;
constexpr int kAfskLeadDw = kAfskHistSamples / 2;          // 16 dwords in front of the step
constexpr int kAfskPadDw = 4;                              // what the last lane's window reads over: zero taps meet them
constexpr int kAfskMaxJ = kAfskMaxWindow / 2 + 1;          // 17 tap pairs a filter
constexpr int kAfskMaskDw = kAfskStep / 32;                // 64 words of a step's bit mask
static_assert(kAfskStep % kAfskBlock == 0, "a step is whole blocks");
static_assert(kAfskMaskDw * 4 == kAfskThreads, "a lane's eight decisions are one byte of the mask");
static_assert(kAfskLeadDw % 4 == 0, "the last lanes' own dwords are the next step's lead");
static_assert(65536u <= kBankMaxWgs, "one workgroup per channel is one launch");

struct AfskParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address
  uint64_t stride;
  const uint32_t *n_pcm;                   // [C][n_blocks] or NULL
  const uint32_t *state_in;                // [C][18]: AfskState
  uint32_t *state_out;
  const uint8_t *reset;                    // [C]: non-zero = this channel starts from a zero state; or NULL
  uint8_t *bits;                           // [C] rows, bits_stride bytes apart; or NULL (then the clock does not run)
  uint64_t bits_stride;
  uint32_t max_bits;                       // afsk_max_bits of this call: the law keeps every count at or below it
  uint32_t *n_bits;                        // [C], with bits
  uint8_t *hard;                           // [C][n_blocks][64] or NULL
  uint64_t min_power;
  uint32_t n_blocks, W, J, A, baud_step, nrzi;
  uint32_t wrap_at;                        // 2^32 - baud_step: a phase at or above it wraps with the next sample
  uint2 taps[kAfskMaxJ][kAfskFilters];     // (even, odd) packed pairs of the time-reversed taps, zero from J on
};

// the four filters for a lane's 8 outputs: J tap pairs against a window of five dwords that moves a dword a pair; PAR: the
// parity of the first output's window start.  Output i starts in dword (PAR + i) >> 1 of the window, on its odd half for
// (PAR + i) & 1
template <int PAR>
__device__ __forceinline__ void afsk_filters(const uint32_t *win, const AfskParams &P, int (&acc)[kAfskFilters][kAfskPer])
{
  uint32_t w[5] = {win[0], win[1], win[2], win[3], win[4]};
  for (uint32_t j = 0; j < P.J; j++)
  {
#pragma unroll
    for (int f = 0; f < kAfskFilters; f++)
    {
      const uint2 t = P.taps[j][f];
#pragma unroll
      for (int i = 0; i < kAfskPer; i++)
      {
        acc[f][i] = dot2(w[(PAR + i) >> 1], ((PAR + i) & 1) ? t.y : t.x, acc[f][i]);
      }
    }
    w[0] = w[1];
    w[1] = w[2];
    w[2] = w[3];
    w[3] = w[4];
    w[4] = win[j + 5];
  }
}

__global__ __launch_bounds__(kAfskThreads) void k_afsk(const AfskParams P)
{
  __shared__ uint32_t xs[kAfskLeadDw + kAfskStepDw + kAfskPadDw];
  __shared__ uint32_t hm[kAfskMaskDw], cm[kAfskMaskDw];
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform for the compiler as well
  const int16_t *row = (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride);
  const uint32_t *n_row = P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * P.n_blocks : nullptr;
  uint8_t *hard_row = P.hard != nullptr ? P.hard + (uint64_t)c * P.n_blocks * kAfskHardPerBlock : nullptr;
  uint8_t *bits_row = P.bits != nullptr ? P.bits + (uint64_t)c * P.bits_stride : nullptr;
  const bool fresh = P.reset != nullptr && P.reset[c] != 0;
  const uint32_t *st_in = P.state_in + (uint64_t)c * kAfskStateDw;
  const uint32_t n = P.n_blocks * kAfskBlock;
  const uint32_t par = (P.W - 1u) & 1u, lead = (P.W - 1u + par) / 2u;      // dwords from the window's start to the lane's own

  if (tid < (uint32_t)kAfskLeadDw)
  {
    xs[tid] = fresh ? 0u : st_in[tid];
  }
  if (tid < (uint32_t)kAfskPadDw)
  {
    xs[kAfskLeadDw + kAfskStepDw + tid] = 0u;
  }
  // the clock, uniform: wave 0 keeps it in scalar registers
  uint32_t phi = 0, flags = 0;
  if (!fresh)
  {
    phi = st_in[kAfskHistSamples / 2];
    flags = st_in[kAfskHistSamples / 2 + 1];
  }
  phi = __builtin_amdgcn_readfirstlane(phi);
  uint32_t h_prev = __builtin_amdgcn_readfirstlane(flags & 1u), last = __builtin_amdgcn_readfirstlane((flags >> 1) & 1u);
  uint32_t count = 0;

  pcm_u4 next = {0u, 0u, 0u, 0u};
  if (tid * kAfskPer < n)
  {
    next = pcm_load8(row + tid * kAfskPer);
  }
  uint32_t m[4] = {0u, 0u, 0u, 0u};            // the lane's samples as the filter sees them
  uint32_t valid = 0;                          // samples of the step at hand
  for (uint32_t s0 = 0; s0 < n; s0 += kAfskStep)
  {
    // 1. the samples.  Behind the first step the 32 in front are the last four lanes' of the step before (a step that has
    // one behind it is whole, so those lanes held samples)
    const uint32_t at = s0 + tid * kAfskPer;               // the lane's first sample
    const bool active = at < n;                            // n is whole blocks: a lane has all of its samples or none
    valid = min((uint32_t)kAfskStep, n - s0);
    if (s0 > 0 && tid >= (uint32_t)(kAfskThreads - kAfskLeadDw / 4))
    {
#pragma unroll
      for (int q = 0; q < 4; q++)
      {
        xs[4 * (tid - (kAfskThreads - kAfskLeadDw / 4)) + q] = m[q];
      }
    }
    const pcm_u4 cur = next;
    if (at + kAfskStep < n)
    {
      next = pcm_load8(row + at + kAfskStep);
    }
    const uint32_t d[4] = {cur.x, cur.y, cur.z, cur.w};
    const uint32_t pos = at % kAfskBlock, lim = active ? pcm_block_limit(n_row, at / kAfskBlock) : 0u;
#pragma unroll
    for (int q = 0; q < 4; q++)
    {
      m[q] = pos + 2 * q + 1 < lim ? d[q] : (pos + 2 * q < lim ? d[q] & 0xffffu : 0u);
      xs[kAfskLeadDw + 4 * tid + q] = m[q];
    }
    __syncthreads();

    // 2. the four filters, the powers, the decisions
    int acc[kAfskFilters][kAfskPer];
#pragma unroll
    for (int f = 0; f < kAfskFilters; f++)
    {
#pragma unroll
      for (int i = 0; i < kAfskPer; i++)
      {
        acc[f][i] = 0;
      }
    }
    const uint32_t *win = xs + kAfskLeadDw + 4 * tid - lead;
    if (par)
    {
      afsk_filters<1>(win, P, acc);
    }
    else
    {
      afsk_filters<0>(win, P, acc);
    }
    uint32_t hb = 0, cb = 0;
#pragma unroll
    for (int i = 0; i < kAfskPer; i++)
    {
      const uint64_t p_mark = afsk_power(acc[kAfskMarkC][i], acc[kAfskMarkS][i]);
      const uint64_t p_space = afsk_power(acc[kAfskSpaceC][i], acc[kAfskSpaceS][i]);
      hb |= afsk_decide(p_mark, p_space) << i;
      cb |= afsk_carrier(p_mark, p_space, P.min_power) << i;
    }
    ((uint8_t *)hm)[tid] = (uint8_t)hb;
    ((uint8_t *)cm)[tid] = (uint8_t)cb;
    if (hard_row != nullptr && active)
    {
      hard_row[at >> 3] = (uint8_t)hb;
    }
    __syncthreads();

    // 3. the clock over the step's masks: wave 0, uniform
    if (bits_row != nullptr && wave == 0)
    {
      for (uint32_t wd = 0; wd < valid / 32u; wd++)
      {
        const uint32_t hw = __builtin_amdgcn_readfirstlane(hm[wd]), cw = __builtin_amdgcn_readfirstlane(cm[wd]);
        const uint32_t tw = hw ^ ((hw << 1) | h_prev);     // bit b: the decision of sample b differs from the one before
        h_prev = hw >> 31;
        // unrolled: the common sample is a compare, an add and a bit test, with the two rare paths out of line
#pragma unroll
        for (uint32_t b = 0; b < 32u; b++)
        {
          const bool wrap = phi >= P.wrap_at;              // phi + baud_step carries (wrap_at = 2^32 - baud_step)
          phi += P.baud_step;
          if (__builtin_expect(wrap, 0))
          {
            const uint32_t h = (hw >> b) & 1u;
            if (tid == 0 && count < P.max_bits)            // (the law's bound, hrfd_afsk.h; a row's end is not staked on it)
            {
              bits_row[count] = (uint8_t)afsk_bit(h, last, P.nrzi != 0, (cw >> b) & 1u);
            }
            count++;
            last = P.nrzi != 0 ? h : last;
          }
          if (__builtin_expect((tw >> b) & 1u, 0))
          {
            phi = afsk_nudge(phi, P.A);
          }
        }
      }
    }
  }

  // 4. the state: the last 32 samples of the call, the phase, the call's last decision and the last sampled one.  Nothing
  // has written xs or the masks behind the last step's second barrier
  uint32_t *st_out = P.state_out + (uint64_t)c * kAfskStateDw;
  if (tid < (uint32_t)kAfskLeadDw)
  {
    st_out[tid] = xs[valid / 2u + tid];
  }
  if (tid == 0)
  {
    const uint32_t h_end = (hm[(valid - 1u) >> 5] >> ((valid - 1u) & 31u)) & 1u;
    st_out[kAfskHistSamples / 2] = phi;
    st_out[kAfskHistSamples / 2 + 1] = h_end | (last << 1);
    if (P.n_bits != nullptr)
    {
      P.n_bits[c] = count;
    }
  }
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_afsk
{
  hrfd::BankCore core;
  uint32_t n_channels = 0;

  // host settings, under core.mu: they travel in the kernel's arguments, so a setter has nothing to upload
  hrfd::AfskModem modem;
  uint64_t min_power = 0;
  uint2 taps[hrfd::kAfskMaxJ][hrfd::kAfskFilters];
  hrfd::BankHistory hist;                  // AfskState per channel as 18 dwords

  hrfd::PinnedBuf<uint8_t> h_stage;        // the fresh flags
  // host-path staging
  hrfd::DevBuf<int16_t> d_pcm;
  hrfd::DevBuf<uint32_t> d_n_pcm, d_n_bits;
  hrfd::DevBuf<uint8_t> d_bits, d_hard;
};

namespace hrfd {

// the modem's taps, packed for the kernel; under core.mu
static void afsk_pack(hrfd_afsk *a)
{
  int16_t taps[kAfskFilters * kAfskMaxWindow];
  afsk_taps(Q_DDC_COS, a->modem.mark_step, a->modem.space_step, a->modem.W, taps);
  memset(a->taps, 0, sizeof(a->taps));
  const int J = bank_packed_len((int)a->modem.W);
  std::vector<uint2> one(J);
  for (int f = 0; f < kAfskFilters; f++)
  {
    bank_pack_taps(taps + f * kAfskMaxWindow, (int)a->modem.W, one.data(), J);
    for (int j = 0; j < J; j++)
    {
      a->taps[j][f] = one[j];
    }
  }
}

} // namespace hrfd

extern "C" int hrfd_afsk_create(uint32_t n_channels, int device, hrfd_afsk **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(afsk_check_create("hrfd_afsk_create", n_channels, out));
  hrfd_afsk *a = nullptr;
  BANK_TRY(bank_new("hrfd_afsk_create", device, &a));
  const size_t C = n_channels;
  a->n_channels = n_channels;
  a->modem = AfskModem{kAfskDefaultMark, kAfskDefaultSpace, kAfskDefaultBaud, kAfskDefaultWindow, kAfskDefaultShift, 1u};
  afsk_pack(a);
  if (!(a->hist.alloc(C, kAfskStateDw) && a->h_stage.alloc(C)))
  {
    (void)hipGetLastError();
    bank_free(a);
    return fail(HRFD_ENOMEM, "hrfd_afsk_create: device allocation failed");
  }
  *out = a;
  return HRFD_OK;
}

extern "C" int hrfd_afsk_destroy(hrfd_afsk *a)
{
  if (a != nullptr)
  {
    hrfd::bank_free(a);
  }
  return HRFD_OK;
}

// every channel starts again: a history of another window length means nothing
extern "C" int hrfd_afsk_set_modem(hrfd_afsk *a, uint32_t mark_step, uint32_t space_step, uint32_t baud_step, uint32_t window,
                                   uint32_t loop_shift, int nrzi)
{
  using namespace hrfd;
  const AfskModem m{mark_step, space_step, baud_step, window, loop_shift, nrzi != 0 ? 1u : 0u};
  BANK_TRY(afsk_check_modem("hrfd_afsk_set_modem", m));
  BANK_TRY(bank_need_handle("hrfd_afsk_set_modem", a));
  std::lock_guard<std::mutex> g(a->core.mu);
  a->modem = m;
  afsk_pack(a);
  a->hist.mark(HRFD_ALL_CHANNELS);
  return HRFD_OK;
}

extern "C" int hrfd_afsk_set_carrier(hrfd_afsk *a, uint64_t min_power)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_afsk_set_carrier", a));
  std::lock_guard<std::mutex> g(a->core.mu);
  a->min_power = min_power;
  return HRFD_OK;
}

extern "C" int hrfd_afsk_reset(hrfd_afsk *a, uint32_t channel) { return hrfd::bank_reset_history(a, "hrfd_afsk_reset", channel); }

extern "C" int hrfd_afsk_max_bits(hrfd_afsk *a, uint32_t n_blocks, uint32_t *max_bits)
{
  using namespace hrfd;
  BANK_TRY(afsk_check_blocks("hrfd_afsk_max_bits", n_blocks));
  if (max_bits == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_afsk_max_bits: NULL result pointer");
  }
  BANK_TRY(bank_need_handle("hrfd_afsk_max_bits", a));
  std::lock_guard<std::mutex> g(a->core.mu);
  *max_bits = afsk_max_bits(a->modem.baud_step, a->modem.A, n_blocks);
  return HRFD_OK;
}

// bits_stride: looked at on the device entry where bits are asked for
static int afsk_check_process(hrfd_afsk *a, const char *who, const void *pcm, uint64_t stride, bool device_entry, const void *n_pcm,
                              uint32_t n_blocks, const void *bits, uint64_t bits_stride, const void *n_bits, const void *hard)
{
  using namespace hrfd;
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text: a row of bits
  // shorter than the slowest modem's is too short for every handle
  BANK_TRY(afsk_check_call(who, pcm, stride, device_entry, n_pcm, n_blocks, bits, n_bits, hard));
  const bool strided = device_entry && bits != nullptr;
  if (strided)
  {
    BANK_TRY(afsk_check_bits_stride(who, bits_stride, afsk_max_bits(1u, kAfskMaxShift, n_blocks), "the slowest modem"));
  }
  BANK_TRY(bank_need_handle(who, a));
  if (strided)
  {
    std::lock_guard<std::mutex> g(a->core.mu);
    BANK_TRY(afsk_check_bits_stride(who, bits_stride, afsk_max_bits(a->modem.baud_step, a->modem.A, n_blocks)));
  }
  return HRFD_OK;
}

// one call on `st`: the fresh flags, then k_afsk, one workgroup per channel
static int afsk_launch(hrfd_afsk *a, const int16_t *d_pcm, uint64_t stride, const uint32_t *d_n_pcm, uint32_t n_blocks, uint8_t *d_bits,
                       uint64_t bits_stride, uint32_t *d_n_bits, uint8_t *d_hard, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(a->core.order_behind_last(st));
  AfskParams P;
  {
    std::lock_guard<std::mutex> g(a->core.mu);
    // the modem of THIS launch decides how long a row may grow: a set_modem between the check and here must not let the
    // kernel write past a row
    P.max_bits = afsk_max_bits(a->modem.baud_step, a->modem.A, n_blocks);
    if (d_bits != nullptr && bits_stride < P.max_bits)
    {
      return fail(HRFD_EINVAL, "hrfd_afsk: the modem changed during the call and bits_stride_bytes %llu no longer holds a row",
                  (unsigned long long)bits_stride);
    }
    P.reset = a->hist.reset();
    P.state_in = a->hist.in();
    P.state_out = a->hist.out();
    a->hist.flip();
    if (a->hist.any_fresh)
    {
      BANK_TRY(a->core.staging_wait());
      BANK_TRY(a->hist.upload(a->h_stage, st));
      BANK_TRY(a->core.staging_sent(st));
    }
    P.min_power = a->min_power;
    P.W = a->modem.W;
    P.J = (uint32_t)bank_packed_len((int)a->modem.W);
    P.A = a->modem.A;
    P.baud_step = a->modem.baud_step;
    P.wrap_at = 0u - a->modem.baud_step;
    P.nrzi = a->modem.nrzi;
    memcpy(P.taps, a->taps, sizeof(P.taps));
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.n_pcm = d_n_pcm;
  P.n_blocks = n_blocks;
  P.bits = d_bits;
  P.bits_stride = bits_stride;
  P.n_bits = d_n_bits;
  P.hard = d_hard;
  hipLaunchKernelGGL(k_afsk, dim3(a->n_channels), dim3(kAfskThreads), 0, st, P);
  BANK_TRY(bank_launch_ok("k_afsk"));
  a->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_afsk_process_device(hrfd_afsk *a, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                                        uint32_t n_blocks, uint8_t *d_bits, uint64_t bits_stride_bytes, uint32_t *d_n_bits,
                                        uint8_t *d_hard, void *stream)
{
  BANK_TRY(afsk_check_process(a, "hrfd_afsk_process_device", d_pcm, channel_stride_bytes, true, d_n_pcm, n_blocks, d_bits,
                              bits_stride_bytes, d_n_bits, d_hard));
  HIP_TRY(hipSetDevice(a->core.device));
  return afsk_launch(a, d_pcm, channel_stride_bytes, d_n_pcm, n_blocks, d_bits, bits_stride_bytes, d_n_bits, d_hard,
                     a->core.stream_or_own(stream));
}

// bits: dense rows of hrfd_afsk_max_bits bytes.  They go up as well as down, so that the bytes of a row from n_bits on come
// back as they were
extern "C" int hrfd_afsk_process(hrfd_afsk *a, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, uint8_t *bits,
                                 uint32_t *n_bits, uint8_t *hard)
{
  using namespace hrfd;
  BANK_TRY(afsk_check_process(a, "hrfd_afsk_process", pcm, 0, false, n_pcm, n_blocks, bits, 0, n_bits, hard));
  uint32_t max_bits;
  {
    std::lock_guard<std::mutex> g(a->core.mu);
    max_bits = afsk_max_bits(a->modem.baud_step, a->modem.A, n_blocks);
  }
  BankHostCall call(a->core);
  const size_t C = a->n_channels, row = 2 * (size_t)kAfskBlock * n_blocks, H = (size_t)kAfskHardPerBlock * n_blocks;
  const int16_t *d_pcm = call.up(a->d_pcm, pcm, row * C);
  const uint32_t *d_n_pcm = call.up(a->d_n_pcm, n_pcm, 4 * C * n_blocks);
  uint8_t *d_bits = call.up(a->d_bits, bits, (size_t)max_bits * C);
  uint32_t *d_n_bits = call.room(a->d_n_bits, n_bits, 4 * C);
  uint8_t *d_hard = call.room(a->d_hard, hard, H * C);
  BANK_TRY(call.rc);
  BANK_TRY(afsk_launch(a, d_pcm, row, d_n_pcm, n_blocks, d_bits, max_bits, d_n_bits, d_hard, call.st));
  call.down(bits, d_bits, (size_t)max_bits * C);
  call.down(n_bits, d_n_bits, 4 * C);
  call.down(hard, d_hard, H * C);
  return call.finish();
}

// ---- read-only introspection (include/hrfd_debug.h): the laws of hrfd_afsk.h on the host, for tests/test_afsk_model.py
extern "C" int hrfd_afsk_debug_taps(uint32_t mark_step, uint32_t space_step, uint32_t window, int16_t *out128)
{
  using namespace hrfd;
  BANK_TRY(afsk_check_modem("hrfd_afsk_debug_taps", AfskModem{mark_step, space_step, 1u, window, kAfskMinShift, 0u}));
  if (out128 == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_afsk_debug_taps: NULL result pointer");
  }
  afsk_taps(Q_DDC_COS, mark_step, space_step, window, out128);
  return HRFD_OK;
}

extern "C" int hrfd_afsk_debug_slow(const uint32_t *modem6, uint64_t min_power, const int16_t *pcm, const uint32_t *n_pcm,
                                    uint32_t n_blocks, uint32_t *state18, uint8_t *bits, uint32_t *n_bits, uint8_t *hard)
{
  using namespace hrfd;
  if (modem6 == nullptr || state18 == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_afsk_debug_slow: NULL argument");
  }
  const AfskModem m{modem6[0], modem6[1], modem6[2], modem6[3], modem6[4], modem6[5] != 0 ? 1u : 0u};
  BANK_TRY(afsk_check_modem("hrfd_afsk_debug_slow", m));
  BANK_TRY(afsk_check_call("hrfd_afsk_debug_slow", pcm, 0, false, n_pcm, n_blocks, bits, n_bits, hard));
  int16_t taps[kAfskFilters * kAfskMaxWindow];
  afsk_taps(Q_DDC_COS, m.mark_step, m.space_step, m.W, taps);
  AfskState st;
  memcpy(&st, state18, sizeof(st));
  afsk_channel_slow(pcm, n_pcm, n_blocks, m, taps, min_power, &st, bits, n_bits, hard);
  memcpy(state18, &st, sizeof(st));
  return HRFD_OK;
}
