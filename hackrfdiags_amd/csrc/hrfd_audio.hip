// hackrfdiags_amd/csrc/hrfd_audio.hip -- hrfd_audio_*: voice filter, gate and monitor mixes over the receive chain's PCM.
//
// PCM rows [C][n_blocks][512] int16 (and n_pcm, and a gate per block) in; the filtered, gated audio of every channel and
// the sums of M buses out.  Exact integer arithmetic, contract in include/hrfd.h; tests/audio_model.py restates it in
// numpy, hrfd_audio.h holds the laws both sides of this file share.
//
// k_audio_fir: one workgroup of 256 threads per (channel, run of kAudioRun = 4 blocks), 8 consecutive outputs per lane.
//   1. the run's samples and the 512 in front of them go into LDS as packed int16 pairs, zero behind each block's n_pcm:
//      the block in front of the run under its own n_pcm, or the handle's history (the side of the ping-pong this call
//      reads) in front of block 0.  The history is kept 512 samples deep whatever T is: a block is 512 samples, so the new
//      history is the last block as the filter saw it, and the workgroup of the last run writes it to the other side
//   2. output n sums the T time-reversed taps from sample n - T + 1 on.  Every lane's first output is even, so the parity
//      of its window's start is that of T - 1 for the whole launch: the taps are packed for both parities like the bank
//      core's (bank_pack_taps), and the samples are laid into LDS at an offset of 0..3 dwords chosen so that every lane's
//      window starts on a 16-byte boundary.  A step takes 8 tap dwords: three ds_read_b128 (lanes 16 bytes apart: no bank
//      conflict) give the 12 sample dwords 8 outputs x 8 tap dwords need, the taps come through the scalar cache, and the
//      64 v_dot2_i32_i16 of the step read nothing else.  The tap list is padded with zeros to whole steps.
//      |acc| <= sum |h| x 32768 <= 65535 x 32768 < 2^31 - 2^14: int32 is exact at every partial sum, and for the rounding
//      constant on top
//   3. y = sat16((acc + 2^13) >> 14), the envelope of the block's gate against the gate of the block before, z = the
//      product; 16 bytes per lane go out as dwords where the row is 4-byte aligned, as halfwords where it is not
// k_audio_mix: one workgroup per (bus, block), a sample pair per thread, the bus's list entry by entry (a dword each: the
//   channel below, the gain above; uniform, so it comes through the scalar cache).  The sums are 64-bit: a term is one
//   v_mad_i64_i32, the same instruction count a split into 32-bit partial sums would need, and the kernel waits for the
//   rows of z anyway.  The samples whose saturation changed them are counted per wave, then per workgroup through LDS: one
//   atomic add per workgroup that has any.
// k_audio_gate: one thread per (channel, block) turns the tone bank's verdicts into the gate.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrfd_audio.h"

namespace hrfd {

constexpr int kAudioThreads = 256;
constexpr int kAudioRun = 4;                               // blocks of one workgroup
constexpr int kAudioPer = 8;                               // consecutive outputs of one lane
constexpr int kAudioStep = 8;                              // tap dwords of one step
constexpr int kAudioHistDw = kAudioBlock / 2;              // 256 dwords of history
constexpr int kAudioXsDw = 4 + (kAudioRun + 1) * kAudioHistDw + 12;      // offset, history, run, what the last step reads over
constexpr int kAudioMaxJ = (kAudioMaxTaps / 2 + 1 + kAudioStep - 1) / kAudioStep * kAudioStep;      // 264
static_assert(kAudioRun * kAudioBlock == kAudioThreads * kAudioPer, "one pass of the workgroup covers the run");

typedef uint32_t audio_u4 __attribute__((ext_vector_type(4)));      // 16 bytes of LDS in one read

struct AudioFirParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address
  uint64_t stride;
  const uint32_t *n_pcm;                   // [C][n_blocks] or NULL
  const uint8_t *open;                     // [C][n_blocks] or NULL
  const uint32_t *hist_in;                 // [C][256] packed pairs
  uint32_t *hist_out;
  const uint8_t *prev_in;                  // [C]
  uint8_t *prev_out;
  const uint8_t *reset;                    // [C]: non-zero = this channel starts from zeros; or NULL
  int16_t *out;                            // [C] rows, out_stride bytes apart, even address
  uint64_t out_stride;
  uint32_t n_blocks, runs;                 // runs per channel
  uint32_t T, J;
  uint32_t n_wgs, first_wg;
};

// 8 outputs of one lane: J tap pairs in steps of 8 against a window that moves 8 dwords a step; PAR: the parity of the
// first output's window start.  Output i starts in dword (PAR + i) >> 1 of the window, on its odd half for (PAR + i) & 1.
template <int PAR>
__device__ __forceinline__ void audio_fir_run(const audio_u4 *win, const uint2 *__restrict__ taps, uint32_t J, int (&acc)[kAudioPer])
{
  for (uint32_t jb = 0; jb < J; jb += kAudioStep)
  {
    audio_u4 w0 = win[jb / 4], w1 = win[jb / 4 + 1], w2 = win[jb / 4 + 2];
    asm volatile("" : "+v"(w0), "+v"(w1), "+v"(w2));         // three whole ds_read_b128: no split into narrower reads
    const uint32_t w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
#pragma unroll
    for (int k = 0; k < kAudioStep; k++)
    {
      const uint2 t = taps[jb + k];
#pragma unroll
      for (int i = 0; i < kAudioPer; i++)
      {
        acc[i] = dot2(w[((PAR + i) >> 1) + k], ((PAR + i) & 1) ? t.y : t.x, acc[i]);
      }
    }
  }
}

// taps: [P.J] (even, odd) pairs, J a multiple of kAudioStep; a parameter of its own so that it can be __restrict__: the
// loads are then known not to alias the kernel's stores and go through the scalar cache
__global__ __launch_bounds__(kAudioThreads) void k_audio_fir(const AudioFirParams P, const uint2 *__restrict__ taps)
{
  __shared__ audio_u4 xs4[(kAudioXsDw + 3) / 4];
  uint32_t *xs = (uint32_t *)xs4;
  const uint32_t tid = threadIdx.x;
  const uint32_t wg = P.first_wg + blockIdx.x;
  const uint32_t c = wg / P.runs, b0 = (wg - c * P.runs) * kAudioRun;
  const uint32_t nb = min((uint32_t)kAudioRun, P.n_blocks - b0);
  const uint32_t par = (P.T - 1) & 1u, lead = (kAudioBlock + 1 - P.T - par) / 2, pad = (4u - (lead & 3u)) & 3u;
  const uint32_t *n_row = P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * P.n_blocks : nullptr;
  const bool fresh = P.reset != nullptr && P.reset[c] != 0;

  // 1. the samples: dword idx holds samples 2 idx - 512 and 2 idx - 511 of the run
  for (uint32_t idx = tid; idx < (uint32_t)kAudioXsDw - pad; idx += kAudioThreads)
  {
    const uint32_t blk = idx / kAudioHistDw, j = idx - blk * kAudioHistDw;
    uint32_t d = 0;
    if (blk == 0 && b0 == 0)
    {
      d = fresh ? 0u : P.hist_in[(uint64_t)c * kAudioHistDw + j];
    }
    else if (blk <= nb)
    {
      const uint32_t sb = b0 + blk - 1, lim = pcm_block_limit(n_row, sb), pos = 2 * j;
      if (pos < lim)
      {
        const int16_t *src = (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride) + (uint64_t)sb * kAudioBlock + pos;
        if (((uintptr_t)src & 3u) == 0)
        {
          d = *(const uint32_t *)src;
        }
        else
        {
          d = (uint32_t)(uint16_t)src[0] | ((uint32_t)(uint16_t)src[1] << 16);
        }
        d = pos + 1 < lim ? d : (d & 0xffffu);
      }
    }
    xs[pad + idx] = d;
  }
  __syncthreads();

  // the last run leaves the handle's next history and gate
  if (b0 + nb == P.n_blocks)
  {
    P.hist_out[(uint64_t)c * kAudioHistDw + tid] = xs[pad + nb * kAudioHistDw + tid];
    if (tid == 0)
    {
      P.prev_out[c] = P.open == nullptr || P.open[(uint64_t)c * P.n_blocks + P.n_blocks - 1] != 0 ? 1 : 0;
    }
  }

  // 2. the filter
  const uint32_t o = tid * kAudioPer;                      // the lane's first output, counted from the run's start
  if (o >= nb * kAudioBlock)
  {
    return;
  }
  int acc[kAudioPer];
#pragma unroll
  for (int i = 0; i < kAudioPer; i++)
  {
    acc[i] = 0;
  }
  const audio_u4 *win = xs4 + (pad + lead + o / 2) / 4;         // 16-byte aligned by the choice of pad
  if (par)
  {
    audio_fir_run<1>(win, taps, P.J, acc);
  }
  else
  {
    audio_fir_run<0>(win, taps, P.J, acc);
  }

  // 3. rounding, gate, store
  const uint32_t blk = o / kAudioBlock, n0 = o - blk * kAudioBlock, b = b0 + blk;
  const uint8_t *open_row = P.open != nullptr ? P.open + (uint64_t)c * P.n_blocks : nullptr;
  const bool q = open_row == nullptr || open_row[b] != 0;
  const bool p = b > 0 ? (open_row == nullptr || open_row[b - 1] != 0) : (!fresh && P.prev_in[c] != 0);
  uint32_t zd[kAudioPer / 2];
#pragma unroll
  for (int i = 0; i < kAudioPer; i += 2)
  {
    const int32_t z0 = audio_gate(pcm_fir_round(acc[i]), audio_envelope(p, q, n0 + i));
    const int32_t z1 = audio_gate(pcm_fir_round(acc[i + 1]), audio_envelope(p, q, n0 + i + 1));
    zd[i / 2] = ((uint32_t)z0 & 0xffffu) | ((uint32_t)z1 << 16);
  }
  int16_t *dst = (int16_t *)((char *)P.out + (uint64_t)c * P.out_stride) + (uint64_t)b0 * kAudioBlock + o;
  if (((uintptr_t)dst & 3u) == 0)
  {
#pragma unroll
    for (int i = 0; i < kAudioPer / 2; i++)
    {
      ((uint32_t *)dst)[i] = zd[i];
    }
  }
  else
  {
#pragma unroll
    for (int i = 0; i < kAudioPer / 2; i++)
    {
      dst[2 * i] = (int16_t)zd[i];
      dst[2 * i + 1] = (int16_t)(zd[i] >> 16);
    }
  }
}

struct AudioMixParams
{
  const int16_t *z;                        // [C] rows, z_stride bytes apart, even address
  uint64_t z_stride;
  const uint32_t *list;                    // [M][kAudioMaxList] entries
  const uint32_t *n_list;                  // [M]
  int16_t *mix;                            // [M][n_blocks][512] at an even address, or NULL
  uint32_t *clips;                         // [M], zeroed in front of the launch, or NULL
  uint32_t n_blocks;
};

__global__ __launch_bounds__(kAudioThreads) void k_audio_mix(const AudioMixParams P)
{
  __shared__ uint32_t wave_clips[kAudioThreads / 64];
  const uint32_t tid = threadIdx.x, b = blockIdx.x, m = blockIdx.y;
  const uint32_t N = P.n_list[m];
  const uint32_t *list = P.list + (uint64_t)m * kAudioMaxList;
  const uint64_t at = ((uint64_t)b * kAudioBlock + 2 * tid) * sizeof(int16_t);
  int64_t s0 = 0, s1 = 0;
  for (uint32_t j = 0; j < N; j++)
  {
    const uint32_t e = list[j];
    const int32_t g = audio_entry_gain(e);
    const int16_t *src = (const int16_t *)((const char *)P.z + (uint64_t)audio_entry_channel(e) * P.z_stride + at);
    int32_t z0, z1;
    if (((uintptr_t)src & 3u) == 0)
    {
      const uint32_t d = *(const uint32_t *)src;
      z0 = (int16_t)d;
      z1 = (int32_t)d >> 16;
    }
    else
    {
      z0 = src[0];
      z1 = src[1];
    }
    s0 += (int64_t)g * z0;
    s1 += (int64_t)g * z1;
  }
  bool c0, c1;
  const int32_t m0 = audio_mix_round(s0, &c0), m1 = audio_mix_round(s1, &c1);
  if (P.mix != nullptr)
  {
    int16_t *dst = (int16_t *)((char *)P.mix + ((uint64_t)m * P.n_blocks * kAudioBlock) * sizeof(int16_t) + at);
    if (((uintptr_t)dst & 3u) == 0)
    {
      *(uint32_t *)dst = ((uint32_t)m0 & 0xffffu) | ((uint32_t)m1 << 16);
    }
    else
    {
      dst[0] = (int16_t)m0;
      dst[1] = (int16_t)m1;
    }
  }
  if (P.clips != nullptr)
  {
    uint32_t n = (c0 ? 1u : 0u) + (c1 ? 1u : 0u);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
      n += __shfl_xor(n, off);
    }
    if ((tid & 63u) == 0)
    {
      wave_clips[tid >> 6] = n;
    }
    __syncthreads();
    if (tid == 0)
    {
      uint32_t total = 0;
#pragma unroll
      for (int w = 0; w < kAudioThreads / 64; w++)
      {
        total += wave_clips[w];
      }
      if (total != 0)
      {
        atomicAdd(P.clips + m, total);
      }
    }
  }
}

// open[c][b] from the tone bank's best / present [C][F][4]
__global__ __launch_bounds__(kAudioThreads) void k_audio_gate(const uint8_t *best, const uint8_t *present, const uint8_t *want,
                                                              uint32_t L, uint32_t group, uint32_t n_blocks, uint32_t n_channels,
                                                              uint8_t *open)
{
  const uint32_t idx = blockIdx.x * kAudioThreads + threadIdx.x;
  if (idx >= n_channels * n_blocks)
  {
    return;
  }
  const uint32_t c = idx / n_blocks, b = idx - c * n_blocks;
  const uint64_t row = (uint64_t)c * (kAudioBlock * n_blocks / L) * kAudioGroups;
  open[idx] = audio_block_open(best + row, present + row, L, group, want[c], b) ? 1 : 0;
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
static_assert(hrfd::kAudioHistDw == hrfd::BankHistory::kDw, "k_audio_fir reads and writes the core's history rows");

struct hrfd_audio
{
  hrfd::BankCore core;
  uint32_t n_channels = 0, n_buses = 0;

  // host settings, under core.mu
  std::vector<int16_t> taps;
  std::vector<std::vector<uint32_t>> bus;  // packed entries
  std::vector<uint8_t> bus_dirty;
  std::vector<uint8_t> want;               // per channel
  bool taps_dirty = true, want_dirty = true, any_bus_dirty = true;
  hrfd::BankHistory hist;                  // the filter's; d_prev follows its sides

  // pinned staging: taps, list lengths, want, fresh flags, lists
  hrfd::PinnedBuf<uint8_t> h_stage;
  size_t off_n = 0, off_want = 0, off_fresh = 0, off_list = 0;
  hrfd::DevBuf<uint2> d_taps;              // [kAudioMaxJ]
  hrfd::DevBuf<uint8_t> d_prev;            // [2][C]: the gate of the block before
  hrfd::DevBuf<uint8_t> d_want;            // [C]
  hrfd::DevBuf<uint32_t> d_list;           // [M][kAudioMaxList]
  hrfd::DevBuf<uint32_t> d_n_list;         // [M]
  hrfd::DevBuf<int16_t> d_z;               // z of a call without d_out

  // host-path staging
  hrfd::DevBuf<int16_t> d_pcm, d_out, d_mix;
  hrfd::DevBuf<uint32_t> d_n_pcm, d_clips;
  hrfd::DevBuf<uint8_t> d_open, d_best, d_present;
};

extern "C" int hrfd_audio_create(uint32_t n_channels, uint32_t n_buses, int device, hrfd_audio **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(audio_check_create("hrfd_audio_create", n_channels, n_buses, out));
  hrfd_audio *a = nullptr;
  BANK_TRY(bank_new("hrfd_audio_create", device, &a));
  const size_t C = n_channels, M = n_buses;
  a->n_channels = n_channels;
  a->n_buses = n_buses;
  a->taps.assign(1, (int16_t)16384);
  a->bus.resize(M);
  a->bus_dirty.assign(M, 1);
  a->want.assign(C, (uint8_t)kAudioNoTone);
  a->off_n = sizeof(uint2) * kAudioMaxJ;
  a->off_want = a->off_n + 4 * M;
  a->off_fresh = a->off_want + C;
  a->off_list = (a->off_fresh + C + 15) / 16 * 16;
  if (!(a->d_taps.alloc(kAudioMaxJ) && a->hist.alloc(C) && a->d_prev.alloc(2 * C) && a->d_want.alloc(C) &&
        a->d_list.alloc(M * kAudioMaxList) && a->d_n_list.alloc(M) && a->h_stage.alloc(a->off_list + 4 * M * kAudioMaxList) &&
        hipMemset(a->d_prev, 0, 2 * C) == hipSuccess))
  {
    (void)hipGetLastError();
    bank_free(a);
    return fail(HRFD_ENOMEM, "hrfd_audio_create: device allocation failed");
  }
  *out = a;
  return HRFD_OK;
}

extern "C" int hrfd_audio_destroy(hrfd_audio *a)
{
  if (a != nullptr)
  {
    hrfd::bank_free(a);
  }
  return HRFD_OK;
}

extern "C" int hrfd_audio_set_taps(hrfd_audio *a, const int16_t *taps, uint32_t n)
{
  BANK_TRY(hrfd::audio_check_taps("hrfd_audio_set_taps", taps, n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_audio_set_taps", a));
  std::lock_guard<std::mutex> g(a->core.mu);
  a->taps.assign(taps, taps + n);
  a->taps_dirty = true;
  a->hist.mark(HRFD_ALL_CHANNELS);
  return HRFD_OK;
}

extern "C" int hrfd_audio_set_bus(hrfd_audio *a, uint32_t bus, const uint32_t *channels, const int16_t *gains, uint32_t n)
{
  using namespace hrfd;
  BANK_TRY(audio_check_bus("hrfd_audio_set_bus", bus, channels, gains, n, 65536, kAudioMaxBuses));
  BANK_TRY(hrfd::bank_need_handle("hrfd_audio_set_bus", a));
  BANK_TRY(audio_check_bus("hrfd_audio_set_bus", bus, channels, gains, n, a->n_channels, a->n_buses));
  std::lock_guard<std::mutex> g(a->core.mu);
  a->bus[bus].resize(n);
  for (uint32_t j = 0; j < n; j++)
  {
    a->bus[bus][j] = audio_pack_entry(channels[j], gains[j]);
  }
  a->bus_dirty[bus] = 1;
  a->any_bus_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_audio_set_want(hrfd_audio *a, uint32_t channel, uint32_t want)
{
  BANK_TRY(hrfd::audio_check_want("hrfd_audio_set_want", channel, want, 65536));
  BANK_TRY(hrfd::bank_need_handle("hrfd_audio_set_want", a));
  BANK_TRY(hrfd::audio_check_want("hrfd_audio_set_want", channel, want, a->n_channels));
  std::lock_guard<std::mutex> g(a->core.mu);
  hrfd::bank_each_selected(a->n_channels, channel, [&](uint32_t c) { a->want[c] = (uint8_t)want; });
  a->want_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_audio_reset(hrfd_audio *a, uint32_t channel) { return hrfd::bank_reset_history(a, "hrfd_audio_reset", channel); }

// test hook: the workgroups of one launch of k_audio_fir, 1 .. 2^22 (2^22 unless set)
extern "C" int hrfd_audio_debug_set_max_wgs(hrfd_audio *a, uint32_t n)
{
  HRFD_HOOK_GATE("hrfd_audio_debug_set_max_wgs");
  return hrfd::bank_set_max_wgs("hrfd_audio_debug_set_max_wgs", a, n);
}

// the wanted tones, if a setter changed them; under core.mu, between staging_wait and staging_sent
static int audio_send_want(hrfd_audio *a, hipStream_t st)
{
  if (a->want_dirty)
  {
    memcpy(a->h_stage + a->off_want, a->want.data(), a->n_channels);
    HIP_TRY(hipMemcpyAsync(a->d_want, a->h_stage + a->off_want, a->n_channels, hipMemcpyHostToDevice, st));
    a->want_dirty = false;
  }
  return HRFD_OK;
}

static int audio_gate_launch(hrfd_audio *a, const uint8_t *d_best, const uint8_t *d_present, uint32_t L, uint32_t group,
                             uint32_t n_blocks, uint8_t *d_open, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(a->core.order_behind_last(st));
  {
    std::lock_guard<std::mutex> g(a->core.mu);
    if (a->want_dirty)
    {
      BANK_TRY(a->core.staging_wait());
      BANK_TRY(audio_send_want(a, st));
      BANK_TRY(a->core.staging_sent(st));
    }
  }
  const uint32_t n = a->n_channels * n_blocks;             // <= 2^26
  hipLaunchKernelGGL(k_audio_gate, dim3((n + kAudioThreads - 1) / kAudioThreads), dim3(kAudioThreads), 0, st, d_best, d_present,
                     a->d_want.p, L, group, n_blocks, a->n_channels, d_open);
  BANK_TRY(bank_launch_ok("k_audio_gate"));
  a->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_audio_gate_device(hrfd_audio *a, const uint8_t *d_best, const uint8_t *d_present, uint32_t frame_len,
                                      uint32_t group, uint32_t n_blocks, uint8_t *d_open, void *stream)
{
  BANK_TRY(hrfd::audio_check_gate("hrfd_audio_gate_device", d_best, d_present, frame_len, group, n_blocks, d_open));
  BANK_TRY(hrfd::bank_need_handle("hrfd_audio_gate_device", a));
  HIP_TRY(hipSetDevice(a->core.device));
  return audio_gate_launch(a, d_best, d_present, frame_len, group, n_blocks, d_open, a->core.stream_or_own(stream));
}

extern "C" int hrfd_audio_gate(hrfd_audio *a, const uint8_t *best, const uint8_t *present, uint32_t frame_len, uint32_t group,
                               uint32_t n_blocks, uint8_t *open)
{
  using namespace hrfd;
  BANK_TRY(audio_check_gate("hrfd_audio_gate", best, present, frame_len, group, n_blocks, open));
  BANK_TRY(hrfd::bank_need_handle("hrfd_audio_gate", a));
  BankHostCall call(a->core);
  const size_t C = a->n_channels, V = C * (kAudioBlock * n_blocks / frame_len) * kAudioGroups;
  const uint8_t *d_best = call.up(a->d_best, best, V), *d_present = call.up(a->d_present, present, V);
  uint8_t *d_open = call.room(a->d_open, open, C * n_blocks);
  BANK_TRY(call.rc);
  BANK_TRY(audio_gate_launch(a, d_best, d_present, frame_len, group, n_blocks, d_open, call.st));
  call.down(open, d_open, C * n_blocks);
  return call.finish();
}

static int audio_check_process(hrfd_audio *a, const char *who, const void *pcm, uint64_t stride, bool device_entry, uint32_t n_blocks,
                               const void *out, uint64_t out_stride, const void *mix, const void *clips)
{
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text
  BANK_TRY(hrfd::audio_check_call(who, pcm, stride, device_entry, n_blocks, out, out_stride, mix, clips, 1));
  BANK_TRY(hrfd::bank_need_handle(who, a));
  return hrfd::audio_check_call(who, pcm, stride, device_entry, n_blocks, out, out_stride, mix, clips, a->n_channels);
}

// one call on `st`: what the setters changed, k_audio_fir over every run, k_audio_mix over every (bus, block)
static int audio_launch(hrfd_audio *a, const int16_t *d_pcm, uint64_t stride, const uint32_t *d_n_pcm, const uint8_t *d_open,
                        uint32_t n_blocks, int16_t *d_out, uint64_t out_stride, int16_t *d_mix, uint32_t *d_clips, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(a->core.order_behind_last(st));
  const size_t C = a->n_channels, M = a->n_buses;
  if (d_out == nullptr)
  {
    out_stride = 2ull * kAudioBlock * n_blocks;
    BANK_TRY(a->d_z.grow_bytes(C * out_stride));
    d_out = a->d_z;
  }
  AudioFirParams P;
  {
    std::lock_guard<std::mutex> g(a->core.mu);
    P.T = (uint32_t)a->taps.size();
    P.J = ((uint32_t)bank_packed_len((int)P.T) + kAudioStep - 1) / kAudioStep * kAudioStep;
    P.reset = a->hist.reset();
    P.hist_in = a->hist.in();
    P.hist_out = a->hist.out();
    P.prev_in = a->d_prev + a->hist.side * C;
    P.prev_out = a->d_prev + (a->hist.side ^ 1u) * C;
    a->hist.flip();
    if (a->taps_dirty || a->want_dirty || a->any_bus_dirty || a->hist.any_fresh)
    {
      BANK_TRY(a->core.staging_wait());
      if (a->taps_dirty)
      {
        bank_pack_taps(a->taps.data(), (int)P.T, (uint2 *)a->h_stage.p, (int)P.J);
        HIP_TRY(hipMemcpyAsync(a->d_taps, a->h_stage, sizeof(uint2) * P.J, hipMemcpyHostToDevice, st));
      }
      BANK_TRY(audio_send_want(a, st));
      BANK_TRY(a->hist.upload(a->h_stage + a->off_fresh, st));
      if (a->any_bus_dirty)
      {
        uint32_t *n_list = (uint32_t *)(a->h_stage + a->off_n);
        for (size_t m = 0; m < M; m++)
        {
          n_list[m] = (uint32_t)a->bus[m].size();
          if (a->bus_dirty[m] && n_list[m] != 0)
          {
            uint8_t *src = a->h_stage + a->off_list + 4 * m * kAudioMaxList;
            memcpy(src, a->bus[m].data(), 4 * (size_t)n_list[m]);
            HIP_TRY(hipMemcpyAsync(a->d_list + m * kAudioMaxList, src, 4 * (size_t)n_list[m], hipMemcpyHostToDevice, st));
          }
          a->bus_dirty[m] = 0;
        }
        HIP_TRY(hipMemcpyAsync(a->d_n_list, n_list, 4 * M, hipMemcpyHostToDevice, st));
      }
      a->taps_dirty = a->any_bus_dirty = false;
      BANK_TRY(a->core.staging_sent(st));
    }
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.n_pcm = d_n_pcm;
  P.open = d_open;
  P.out = d_out;
  P.out_stride = out_stride;
  P.n_blocks = n_blocks;
  P.runs = (n_blocks + kAudioRun - 1) / kAudioRun;
  P.n_wgs = a->n_channels * P.runs;                        // <= 2^24
  BANK_TRY(bank_launch_chunked("k_audio_fir", a->core, P.n_wgs, P, [&](dim3 grid) {
    hipLaunchKernelGGL(k_audio_fir, grid, dim3(kAudioThreads), 0, st, P, (const uint2 *)a->d_taps.p);
  }));
  if (d_mix != nullptr || d_clips != nullptr)
  {
    if (d_clips != nullptr)
    {
      HIP_TRY(hipMemsetAsync(d_clips, 0, 4 * M, st));
    }
    AudioMixParams Q;
    Q.z = d_out;
    Q.z_stride = out_stride;
    Q.list = a->d_list;
    Q.n_list = a->d_n_list;
    Q.mix = d_mix;
    Q.clips = d_clips;
    Q.n_blocks = n_blocks;
    hipLaunchKernelGGL(k_audio_mix, dim3(n_blocks, a->n_buses), dim3(kAudioThreads), 0, st, Q);
    BANK_TRY(bank_launch_ok("k_audio_mix"));
  }
  a->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_audio_process_device(hrfd_audio *a, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                                         const uint8_t *d_open, uint32_t n_blocks, int16_t *d_out, uint64_t out_stride_bytes,
                                         int16_t *d_mix, uint32_t *d_clips, void *stream)
{
  BANK_TRY(audio_check_process(a, "hrfd_audio_process_device", d_pcm, channel_stride_bytes, true, n_blocks, d_out, out_stride_bytes,
                               d_mix, d_clips));
  HIP_TRY(hipSetDevice(a->core.device));
  return audio_launch(a, d_pcm, channel_stride_bytes, d_n_pcm, d_open, n_blocks, d_out, out_stride_bytes, d_mix, d_clips,
                      a->core.stream_or_own(stream));
}

extern "C" int hrfd_audio_process(hrfd_audio *a, const int16_t *pcm, const uint32_t *n_pcm, const uint8_t *open, uint32_t n_blocks,
                                  int16_t *out, int16_t *mix, uint32_t *clips)
{
  using namespace hrfd;
  BANK_TRY(audio_check_process(a, "hrfd_audio_process", pcm, 0, false, n_blocks, out, 0, mix, clips));
  BankHostCall call(a->core);
  const size_t C = a->n_channels, M = a->n_buses, row = 2 * (size_t)kAudioBlock * n_blocks;
  const int16_t *d_pcm = call.up(a->d_pcm, pcm, row * C);
  const uint32_t *d_n_pcm = call.up(a->d_n_pcm, n_pcm, 4 * C * n_blocks);
  const uint8_t *d_open = call.up(a->d_open, open, C * n_blocks);
  int16_t *d_out = call.room(a->d_out, out, row * C), *d_mix = call.room(a->d_mix, mix, row * M);
  uint32_t *d_clips = call.room(a->d_clips, clips, 4 * M);
  BANK_TRY(call.rc);
  BANK_TRY(audio_launch(a, d_pcm, row, d_n_pcm, d_open, n_blocks, d_out, row, d_mix, d_clips, call.st));
  call.down(out, d_out, row * C);
  call.down(mix, d_mix, row * M);
  call.down(clips, d_clips, 4 * M);
  return call.finish();
}
