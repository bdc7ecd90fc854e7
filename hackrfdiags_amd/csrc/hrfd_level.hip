// hackrfdiags_amd/csrc/hrfd_level.hip -- hrfd_level_*: per-channel automatic gain control over the receive chain's PCM.
//
// PCM rows [C][n_blocks][512] int16 (and n_pcm) in; the levelled audio, the gain and the peak of every frame of 64 samples
// out.  Exact integer arithmetic, contract in include/hrfd.h; tests/level_model.py restates it in numpy, hrfd_level.h holds
// the laws both sides of this file share.
//
// k_level: ONE fused pass, one workgroup of 256 threads per channel, which walks its row in steps of kLevelStep = 2048
// samples (4 blocks, 32 frames): 8 consecutive samples per lane, 8 lanes per frame.
//   1. a lane loads its 16 bytes (the load of the next step is issued in front of the work on this one), zeroes what lies
//      behind the block's n_pcm, and takes max |x| in 32 bits (|-32768| = 32768); three xor-shuffles give the 8 lanes of a
//      frame its peak, which goes into a ring of 128 peaks in LDS: slot (f + 64) & 127 for frame f, frames -64 .. -1 from the
//      handle's history (the side of the ping-pong this call reads)
//   2. behind one barrier the 8 lanes of frame f compute E[f] and E[f-1] from the ring, 8 of the 64 weights each (the
//      weights lie in LDS, zero from W on: a zero weight gives 0, below every floor) and the same shuffles, then g[f] and
//      g[f-1]: two divisions per frame, none per sample, and no second barrier for a neighbour's gain.  g[f-1] of the call's
//      first frame comes out of the same code from the history peaks under this call's settings, as the contract asks
//   3. y = (x gs + 2^11) >> 12 with v_mad_i32_i24 (the bound: hrfd_level.h), 16 bytes per lane out.
//      The step s + 1 writes ring slots of frames f0 + 32 .. f0 + 63 = those of frames f0 - 96 .. f0 - 65, which step s
//      (frames f0 - 64 .. f0 + 31) does not read: one barrier per step is enough
//   4. behind the last step lanes 0..63 write the ring's newest 64 peaks to the other side of the history.
// In place: every sample is loaded once, by the lane that stores it, and a row is touched by its own workgroup only; so out
// at the input's own address and stride is correct, and any other overlap is refused.
// Rows at any even address and stride take one path: the 16 bytes of a lane go through a vector type of alignment 2, which
// the compiler lowers to what the target takes at such an address (on gfx950 one global_load_dwordx4 / global_store_dwordx4
// either way), so a lane reads exactly the samples it writes, which a shifted head-and-tail layout would give up.
// The grid is the channel count, at most 65536 workgroups: below kBankMaxWgs for every call the checks let through, so the
// launch is never cut (no first_wg, no max_wgs hook).  The price is that a row is walked by one workgroup: a call of few
// channels and many blocks does not fill the device (DESIGN.md 3.13 has the figures).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "hrfd_level.h"

namespace hrfd {

constexpr int kLevelThreads = 256;
constexpr int kLevelPer = 8;                               // consecutive samples of one lane: 16 bytes
constexpr int kLevelStep = kLevelThreads * kLevelPer;      // samples of one step
constexpr int kLevelStepFrames = kLevelStep / (int)kLevelFrame;      // 32
constexpr int kLevelRing = 128;                            // peaks in LDS
constexpr int kLevelHistDw = kLevelHist / 2;               // 32 dwords of history per channel
static_assert(kLevelFrame == 8 * kLevelPer, "eight lanes per frame");
static_assert(kLevelStep % kLevelBlock == 0, "a step is whole blocks");
static_assert(kLevelRing >= (int)kLevelHist + 2 * kLevelStepFrames && (kLevelRing & (kLevelRing - 1)) == 0,
              "the next step's peaks fall on slots this step does not read");
static_assert(65536u <= kBankMaxWgs, "one workgroup per channel is one launch");

struct LevelParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address
  uint64_t stride;
  const uint32_t *n_pcm;                   // [C][n_blocks] or NULL
  const uint16_t *hist_in;                 // [C][64] peaks, the newest last
  uint16_t *hist_out;
  const uint8_t *reset;                    // [C]: non-zero = this channel starts from zero peaks; or NULL
  const LevelSetting *set;                 // [C]
  int16_t *out;                            // [C] rows, out_stride bytes apart, even address; may be pcm itself; or NULL
  uint64_t out_stride;
  uint32_t *gain;                          // [C][8 n_blocks] or NULL
  uint16_t *peak;                          // [C][8 n_blocks] or NULL
  uint32_t n_blocks;
};

// a lane's eight samples: the type promises an even address only, and the compiler picks what the target takes there
// the maximum over the eight lanes of a frame (lanes 8 j .. 8 j + 7 of a wave)
__device__ __forceinline__ uint32_t level_max8(uint32_t v)
{
  v = max(v, (uint32_t)__shfl_xor((int)v, 1));
  v = max(v, (uint32_t)__shfl_xor((int)v, 2));
  return max(v, (uint32_t)__shfl_xor((int)v, 4));
}

// lane `sub` of a frame's eight: its share of rule 2 for frame f, the weights sub, sub + 8, ..
__device__ __forceinline__ uint32_t level_envelope_share(const uint32_t *ring, const uint32_t *wl, int32_t f, uint32_t sub)
{
  uint32_t e = 0;
#pragma unroll
  for (uint32_t k = sub; k < kLevelMaxWeights; k += 8)
  {
    e = max(e, level_weighted(ring[(uint32_t)(f - (int32_t)k + (int32_t)kLevelHist) & (kLevelRing - 1)], wl[k]));
  }
  return e;
}

// w: the handle's 64 weights, zero from W on; a parameter of its own so that it can be __restrict__
__global__ __launch_bounds__(kLevelThreads) void k_level(const LevelParams P, const uint16_t *__restrict__ w)
{
  __shared__ uint32_t ring[kLevelRing];
  __shared__ uint32_t wl[kLevelMaxWeights];
  const uint32_t tid = threadIdx.x, c = blockIdx.x;
  const uint32_t sub = tid & 7u, fr = tid >> 3;
  const int16_t *row = (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride);
  int16_t *orow = P.out != nullptr ? (int16_t *)((char *)P.out + (uint64_t)c * P.out_stride) : nullptr;
  const uint32_t *n_row = P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * P.n_blocks : nullptr;
  const bool fresh = P.reset != nullptr && P.reset[c] != 0;
  const LevelSetting set = P.set[c];
  const uint32_t target = level_word_target(set.word), floor = set.floor;
  const bool bypass = level_word_bypass(set.word);
  const uint32_t n = P.n_blocks * kLevelBlock, F = P.n_blocks * kLevelFramesPerBlock;

  if (tid < kLevelHist)
  {
    ring[tid] = fresh ? 0u : P.hist_in[(uint64_t)c * kLevelHist + tid];      // frame tid - 64 in slot tid
    wl[tid] = w[tid];
  }

  pcm_u4 next = {0u, 0u, 0u, 0u};
  if (tid * kLevelPer < n)
  {
    next = pcm_load8(row + tid * kLevelPer);
  }
  for (uint32_t s0 = 0; s0 < n; s0 += kLevelStep)
  {
    // 1. the samples and the frame's peak
    const uint32_t at = s0 + tid * kLevelPer;              // the lane's first sample
    const bool active = at < n;                            // n is whole blocks: a lane has all of its samples or none
    const pcm_u4 cur = next;
    if (at + kLevelStep < n)
    {
      next = pcm_load8(row + at + kLevelStep);
    }
    const uint32_t d[4] = {cur.x, cur.y, cur.z, cur.w};
    int32_t x[kLevelPer];
    uint32_t m = 0;
    const uint32_t pos = at % kLevelBlock, lim = active ? pcm_block_limit(n_row, at / kLevelBlock) : 0u;
#pragma unroll
    for (int i = 0; i < kLevelPer; i++)
    {
      const int32_t v = (i & 1) ? (int32_t)d[i / 2] >> 16 : (int32_t)(int16_t)d[i / 2];
      x[i] = pos + i < lim ? v : 0;
      m = max(m, level_abs(x[i]));
    }
    m = level_max8(m);
    const int32_t f = (int32_t)(s0 / kLevelFrame + fr);    // the lane's frame; behind the row's end in idle lanes
    if (sub == 0 && active)                                // (an idle lane's slot is that of frame f - 128 + 64: history)
    {
      ring[(uint32_t)(f + (int32_t)kLevelHist) & (kLevelRing - 1)] = m;
    }
    __syncthreads();

    // 2. the envelopes and gains of frame f and of the frame before it
    const uint32_t e = level_max8(level_envelope_share(ring, wl, f, sub));
    const uint32_t e_prev = level_max8(level_envelope_share(ring, wl, f - 1, sub));
    const uint32_t g = level_gain(target, max(e, floor)), g_prev = level_gain(target, max(e_prev, floor));
    if (!active)
    {
      continue;                                            // (no barrier behind this point)
    }
    if (sub == 0)
    {
      if (P.gain != nullptr)
      {
        P.gain[(uint64_t)c * F + (uint32_t)f] = g;
      }
      if (P.peak != nullptr)
      {
        P.peak[(uint64_t)c * F + (uint32_t)f] = (uint16_t)m;
      }
    }

    // 3. the output
    if (orow != nullptr)
    {
      uint32_t y[kLevelPer];
#pragma unroll
      for (int i = 0; i < kLevelPer; i++)
      {
        y[i] = (uint32_t)(bypass ? x[i] : level_output(x[i], level_sample_gain(g_prev, g, sub * kLevelPer + i)));
      }
      pcm_u4 v;
      v.x = (y[0] & 0xffffu) | (y[1] << 16);
      v.y = (y[2] & 0xffffu) | (y[3] << 16);
      v.z = (y[4] & 0xffffu) | (y[5] << 16);
      v.w = (y[6] & 0xffffu) | (y[7] << 16);
      pcm_store8(orow + at, v);
    }
  }

  // 4. the last 64 peaks: frames F - 64 .. F - 1
  __syncthreads();
  if (tid < kLevelHist)
  {
    P.hist_out[(uint64_t)c * kLevelHist + tid] = (uint16_t)ring[(F + tid) & (kLevelRing - 1)];
  }
}

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_level
{
  hrfd::BankCore core;
  uint32_t n_channels = 0;

  // host settings, under core.mu
  uint16_t w[hrfd::kLevelMaxWeights];      // zero from W on
  std::vector<hrfd::LevelSetting> set;     // per channel
  bool w_dirty = true, set_dirty = true;
  hrfd::BankHistory hist;                  // 64 peaks per channel as 32 dwords

  // pinned staging: the weights, the settings, the fresh flags
  hrfd::PinnedBuf<uint8_t> h_stage;
  size_t off_set = 0, off_fresh = 0;
  hrfd::DevBuf<uint16_t> d_w;              // [64]
  hrfd::DevBuf<hrfd::LevelSetting> d_set;  // [C]

  // host-path staging
  hrfd::DevBuf<int16_t> d_pcm, d_out;
  hrfd::DevBuf<uint32_t> d_n_pcm, d_gain;
  hrfd::DevBuf<uint16_t> d_peak;
};

extern "C" int hrfd_level_create(uint32_t n_channels, int device, hrfd_level **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(level_check_create("hrfd_level_create", n_channels, out));
  hrfd_level *l = nullptr;
  BANK_TRY(bank_new("hrfd_level_create", device, &l));
  const size_t C = n_channels;
  l->n_channels = n_channels;
  level_default_weights(l->w);
  l->set.assign(C, LevelSetting{level_pack_word(kLevelDefaultTarget, false), kLevelDefaultFloor});
  l->off_set = sizeof(l->w);
  l->off_fresh = l->off_set + sizeof(LevelSetting) * C;
  if (!(l->d_w.alloc(kLevelMaxWeights) && l->d_set.alloc(C) && l->hist.alloc(C, kLevelHistDw) && l->h_stage.alloc(l->off_fresh + C)))
  {
    (void)hipGetLastError();
    bank_free(l);
    return fail(HRFD_ENOMEM, "hrfd_level_create: device allocation failed");
  }
  *out = l;
  return HRFD_OK;
}

extern "C" int hrfd_level_destroy(hrfd_level *l)
{
  if (l != nullptr)
  {
    hrfd::bank_free(l);
  }
  return HRFD_OK;
}

// the peaks stay: they are facts about the signal, whatever table weighs them
extern "C" int hrfd_level_set_weights(hrfd_level *l, const uint16_t *w, uint32_t n)
{
  BANK_TRY(hrfd::level_check_weights("hrfd_level_set_weights", w, n));
  BANK_TRY(hrfd::bank_need_handle("hrfd_level_set_weights", l));
  std::lock_guard<std::mutex> g(l->core.mu);
  memset(l->w, 0, sizeof(l->w));
  memcpy(l->w, w, sizeof(uint16_t) * n);
  l->w_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_level_set(hrfd_level *l, uint32_t channel, uint32_t target, uint32_t floor)
{
  using namespace hrfd;
  BANK_TRY(level_check_set("hrfd_level_set", channel, target, floor, 65536));
  BANK_TRY(bank_need_handle("hrfd_level_set", l));
  BANK_TRY(level_check_set("hrfd_level_set", channel, target, floor, l->n_channels));
  std::lock_guard<std::mutex> g(l->core.mu);
  bank_each_selected(l->n_channels, channel, [&](uint32_t c) {
    l->set[c].word = level_pack_word(target, level_word_bypass(l->set[c].word));
    l->set[c].floor = floor;
  });
  l->set_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_level_set_bypass(hrfd_level *l, uint32_t channel, int on)
{
  using namespace hrfd;
  BANK_TRY(pcm_check_channel("hrfd_level_set_bypass", channel, 65536));
  BANK_TRY(bank_need_handle("hrfd_level_set_bypass", l));
  BANK_TRY(pcm_check_channel("hrfd_level_set_bypass", channel, l->n_channels));
  std::lock_guard<std::mutex> g(l->core.mu);
  bank_each_selected(l->n_channels, channel,
                     [&](uint32_t c) { l->set[c].word = level_pack_word(level_word_target(l->set[c].word), on != 0); });
  l->set_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_level_reset(hrfd_level *l, uint32_t channel) { return hrfd::bank_reset_history(l, "hrfd_level_reset", channel); }

static int level_check_process(hrfd_level *l, const char *who, const void *pcm, uint64_t stride, bool device_entry, const void *n_pcm,
                               uint32_t n_blocks, const void *out, uint64_t out_stride, const void *gain, const void *peak)
{
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text
  BANK_TRY(hrfd::level_check_call(who, pcm, stride, device_entry, n_pcm, n_blocks, out, out_stride, gain, peak, 1));
  BANK_TRY(hrfd::bank_need_handle(who, l));
  return hrfd::level_check_call(who, pcm, stride, device_entry, n_pcm, n_blocks, out, out_stride, gain, peak, l->n_channels);
}

// one call on `st`: what the setters changed, then k_level, one workgroup per channel
static int level_launch(hrfd_level *l, const int16_t *d_pcm, uint64_t stride, const uint32_t *d_n_pcm, uint32_t n_blocks,
                        int16_t *d_out, uint64_t out_stride, uint32_t *d_gain, uint16_t *d_peak, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(l->core.order_behind_last(st));
  const size_t C = l->n_channels;
  LevelParams P;
  {
    std::lock_guard<std::mutex> g(l->core.mu);
    P.reset = l->hist.reset();
    P.hist_in = (const uint16_t *)l->hist.in();
    P.hist_out = (uint16_t *)l->hist.out();
    l->hist.flip();
    if (l->w_dirty || l->set_dirty || l->hist.any_fresh)
    {
      BANK_TRY(l->core.staging_wait());
      if (l->w_dirty)
      {
        memcpy(l->h_stage, l->w, sizeof(l->w));
        HIP_TRY(hipMemcpyAsync(l->d_w, l->h_stage, sizeof(l->w), hipMemcpyHostToDevice, st));
      }
      if (l->set_dirty)
      {
        memcpy(l->h_stage + l->off_set, l->set.data(), sizeof(LevelSetting) * C);
        HIP_TRY(hipMemcpyAsync(l->d_set, l->h_stage + l->off_set, sizeof(LevelSetting) * C, hipMemcpyHostToDevice, st));
      }
      BANK_TRY(l->hist.upload(l->h_stage + l->off_fresh, st));
      l->w_dirty = l->set_dirty = false;
      BANK_TRY(l->core.staging_sent(st));
    }
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.n_pcm = d_n_pcm;
  P.set = l->d_set;
  P.out = d_out;
  P.out_stride = out_stride;
  P.gain = d_gain;
  P.peak = d_peak;
  P.n_blocks = n_blocks;
  hipLaunchKernelGGL(k_level, dim3(l->n_channels), dim3(kLevelThreads), 0, st, P, (const uint16_t *)l->d_w.p);
  BANK_TRY(bank_launch_ok("k_level"));
  l->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_level_process_device(hrfd_level *l, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                                         uint32_t n_blocks, int16_t *d_out, uint64_t out_stride_bytes, uint32_t *d_gain,
                                         uint16_t *d_peak, void *stream)
{
  BANK_TRY(level_check_process(l, "hrfd_level_process_device", d_pcm, channel_stride_bytes, true, d_n_pcm, n_blocks, d_out,
                               out_stride_bytes, d_gain, d_peak));
  HIP_TRY(hipSetDevice(l->core.device));
  return level_launch(l, d_pcm, channel_stride_bytes, d_n_pcm, n_blocks, d_out, out_stride_bytes, d_gain, d_peak,
                      l->core.stream_or_own(stream));
}

extern "C" int hrfd_level_process(hrfd_level *l, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, int16_t *out,
                                  uint32_t *gain, uint16_t *peak)
{
  using namespace hrfd;
  BANK_TRY(level_check_process(l, "hrfd_level_process", pcm, 0, false, n_pcm, n_blocks, out, 0, gain, peak));
  BankHostCall call(l->core);
  const size_t C = l->n_channels, row = 2 * (size_t)kLevelBlock * n_blocks, F = (size_t)kLevelFramesPerBlock * n_blocks;
  const int16_t *d_pcm = call.up(l->d_pcm, pcm, row * C);
  const uint32_t *d_n_pcm = call.up(l->d_n_pcm, n_pcm, 4 * C * n_blocks);
  int16_t *d_out = call.room(l->d_out, out, row * C);
  uint32_t *d_gain = call.room(l->d_gain, gain, 4 * F * C);
  uint16_t *d_peak = call.room(l->d_peak, peak, 2 * F * C);
  BANK_TRY(call.rc);
  BANK_TRY(level_launch(l, d_pcm, row, d_n_pcm, n_blocks, d_out, row, d_gain, d_peak, call.st));
  call.down(out, d_out, row * C);
  call.down(gain, d_gain, 4 * F * C);
  call.down(peak, d_peak, 2 * F * C);
  return call.finish();
}
