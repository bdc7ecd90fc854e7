// hackrfdiags_amd/csrc/hrfd_tone.hip -- hrfd_tone_*: a bank of tone detectors over the receive chain's PCM.
//
// PCM rows [C][n_blocks][512] int16 (and n_pcm) in; per frame of L samples the power at K tone frequencies, the frame's
// energy, its valid count and a verdict per tone group out.  Exact integer arithmetic, contract in include/hrfd.h;
// tests/tone_model.py restates it in numpy, hrfd_tone.h holds the per-sample law both sides of this file share.
//
// The phase is frame-local, so (c_k[n], s_k[n]) is the same for every channel and frame: k_tone_table writes it once per
// tone list as [K][L / 2] pairs of dwords ((c[2j], c[2j+1]), (s[2j], s[2j+1])), and the hot kernel is a dense integer
// product [frames][L] x [L][2K] whose reads are all consecutive.
//
// k_tone<FT>: one workgroup of 256 threads per FT consecutive frames (frames are numbered c F + f; FT L = 16384 samples,
// at most 16 frames).
//   1. every thread windows sample pairs of the tile into LDS as packed int16 (32 KiB): one dword load where the row is
//      4-byte aligned, two halfword loads where it is not; samples behind n_pcm are 0 whatever lies there
//   2. the waves share the frames: E by a dot2 of the dword with itself, valid from n_pcm alone
//   3. the waves share the tones: lanes along n, one table row dword pair per step, FT frames per loaded pair.  A table
//      entry is split into its high byte (arithmetic) and low byte, c = 256 ch + cl: a dot2 against two high bytes adds at
//      most 2 x 32767 x 128 = 2^23, against two low bytes 2 x 32767 x 255 < 2^24, and a lane takes L / 128 <= 64 steps, so
//      four int32 partial sums per frame cannot overflow and nothing is widened inside the loop.  I = 256 Ih + Il in
//      int64 per lane, then a wave reduction that halves the values with every step (FT values reach FT lane groups in
//      FT - 1 + log2(64 / FT) exchanges); one lane per frame rounds, squares and puts P into LDS
//   4. P, E, valid go out with consecutive stores, and one thread per (frame, group) gives the verdict
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "hrfd_tone.h"

namespace hrfd {

constexpr int kToneThreads = 256;
constexpr int kToneWaves = kToneThreads / 64;
constexpr int kToneTile = 16384;           // samples of one workgroup's frames
constexpr int kToneMaxFrames = 16;         // frames of one workgroup

typedef short tone_s2 __attribute__((ext_vector_type(2)));
// signed 16-bit dot product of two dwords plus acc, without clamping; device code only
#define TONE_DOT2(a, b, acc) \
  __builtin_amdgcn_sdot2(__builtin_bit_cast(hrfd::tone_s2, (a)), __builtin_bit_cast(hrfd::tone_s2, (b)), (acc), false)

struct ToneParams
{
  const int16_t *pcm;                      // [C] rows of n_blocks x 512 samples, stride bytes apart, even address
  uint64_t stride;
  const uint32_t *n_pcm;                   // [C][n_blocks] or NULL
  const uint32_t *window;                  // [L / 2] packed int16 pairs
  const uint2 *table;                      // [K][L / 2]
  uint64_t *power;                         // [G][K] or NULL
  uint64_t *energy;                        // [G] or NULL
  uint32_t *valid;                         // [G] or NULL
  uint8_t *best, *present;                 // [G][4] or NULL
  ToneThresholds th;
  uint8_t groups[kToneMaxTones];
  uint32_t L, K, n_blocks;
  uint32_t F;                              // frames per channel
  uint32_t G;                              // frames in all, C F <= 2^28
  uint32_t first_wg;                       // this launch's first workgroup
};

// [K][L / 2]: the cosines and sines of two consecutive samples of a frame; cs is the mixers' packed table
__global__ __launch_bounds__(kToneThreads) void k_tone_table(const uint32_t *cs, const uint32_t *steps, uint2 *table, uint32_t L,
                                                             uint32_t K)
{
  const uint32_t idx = blockIdx.x * kToneThreads + threadIdx.x, half = L / 2;
  if (idx >= K * half)
  {
    return;
  }
  const uint32_t k = idx / half, j = idx - k * half, step = steps[k];
  const uint32_t d0 = cs[tone_cos_index(step * (2 * j))], d1 = cs[tone_cos_index(step * (2 * j + 1))];
  table[idx] = make_uint2((d0 & 0xffffu) | (d1 << 16), (d0 >> 16) | (d1 & 0xffff0000u));
}

// N values per lane, N a power of two up to 64: every step with more than one value left keeps one half, sends the other
// to the lane `off` away and adds what comes back; the steps after that add whole values.  Lane l ends with the total of
// value l >> (6 - log2 N) in v[0].
template <int N>
__device__ __forceinline__ long long tone_reduce(long long (&v)[N], uint32_t lane)
{
  int n = N;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
  {
    if (n > 1)
    {
      const int h = n / 2;
      const bool up = (lane & (uint32_t)off) != 0;
#pragma unroll
      for (int i = 0; i < h; i++)
      {
        const long long keep = up ? v[i + h] : v[i], send = up ? v[i] : v[i + h];
        v[i] = keep + __shfl_xor(send, off);
      }
      n = h;
    }
    else
    {
      v[0] += __shfl_xor(v[0], off);
    }
  }
  return v[0];
}

constexpr int tone_log2(int v) { return v <= 1 ? 0 : 1 + tone_log2(v / 2); }

template <int FT>
__global__ __launch_bounds__(kToneThreads) void k_tone(const ToneParams P)
{
  __shared__ uint32_t u2[kToneTile / 2];
  __shared__ uint64_t pw[kToneMaxFrames * kToneMaxTones];
  __shared__ uint64_t en[kToneMaxFrames];
  __shared__ uint32_t va[kToneMaxFrames];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t L = P.L, half = L / 2, K = P.K, F = P.F, G = P.G;
  const uint64_t g0 = ((uint64_t)P.first_wg + blockIdx.x) * FT;

  // 1. the tile's samples, windowed
  for (uint32_t idx = tid; idx < FT * half; idx += kToneThreads)
  {
    const uint32_t f = idx / half, j = idx - f * half;
    const uint64_t g = g0 + f;
    uint32_t ud = 0;
    if (g < G)
    {
      const uint32_t c = (uint32_t)g / F, fr = (uint32_t)g - c * F;
      const uint32_t js = fr * L + 2 * j, pos = js & (kToneBlock - 1);
      const uint32_t lim = pcm_block_limit(P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * P.n_blocks : nullptr, js / kToneBlock);
      const int16_t *row = (const int16_t *)((const char *)P.pcm + (uint64_t)c * P.stride) + js;
      int32_t x0 = 0, x1 = 0;
      if (pos < lim)
      {
        if (((uintptr_t)row & 3u) == 0)
        {
          const uint32_t d = *(const uint32_t *)row;
          x0 = (int16_t)d;
          x1 = (int32_t)d >> 16;
        }
        else
        {
          x0 = row[0];
          x1 = row[1];
        }
        x1 = pos + 1 < lim ? x1 : 0;
      }
      const uint32_t wd = P.window[j];
      const int32_t u0 = tone_window(x0, (int16_t)wd), u1 = tone_window(x1, (int32_t)wd >> 16);
      ud = ((uint32_t)u0 & 0xffffu) | ((uint32_t)u1 << 16);
    }
    u2[idx] = ud;
  }
  __syncthreads();

  // 2. E and valid, a frame per wave
  for (uint32_t f = wv; f < FT; f += kToneWaves)
  {
    uint64_t e = 0;
    for (uint32_t j = lane; j < half; j += 64)
    {
      const uint32_t d = u2[f * half + j];
      e += (uint32_t)TONE_DOT2(d, d, 0);                   // 2 x 32767^2 < 2^31
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
    {
      e += __shfl_xor(e, o);
    }
    if (lane == 0)
    {
      const uint64_t g = g0 + f;
      uint32_t v = 0;
      if (g < G)
      {
        const uint32_t c = (uint32_t)g / F, fr = (uint32_t)g - c * F;
        v = tone_frame_valid(P.n_pcm != nullptr ? P.n_pcm + (uint64_t)c * P.n_blocks : nullptr, fr, L);
      }
      en[f] = e;
      va[f] = v;
    }
  }

  // 3. the tones, one per wave at a time
  for (uint32_t k = wv; k < K; k += kToneWaves)
  {
    const uint2 *row = P.table + (uint64_t)k * half;
    int ih[FT], il[FT], qh[FT], ql[FT];
#pragma unroll
    for (int f = 0; f < FT; f++)
    {
      ih[f] = il[f] = qh[f] = ql[f] = 0;
    }
    for (uint32_t j = lane; j < half; j += 64)
    {
      const uint2 t = row[j];
      const tone_s2 ch = __builtin_bit_cast(tone_s2, t.x) >> 8, sh = __builtin_bit_cast(tone_s2, t.y) >> 8;
      const uint32_t cl = t.x & 0x00ff00ffu, sl = t.y & 0x00ff00ffu;
#pragma unroll
      for (int f = 0; f < FT; f++)
      {
        const uint32_t d = u2[f * half + j];
        ih[f] = TONE_DOT2(d, ch, ih[f]);
        il[f] = TONE_DOT2(d, cl, il[f]);
        qh[f] = TONE_DOT2(d, sh, qh[f]);
        ql[f] = TONE_DOT2(d, sl, ql[f]);
      }
    }
    long long I[FT], Q[FT];
#pragma unroll
    for (int f = 0; f < FT; f++)
    {
      I[f] = (long long)ih[f] * 256 + il[f];
      Q[f] = (long long)qh[f] * 256 + ql[f];
    }
    const long long Ir = tone_reduce<FT>(I, lane), Qr = tone_reduce<FT>(Q, lane);
    constexpr uint32_t kShift = 6 - tone_log2(FT);
    if ((lane & ((1u << kShift) - 1u)) == 0)
    {
      pw[(lane >> kShift) * K + k] = tone_power(Ir, Qr);
    }
  }
  __syncthreads();

  // 4. the results of the frames that exist
  const uint32_t frames = (uint32_t)(G - g0 < (uint64_t)FT ? G - g0 : (uint64_t)FT);
  if (P.power != nullptr)
  {
    for (uint32_t idx = tid; idx < frames * K; idx += kToneThreads)
    {
      P.power[g0 * K + idx] = pw[idx];
    }
  }
  if (tid < frames)
  {
    if (P.energy != nullptr)
    {
      P.energy[g0 + tid] = en[tid];
    }
    if (P.valid != nullptr)
    {
      P.valid[g0 + tid] = va[tid];
    }
  }
  if (tid < frames * kToneGroups && (P.best != nullptr || P.present != nullptr))
  {
    const uint32_t f = tid / kToneGroups, grp = tid % kToneGroups;
    const uint32_t bi = tone_best(&pw[f * K], P.groups, K, grp);
    if (P.best != nullptr)
    {
      P.best[g0 * kToneGroups + tid] = (uint8_t)bi;
    }
    if (P.present != nullptr)
    {
      P.present[g0 * kToneGroups + tid] =
          bi != kToneNoBest && tone_present(va[f], L, en[f], P.th.min_energy[grp], pw[f * K + bi], P.th.ratio_q8[grp]) ? 1 : 0;
    }
  }
}

template __global__ void k_tone<16>(const ToneParams);
template __global__ void k_tone<8>(const ToneParams);
template __global__ void k_tone<4>(const ToneParams);
template __global__ void k_tone<2>(const ToneParams);

} // namespace hrfd

// ------------------------------------------------------------------ host side
struct hrfd_tone
{
  hrfd::BankCore core;
  uint32_t n_channels = 0;
  uint32_t L = 0;

  // host settings, under core.mu
  std::vector<uint32_t> steps;
  std::vector<uint8_t> groups;
  std::vector<int16_t> window;
  hrfd::ToneThresholds th;
  bool tones_dirty = false, window_dirty = true;

  hrfd::PinnedBuf<uint8_t> h_stage;        // the window's 2 L bytes, then 128 steps
  hrfd::DevBuf<uint32_t> d_cs;             // the mixers' table
  hrfd::DevBuf<uint32_t> d_window;         // [L / 2]
  hrfd::DevBuf<uint32_t> d_steps;          // [128]
  hrfd::DevBuf<uint2> d_table;             // [128][L / 2]

  // host-path staging
  hrfd::DevBuf<int16_t> d_pcm;
  hrfd::DevBuf<uint32_t> d_n_pcm;
  hrfd::DevBuf<uint64_t> d_power, d_energy;
  hrfd::DevBuf<uint32_t> d_valid;
  hrfd::DevBuf<uint8_t> d_best, d_present;
};

static void tone_default_window(uint32_t L, std::vector<int16_t> &w)
{
  w.resize(L);
  for (uint32_t n = 0; n < L; n++)
  {
    w[n] = (int16_t)lround(32767.0 * 0.5 * (1.0 - cos(2.0 * M_PI * (double)n / (double)L)));
  }
}

extern "C" int hrfd_tone_create(uint32_t n_channels, uint32_t frame_len, int device, hrfd_tone **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  BANK_TRY(tone_check_create("hrfd_tone_create", n_channels, frame_len, out));
  hrfd_tone *t = nullptr;
  BANK_TRY(bank_new("hrfd_tone_create", device, &t));
  t->n_channels = n_channels;
  t->L = frame_len;
  tone_default_window(frame_len, t->window);
  for (uint32_t g = 0; g < kToneGroups; g++)
  {
    t->th.ratio_q8[g] = 16u * frame_len;
    t->th.min_energy[g] = 256ull * frame_len;
  }
  if (!(bank_upload_cos(t->d_cs) && t->d_window.alloc(frame_len / 2) && t->d_steps.alloc(kToneMaxTones) &&
        t->d_table.alloc((size_t)kToneMaxTones * (frame_len / 2)) && t->h_stage.alloc(2 * (size_t)frame_len + 4 * kToneMaxTones)))
  {
    (void)hipGetLastError();
    bank_free(t);
    return fail(HRFD_ENOMEM, "hrfd_tone_create: device allocation failed");
  }
  *out = t;
  return HRFD_OK;
}

extern "C" int hrfd_tone_destroy(hrfd_tone *t)
{
  if (t != nullptr)
  {
    hrfd::bank_free(t);
  }
  return HRFD_OK;
}

extern "C" int hrfd_tone_set_tones(hrfd_tone *t, const uint32_t *steps, const uint8_t *groups, uint32_t n_tones)
{
  BANK_TRY(hrfd::tone_check_tones("hrfd_tone_set_tones", steps, groups, n_tones));
  BANK_TRY(hrfd::bank_need_handle("hrfd_tone_set_tones", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  t->steps.assign(steps, steps + n_tones);
  if (groups != nullptr)
  {
    t->groups.assign(groups, groups + n_tones);
  }
  else
  {
    t->groups.assign(n_tones, 0);
  }
  t->tones_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_tone_n_tones(hrfd_tone *t, uint32_t *n_tones)
{
  if (t == nullptr || n_tones == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_tone_n_tones: NULL handle or result");
  }
  std::lock_guard<std::mutex> g(t->core.mu);
  *n_tones = (uint32_t)t->steps.size();
  return HRFD_OK;
}

extern "C" int hrfd_tone_set_window(hrfd_tone *t, const int16_t *w)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_tone_set_window", t));
  BANK_TRY(hrfd::tone_check_window("hrfd_tone_set_window", w, t->L));
  std::lock_guard<std::mutex> g(t->core.mu);
  if (w == nullptr)
  {
    tone_default_window(t->L, t->window);
  }
  else
  {
    t->window.assign(w, w + t->L);
  }
  t->window_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_tone_set_threshold(hrfd_tone *t, uint32_t group, uint32_t ratio_q8, uint64_t min_energy)
{
  BANK_TRY(hrfd::tone_check_threshold("hrfd_tone_set_threshold", group, ratio_q8, min_energy));
  BANK_TRY(hrfd::bank_need_handle("hrfd_tone_set_threshold", t));
  std::lock_guard<std::mutex> g(t->core.mu);
  hrfd::bank_each_selected(hrfd::kToneGroups, group, [&](uint32_t i) {
    t->th.ratio_q8[i] = ratio_q8;
    t->th.min_energy[i] = min_energy;
  });
  return HRFD_OK;
}

// test hook: the workgroups of one launch of k_tone, 1 .. 2^22 (2^22 unless set)
extern "C" int hrfd_tone_debug_set_max_wgs(hrfd_tone *t, uint32_t n)
{
  HRFD_HOOK_GATE("hrfd_tone_debug_set_max_wgs");
  return hrfd::bank_set_max_wgs("hrfd_tone_debug_set_max_wgs", t, n);
}

// the checks of both process entries; the tone count is read under the lock again at the launch
static int tone_check_process(hrfd_tone *t, const char *who, const void *pcm, uint64_t stride, bool device_entry, uint32_t n_blocks,
                              const void *power, const void *energy, const void *valid, const void *best, const void *present)
{
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text
  BANK_TRY(hrfd::tone_check_call(who, pcm, stride, device_entry, n_blocks, power, energy, valid, best, present));
  BANK_TRY(hrfd::bank_need_handle(who, t));
  std::lock_guard<std::mutex> g(t->core.mu);
  return hrfd::tone_check_frames(who, t->L, n_blocks, (uint32_t)t->steps.size());
}

// one call on `st`: what the setters changed, the table if the tones changed, then k_tone over every frame
static int tone_launch(hrfd_tone *t, const int16_t *d_pcm, uint64_t stride, const uint32_t *d_n_pcm, uint32_t n_blocks,
                       uint64_t *d_power, uint64_t *d_energy, uint32_t *d_valid, uint8_t *d_best,
                       uint8_t *d_present, hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(t->core.order_behind_last(st));
  ToneParams P;
  const uint32_t L = t->L;
  {
    std::lock_guard<std::mutex> g(t->core.mu);
    P.K = (uint32_t)t->steps.size();
    memset(P.groups, 0, sizeof(P.groups));
    memcpy(P.groups, t->groups.data(), P.K);
    P.th = t->th;
    if (t->window_dirty || t->tones_dirty)
    {
      BANK_TRY(t->core.staging_wait());
      if (t->window_dirty)
      {
        memcpy(t->h_stage, t->window.data(), 2 * (size_t)L);
        HIP_TRY(hipMemcpyAsync(t->d_window, t->h_stage, 2 * (size_t)L, hipMemcpyHostToDevice, st));
      }
      if (t->tones_dirty)
      {
        memcpy(t->h_stage + 2 * (size_t)L, t->steps.data(), 4 * (size_t)P.K);
        HIP_TRY(hipMemcpyAsync(t->d_steps, t->h_stage + 2 * (size_t)L, 4 * (size_t)P.K, hipMemcpyHostToDevice, st));
        const uint32_t entries = P.K * (L / 2);
        hipLaunchKernelGGL(k_tone_table, dim3((entries + kToneThreads - 1) / kToneThreads), dim3(kToneThreads), 0, st, t->d_cs.p,
                           t->d_steps.p, t->d_table.p, L, P.K);
        BANK_TRY(bank_launch_ok("k_tone_table"));
      }
      t->window_dirty = t->tones_dirty = false;
      BANK_TRY(t->core.staging_sent(st));
    }
  }
  P.pcm = d_pcm;
  P.stride = stride;
  P.n_pcm = d_n_pcm;
  P.window = t->d_window;
  P.table = t->d_table;
  P.power = d_power;
  P.energy = d_energy;
  P.valid = d_valid;
  P.best = d_best;
  P.present = d_present;
  P.L = L;
  P.n_blocks = n_blocks;
  P.F = kToneBlock * n_blocks / L;
  P.G = t->n_channels * P.F;
  const uint32_t FT = std::min((uint32_t)kToneMaxFrames, (uint32_t)kToneTile / L);
  BANK_TRY(bank_launch_chunked("k_tone", t->core, (P.G + FT - 1) / FT, P, [&](dim3 grid) {
    const dim3 block(kToneThreads);
    switch (FT)
    {
    case 16: hipLaunchKernelGGL(k_tone<16>, grid, block, 0, st, P); break;
    case 8: hipLaunchKernelGGL(k_tone<8>, grid, block, 0, st, P); break;
    case 4: hipLaunchKernelGGL(k_tone<4>, grid, block, 0, st, P); break;
    default: hipLaunchKernelGGL(k_tone<2>, grid, block, 0, st, P); break;
    }
  }));
  t->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_tone_process_device(hrfd_tone *t, const int16_t *d_pcm, uint64_t channel_stride_bytes, const uint32_t *d_n_pcm,
                                        uint32_t n_blocks, uint64_t *d_power, uint64_t *d_energy, uint32_t *d_valid,
                                        uint8_t *d_best, uint8_t *d_present, void *stream)
{
  BANK_TRY(tone_check_process(t, "hrfd_tone_process_device", d_pcm, channel_stride_bytes, true, n_blocks, d_power, d_energy, d_valid,
                              d_best, d_present));
  HIP_TRY(hipSetDevice(t->core.device));
  return tone_launch(t, d_pcm, channel_stride_bytes, d_n_pcm, n_blocks, d_power,
                     d_energy, d_valid, d_best, d_present, t->core.stream_or_own(stream));
}

extern "C" int hrfd_tone_process(hrfd_tone *t, const int16_t *pcm, const uint32_t *n_pcm, uint32_t n_blocks, uint64_t *power,
                                 uint64_t *energy, uint32_t *valid, uint8_t *best, uint8_t *present)
{
  using namespace hrfd;
  BANK_TRY(tone_check_process(t, "hrfd_tone_process", pcm, 0, false, n_blocks, power, energy, valid, best, present));
  BankHostCall call(t->core);
  uint32_t K;
  {
    std::lock_guard<std::mutex> g(t->core.mu);
    K = (uint32_t)t->steps.size();
  }
  const size_t C = t->n_channels, G = C * (kToneBlock * n_blocks / t->L);
  const size_t row = 2 * (size_t)kToneBlock * n_blocks;
  const int16_t *d_pcm = call.up(t->d_pcm, pcm, row * C);
  const uint32_t *d_n_pcm = call.up(t->d_n_pcm, n_pcm, 4 * C * n_blocks);
  uint64_t *d_power = call.room(t->d_power, power, 8 * G * K), *d_energy = call.room(t->d_energy, energy, 8 * G);
  uint32_t *d_valid = call.room(t->d_valid, valid, 4 * G);
  uint8_t *d_best = call.room(t->d_best, best, kToneGroups * G), *d_present = call.room(t->d_present, present, kToneGroups * G);
  BANK_TRY(call.rc);
  BANK_TRY(tone_launch(t, d_pcm, row, d_n_pcm, n_blocks, d_power, d_energy, d_valid, d_best, d_present, call.st));
  call.down(power, d_power, 8 * G * K);
  call.down(energy, d_energy, 8 * G);
  call.down(valid, d_valid, 4 * G);
  call.down(best, d_best, kToneGroups * G);
  call.down(present, d_present, kToneGroups * G);
  return call.finish();
}
