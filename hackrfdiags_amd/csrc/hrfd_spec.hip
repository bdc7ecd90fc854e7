// hackrfdiags_amd/csrc/hrfd_spec.hip -- hrfd_spec_*: a bank of windowed integer FFTs over wideband captures.
//
// W int8 IQ captures in, the power of every bin of an N = 2^L point transform summed over the call's frames out, plus the
// sums over K bands and their verdicts.  Exact integer arithmetic, contract in include/hrfd.h; tests/spec_model.py restates
// it in numpy.
//
// k_spec<L>: one workgroup of T = N / 8 threads (32 .. 1024) per (capture, contiguous share of the call's frames).  A frame's N
// (re, im) int16 pairs live in LDS as one dword each, at index i ^ ((i >> 3) & 31): with that swizzle every ds_read_b32 /
// ds_write_b32 of every pass puts the 32 lanes of a half wave on 32 different banks, for every L (the strides of the
// passes are N / 8, N / 64, ..., down to 1).  Per frame:
//   1. every lane reads 16 bytes (8 samples) of the capture and of the window, windows them and writes 8 dwords
//   2. passes of three stages each in registers: a lane holds the 8 points base + q S (q = 0..7; S = N / 8 in the first
//      pass, an eighth of that in the next), does the stages with h = 4 S, 2 S, S on them and writes them back in place;
//      the twiddles of a pass are a table of 7 S packed (c, s) pairs, consecutive in the lane's position inside S
//   3. the last pass (S = 1, the 1..3 stages that are left) keeps its results: p = re^2 + im^2 is added to the lane's
//      uint64 sums, which stay at the transform's bit-reversed positions for the whole call
// After the last frame the sums go to P[w][bitrev(i)]: a plain store when the capture has one workgroup, an atomic add into
// the zeroed row when it has several (integer sums: the order does not matter).  k_spec_bands then sums the bands over P.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace hrfd {

constexpr int kSpecMinL = 8, kSpecMaxL = 13;
constexpr int kSpecBandThreads = 256;

typedef short spec_s2 __attribute__((ext_vector_type(2)));

#if defined(__HIP_DEVICE_COMPILE__)
#define SPEC_DOT2(a, b, acc) __builtin_amdgcn_sdot2(__builtin_bit_cast(spec_s2, (a)), __builtin_bit_cast(spec_s2, (b)), (acc), false)
#else
#define SPEC_DOT2(a, b, acc)                                                                   \
  ((int)(int16_t)((a) & 0xffffu) * (int)(int16_t)((b) & 0xffffu) + (int)(int16_t)((a) >> 16) * (int)(int16_t)((b) >> 16) + (acc))
#endif

__host__ __device__ constexpr int spec_threads(int L) { return (1 << L) / 8; }
// the stages of the last pass: what three-stage passes leave over, 1..3
__host__ __device__ constexpr int spec_last_stages(int L) { return L - 3 * ((L - 1) / 3); }
__host__ __device__ constexpr int spec_swz(int i) { return i ^ ((i >> 3) & 31); }

// (x + y + 1) >> 1 and (x + y) >> 1 per int16 half, without the 17th bit: the sum is never formed
__host__ __device__ __forceinline__ spec_s2 spec_avg_up(spec_s2 x, spec_s2 y) { return (x | y) - ((x ^ y) >> (short)1); }
__host__ __device__ __forceinline__ spec_s2 spec_avg_down(spec_s2 x, spec_s2 y) { return (x & y) + ((x ^ y) >> (short)1); }

// one butterfly of stage t on packed (re, im), r = 1 in the even stages (up), 0 in the odd ones: a' = (a + b + r) >> 1,
// b' = ((a - b + r) >> 1) rotated by the twiddle t = (c, s).  With y = ~b = -b - 1: (a - b + 1) >> 1 = ((a + y) >> 1) + 1,
// (a - b) >> 1 = (a + y + 1) >> 1.
__host__ __device__ __forceinline__ void spec_bfly(uint32_t &a, uint32_t &b, uint32_t t, bool up)
{
  const spec_s2 x = __builtin_bit_cast(spec_s2, a), y = __builtin_bit_cast(spec_s2, b), ny = __builtin_bit_cast(spec_s2, ~b);
  const uint32_t d = __builtin_bit_cast(uint32_t, (spec_s2)(up ? spec_avg_down(x, ny) + (short)1 : spec_avg_up(x, ny)));
  a = __builtin_bit_cast(uint32_t, (spec_s2)(up ? spec_avg_up(x, y) : spec_avg_down(x, y)));
  const uint32_t nsc = ((0u - (t >> 16)) & 0xffffu) | (t << 16);             // (-s, c)
  const int re = SPEC_DOT2(d, t, 1 << 14) >> 15;                              // d_re c + d_im s
  const int im = SPEC_DOT2(d, nsc, 1 << 14) >> 15;                            // d_im c - d_re s
  b = ((uint32_t)re & 0xffffu) | ((uint32_t)im << 16);
}

// the stages with h = 4 S, 2 S, S (the last STAGES of them) on the 8 points z[q] = point base + q S; tw: the pass's table
// at the lane's position inside S (rows S dwords apart); t1: the index of the stage with h = S (it decides which stages
// round up)
template <int STAGES>
__host__ __device__ __forceinline__ void spec_radix8(uint32_t z[8], const uint32_t *tw, int S, int t1)
{
  const bool up1 = (t1 & 1) == 0;
  if (STAGES >= 3)
  {
#pragma unroll
    for (int q = 0; q < 4; q++)
    {
      spec_bfly(z[q], z[q + 4], tw[q * S], up1);
    }
  }
  if (STAGES >= 2)
  {
#pragma unroll
    for (int q = 0; q < 2; q++)
    {
      const uint32_t t = tw[(4 + q) * S];
      spec_bfly(z[q], z[q + 2], t, !up1);
      spec_bfly(z[q + 4], z[q + 6], t, !up1);
    }
  }
  const uint32_t t = tw[6 * S];
#pragma unroll
  for (int q = 0; q < 8; q += 2)
  {
    spec_bfly(z[q], z[q + 1], t, up1);
  }
}

// a three-stage pass (stages t0 .. t0 + 2) with stride S over the frame in `lds`, group g (0 .. N / 8 - 1), in place
__host__ __device__ __forceinline__ void spec_pass(uint32_t *lds, const uint32_t *tw_pass, int S, int g, int t0)
{
  const int gm = g & (S - 1);
  const int base = (g - gm) * 8 + gm;
  uint32_t z[8];
#pragma unroll
  for (int q = 0; q < 8; q++)
  {
    z[q] = lds[spec_swz(base + q * S)];
  }
  spec_radix8<3>(z, tw_pass + gm, S, t0 + 2);
#pragma unroll
  for (int q = 0; q < 8; q++)
  {
    lds[spec_swz(base + q * S)] = z[q];
  }
}

// the last pass over group g: points 8 g .. 8 g + 7, results stay in z
template <int L>
__host__ __device__ __forceinline__ void spec_last_pass(const uint32_t *lds, const uint32_t *tw_last, int g, uint32_t z[8])
{
#pragma unroll
  for (int q = 0; q < 8; q++)
  {
    z[q] = lds[spec_swz(8 * g + q)];
  }
  spec_radix8<spec_last_stages(L)>(z, tw_last, 1, L - 1);
}

// windows 8 samples (16 capture bytes in x, 8 int16 window entries in w) into the frame at 8 g .. 8 g + 7
__host__ __device__ __forceinline__ void spec_window8(uint32_t *lds, int g, const uint32_t x[4], const uint32_t w[4])
{
#pragma unroll
  for (int j = 0; j < 8; j++)
  {
    const uint32_t iq = x[j >> 1] >> (16 * (j & 1));
    const int wj = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
    const int re = ((int)(int8_t)iq * wj + 128) >> 8, im = ((int)(int8_t)(iq >> 8) * wj + 128) >> 8;
    lds[spec_swz(8 * g + j)] = ((uint32_t)re & 0xffffu) | ((uint32_t)im << 16);
  }
}

__host__ __device__ __forceinline__ uint32_t spec_bitrev(uint32_t i, int L)
{
  uint32_t r = 0;
  for (int b = 0; b < L; b++)
  {
    r |= ((i >> b) & 1u) << (L - 1 - b);
  }
  return r;
}

// dwords of the per-pass twiddle tables of a transform of 2^L points: 7 S for every pass, S = N / 8, N / 64, .., and S = 1
// for the last pass (which comes after the strides > 1, also when N / 8^k reaches 1 on its own)
__host__ __device__ constexpr int spec_tw_dwords(int L)
{
  int n = 7;
  for (int t = 0; L - t > 3; t += 3)
  {
    n += 7 * (1 << (L - t - 3));
  }
  return n;
}

struct SpecParams
{
  const int8_t *cap;            // [W] rows of 2 N n_frames bytes, cap_stride apart
  uint64_t cap_stride;
  const uint32_t *win;          // [N / 2] the window as packed int16 pairs
  const uint32_t *tw;           // [spec_tw_dwords(L)] packed (c, s), pass after pass
  unsigned long long *power;    // [W][N]
  uint32_t n_frames;
  uint32_t frames_per_wg;
  uint32_t wg_per_capture;
};

struct SpecBandDev
{
  uint32_t capture, first, n_bins, pad;
  unsigned long long threshold;
};

template <int L>
__global__ __launch_bounds__(spec_threads(L)) void k_spec(const SpecParams P)
{
  constexpr int N = 1 << L, T = spec_threads(L), NG = N / 8 / T, TW = spec_tw_dwords(L);
  __shared__ uint32_t frame[N];
  __shared__ uint32_t tw[TW];
  const int tid = threadIdx.x;
  const uint32_t w = blockIdx.x / P.wg_per_capture;
  const uint32_t f0 = (blockIdx.x - w * P.wg_per_capture) * P.frames_per_wg;
  const uint32_t f1 = min(P.n_frames, f0 + P.frames_per_wg);
  for (int i = tid; i < TW; i += T)
  {
    tw[i] = P.tw[i];
  }
  const int8_t *row = P.cap + (uint64_t)w * P.cap_stride;
  const bool aligned = ((uintptr_t)row & 15u) == 0;
  unsigned long long sum[NG][8];
#pragma unroll
  for (int j = 0; j < NG; j++)
  {
#pragma unroll
    for (int q = 0; q < 8; q++)
    {
      sum[j][q] = 0ull;
    }
  }
  for (uint32_t f = f0; f < f1; f++)
  {
    const int8_t *src = row + (uint64_t)f * (2u * N);
    __syncthreads();                                     // the last pass of the frame before has read, the tables are in
#pragma unroll
    for (int j = 0; j < NG; j++)
    {
      const int g = tid + j * T;
      uint32_t x[4];
      if (aligned)
      {
        const uint4 v = *(const uint4 *)(src + 16 * g);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      }
      else
      {
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
          const uint8_t *b = (const uint8_t *)src + 16 * g + 4 * k;
          x[k] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
      }
      const uint4 wv = *(const uint4 *)(P.win + 4 * g);
      const uint32_t ww[4] = {wv.x, wv.y, wv.z, wv.w};
      spec_window8(frame, g, x, ww);
    }
    int off = 0;
#pragma unroll
    for (int t = 0; L - t > 3; t += 3)
    {
      const int S = 1 << (L - t - 3);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < NG; j++)
      {
        spec_pass(frame, tw + off, S, tid + j * T, t);
      }
      off += 7 * S;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NG; j++)
    {
      uint32_t z[8];
      spec_last_pass<L>(frame, tw + off, tid + j * T, z);
#pragma unroll
      for (int q = 0; q < 8; q++)
      {
        sum[j][q] += (unsigned long long)(uint32_t)SPEC_DOT2(z[q], z[q], 0);
      }
    }
  }
  unsigned long long *out = P.power + (uint64_t)w * N;
#pragma unroll
  for (int j = 0; j < NG; j++)
  {
#pragma unroll
    for (int q = 0; q < 8; q++)
    {
      const uint32_t k = spec_bitrev((uint32_t)(8 * (tid + j * T) + q), L);
      if (P.wg_per_capture == 1)
      {
        out[k] = sum[j][q];
      }
      else
      {
        atomicAdd(out + k, sum[j][q]);
      }
    }
  }
}

template __global__ void k_spec<8>(const SpecParams);
template __global__ void k_spec<9>(const SpecParams);
template __global__ void k_spec<10>(const SpecParams);
template __global__ void k_spec<11>(const SpecParams);
template __global__ void k_spec<12>(const SpecParams);
template __global__ void k_spec<13>(const SpecParams);

// one workgroup per band: the sum of P[capture] over n_bins bins from `first`, modulo N, and the verdict
__global__ __launch_bounds__(kSpecBandThreads) void k_spec_bands(const unsigned long long *power, const SpecBandDev *bands,
                                                                 uint32_t N, uint32_t n_frames,
                                                                 unsigned long long *band_power, uint8_t *present)
{
  __shared__ unsigned long long part[kSpecBandThreads / 64];
  const SpecBandDev b = bands[blockIdx.x];
  const unsigned long long *row = power + (uint64_t)b.capture * N;
  unsigned long long s = 0ull;
  for (uint32_t i = threadIdx.x; i < b.n_bins; i += kSpecBandThreads)
  {
    s += row[(b.first + i) & (N - 1u)];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
  {
    s += __shfl_xor(s, o);
  }
  if ((threadIdx.x & 63) == 0)
  {
    part[threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    unsigned long long total = 0ull;
    for (int i = 0; i < kSpecBandThreads / 64; i++)
    {
      total += part[i];
    }
    band_power[blockIdx.x] = total;
    present[blockIdx.x] = total >= b.threshold * (unsigned long long)n_frames ? 1 : 0;
  }
}

// host tables: c, s for k = 0 .. N / 2 - 1 and the default window, in double
static void spec_cos_sin(int L, std::vector<int16_t> &c, std::vector<int16_t> &s)
{
  const int N = 1 << L;
  c.resize(N / 2);
  s.resize(N / 2);
  for (int k = 0; k < N / 2; k++)
  {
    const double a = 2.0 * M_PI * (double)k / (double)N;
    c[k] = (int16_t)lround(32767.0 * cos(a));
    s[k] = (int16_t)lround(32767.0 * sin(a));
  }
}

static void spec_hann(int L, std::vector<int16_t> &w)
{
  const int N = 1 << L;
  w.resize(N);
  for (int n = 0; n < N; n++)
  {
    w[n] = (int16_t)lround(32767.0 * 0.5 * (1.0 - cos(2.0 * M_PI * (double)n / (double)N)));
  }
}

// the per-pass tables k_spec reads: for a pass with stride S and a lane at position gm inside S, row r holds the
// twiddle of the pair's first point i = qq S + gm in a stage with half span h = hq S: index (i mod 2 h) (N / 2 h)
static void spec_pass_tables(int L, std::vector<uint32_t> &out)
{
  const int N = 1 << L;
  std::vector<int16_t> c, s;
  spec_cos_sin(L, c, s);
  out.clear();
  auto one_pass = [&](int S) {
    static const int hq_of[7] = {4, 4, 4, 4, 2, 2, 1}, qq_of[7] = {0, 1, 2, 3, 0, 1, 0};
    for (int r = 0; r < 7; r++)
    {
      for (int gm = 0; gm < S; gm++)
      {
        const int h = hq_of[r] * S;
        const int k = (qq_of[r] * S + gm) * (N / (2 * h));
        out.push_back((uint32_t)(uint16_t)c[k] | ((uint32_t)(uint16_t)s[k] << 16));
      }
    }
  };
  for (int t = 0; L - t > 3; t += 3)
  {
    one_pass(1 << (L - t - 3));
  }
  one_pass(1);
}

} // namespace hrfd

#ifndef HRFD_SPEC_KERNEL_ONLY
// named tables of the spectrum bank for hrfd_q15_table: "SPEC_HANN_<L>", "SPEC_COS_<L>", "SPEC_SIN_<L>"
static int spec_named_table(const char *name, int16_t *out, int cap)
{
  int kind = -1, L = 0;
  if (strncmp(name, "SPEC_HANN_", 10) == 0) { kind = 0; L = atoi(name + 10); }
  else if (strncmp(name, "SPEC_COS_", 9) == 0) { kind = 1; L = atoi(name + 9); }
  else if (strncmp(name, "SPEC_SIN_", 9) == 0) { kind = 2; L = atoi(name + 9); }
  if (kind < 0 || L < hrfd::kSpecMinL || L > hrfd::kSpecMaxL)
  {
    return 0;
  }
  std::vector<int16_t> a, b;
  if (kind == 0)
  {
    hrfd::spec_hann(L, a);
  }
  else
  {
    hrfd::spec_cos_sin(L, a, b);
    if (kind == 2) a.swap(b);
  }
  if (out != nullptr && cap > 0)
  {
    memcpy(out, a.data(), sizeof(int16_t) * (size_t)std::min(cap, (int)a.size()));
  }
  return (int)a.size();
}

// ------------------------------------------------------------------ host side
struct SpecBand
{
  uint32_t capture, first, n_bins;
  uint64_t threshold;
};

struct hrfd_spec
{
  hrfd::BankCore core;
  uint32_t n_captures = 0, R = 1;
  int L = 0;
  uint32_t N = 0;
  uint32_t target_wgs = 512;               // workgroups a launch aims for (two per CU fit beside each other)
  hrfd::PinnedBuf<uint32_t> h_stage_win;   // [N / 2]
  hrfd::PinnedBuf<hrfd::SpecBandDev> h_stage_bands;   // [cap_stage_bands]
  size_t cap_stage_bands = 0;

  // host records, under core.mu
  std::vector<int16_t> window;
  std::vector<SpecBand> bands;
  bool dirty_win = true, dirty_bands = true;

  hrfd::DevBuf<uint32_t> d_win, d_tw;
  hrfd::DevBuf<hrfd::SpecBandDev> d_bands;
  hrfd::DevBuf<int8_t> d_in;               // host-path staging
  hrfd::DevBuf<unsigned long long> d_power, d_band_power;
  hrfd::DevBuf<uint8_t> d_present;
};

extern "C" int hrfd_spec_create(uint32_t n_captures, uint32_t decimation, uint32_t log2_n, int device, hrfd_spec **out)
{
  using namespace hrfd;
  if (out != nullptr)
  {
    *out = nullptr;
  }
  if (out == nullptr || n_captures == 0 || n_captures > 65536)
  {
    return fail(HRFD_EINVAL, "hrfd_spec_create: need 1..65536 captures and a result pointer (got %u)", n_captures);
  }
  BANK_TRY(bank_rate_ok("hrfd_spec_create", "decimation", decimation));
  if (log2_n < (uint32_t)kSpecMinL || log2_n > (uint32_t)kSpecMaxL)
  {
    return fail(HRFD_EINVAL, "hrfd_spec_create: log2_n must be %d..%d (got %u)", kSpecMinL, kSpecMaxL, log2_n);
  }
  hrfd_spec *s = nullptr;
  BANK_TRY(bank_new("hrfd_spec_create", device, &s));
  s->n_captures = n_captures;
  s->R = decimation;
  s->L = (int)log2_n;
  s->N = 1u << log2_n;
  spec_hann(s->L, s->window);
  std::vector<uint32_t> tw;
  spec_pass_tables(s->L, tw);
  const bool ok = tw.size() == (size_t)spec_tw_dwords(s->L) && s->d_win.alloc(s->N / 2) && s->d_tw.alloc(tw.size()) &&
                  hipMemcpy(s->d_tw, tw.data(), sizeof(uint32_t) * tw.size(), hipMemcpyHostToDevice) == hipSuccess &&
                  s->h_stage_win.alloc(s->N / 2);
  if (!ok)
  {
    (void)hipGetLastError();
    bank_free(s);
    return fail(HRFD_ENOMEM, "hrfd_spec_create: device allocation failed");
  }
  *out = s;
  return HRFD_OK;
}

extern "C" int hrfd_spec_destroy(hrfd_spec *s)
{
  if (s != nullptr)
  {
    hrfd::bank_free(s);
  }
  return HRFD_OK;
}

extern "C" int hrfd_spec_set_window(hrfd_spec *s, const int16_t *w)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_spec_set_window", s));
  std::lock_guard<std::mutex> g(s->core.mu);
  if (w == nullptr)
  {
    hrfd::spec_hann(s->L, s->window);
  }
  else
  {
    s->window.assign(w, w + s->N);
  }
  s->dirty_win = true;
  return HRFD_OK;
}

extern "C" int hrfd_spec_set_band(hrfd_spec *s, uint32_t band, uint32_t capture, uint32_t first_bin, uint32_t n_bins,
                                  uint64_t threshold)
{
  if (threshold > HRFD_SPEC_MAX_THRESHOLD)
  {
    return fail(HRFD_EINVAL, "hrfd_spec_set_band: threshold above 2^44 (threshold * n_frames must stay inside uint64)");
  }
  if (s == nullptr || capture >= s->n_captures || first_bin >= s->N || n_bins == 0 || n_bins > s->N)
  {
    return fail(HRFD_EINVAL, "hrfd_spec_set_band: bad handle or capture, first_bin >= N, or n_bins not in 1..N");
  }
  std::lock_guard<std::mutex> g(s->core.mu);
  if (band > s->bands.size() || band >= HRFD_SPEC_MAX_BANDS)
  {
    return fail(HRFD_EINVAL, "hrfd_spec_set_band: band %u, the handle has %zu (band == K appends; at most %u)", band,
                s->bands.size(), HRFD_SPEC_MAX_BANDS);
  }
  const SpecBand b{capture, first_bin, n_bins, threshold};
  if (band == s->bands.size())
  {
    s->bands.push_back(b);
  }
  else
  {
    s->bands[band] = b;
  }
  s->dirty_bands = true;
  return HRFD_OK;
}

extern "C" int hrfd_spec_clear_bands(hrfd_spec *s)
{
  BANK_TRY(hrfd::bank_need_handle("hrfd_spec_clear_bands", s));
  std::lock_guard<std::mutex> g(s->core.mu);
  s->bands.clear();
  s->dirty_bands = true;
  return HRFD_OK;
}

extern "C" int hrfd_spec_n_bands(hrfd_spec *s, uint32_t *k)
{
  if (s == nullptr || k == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_spec_n_bands: NULL argument");
  }
  std::lock_guard<std::mutex> g(s->core.mu);
  *k = (uint32_t)s->bands.size();
  return HRFD_OK;
}

static int spec_check_call(hrfd_spec *s, const void *captures, uint64_t capture_stride, uint32_t n_frames, const void *power,
                           const void *band_power, const void *present, const char *who)
{
  if (s == nullptr || captures == nullptr || power == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL argument", who);
  }
  if (n_frames == 0 || n_frames > HRFD_SPEC_MAX_FRAMES)
  {
    return fail(HRFD_EINVAL, "%s: n_frames must be 1..%u (got %u)", who, HRFD_SPEC_MAX_FRAMES, n_frames);
  }
  if (capture_stride < 2ull * s->N * n_frames)
  {
    return fail(HRFD_EINVAL, "%s: capture_stride %llu is shorter than a row of %u frames", who,
                (unsigned long long)capture_stride, n_frames);
  }
  if (((uintptr_t)power & 7u) != 0 || ((uintptr_t)band_power & 7u) != 0)
  {
    return fail(HRFD_EINVAL, "%s: power and band_power must be 8-byte aligned", who);
  }
  bool need;
  {
    std::lock_guard<std::mutex> g(s->core.mu);
    need = !s->bands.empty();
  }
  if (need && (band_power == nullptr || present == nullptr))
  {
    return fail(HRFD_EINVAL, "%s: the handle has bands: band_power and present are needed", who);
  }
  return HRFD_OK;
}

// one call on `st`: uploads, k_spec<L> over every capture, k_spec_bands when the handle has bands
static int spec_launch(hrfd_spec *s, const int8_t *d_captures, uint64_t capture_stride, uint32_t n_frames,
                       unsigned long long *d_power, unsigned long long *d_band_power, uint8_t *d_present, uint32_t max_bands,
                       hipStream_t st)
{
  using namespace hrfd;
  BANK_TRY(s->core.order_behind_last(st));
  uint32_t K;
  {
    std::lock_guard<std::mutex> g(s->core.mu);
    K = std::min((uint32_t)s->bands.size(), max_bands);   // bands appended since the caller sized its outputs wait a call
    if (s->dirty_win || s->dirty_bands)
    {
      BANK_TRY(s->core.staging_wait());
      if (s->dirty_win)
      {
        memcpy(s->h_stage_win, s->window.data(), sizeof(int16_t) * s->N);
        HIP_TRY(hipMemcpyAsync(s->d_win, s->h_stage_win, sizeof(int16_t) * s->N, hipMemcpyHostToDevice, st));
        s->dirty_win = false;
      }
      if (s->dirty_bands && K > 0)
      {
        if (K > s->cap_stage_bands)
        {
          HIP_TRY(hipStreamSynchronize(s->core.last_stream));   // the last band kernel may still read the old table
          s->cap_stage_bands = 0;
          const size_t cap = std::max<size_t>(64, 2 * (size_t)K);
          if (!s->h_stage_bands.alloc(cap))
          {
            return fail(HRFD_ENODEV, "hrfd_spec: no pinned memory for %zu bands: %s", cap, hipGetErrorString(hipGetLastError()));
          }
          s->cap_stage_bands = cap;
          BANK_TRY(s->d_bands.grow_bytes(sizeof(SpecBandDev) * cap));
        }
        for (uint32_t b = 0; b < K; b++)
        {
          s->h_stage_bands.p[b] = SpecBandDev{s->bands[b].capture, s->bands[b].first, s->bands[b].n_bins, 0u,
                                            (unsigned long long)s->bands[b].threshold};
        }
        HIP_TRY(hipMemcpyAsync(s->d_bands, s->h_stage_bands, sizeof(SpecBandDev) * K, hipMemcpyHostToDevice, st));
      }
      s->dirty_bands = K < s->bands.size();
      BANK_TRY(s->core.staging_sent(st));
    }
  }
  SpecParams P;
  P.cap = d_captures;
  P.cap_stride = capture_stride;
  P.win = s->d_win;
  P.tw = s->d_tw;
  P.power = d_power;
  P.n_frames = n_frames;
  const uint32_t want = std::max(1u, s->target_wgs / s->n_captures);
  P.frames_per_wg = (n_frames + want - 1) / want;
  P.wg_per_capture = (n_frames + P.frames_per_wg - 1) / P.frames_per_wg;
  if (P.wg_per_capture > 1)
  {
    HIP_TRY(hipMemsetAsync(d_power, 0, sizeof(unsigned long long) * (size_t)s->n_captures * s->N, st));
  }
  const dim3 grid(s->n_captures * P.wg_per_capture);
  switch (s->L)
  {
  case 8: hipLaunchKernelGGL(k_spec<8>, grid, dim3(spec_threads(8)), 0, st, P); break;
  case 9: hipLaunchKernelGGL(k_spec<9>, grid, dim3(spec_threads(9)), 0, st, P); break;
  case 10: hipLaunchKernelGGL(k_spec<10>, grid, dim3(spec_threads(10)), 0, st, P); break;
  case 11: hipLaunchKernelGGL(k_spec<11>, grid, dim3(spec_threads(11)), 0, st, P); break;
  case 12: hipLaunchKernelGGL(k_spec<12>, grid, dim3(spec_threads(12)), 0, st, P); break;
  default: hipLaunchKernelGGL(k_spec<13>, grid, dim3(spec_threads(13)), 0, st, P); break;
  }
  BANK_TRY(bank_launch_ok("k_spec"));
  if (K > 0)
  {
    hipLaunchKernelGGL(k_spec_bands, dim3(K), dim3(kSpecBandThreads), 0, st, d_power, s->d_bands, s->N, n_frames, d_band_power,
                       d_present);
    BANK_TRY(bank_launch_ok("k_spec"));
  }
  s->core.launched_on(st);
  return HRFD_OK;
}

extern "C" int hrfd_spec_process_device(hrfd_spec *s, const int8_t *d_captures, uint64_t capture_stride, uint32_t n_frames,
                                        uint64_t *d_power, uint64_t *d_band_power, uint8_t *d_present, void *stream)
{
  BANK_TRY(spec_check_call(s, d_captures, capture_stride, n_frames, d_power, d_band_power, d_present, "hrfd_spec_process_device"));
  HIP_TRY(hipSetDevice(s->core.device));
  return spec_launch(s, d_captures, capture_stride, n_frames, (unsigned long long *)d_power, (unsigned long long *)d_band_power,
                     d_present, 0xffffffffu, s->core.stream_or_own(stream));
}

extern "C" int hrfd_spec_process(hrfd_spec *s, const int8_t *captures, uint32_t n_frames, uint64_t *power, uint64_t *band_power,
                                 uint8_t *present)
{
  BANK_TRY(spec_check_call(s, captures, s ? 2ull * s->N * n_frames : 0, n_frames, power, band_power, present, "hrfd_spec_process"));
  hrfd::BankHostCall call(s->core);
  uint32_t K;
  {
    std::lock_guard<std::mutex> g(s->core.mu);
    K = (uint32_t)s->bands.size();
  }
  const size_t row = 2 * (size_t)s->N * n_frames, in_total = row * s->n_captures;
  const size_t p_total = sizeof(uint64_t) * (size_t)s->n_captures * s->N;
  if (K == 0 || band_power == nullptr || present == nullptr)
  {
    K = 0;                                                 // no bands, or bands set behind the check: they wait a call
    band_power = nullptr;
    present = nullptr;
  }
  const int8_t *d_in = call.up(s->d_in, captures, in_total);
  unsigned long long *d_power = call.room(s->d_power, power, p_total);
  unsigned long long *d_band_power = call.room(s->d_band_power, band_power, sizeof(uint64_t) * K);
  uint8_t *d_present = call.room(s->d_present, present, K);
  BANK_TRY(call.rc);
  BANK_TRY(spec_launch(s, d_in, row, n_frames, d_power, d_band_power, d_present, K, call.st));
  call.down(power, d_power, p_total);
  call.down(band_power, d_band_power, sizeof(uint64_t) * K);
  call.down(present, d_present, K);
  return call.finish();
}
#endif /* HRFD_SPEC_KERNEL_ONLY */
