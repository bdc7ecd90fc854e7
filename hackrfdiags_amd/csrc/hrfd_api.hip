// hackrfdiags_amd/csrc/hrfd_api.hip -- host side of the C ABI declared in
// include/hrfd.h.  Owns device memory, per-channel state, streams and launches;
// contains no signal processing of its own and NO CPU fallback: without a HIP
// device every create call fails with HRFD_ENODEV.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/hrfd.h"
#include "hrfd_device.h"
#include "hrfd_tables.h"

namespace hrfd {
template <int MODE, bool S256, bool ARITH> __global__ void k_rx_wbfm(const RxParams);
__global__ void k_build_atan_corr(const float *, const float *, uint8_t *, uint32_t *);
template <bool TAB> __global__ void k_atan_eval(const uint8_t *, const float *, float *);
template <int MODE, bool S256, bool ARITH> __global__ void k_rx_fir(const RxParams);
template <int MODE> __global__ void k_rx_post(const RxParams);
__global__ void k_rx_ragged(const RagParams);
__global__ void k_rag_expand(const ChanState *, RagState *, const float *, const uint32_t);
__global__ void k_rx_finish(const EpilogueParams);
} // namespace hrfd

using namespace hrfd;

// ------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                    \
  do                                                                                     \
  {                                                                                      \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
    {                                                                                    \
      return fail(HRFD_ENODEV, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                  __FILE__, __LINE__);                                                   \
    }                                                                                    \
  } while (0)

#include "hrfd_buf.h"
#include "hrfd_rx_plan.h"

extern "C" const char *hrfd_last_error(void) { return g_err; }
extern "C" int hrfd_version(void) { return HRFD_VERSION; }

extern "C" int hrfd_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
  {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

// ------------------------------------------------------------------ host-built tables
// Built with the host libm exactly as the reference constructors do, never with
// device intrinsics:
//   atan2 table  WbFmDemodulator.cc:137-148 / FmDemodulator.cc:159-170
//   dBFS table   DbfsCalculator.cc:58-65 (20*log10f(i), truncated)
static void build_atan2(float *out)
{
  for (int x = 0; x < 256; x++)
  {
    for (int y = 0; y < 256; y++)
    {
      const double xa = (double)x - 128;
      const double ya = (double)y - 128;
      out[y * 256 + x] = (float)atan2(ya, xa);
    }
  }
}

// First-quadrant table of the re-split flow kernel (theta_quad, hrfd_rx_kernels.hip): TQ[|q| * 129 + |i|] =
// (float)atan2((double)|q|, (double)|i|) -- the reference's own entry for i, q >= 0 -- with, in its two free top bits,
// the signed correction (ulps) that makes bits(pi_f - t) + fix the reference's entry for i < 0.  Derived from the
// reference table `lut` itself and PROVEN here, entry by entry: the corrections fit two bits, the table is odd in q
// (row q = -128 included), every word is below 2.0.  Returns false when any of that fails on this libm (the library
// then keeps the kernels that do not use this table).
static bool build_atan_quadrant(const float *lut, uint32_t *out)
{
  auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
  const float pi_f = 3.14159274f;
  bool ok = true;
  for (int i = 0; i < kQuadDwords; i++)
  {
    out[i] = 0u;
  }
  for (int aq = 0; aq <= 128; aq++)
  {
    for (int ai = 0; ai <= 128; ai++)
    {
      const float t = (float)atan2((double)aq, (double)ai);
      const uint32_t tb = bits(t);
      ok = ok && tb < 0x40000000u;
      if (aq <= 127 && ai <= 127)
      {
        ok = ok && tb == bits(lut[(aq + 128) * 256 + (ai + 128)]);          // i, q >= 0: the reference's entry itself
      }
      if (aq >= 1 && ai <= 127)
      {
        ok = ok && (tb ^ 0x80000000u) == bits(lut[(128 - aq) * 256 + (ai + 128)]);   // q < 0, i >= 0: the exact negation
      }
      int32_t fix = 0;
      if (ai >= 1)
      {
        // i = -ai: the entry of q = +aq where it exists, else (q = -128) the negated one
        const uint32_t target = (aq <= 127) ? bits(lut[(aq + 128) * 256 + (128 - ai)]) : (bits(lut[0 * 256 + (128 - ai)]) ^ 0x80000000u);
        fix = (int32_t)(target - bits(pi_f - t));
        ok = ok && fix >= -2 && fix <= 1;
        if (aq >= 1 && aq <= 127)
        {
          ok = ok && (target ^ 0x80000000u) == bits(lut[(128 - aq) * 256 + (128 - ai)]);   // q < 0, i < 0: odd in q as well
        }
      }
      out[aq * kQuadRow + ai] = tb | ((uint32_t)(fix & 3) << 30);
    }
  }
  return ok;
}

static void build_dbfs(int32_t *out)
{
  rx_build_dbfs(out);                                      // (hrfd_rx_plan.h: tests/cpp/san_rx_mag.cc reads the same table)
}

extern "C" int hrfd_atan2_table(float *out)
{
  if (out == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_atan2_table: NULL");
  }
  build_atan2(out);
  return HRFD_OK;
}

extern "C" int hrfd_dbfs_table(int32_t *out)
{
  if (out == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_dbfs_table: NULL");
  }
  build_dbfs(out);
  return HRFD_OK;
}

static int spec_named_table(const char *name, int16_t *out, int cap);   // hrfd_spec.hip: the tables built on the host

extern "C" int hrfd_q15_table(const char *name, int16_t *out, int cap)
{
  if (name == nullptr)
  {
    return 0;
  }
  if (strncmp(name, "SPEC_", 5) == 0)
  {
    return spec_named_table(name, out, cap);
  }
  for (const NamedTable &t : kNamedTables)
  {
    if (strcmp(t.name, name) == 0)
    {
      if (out != nullptr)
      {
        memcpy(out, t.taps, sizeof(int16_t) * (size_t)std::min(cap, t.n));
      }
      return t.n;
    }
  }
  return 0;
}

// ------------------------------------------------------------------ rx handle
struct hrfd_rx
{
  int device = 0;
  int n_cus = 256;                     // compute units of the device
  uint32_t n_channels = 0;
  hipStream_t stream = nullptr;
  hipStream_t last_stream = nullptr;

  std::mutex mu;                       // guards h_cfg / dirty (setters may come from another thread)
  std::vector<ChanCfg> h_cfg;
  bool cfg_dirty = true;
  std::vector<std::pair<uint32_t, int>> pending_resets;   // (channel, mode)

  // device memory: every buffer is owned here and freed with the handle (DevBuf)
  DevBuf<ChanCfg> d_cfg;
  DevBuf<ChanState> d_state, d_state_out;
  DevBuf<float> d_lut;
  DevBuf<uint8_t> d_atcorr;            // arithmetic atan2 (theta_arith): correction bytes, 1/a
  DevBuf<float> d_atinv;
  DevBuf<uint8_t> d_atcorr2;           // first-octant table atan2 (theta_tab): correction bytes, T0
  DevBuf<float> d_att0;
  bool tab_ok = false;                 // its corrections fit: k_rx_wbfm_flow may run
  DevBuf<uint32_t> d_atquad;           // first-quadrant table with embedded corrections (theta_quad: the re-split WBFM flow kernel)
  bool quad_ok = false;
  bool arith_ok = false;               // corrections fit: k_rx_wbfm computes theta instead of gathering it
  int atan_mode = -1;                  // test hook: -1 auto, 0 force the table gather, 1 require arithmetic
  DevBuf<int32_t> d_dbfs;
  DevBuf<uint32_t> d_counters;          // [kNumDevCounters] + a second set of the per-launch counters [kCntSticky]
  uint32_t *d_local = nullptr;          // the per-launch counters of the latest launch (set 0 = d_counters, set 1 behind it)
  int parity = 0;
  DevBuf<uint32_t> d_lists;            // [10][n_channels] channel ids grouped by mode; list 6: every channel that is not WBFM,
                                       // list 7: the AM and SSB channels, list 9: every channel but those in mode NONE
  uint32_t list_count[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  DevBuf<uint32_t> d_sub_lists;        // the same for a launch over a subset of the channels (replay of failed channels);
                                       // list 6 there: the subset itself
  DevBuf<uint32_t> d_chan;             // [4][n_channels]: chan_fail, chan_poison, chan_expired, chan_arrived (EpilogueParams)
  std::vector<uint32_t> h_fail;        // chan_fail of the latest synchronised launch

  // per-call scratch, grown on demand (units = channels * blocks); the four per-unit buffers grow together
  DevBuf<uint8_t> d_present;
  DevBuf<uint32_t> d_magnitude;
  DevBuf<float> d_chk_pub, d_chk_spec;
  size_t unit_cap() const { return std::min({d_present.cap, d_magnitude.cap / 4, d_chk_pub.cap / 4, d_chk_spec.cap / 4}); }
  DevBuf<int16_t> d_ssb_iq;            // 8 kS/s I/Q of the SSB channels, [units][2][npcm]

  // staging for the host-buffer entry
  DevBuf<int8_t> d_iq, d_iq256;
  DevBuf<int16_t> d_pcm;
  DevBuf<uint32_t> d_npcm, d_mag_out;
  DevBuf<uint8_t> d_allowed;
  uint32_t replays = 0;                // launches redone on the exact path (diagnostic)
  uint32_t total_repairs = 0;          // de-emphasis tiles repaired in place since creation

  // measurement hook: HIP events around the demodulator kernels of a launch
  std::vector<hipEvent_t> ev;           // 2 events per slot; slot = launch index % slots
  uint32_t ev_launches = 0;                               // launches that were bracketed with events so far
  uint32_t ev_every = 1, ev_seen = 0;                     // every ev_every-th launch is bracketed (hrfd_rx_debug_timing_every)

  // test hooks
  DevBuf<unsigned long long> d_dbg;     // optional phase stamps (hrfd_rx_debug_stamps)
  int warm = kWarm;
  int stagger = 4;
  int run_len = 0;                     // test hook: blocks per workgroup run of k_rx_wbfm (0 = automatic)
  int use_stream = 2;                  // test hook: 0 = WBFM batches on k_rx_wbfm (runs of blocks, phases in sequence) instead of k_rx_wbfm_flow
  int32_t wbfm_max_threshold = -200;   // the highest squelch threshold among the channels with a demodulator (can a gate close at all?)
  int fir_flow = -1;                   // test hook: AM / SSB / FM batches on the flow kernel's FIR modes: -1 when the bank is large enough, 0 never, 1 always
  int gated_pass = 1;                  // test hook: 0 = no gated second pass on the device (closed gates go back to the host's replay)
  int expire_once = 0;                 // test hook: the next k_rx_wbfm_flow launch treats this wait (1..6) of workgroup 0 as expired
  uint32_t last_counters[kNumCounters] = {0};

  // any block length (hrfd_rx_ragged.hip).  A handle is "on the grid" while every block it was given was a multiple of
  // 512 bytes (inner API: 64): every commutator of the chain is at 0 between calls and ChanState is the whole state.
  // The first block of another length takes it off the grid, for good: RagState per channel, every call on k_rx_ragged.
  bool offgrid = false;
  bool rag_built = false;              // k_rag_expand has run (ChanState -> RagState)
  DevBuf<RagState> d_rag;
  uint64_t ragged_launches = 0;        // launches that ran on k_rx_ragged (diagnostic: hrfd_rx_debug_ragged)
  uint64_t mag_skipped_launches = 0;   // launches of k_rx_wbfm_flow<.., MAG = false> (diagnostic: hrfd_rx_debug_mag_skipped)
};

static int rx_free(hrfd_rx *h)
{
  if (h == nullptr)
  {
    return HRFD_OK;
  }
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (hipEvent_t e : h->ev)
  {
    (void)hipEventDestroy(e);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;                            // with every buffer it owns
  return HRFD_OK;
}

static ChanCfg default_cfg()
{
  ChanCfg c;
  memset(&c, 0, sizeof(c));
  c.mode = HRFD_MODE_NONE;                               // IqDataProcessor.cc:63
  c.threshold = -200;                                    // IqDataProcessor.cc:121
  c.gain_am = 300;                                       // AmDemodulator.cc:102
  c.gain_fm = (float)(64000 / (2 * M_PI));               // FmDemodulator.cc:173
  c.gain_wbfm = (float)(256000 / (2 * M_PI));            // WbFmDemodulator.cc:151
  c.gain_ssb = 300;                                      // SsbDemodulator.cc ctor
  c.lsb = 1;                                             // SsbDemodulator.cc ctor
  return c;
}

extern "C" int hrfd_rx_create(uint32_t n_channels, int device, hrfd_rx **out)
{
  if (out == nullptr || n_channels == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_create: need n_channels > 0 and a result pointer");
  }
  *out = nullptr;
  if (hrfd_device_count() <= 0)
  {
    return fail(HRFD_ENODEV, "hrfd_rx_create: no HIP device visible (this library has no CPU path)");
  }
  if (device < 0)
  {
    HIP_TRY(hipGetDevice(&device));
  }
  HIP_TRY(hipSetDevice(device));
  hrfd_rx *h = new hrfd_rx;
  h->device = device;
  h->n_channels = n_channels;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
    {
      h->n_cus = cus;
    }
  }
  h->h_cfg.assign(n_channels, default_cfg());
  int rc = HRFD_OK;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
  {
    rc = fail(HRFD_ENODEV, "hrfd_rx_create: stream creation failed");
  }
  else if (!(h->d_cfg.alloc(n_channels) && h->d_state.alloc(n_channels) && h->d_state_out.alloc(n_channels) && h->d_lut.alloc(65536) &&
             h->d_atcorr.alloc(kCorrBytes) && h->d_atinv.alloc(kInvEntries) && h->d_atcorr2.alloc(kCorrBytes) && h->d_att0.alloc(kCorrBytes) &&
             h->d_atquad.alloc(kQuadDwords) && h->d_dbfs.alloc(257) && h->d_counters.alloc(kNumDevCounters + kCntSticky) &&
             h->d_lists.alloc((size_t)kRxLists * n_channels) && h->d_sub_lists.alloc((size_t)kRxLists * n_channels) &&
             h->d_chan.alloc((size_t)4 * n_channels)))
  {
    rc = HRFD_ENOMEM;                                      // (the text is the failed allocation's)
  }
  if (rc != HRFD_OK)
  {
    rx_free(h);
    return rc;
  }
  // Zero state == the reference's freshly constructed objects: zero filter
  // pipelines, previousTheta = 0, tracker in NoSignal.  A zero raw/iq256
  // history is exactly equivalent to zero filter state.
  // (offset-binary tails hold 0x80 = value 0.)
  std::vector<ChanState> init(n_channels);
  memset(init.data(), 0, sizeof(ChanState) * n_channels);
  for (auto &s : init)
  {
    memset(s.fm_tail, 0x80, sizeof(s.fm_tail));
    memset(s.am_tail, 0x80, sizeof(s.am_tail));
    memset(s.ssb_tail, 0x80, sizeof(s.ssb_tail));
  }
  std::vector<float> lut(65536);
  int32_t dbfs[257];
  build_atan2(lut.data());
  build_dbfs(dbfs);
  hipError_t e = hipMemcpy(h->d_state, init.data(), sizeof(ChanState) * n_channels, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_state_out, init.data(), sizeof(ChanState) * n_channels, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_lut, lut.data(), sizeof(float) * 65536, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_dbfs, dbfs, sizeof(dbfs), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(h->d_counters, 0, sizeof(uint32_t) * (kNumDevCounters + kCntSticky));
  if (e == hipSuccess) e = hipMemset(h->d_chan, 0, sizeof(uint32_t) * 4 * n_channels);
  h->h_fail.assign(n_channels, 0u);
  h->d_local = h->d_counters;
  // arithmetic atan2: reciprocals from the host (correctly rounded), correction bytes derived on
  // the device from the table just uploaded, with the kernel's own arithmetic (k_build_atan_corr)
  float inv[kInvEntries];
  memset(inv, 0, sizeof(inv));
  for (int a = 1; a <= 128; a++)
  {
    inv[a] = 1.0f / (float)a;
  }
  uint32_t bad = 0;
  if (e == hipSuccess) e = hipMemcpy(h->d_atinv, inv, sizeof(inv), hipMemcpyHostToDevice);
  if (e == hipSuccess)
  {
    hipLaunchKernelGGL(k_build_atan_corr<false>, dim3((kCorrBytes + 255) / 256), dim3(256), 0, 0, h->d_lut.p, h->d_atinv.p,
                       h->d_atcorr.p, h->d_counters + kCntScratch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&bad, h->d_counters + kCntScratch, sizeof(bad), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemset(h->d_counters + kCntScratch, 0, sizeof(uint32_t));
  // first-octant table T0[a(a+1)/2 + b] = (float)atan2((double)b, (double)a): the host's libm, the formula of
  // WbFmDemodulator.cc:137-148; its corrections for the other octants are derived the same way
  uint32_t bad2 = 0;
  {
    std::vector<float> t0(kCorrBytes, 0.0f);
    for (int a = 0; a <= 128; a++)
    {
      for (int b = 0; b <= a; b++)
      {
        t0[(size_t)a * (a + 1) / 2 + b] = (float)atan2((double)b, (double)a);
      }
    }
    if (e == hipSuccess) e = hipMemcpy(h->d_att0, t0.data(), sizeof(float) * kCorrBytes, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess)
  {
    hipLaunchKernelGGL(k_build_atan_corr<true>, dim3((kCorrBytes + 255) / 256), dim3(256), 0, 0, h->d_lut.p, h->d_att0.p,
                       h->d_atcorr2.p, h->d_counters + kCntScratch);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&bad2, h->d_counters + kCntScratch, sizeof(bad2), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemset(h->d_counters + kCntScratch, 0, sizeof(uint32_t));
  {
    std::vector<uint32_t> tq(kQuadDwords);
    h->quad_ok = build_atan_quadrant(lut.data(), tq.data());
    if (e == hipSuccess) e = hipMemcpy(h->d_atquad, tq.data(), sizeof(uint32_t) * kQuadDwords, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess)
  {
    rc = fail(HRFD_ENODEV, "hrfd_rx_create: initial upload failed: %s", hipGetErrorString(e));
    rx_free(h);
    return rc;
  }
  h->arith_ok = (bad == 0) || (HRFD_ABLATE & 512) != 0;   // (512: TIMING EXPERIMENT ONLY)
  h->tab_ok = (bad2 == 0);
  *out = h;
  return HRFD_OK;
}

extern "C" int hrfd_rx_destroy(hrfd_rx *h) { return rx_free(h); }

template <typename F>
static int for_channels(hrfd_rx *h, uint32_t channel, F f)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  if (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels)
  {
    return fail(HRFD_EINVAL, "channel %u out of range (%u channels)", channel, h->n_channels);
  }
  std::lock_guard<std::mutex> g(h->mu);
  const uint32_t lo = (channel == HRFD_ALL_CHANNELS) ? 0 : channel;
  const uint32_t hi = (channel == HRFD_ALL_CHANNELS) ? h->n_channels : channel + 1;
  for (uint32_t c = lo; c < hi; c++)
  {
    f(c);
  }
  h->cfg_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_rx_set_mode(hrfd_rx *h, uint32_t channel, int mode)
{
  if (mode < HRFD_MODE_NONE || mode > HRFD_MODE_USB)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_set_mode: bad mode %d", mode);
  }
  return for_channels(h, channel, [&](uint32_t c) {
    h->h_cfg[c].mode = mode;
    // IqDataProcessor::setDemodulatorMode also selects the SSB sideband (:357-372)
    if (mode == HRFD_MODE_LSB) h->h_cfg[c].lsb = 1;
    if (mode == HRFD_MODE_USB) h->h_cfg[c].lsb = 0;
  });
}

extern "C" int hrfd_rx_set_gain(hrfd_rx *h, uint32_t channel, int mode, float gain)
{
  if (mode < HRFD_MODE_AM || mode > HRFD_MODE_USB)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_set_gain: bad mode %d", mode);
  }
  return for_channels(h, channel, [&](uint32_t c) {
    switch (mode)
    {
      case HRFD_MODE_AM: h->h_cfg[c].gain_am = gain; break;
      case HRFD_MODE_FM: h->h_cfg[c].gain_fm = gain; break;
      case HRFD_MODE_WBFM: h->h_cfg[c].gain_wbfm = gain; break;
      default: h->h_cfg[c].gain_ssb = gain; break;
    }
  });
}

extern "C" int hrfd_rx_set_threshold(hrfd_rx *h, uint32_t channel, int32_t threshold)
{
  return for_channels(h, channel, [&](uint32_t c) { h->h_cfg[c].threshold = threshold; });
}

extern "C" int hrfd_rx_reset_demod(hrfd_rx *h, uint32_t channel, int mode)
{
  if (mode < HRFD_MODE_AM || mode > HRFD_MODE_USB)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_reset_demod: bad mode %d", mode);
  }
  return for_channels(h, channel, [&](uint32_t c) { h->pending_resets.push_back({c, mode}); });
}

// apply queued X::resetDemodulator calls to the device state
static int apply_resets(hrfd_rx *h, hipStream_t s, std::vector<std::pair<uint32_t, int>> &resets)
{
  for (auto &r : resets)
  {
    if (h->rag_built)
    {
      // off the grid the state is RagState: Decimator_int16::resetFilterState (Decimator_int16.cc:131-147) clears the
      // pipeline AND the commutator position
      RagState *g = h->d_rag + r.first;
      switch (r.second)
      {
        case HRFD_MODE_WBFM:
          HIP_TRY(hipMemsetAsync(&g->wb.theta, 0, sizeof(float), s));
          HIP_TRY(hipMemsetAsync(&g->wb.d1, 0, 3 * sizeof(RagQ15), s));
          break;
        case HRFD_MODE_FM:
          HIP_TRY(hipMemsetAsync(&g->fm, 0, sizeof(RagFm), s));
          break;
        case HRFD_MODE_AM:
          HIP_TRY(hipMemsetAsync(&g->am, 0, sizeof(RagAs), s));
          break;
        default:
          HIP_TRY(hipMemsetAsync(&g->ssb, 0, sizeof(RagAs), s));
          break;
      }
      continue;
    }
    ChanState *d = h->d_state + r.first;
    switch (r.second)
    {
      case HRFD_MODE_WBFM:
        // WbFmDemodulator.cc:265-278: the three decimators and previousTheta;
        // the de-emphasis filter (wb_p, wb_y) is left alone.
        HIP_TRY(hipMemsetAsync(&d->wb_theta, 0, sizeof(float), s));
        HIP_TRY(hipMemsetAsync(d->wb_s, 0, sizeof(d->wb_s) + sizeof(d->wb_u) + sizeof(d->wb_v), s));
        break;
      case HRFD_MODE_FM:
        HIP_TRY(hipMemsetAsync(d->fm_tail, 0x80, sizeof(d->fm_tail), s));
        HIP_TRY(hipMemsetAsync(d->fm_u, 0, sizeof(d->fm_u) + sizeof(d->fm_v), s));
        break;
      case HRFD_MODE_AM:
        HIP_TRY(hipMemsetAsync(d->am_tail, 0x80, sizeof(d->am_tail), s));
        HIP_TRY(hipMemsetAsync(&d->am_x1, 0, 2 * sizeof(float), s));
        break;
      default:
        HIP_TRY(hipMemsetAsync(d->ssb_tail, 0x80, sizeof(d->ssb_tail), s));
        HIP_TRY(hipMemsetAsync(&d->ssb_x1, 0, 2 * sizeof(float) + sizeof(d->ssb_i) + sizeof(d->ssb_q), s));
        break;
    }
  }
  resets.clear();
  return HRFD_OK;
}

struct LaunchOpts
{
  uint32_t out_blocks;     // layout [C][out_blocks] of the caller's output buffers
  uint32_t out_b0;         // first block of that layout this launch fills
  int serial;              // exact one-lane de-emphasis (replay path)
  int src256;              // input is the 256 kS/s mixed stream (hrfd_demod_*)
  const std::vector<uint32_t> *subset = nullptr;   // launch for these channels only (ascending ids), nullptr = all
};

// the arguments of rx_launch, for its steps
struct RxCall
{
  const int8_t *d_iq;
  uint64_t channel_stride;
  uint32_t block_bytes, n_blocks, gain_db;
  int16_t *d_pcm;
  uint32_t *d_n_pcm, *d_magnitude;
  uint8_t *d_allowed;
  int8_t *d_iq256;
  hipStream_t s;
  const LaunchOpts &opt;
};

// The configuration snapshot, under the handle's lock: the queued resets are taken over, the per-mode lists are rebuilt
// and uploaded when a setter has run, and a subset gets lists of its own (sub_count).
static int rx_snapshot(hrfd_rx *h, const RxCall &c, uint32_t sub_count[kRxLists], std::vector<std::pair<uint32_t, int>> &resets)
{
  const std::vector<uint32_t> *const subset = c.opt.subset;
  std::vector<uint32_t> lists;
  {
    std::lock_guard<std::mutex> g(h->mu);
    resets.swap(h->pending_resets);
    if (h->cfg_dirty)
    {
      lists.assign((size_t)kRxLists * h->n_channels, 0u);
      rx_build_lists(h->h_cfg.data(), h->n_channels, false, nullptr, 0, lists.data(), h->list_count);
      h->wbfm_max_threshold = rx_max_threshold(h->h_cfg.data(), h->n_channels);
      // synchronous uploads: the host vectors are only valid under the lock
      HIP_TRY(hipStreamSynchronize(c.s));
      HIP_TRY(hipMemcpy(h->d_cfg, h->h_cfg.data(), sizeof(ChanCfg) * h->n_channels, hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(h->d_lists, lists.data(), sizeof(uint32_t) * lists.size(), hipMemcpyHostToDevice));
      h->cfg_dirty = false;
    }
    if (subset != nullptr)
    {
      // only the modes are read under the lock
      lists.assign((size_t)kRxLists * h->n_channels, 0u);
      rx_build_lists(h->h_cfg.data(), h->n_channels, true, subset->data(), (uint32_t)subset->size(), lists.data(), sub_count);
    }
  }
  if (subset != nullptr && !subset->empty())
  {
    // (outside the configuration lock: the CLI thread's setters do not wait for this upload)
    HIP_TRY(hipStreamSynchronize(c.s));
    HIP_TRY(hipMemcpy(h->d_sub_lists, lists.data(), sizeof(uint32_t) * lists.size(), hipMemcpyHostToDevice));
  }
  return HRFD_OK;
}

// launch-local scratch (present flags, cross-block check values), the magnitude buffer used when the caller does not
// want one, and the SSB channels' 8 kS/s rails
static int rx_grow_scratch(hrfd_rx *h, const RxCall &c, uint32_t n256, bool has_ssb)
{
  const size_t units = (size_t)h->n_channels * c.n_blocks;
  const size_t need = std::max(units, (size_t)h->n_channels * c.opt.out_blocks);
  if (need > h->unit_cap())
  {
    HIP_TRY(hipStreamSynchronize(c.s));
    int rc;
    if ((rc = h->d_present.grow_bytes(need)) != HRFD_OK) return rc;
    if ((rc = h->d_magnitude.grow_bytes(need * 4)) != HRFD_OK) return rc;
    if ((rc = h->d_chk_pub.grow_bytes(need * 4)) != HRFD_OK) return rc;
    if ((rc = h->d_chk_spec.grow_bytes(need * 4)) != HRFD_OK) return rc;
  }
  const size_t ssb = units * (size_t)(n256 / 32) * 2 * sizeof(int16_t);
  if (has_ssb && ssb > h->d_ssb_iq.cap)
  {
    HIP_TRY(hipStreamSynchronize(c.s));
    return h->d_ssb_iq.grow_bytes(ssb);
  }
  return HRFD_OK;
}

// what every kernel of the launch is given; a step of the plan sets its own list, runs and flags on a copy (rx_execute)
static void rx_fill_params(hrfd_rx *h, const RxCall &c, const RxGeometry &g, RxParams &P)
{
  // per-launch counters: two sets used alternately, each cleared by the previous launch's k_rx_commit
  h->parity ^= 1;
  uint32_t *const local = h->parity ? h->d_counters + kNumDevCounters : h->d_counters.p;
  uint32_t *const other = h->parity ? h->d_counters.p : h->d_counters + kNumDevCounters;
  h->d_local = local;

  memset(&P, 0, sizeof(P));
  P.iq = c.d_iq;
  P.ch_stride = c.channel_stride;
  P.block_bytes = c.block_bytes;
  P.n_blocks = c.n_blocks;
  P.n256 = g.n256;
  P.ntiles = g.ntiles;
  P.origin = g.origin;
  P.hal = g.hal;
  P.warm_tiles = g.warm_tiles;
  P.seed_terms = g.seed_terms;
  P.seed_ct = (float)pow(-(double)DEEMPH_A1, (double)kTile);
  P.serial = c.opt.serial;
  P.src256 = c.opt.src256;
  P.stagger = h->stagger & 63;
  P.run_len = 1;
  P.n_runs = c.n_blocks;
  P.dbg_flags = h->stagger >> 8;
  P.out_blocks = c.opt.out_blocks;
  P.out_b0 = c.opt.out_b0;
  P.gain_db = c.gain_db;
  P.state = h->d_state;
  P.state_out = h->d_state_out;
  P.cfg = h->d_cfg;
  P.pcm = c.d_pcm;
  P.magnitude = (c.d_magnitude != nullptr) ? c.d_magnitude : h->d_magnitude.p;
  P.present = h->d_present;
  P.iq256 = c.d_iq256;
  P.ssb_iq = h->d_ssb_iq;
  P.atan2_lut = h->d_lut;
  P.at_corr = h->d_atcorr;
  P.at_inv = h->d_atinv;
  P.at_corr2 = h->d_atcorr2;
  P.at_t0 = h->d_att0;
  P.at_quad = h->d_atquad;
  P.dbfs = h->d_dbfs;
  P.chk_pub = h->d_chk_pub;
  P.chk_spec = h->d_chk_spec;
  P.counters = local;
  P.flow_hal = 1536;           // >= 768 + 64 * (warm_tiles + seed_terms + 1), whole units
  P.flow_seed_ct = (float)pow(-(double)DEEMPH_A1, 64.0);
  P.dbg = nullptr;
  // (wbfm_max_threshold is the snapshot's: rx_snapshot runs in front of this)
  P.mag_unobservable = rx_magnitude_unobservable(h->wbfm_max_threshold, c.gain_db, c.d_magnitude != nullptr) ? 1 : 0;

  EpilogueParams E;
  memset(&E, 0, sizeof(E));
  E.n_channels = h->n_channels;
  E.n_blocks = c.n_blocks;
  E.n_pcm_per_block = g.n256 / 32;
  E.out_blocks = c.opt.out_blocks;
  E.out_b0 = c.opt.out_b0;
  E.cfg = h->d_cfg;
  E.state = h->d_state;
  E.state_out = h->d_state_out;
  E.present = h->d_present;
  E.allowed = c.d_allowed;
  E.n_pcm = c.d_n_pcm;
  E.chk_pub = h->d_chk_pub;
  E.chk_spec = h->d_chk_spec;
  E.counters = local;
  E.sticky = h->d_counters;
  E.next_local = other;
  E.chan_list = nullptr;
  E.first_channel = (c.opt.subset != nullptr) ? c.opt.subset->front() : 0u;
  E.chan_fail = h->d_chan;
  E.chan_poison = h->d_chan + h->n_channels;
  E.chan_expired = h->d_chan + 2 * (size_t)h->n_channels;
  E.chan_arrived = h->d_chan + 3 * (size_t)h->n_channels;
  P.fin = E;
  P.self_finish = 0;
  P.sticky = h->d_counters;
}

// Any block length: k_rx_ragged.  One workgroup per channel, the call's blocks in order, every stage with its commutator
// position: exact, no speculation, every channel commits.  A length that is not a whole number of PCM samples (512 bytes;
// inner API 64) takes the handle off the grid for good: its state moves from ChanState to RagState (k_rag_expand, once).
// E: the launch's bookkeeping (rx_fill_params); sub_list: the subset's channels, or nullptr with n_list = all of them.
static int launch_ragged(hrfd_rx *h, const RxCall &c, const EpilogueParams &E, const uint32_t *sub_list, uint32_t n_list)
{
  const int src256 = c.opt.src256;
  if ((c.block_bytes % (src256 ? 64u : 512u)) != 0)
  {
    h->offgrid = true;
  }
  if (h->offgrid && !h->rag_built)
  {
    if (h->d_rag == nullptr)
    {
      HIP_TRY(hipStreamSynchronize(c.s));
      if (!h->d_rag.alloc(h->n_channels))
      {
        return HRFD_ENOMEM;
      }
    }
    HIP_TRY(hipMemsetAsync(h->d_rag, 0, sizeof(RagState) * h->n_channels, c.s));
    hipLaunchKernelGGL(k_rag_expand, dim3(h->n_channels), dim3(kRagThreads), 0, c.s, h->d_state.p, h->d_rag.p, h->d_lut.p, h->n_channels);
    HIP_TRY(hipGetLastError());
    h->rag_built = true;
  }
  RagParams R;
  memset(&R, 0, sizeof(R));
  R.iq = c.d_iq;
  R.ch_stride = c.channel_stride;
  R.block_bytes = c.block_bytes;
  R.n_blocks = c.n_blocks;
  R.src256 = src256;
  R.offgrid = h->offgrid ? 1 : 0;
  R.pcm_cap = src256 ? (c.block_bytes + 63u) / 64u : (c.block_bytes + 511u) / 512u;
  R.iq256_cap = 2u * ((c.block_bytes / 2u + 7u) / 8u);
  R.out_blocks = c.opt.out_blocks;
  R.out_b0 = c.opt.out_b0;
  R.chan_list = sub_list;
  R.n_list = n_list;
  R.gain_db = c.gain_db;
  R.state = h->d_state;
  R.rag = h->d_rag;
  R.cfg = h->d_cfg;
  R.pcm = c.d_pcm;
  R.n_pcm = c.d_n_pcm;
  R.magnitude = (c.d_magnitude != nullptr) ? c.d_magnitude : h->d_magnitude.p;
  R.allowed = c.d_allowed;
  R.iq256 = c.d_iq256;
  R.atan2_lut = h->d_lut;
  R.dbfs = h->d_dbfs;
  R.counters = E.counters;
  R.sticky = E.sticky;
  R.next_local = E.next_local;
  R.first_channel = E.first_channel;
  R.chan_fail = E.chan_fail;
  R.chan_poison = E.chan_poison;
  hipLaunchKernelGGL(k_rx_ragged, dim3(R.n_list), dim3(kRagThreads), 0, c.s, R);
  HIP_TRY(hipGetLastError());
  h->ragged_launches++;
  return HRFD_OK;
}

// the plan's input: the lists' sizes, the call, the handle's knobs
static RxPlanIn rx_plan_input(const hrfd_rx *h, const RxCall &c, const RxGeometry &g, const uint32_t *count)
{
  RxPlanIn in;
  memcpy(in.count, count, sizeof(in.count));
  in.n_channels = h->n_channels;
  in.n_blocks = c.n_blocks;
  in.n256 = g.n256;
  in.gain_db = c.gain_db;
  in.max_threshold = h->wbfm_max_threshold;
  in.warm_tiles = g.warm_tiles;
  in.serial = c.opt.serial != 0;
  in.src256 = c.opt.src256 != 0;
  in.subset = c.opt.subset != nullptr;
  in.dump = c.d_iq256 != nullptr;
  in.use_stream = h->use_stream;
  in.atan_mode = h->atan_mode;
  in.fir_flow = h->fir_flow;
  in.gated_pass = h->gated_pass;
  in.run_len = h->run_len;
  in.tab_ok = h->tab_ok;
  in.quad_ok = h->quad_ok;
  in.arith_ok = h->arith_ok;
  in.has_dbg = h->d_dbg != nullptr;
  in.dbg_cap = h->d_dbg.cap / sizeof(unsigned long long);
  return in;
}

// the plan's steps, in order, on the caller's stream: each on its own copy of the launch's parameters
static int rx_execute(hrfd_rx *h, const RxPlan &plan, const RxParams &base, const uint32_t *d_lists, hipStream_t s)
{
  for (int i = 0; i < plan.n; i++)
  {
    const RxStep &st = plan.step[i];
    const uint32_t *const list = (st.list >= 0) ? d_lists + (size_t)st.list * h->n_channels : nullptr;
    const dim3 grid(st.grid), block(st.block);
    if (st.kernel == kRxFinish)
    {
      EpilogueParams G = base.fin;
      G.chan_list = list;
      G.n_channels = st.n_list;
      hipLaunchKernelGGL(k_rx_finish, grid, block, 0, s, G);
      HIP_TRY(hipGetLastError());
      continue;
    }
    RxParams P = base;
    P.chan_list = list;
    P.n_list = st.n_list;
    P.run_len = st.run_len;
    P.n_runs = st.n_runs;
    P.warm_tiles = st.warm_tiles;
    P.self_finish = st.self_finish ? 1 : 0;
    P.dbg = st.dbg ? h->d_dbg.p : nullptr;
    if (st.expire_once)
    {
      P.dbg_flags |= h->expire_once << 16;
      h->expire_once = 0;
    }
    switch (st.kernel)
    {
      case kRxFlowBank: hipLaunchKernelGGL((k_rx_flow_bank<HRFD_FLOW_SVC, false>), grid, block, 0, s, P); break;
      case kRxFlowBankDump: hipLaunchKernelGGL((k_rx_flow_bank<HRFD_FLOW_SVC, true>), grid, block, 0, s, P); break;
      case kRxFlowAs: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, false, 14>), grid, block, 0, s, P); break;
      case kRxFlowAsDump: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, true, 14>), grid, block, 0, s, P); break;
      case kRxFlowFm: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, false, 2>), grid, block, 0, s, P); break;
      case kRxFlowFmDump: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, true, 2>), grid, block, 0, s, P); break;
      case kRxFlowWb:
#if HRFD_FLOW_NOMAG
        if (P.mag_unobservable != 0)
        {
          // nobody can see the block magnitudes: the instantiation whose stream waves do not compute them
          hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, false, 3, false>), grid, block, 0, s, P);
          h->mag_skipped_launches++;
          break;
        }
#endif
        hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, false>), grid, block, 0, s, P);
        break;
      case kRxFlowWbDump: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, false, true>), grid, block, 0, s, P); break;
      case kRxGatedWb: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, true, false>), grid, block, 0, s, P); break;
      case kRxGatedFm: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, true, false, 2>), grid, block, 0, s, P); break;
      case kRxGatedAs: hipLaunchKernelGGL((k_rx_wbfm_flow<HRFD_FLOW_SVC, true, false, 14>), grid, block, 0, s, P); break;
      case kRxFirAs: hipLaunchKernelGGL((k_rx_fir<14, false, false>), grid, block, 0, s, P); break;
      case kRxFirAs256: hipLaunchKernelGGL((k_rx_fir<14, true, false>), grid, block, 0, s, P); break;
      case kRxPostAs: hipLaunchKernelGGL((k_rx_post<14>), grid, block, 0, s, P); break;
      case kRxFirFm: hipLaunchKernelGGL((k_rx_fir<2, false, false>), grid, block, 0, s, P); break;
      case kRxFirFm256: hipLaunchKernelGGL((k_rx_fir<2, true, false>), grid, block, 0, s, P); break;
      case kRxFirFmArith: hipLaunchKernelGGL((k_rx_fir<2, false, true>), grid, block, 0, s, P); break;
      case kRxBlocksNone: hipLaunchKernelGGL((k_rx_wbfm<0, false, false>), grid, block, 0, s, P); break;
      case kRxBlocksWb: hipLaunchKernelGGL((k_rx_wbfm<3, false, false>), grid, block, 0, s, P); break;
      case kRxBlocksWb256: hipLaunchKernelGGL((k_rx_wbfm<3, true, false>), grid, block, 0, s, P); break;
      case kRxBlocksWbArith: hipLaunchKernelGGL((k_rx_wbfm<3, false, true>), grid, block, 0, s, P); break;
      default: return fail(HRFD_ESTATE, "internal: no kernel %d", (int)st.kernel);
    }
    HIP_TRY(hipGetLastError());
  }
  return HRFD_OK;
}

// The measurement hook's bracket around the kernels of a launch: returns the slot whose events take it, or -1.
// (an event record is a packet of its own on the queue, ~3 us each: bracketing EVERY launch of a back-to-back
//  sequence puts ~6 us of gap between kernels that otherwise follow each other without any -- measured, 256 x 16:
//  0.2237 ms per step with the events, 0.2166 without; hrfd_rx_debug_timing_every samples instead)
static int rx_timing_slot(hrfd_rx *h)
{
  const size_t slots = h->ev.size() / 2;
  return (slots != 0 && (h->ev_seen++ % h->ev_every) == 0) ? (int)(h->ev_launches % slots) : -1;
}

static int rx_launch(hrfd_rx *h, const int8_t *d_iq, uint64_t channel_stride, uint32_t block_bytes,
                     uint32_t n_blocks, uint32_t gain_db, int16_t *d_pcm, uint32_t *d_n_pcm,
                     uint32_t *d_magnitude, uint8_t *d_allowed, int8_t *d_iq256, hipStream_t s,
                     const LaunchOpts &opt)
{
  if (h == nullptr || d_iq == nullptr || d_pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_process: NULL handle or buffer");
  }
  const RxCall call = {d_iq, channel_stride, block_bytes, n_blocks, gain_db, d_pcm, d_n_pcm, d_magnitude, d_allowed, d_iq256, s, opt};
  int rc;
  // 1. geometry
  RxGeometry g;
  if ((rc = rx_geometry(block_bytes, n_blocks, channel_stride, opt.out_b0, opt.out_blocks, opt.serial, opt.src256, h->offgrid,
                        h->warm, &g)) != HRFD_OK)
  {
    return rc;
  }
  HIP_TRY(hipSetDevice(h->device));
  // 2. configuration snapshot
  const bool subset = opt.subset != nullptr;
  uint32_t sub_count[kRxLists] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<std::pair<uint32_t, int>> resets;
  if ((rc = rx_snapshot(h, call, sub_count, resets)) != HRFD_OK)
  {
    return rc;
  }
  if (subset && opt.subset->empty())
  {
    return HRFD_OK;
  }
  const uint32_t *const list_count = subset ? sub_count : h->list_count;
  const uint32_t *const d_lists = subset ? h->d_sub_lists.p : h->d_lists.p;
  if ((rc = apply_resets(h, s, resets)) != HRFD_OK)
  {
    return rc;
  }
  // 3. scratch
  if ((rc = rx_grow_scratch(h, call, g.n256, list_count[HRFD_MODE_LSB] + list_count[HRFD_MODE_USB] != 0)) != HRFD_OK)
  {
    return rc;
  }
  // 4. parameters
  RxParams P;
  rx_fill_params(h, call, g, P);
  const int ev_slot = rx_timing_slot(h);
  if (ev_slot >= 0)
  {
    HIP_TRY(hipEventRecord(h->ev[2 * ev_slot], s));
  }
  if (g.ragged)
  {
    rc = launch_ragged(h, call, P.fin, subset ? d_lists + (size_t)kRxListNotWb * h->n_channels : nullptr,
                       subset ? list_count[kRxListNotWb] : h->n_channels);
  }
  else
  {
    // 5. plan, 6. execute
    rc = rx_execute(h, rx_plan(rx_plan_input(h, call, g, list_count)), P, d_lists, s);
  }
  if (rc != HRFD_OK)
  {
    return rc;
  }
  if (ev_slot >= 0)
  {
    HIP_TRY(hipEventRecord(h->ev[2 * ev_slot + 1], s));
    h->ev_launches++;
  }
  h->last_stream = s;
  return HRFD_OK;
}

extern "C" int hrfd_rx_process_device(hrfd_rx *h, const int8_t *d_iq, uint64_t channel_stride,
                                      uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db,
                                      int16_t *d_pcm, uint32_t *d_n_pcm, uint32_t *d_magnitude,
                                      uint8_t *d_signal_allowed, int8_t *d_iq256k_opt, void *stream)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  hipStream_t s = (stream != nullptr) ? (hipStream_t)stream : h->stream;
  const LaunchOpts opt = {n_blocks, 0, 0, 0};
  return rx_launch(h, d_iq, channel_stride, block_bytes, n_blocks, gain_db, d_pcm, d_n_pcm,
                   d_magnitude, d_signal_allowed, d_iq256k_opt, s, opt);
}

extern "C" int hrfd_rx_sync(hrfd_rx *h, uint32_t *n_violations)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->last_stream ? h->last_stream : h->stream;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(h->last_counters, h->d_counters, sizeof(h->last_counters), hipMemcpyDeviceToHost));   // the totals
  HIP_TRY(hipMemcpy(h->last_counters, h->d_local, sizeof(uint32_t) * kCntSticky, hipMemcpyDeviceToHost)); // the latest launch
  h->total_repairs = h->last_counters[kCntTotRepair];
  // channels of the latest launch that did not commit (their own checks failed, or they ran behind an unrepaired failure)
  const uint32_t viol = (h->last_counters[kCntTotLaunch] != 0) ? h->last_counters[kCntFail] : 0u;
  h->last_counters[kCntCommit] = (viol == 0) ? 1u : 0u;  // shown as "all committed" by hrfd_rx_debug_counters
  if (viol != 0)
  {
    // the caller repairs those channels from here (resubmits them block by block, hrfd_rx_failed_channels says
    // which): they may commit again
    HIP_TRY(hipMemcpy(h->h_fail.data(), h->d_chan, sizeof(uint32_t) * h->n_channels, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(h->d_chan + h->n_channels, 0, sizeof(uint32_t) * h->n_channels));
  }
  else
  {
    std::fill(h->h_fail.begin(), h->h_fail.end(), 0u);
  }
  if (n_violations != nullptr)
  {
    *n_violations = viol;
  }
  return HRFD_OK;
}

// Which channels of the launch that hrfd_rx_sync last waited for did not commit: out[c] != 0 (kFail* bits:
// 1 closed gate in a batch, 2 failed time-parallel speculation, 4 behind an unrepaired failure, 8 internal wait expired).
extern "C" int hrfd_rx_failed_channels(hrfd_rx *h, uint8_t *out, uint32_t n)
{
  if (h == nullptr || out == nullptr || n != h->n_channels)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_failed_channels: need a handle and room for n_channels flags");
  }
  for (uint32_t c = 0; c < n; c++)
  {
    out[c] = (uint8_t)h->h_fail[c];
  }
  return HRFD_OK;
}

// Replays `subset` (ascending channel ids) through the exact path: one block per launch (state advances in
// order); a channel whose de-emphasis tiles did not re-synchronise is redone on the one-lane path.  Inputs and
// outputs are the full [n_channels][n_blocks][...] device buffers of the call being repaired.
// (round 6: the blocks [b0, b0 + nb) of the call -- hrfd_rx_process_block repairs a long call chunk by chunk)
static int rx_replay(hrfd_rx *h, const std::vector<uint32_t> &subset, const int8_t *d_iq, uint64_t stride,
                     uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db, int16_t *d_pcm, uint32_t *d_npcm,
                     uint32_t *d_mag, uint8_t *d_allowed, int8_t *d_iq256, hipStream_t s, bool pcm_is_clear,
                     uint32_t b0 = 0, uint32_t nb = 0)
{
  if (subset.empty())
  {
    return HRFD_OK;
  }
  if (nb == 0)
  {
    nb = n_blocks - b0;
  }
  // squelched units write no PCM: they must read as zeros, not as what a failed batch left there
  const size_t blk_row = (size_t)((block_bytes + 511u) / 512u) * sizeof(int16_t);
  const size_t row = (size_t)n_blocks * blk_row;
  const bool whole_bank = subset.size() == h->n_channels;
  if (pcm_is_clear)
  {
    // (no batch ran over this buffer: the caller's memset still stands)
  }
  else if (whole_bank && nb == n_blocks)
  {
    HIP_TRY(hipMemsetAsync(d_pcm, 0, row * h->n_channels, s));
  }
  else
  {
    for (uint32_t c : subset)
    {
      HIP_TRY(hipMemsetAsync(reinterpret_cast<char *>(d_pcm) + row * c + blk_row * b0, 0, blk_row * nb, s));
    }
  }
  for (uint32_t b = b0; b < b0 + nb; b++)
  {
    // attempt 0: the exact per-block kernel; attempt 1: its one-lane de-emphasis for the channels whose tiles did not
    // re-synchronise.  The whole bank runs on the cached per-mode lists (no subset, no upload: the reference's own
    // cadence of one block per call takes this path on every call).
    bool all = whole_bank, clean = false;
    std::vector<uint32_t> todo;
    if (!all)
    {
      todo = subset;
    }
    for (int attempt = 0; attempt < 2 && !clean; attempt++)
    {
      LaunchOpts opt = {n_blocks, b, attempt, 0};
      opt.subset = all ? nullptr : &todo;
      int rc = rx_launch(h, d_iq + (size_t)b * block_bytes, stride, block_bytes, 1, gain_db, d_pcm, d_npcm, d_mag,
                         d_allowed, d_iq256, s, opt);
      if (rc != HRFD_OK) return rc;
      uint32_t viol = 0;
      if ((rc = hrfd_rx_sync(h, &viol)) != HRFD_OK) return rc;
      if (viol == 0)
      {
        clean = true;
        break;
      }
      h->replays++;
      std::vector<uint32_t> again;
      for (uint32_t c : (all ? subset : todo))
      {
        if (h->h_fail[c] != 0) again.push_back(c);
      }
      todo.swap(again);
      all = false;
    }
    if (!clean)
    {
      return fail(HRFD_ESTATE, "internal: exact replay still reports %zu failed channel(s)", todo.size());
    }
  }
  return HRFD_OK;
}

// The device part of hrfd_rx_process_block: d_iq [C][n_blocks][block_bytes] already on the device, PCM rows cleared;
// returns when every channel is exact.  *n_replayed (may be NULL): channels of batch launches that failed their
// speculation and were replayed (hrfd_ddc_receive runs the same flow on the DDC's output).
static int rx_run_batch(hrfd_rx *h, const int8_t *d_iq, uint32_t block_bytes, uint32_t n_blocks, uint32_t gain_db,
                        int16_t *d_pcm, uint32_t *d_npcm, uint32_t *d_mag, uint8_t *d_allowed, int8_t *d_iq256,
                        hipStream_t s, uint32_t *n_replayed)
{
  const uint32_t C = h->n_channels;
  int rc;
  uint32_t replayed = 0;
  const uint64_t stride = (uint64_t)block_bytes * n_blocks;
  uint32_t viol = 0;
  if (h->offgrid || (block_bytes % 1024u) != 0)
  {
    // any length: one launch of k_rx_ragged takes the whole call, block by block and exactly (rx_launch)
    if (d_iq256 != nullptr)
    {
      HIP_TRY(hipMemsetAsync(d_iq256, 0, (size_t)h->n_channels * n_blocks * 2u * ((block_bytes / 2u + 7u) / 8u), s));   // (a row is filled up to the call's own count)
    }
    const LaunchOpts opt = {n_blocks, 0, 0, 0};
    rc = rx_launch(h, d_iq, stride, block_bytes, n_blocks, gain_db, d_pcm, d_npcm, d_mag, d_allowed,
                   d_iq256, s, opt);
    if (rc != HRFD_OK) return rc;
    if ((rc = hrfd_rx_sync(h, &viol)) != HRFD_OK) return rc;
    if (viol != 0)
    {
      return fail(HRFD_ESTATE, "internal: the exact path reported %u uncommitted channel(s)", viol);
    }
  }
  else
  {
  // Round 6: a call of more than 64 blocks runs as CHUNKS of at most 64, one batch launch each (every chunk then has the
  // shapes a 64-block call has: the flow kernels for the FIR modes, and the gated pass on the device behind them -- until
  // round 5 a long call with closing gates went back to the host block by block: +6 ms for 64 channels x 80 blocks).  The
  // chunks follow each other on the stream; the host looks at every chunk's verdict before the next one starts, so a
  // channel that did not commit is replayed over ITS chunk's blocks from the state the chunk in front left.
  const bool batch_ok = (uint32_t)(kMaxHal + 64) * 16u <= block_bytes;
  for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64u)
  {
    const uint32_t nb = std::min(64u, n_blocks - b0);
    std::vector<uint32_t> redo;                            // channels to run on the exact per-block path
    const bool batch_ran = nb > 1 && batch_ok;
    if (batch_ran)
    {
      // the chunk in one launch, blocks of a channel in parallel (speculative)
      const LaunchOpts opt = {n_blocks, b0, 0, 0};
      rc = rx_launch(h, d_iq + (size_t)b0 * block_bytes, stride, block_bytes, nb, gain_db, d_pcm, d_npcm,
                     d_mag, d_allowed, d_iq256, s, opt);
      if (rc != HRFD_OK) return rc;
      if ((rc = hrfd_rx_sync(h, &viol)) != HRFD_OK) return rc;
      for (uint32_t c = 0; c < C && viol != 0; c++)
      {
        if (h->h_fail[c] != 0) redo.push_back(c);
      }
      replayed += (uint32_t)redo.size();
    }
    else
    {
      for (uint32_t c = 0; c < C; c++) redo.push_back(c);
    }
    if ((rc = rx_replay(h, redo, d_iq, stride, block_bytes, n_blocks, gain_db, d_pcm, d_npcm, d_mag,
                        d_allowed, d_iq256, s, !batch_ran, b0, nb)) != HRFD_OK)
    {
      return rc;
    }
  }
  }
  if (n_replayed != nullptr)
  {
    *n_replayed = replayed;
  }
  return HRFD_OK;
}

extern "C" int hrfd_rx_process_block(hrfd_rx *h, const int8_t *iq, uint32_t block_bytes,
                                     uint32_t n_blocks, uint32_t gain_db, int16_t *pcm,
                                     uint32_t *n_pcm, uint32_t *magnitude, uint8_t *signal_allowed,
                                     int8_t *iq256k_opt)
{
  if (h == nullptr || iq == nullptr || pcm == nullptr || n_pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_process_block: NULL argument");
  }
  if (block_bytes == 0 || (block_bytes & 1u) != 0 || block_bytes > HRFD_BLOCK_BYTES || n_blocks == 0)
  {
    return fail(HRFD_EINVAL, "block_bytes must be even, > 0 and <= %u, n_blocks > 0 (got %u, %u)", HRFD_BLOCK_BYTES,
                block_bytes, n_blocks);
  }
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t C = h->n_channels;
  const size_t units = (size_t)C * n_blocks;
  const uint32_t npcm = (block_bytes + 511u) / 512u;        // row lengths: hrfd_rx_pcm_capacity / hrfd_rx_iq256_capacity
  const uint32_t n256b = 2u * ((block_bytes / 2u + 7u) / 8u);
  const size_t iq_bytes = units * block_bytes;
  const size_t pcm_bytes = units * npcm * sizeof(int16_t);
  const size_t iq256_bytes = units * n256b;
  hipStream_t s = h->stream;
  int rc;
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = h->d_iq.grow_bytes(iq_bytes)) != HRFD_OK) return rc;
  if ((rc = h->d_pcm.grow_bytes(pcm_bytes)) != HRFD_OK) return rc;
  if (iq256k_opt != nullptr)
  {
    if ((rc = h->d_iq256.grow_bytes(iq256_bytes)) != HRFD_OK) return rc;
  }
  if ((rc = h->d_npcm.grow_bytes(units * 4)) != HRFD_OK) return rc;
  if ((rc = h->d_allowed.grow_bytes(units)) != HRFD_OK) return rc;
  if ((rc = h->d_mag_out.grow_bytes(units * 4)) != HRFD_OK) return rc;
  HIP_TRY(hipMemcpyAsync(h->d_iq, iq, iq_bytes, hipMemcpyHostToDevice, s));
  // mode NONE / squelched units produce no PCM: hand back zeros rather than stale bytes
  HIP_TRY(hipMemsetAsync(h->d_pcm, 0, pcm_bytes, s));

  if ((rc = rx_run_batch(h, h->d_iq, block_bytes, n_blocks, gain_db, h->d_pcm, h->d_npcm, h->d_mag_out, h->d_allowed,
                         iq256k_opt ? h->d_iq256 : nullptr, s, nullptr)) != HRFD_OK)
  {
    return rc;
  }
  HIP_TRY(hipMemcpyAsync(pcm, h->d_pcm, pcm_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(n_pcm, h->d_npcm, units * 4, hipMemcpyDeviceToHost, s));
  if (signal_allowed != nullptr)
  {
    HIP_TRY(hipMemcpyAsync(signal_allowed, h->d_allowed, units, hipMemcpyDeviceToHost, s));
  }
  if (magnitude != nullptr)
  {
    HIP_TRY(hipMemcpyAsync(magnitude, h->d_mag_out, units * 4, hipMemcpyDeviceToHost, s));
  }
  if (iq256k_opt != nullptr)
  {
    HIP_TRY(hipMemcpyAsync(iq256k_opt, h->d_iq256, iq256_bytes, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return HRFD_OK;
}

// IqDataProcessor::reduceSampleRate as a call of its own (IqDataProcessor.cc:429-500: public in the reference): the
// three half-band stages per rail over one block of every channel, the decimator pipelines advanced, nothing else --
// no squelch, no demodulator.  Here the front end only exists fused with the Fs/4 mixer and the squelch detector, so a
// mode-NONE block runs and the squelch tracker's state is put back afterwards; iq256k receives the MIXED stream
// (upconvertByFsOver4 applied: the caller takes it out again if it wants the reference's decimatedData).
extern "C" int hrfd_rx_reduce_sample_rate(hrfd_rx *h, const int8_t *iq, uint32_t block_bytes, int8_t *iq256k)
{
  if (h == nullptr || iq == nullptr || iq256k == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_reduce_sample_rate: NULL argument");
  }
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t C = h->n_channels;
  std::vector<int> modes(C);
  std::vector<uint32_t> tracking(C), npcm(C);
  std::vector<int16_t> pcm((size_t)C * (block_bytes / 512 + 2));
  {
    std::lock_guard<std::mutex> g(h->mu);
    for (uint32_t c = 0; c < C; c++)
    {
      modes[c] = h->h_cfg[c].mode;
      h->h_cfg[c].mode = HRFD_MODE_NONE;
    }
    h->cfg_dirty = true;
  }
  // (from here on every path puts the modes back)
  int rc = HRFD_OK;
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e == hipSuccess)
  {
    e = hipMemcpy2D(tracking.data(), sizeof(uint32_t), &h->d_state->tracking, sizeof(ChanState), sizeof(uint32_t), C, hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess)
  {
    rc = hrfd_rx_process_block(h, iq, block_bytes, 1, 0, pcm.data(), npcm.data(), nullptr, nullptr, iq256k);
    e = hipMemcpy2D(&h->d_state->tracking, sizeof(ChanState), tracking.data(), sizeof(uint32_t), sizeof(uint32_t), C, hipMemcpyHostToDevice);
  }
  {
    std::lock_guard<std::mutex> g(h->mu);
    for (uint32_t c = 0; c < C; c++)
    {
      h->h_cfg[c].mode = modes[c];
    }
    h->cfg_dirty = true;
  }
  if (e != hipSuccess)
  {
    return fail(HRFD_ENODEV, "hrfd_rx_reduce_sample_rate: %s", hipGetErrorString(e));
  }
  return rc;
}

// Row lengths of the outputs for a block length, and what the front end holds back between calls.
extern "C" uint32_t hrfd_rx_pcm_capacity(uint32_t block_bytes) { return (block_bytes + 511u) / 512u; }
extern "C" uint32_t hrfd_rx_iq256_capacity(uint32_t block_bytes) { return 2u * ((block_bytes / 2u + 7u) / 8u); }
extern "C" uint32_t hrfd_demod_pcm_capacity(uint32_t bytes_per_channel) { return (bytes_per_channel + 63u) / 64u; }

extern "C" int hrfd_rx_pending_samples(hrfd_rx *h, uint32_t *pending)
{
  if (h == nullptr || pending == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_rx_pending_samples: NULL argument");
  }
  *pending = 0;
  if (!h->rag_built)
  {
    return HRFD_OK;                                        // on the grid: every call ended on a whole 256 kS/s sample
  }
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->last_stream ? h->last_stream : h->stream;
  HIP_TRY(hipStreamSynchronize(s));
  uint32_t p = 0;
  HIP_TRY(hipMemcpy(&p, &h->d_rag->fe_phase, sizeof(p), hipMemcpyDeviceToHost));   // the same for every channel of the handle
  *pending = p & 7u;
  return HRFD_OK;
}

// ------------------------------------------------------------------ inner boundary
// hrfd_demod: n_channels instances of ONE demodulator class, fed with the
// 256 kS/s, already mixed, int8 IQ stream -- X::acceptIqData(int8_t*,uint32_t).
// Same kernels as the outer boundary, entered behind the front end (src256).
struct hrfd_demod
{
  hrfd_rx *rx = nullptr;
  int mode = 0;
};

extern "C" int hrfd_demod_create(int mode, uint32_t n_channels, int device, hrfd_demod **out)
{
  if (out == nullptr || mode < HRFD_MODE_AM || mode > HRFD_MODE_USB)
  {
    return fail(HRFD_EINVAL, "hrfd_demod_create: mode must be AM, FM, WBFM, LSB or USB");
  }
  *out = nullptr;
  hrfd_rx *rx = nullptr;
  int rc = hrfd_rx_create(n_channels, device, &rx);
  if (rc != HRFD_OK)
  {
    return rc;
  }
  rc = hrfd_rx_set_mode(rx, HRFD_ALL_CHANNELS, mode);
  if (rc != HRFD_OK)
  {
    rx_free(rx);
    return rc;
  }
  hrfd_demod *h = new hrfd_demod;
  h->rx = rx;
  h->mode = mode;
  *out = h;
  return HRFD_OK;
}

extern "C" int hrfd_demod_destroy(hrfd_demod *h)
{
  if (h != nullptr)
  {
    rx_free(h->rx);
    delete h;
  }
  return HRFD_OK;
}

extern "C" int hrfd_demod_reset(hrfd_demod *h, uint32_t channel)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  return hrfd_rx_reset_demod(h->rx, channel, h->mode);
}

extern "C" int hrfd_demod_set_gain(hrfd_demod *h, uint32_t channel, float gain)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  return hrfd_rx_set_gain(h->rx, channel, h->mode, gain);
}

extern "C" int hrfd_demod_set_sideband(hrfd_demod *h, uint32_t channel, int lsb)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  if (h->mode != HRFD_MODE_LSB && h->mode != HRFD_MODE_USB)
  {
    return fail(HRFD_ESTATE, "hrfd_demod_set_sideband: not an SSB demodulator");
  }
  // SsbDemodulator::set{Lsb,Usb}DemodulationMode (SsbDemodulator.cc): a flag, no state change
  return hrfd_rx_set_mode(h->rx, channel, lsb ? HRFD_MODE_LSB : HRFD_MODE_USB);
}

extern "C" int hrfd_demod_process(hrfd_demod *dh, const int8_t *iq256k, uint32_t bytes_per_channel,
                                  int16_t *pcm, uint32_t *n_pcm)
{
  if (dh == nullptr || iq256k == nullptr || pcm == nullptr)
  {
    return fail(HRFD_EINVAL, "hrfd_demod_process: NULL argument");
  }
  hrfd_rx *h = dh->rx;
  if (bytes_per_channel == 0 || (bytes_per_channel & 1u) != 0 || bytes_per_channel > 32768u)
  {
    return fail(HRFD_EINVAL, "hrfd_demod_process: bytes_per_channel must be even, > 0 and <= 32768 (got %u)", bytes_per_channel);
  }
  HIP_TRY(hipSetDevice(h->device));
  const uint32_t C = h->n_channels;
  const uint32_t npcm = (bytes_per_channel + 63u) / 64u;   // hrfd_demod_pcm_capacity
  const size_t iq_bytes = (size_t)C * bytes_per_channel;
  const size_t pcm_bytes = (size_t)C * npcm * sizeof(int16_t);
  hipStream_t s = h->stream;
  int rc;
  HIP_TRY(hipStreamSynchronize(s));
  if ((rc = h->d_iq.grow_bytes(iq_bytes)) != HRFD_OK) return rc;
  if ((rc = h->d_pcm.grow_bytes(pcm_bytes)) != HRFD_OK) return rc;
  if ((rc = h->d_npcm.grow_bytes((size_t)C * 4)) != HRFD_OK) return rc;
  HIP_TRY(hipMemsetAsync(h->d_pcm, 0, pcm_bytes, s));
  HIP_TRY(hipMemcpyAsync(h->d_iq, iq256k, iq_bytes, hipMemcpyHostToDevice, s));
  const LaunchOpts opt = {1, 0, 0, 1};
  rc = rx_launch(h, h->d_iq, bytes_per_channel, bytes_per_channel, 1, 0, h->d_pcm, h->d_npcm, nullptr,
                 nullptr, nullptr, s, opt);
  if (rc != HRFD_OK) return rc;
  uint32_t viol = 0;
  if ((rc = hrfd_rx_sync(h, &viol)) != HRFD_OK) return rc;
  if (viol != 0)
  {
    return fail(HRFD_ESTATE, "internal: single-block launch reported %u violations", viol);
  }
  HIP_TRY(hipMemcpyAsync(pcm, h->d_pcm, pcm_bytes, hipMemcpyDeviceToHost, s));
  if (n_pcm != nullptr)
  {
    HIP_TRY(hipMemcpyAsync(n_pcm, h->d_npcm, (size_t)C * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return HRFD_OK;
}
