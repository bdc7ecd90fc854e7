// hackrfdiags_amd/csrc/hrfd_api_tx.hip -- the transmit side of the C ABI (include/hrfd.h): hrfd_mod_* (the four modulators,
// interpolateSignal and the signals/ generators over k_mod and its baseband passes) and hrfd_nco_*.  Part of the unity
// translation unit hrfd_lib.hip, behind hrfd_api.hip (errors, HIP_TRY), hrfd_buf.h (DevBuf: the handles own their
// device buffers) and hrfd_bank.hip (BankCore: both handles sit on the banks' host core).
// hrfd_tx_slices.h holds what a launch decides without the device: the refusal, the time slices, the grids.
#include "hrfd_tx_slices.h"
static_assert(kTxTile == kModTile && kTxModThreads == kModThreads && kTxWtRun == kWtRun && kTxWtThreads == kWtThreads &&
              kTxWbRailsThreads == kWbRailsThreads, "hrfd_tx_slices.h restates the kernels' shapes");
// ------------------------------------------------------------------ transmit
#ifndef HRFD_WB_FUSED
#define HRFD_WB_FUSED 1                 // round 6: the WBFM modulator's lookup pass and x8 cascade as ONE kernel (k_wb_tail)
#endif
struct hrfd_mod
{
  BankCore core;                             // device, stream, the ordering rules; core.mu guards the host fields below
  int kind = 0;
  uint32_t n_channels = 0;
  DevBuf<int16_t> d_tail[2];                 // ping-pong: [C][4][kModTail]
  int cur = 0;
  DevBuf<uint8_t> d_lsb;
  std::vector<uint8_t> h_lsb;
  bool lsb_dirty = true;
  std::vector<uint32_t> resets;
  // AM / FM: per-channel parameter (modulation index / deviation), FM phase accumulators, and
  // the baseband rails of a call
  DevBuf<float> d_param, d_acc, d_phase;
  DevBuf<int16_t> d_rails;
  std::vector<float> h_param;
  bool param_dirty = true;
  // WBFM: the PCM at 256 kS/s, the step/phase/rails cells, Nco::runFast tables, rail history
  DevBuf<uint32_t> d_wb, d_wbtail[2];
  DevBuf<float> d_sin, d_cos;
  DevBuf<uint32_t> d_wbpack;            // the two tables x900 as int16 rail pairs (k_wb_rails)
  DevBuf<uint32_t> d_err;               // k_phase_scan: waits that expired (never, unless the kernel is broken)
  // WBFM: the call's passes run in time slices on three streams (mod_launch_wbfm)
  static constexpr int kMaxSlices = kTxMaxSlices;
  hipStream_t s_scan = nullptr, s_tail = nullptr;  // the recurrence's stream; the stream of every other pass of a sliced call
  bool cu_masked = false;               // the recurrence's stream has CUs of its own
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_head[kMaxSlices] = {}, ev_scan[kMaxSlices] = {};
  int sliced = 1;                        // test hook: 0 = one pass after the other on the caller's stream
  int scan_kind = 0;                     // test hook: 1 = k_phase_scan<64> / k_phase_scan_plain whatever the bank size, 2 = k_phase_rows (four steps per lane) where k_phase_rows8 would run
  int wb_fused = HRFD_WB_FUSED;          // test hook: 0 = the lookup pass and the x8 cascade as two kernels (rounds 2-5), 1 = k_wb_tail
  // staging for the host entry
  DevBuf<int16_t> d_in;
  DevBuf<int8_t> d_out;
};

// create's failure path and destroy: the modulator's own streams and events, then the core and the handle (bank_free)
static void mod_free(hrfd_mod *h)
{
  (void)hipSetDevice(h->core.device);
  (void)h->core.drain();                                   // (a sliced call's streams wait for each other's events)
  for (hipStream_t st : {h->s_scan, h->s_tail})
  {
    if (st)
    {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
    }
  }
  for (hipEvent_t e : {h->ev_fork, h->ev_join})
  {
    if (e) (void)hipEventDestroy(e);
  }
  for (int i = 0; i < hrfd_mod::kMaxSlices; i++)
  {
    if (h->ev_head[i]) (void)hipEventDestroy(h->ev_head[i]);
    if (h->ev_scan[i]) (void)hipEventDestroy(h->ev_scan[i]);
  }
  bank_free(h);
}

// Which build of glibc's sinf / cosf does this host run?  x86-64 glibc dispatches between a plain and an -mfma build of
// the same source; they differ on 34 floats with |x| < 120 (all above 17: tools/proofs/sincosf_glibc.c).  1: the fused
// build (what an FMA-capable CPU gets), 0: the plain one.  The device restates that one (glibc_sinf / glibc_cosf).
// MEASURED AND SWITCHED OFF: the FM modulator's cos / sin pass (k_fm_rails) as part of the cascade's stage-0 load
// (k_mod<FM_PHASE>: VERDICT round 4, item 5).  Bit-exact, but 0.958 ms against 0.940 for the pass on the second stream
// (profiles/r5_fmmod_fused_ab_LOSES.txt, alternating runs): a tile also makes the rails of the 64 samples of history in
// front of it, so every cos / sin is evaluated twice, and in the cascade's own waves instead of beside them.
#ifndef HRFD_FM_FUSED
#define HRFD_FM_FUSED 0
#endif
// Which build of glibc's sinf / cosf the host's libm is (glibc_sincosf on the device follows it, hrfd_tx_kernels.hip):
// 1 = the -mfma build x86-64 glibc dispatches to on an FMA-capable CPU, 0 = without fused multiply-adds, -1 = neither
// (a libm that is not glibc's, another architecture's): the device then follows the FMA build and the outputs that go
// through cosf / sinf in the reference (FM modulator, Nco::run, pm / fm generators) may differ from THAT host's libm by
// +-1 LSB -- visible through hrfd_libm_variant() (bench.py prints it, the tests key their tolerance on it).  Probed once.
static int libm_probe()
{
  static const int v = [] {
    auto f = [](uint32_t u) { float x; memcpy(&x, &u, 4); return x; };
    auto b = [](float x) { uint32_t u; memcpy(&u, &x, 4); return u; };
    volatile float x1 = f(0x418a3adbu), x2 = f(0x4255b0a9u);
    const uint32_t c = b(cosf(x1)), s = b(sinf(x2));
    if (c == 0xb7b4f770u && s == 0xbc7d08a9u) return 1;
    if (c == 0xb7b4f76fu && s == 0xbc7d08a8u) return 0;
    return -1;
  }();
  return v;
}
static int libm_variant()
{
  const int v = libm_probe();
  return v < 0 ? 1 : v;
}
extern "C" int hrfd_libm_variant(void)
{
  return libm_probe();
}

// Nco.cc:50-61: the 16384-entry tables from a float angle accumulated by float increments; sin / cos of a float argument
// are sinf / cosf under the C++ overloads -> host libm
static void nco_tables(std::vector<float> &st, std::vector<float> &ct)
{
  st.resize(16384);
  ct.resize(16384);
  const float inc = (float)(2 * M_PI / 16384);
  float ang = (float)(-M_PI);
  for (int i = 0; i < 16384; i++)
  {
    st[i] = sinf(ang);
    ct[i] = cosf(ang);
    ang += inc;
  }
}

extern "C" int hrfd_mod_create(int kind, uint32_t n_channels, int device, hrfd_mod **out)
{
  if (out == nullptr || n_channels == 0 ||
      kind < HRFD_MOD_SSB || kind > HRFD_MOD_SIG_FM)
  {
    return fail(HRFD_EINVAL, "hrfd_mod_create: kind must be HRFD_MOD_SSB, _INTERP, _AM, _FM, _WBFM or _SIG_*, n_channels > 0");
  }
  *out = nullptr;
  hrfd_mod *h = nullptr;
  BANK_TRY(bank_new("hrfd_mod_create", device, &h));
  device = h->core.device;
  h->kind = kind;
  h->n_channels = n_channels;
  h->h_lsb.assign(n_channels, 1);                        // SsbModulator starts in LSB (SsbModulator.cc ctor)
  const size_t tail_bytes = (size_t)n_channels * 4 * kModTail * sizeof(int16_t);
  hipError_t e = hipSuccess;
  auto alloc = [&e](auto &buf, size_t n) {
    if (e == hipSuccess && !buf.alloc(n)) e = hipErrorOutOfMemory;
  };
  alloc(h->d_tail[0], tail_bytes / sizeof(int16_t));
  alloc(h->d_tail[1], tail_bytes / sizeof(int16_t));
  alloc(h->d_lsb, n_channels);
  if (e == hipSuccess) e = hipMemset(h->d_tail[0], 0, tail_bytes);   // zero pipelines == resetModulator()
  if (e == hipSuccess) e = hipMemset(h->d_tail[1], 0, tail_bytes);
  // AmModulator.cc:218 modulationIndex = 0.8; FmModulator.cc:218 frequencyDeviation = 3500, Nco phase 0
  // WbFmModulator.cc:204 frequencyDeviation = 70000
  h->h_param.assign(n_channels, kind == HRFD_MOD_FM ? 3500.0f : kind == HRFD_MOD_WBFM ? 70000.0f : (float)0.8);
  alloc(h->d_param, n_channels);
  alloc(h->d_acc, n_channels);
  if (e == hipSuccess) e = hipMemset(h->d_acc, 0, sizeof(float) * n_channels);
  // [0] waits that expired; [1], [2] counters of the -DHRFD_PS_PROBE diagnostic build of k_phase_scan
  alloc(h->d_err, 3);
  if (e == hipSuccess) e = hipMemset(h->d_err, 0, 3 * sizeof(uint32_t));
  if (kind == HRFD_MOD_WBFM)
  {
    std::vector<float> st, ct;
    nco_tables(st, ct);
    alloc(h->d_sin, 16384);
    alloc(h->d_cos, 16384);
    if (e == hipSuccess) e = hipMemcpy(h->d_sin, st.data(), sizeof(float) * 16384, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_cos, ct.data(), sizeof(float) * 16384, hipMemcpyHostToDevice);
    // WbFmModulator.cc:604-612: iv = cos * 900 (float), (int16_t) -- per table entry instead of per sample
    std::vector<uint32_t> pack(16384);
    for (int i = 0; i < 16384; i++)
    {
      volatile float iv = ct[i] * 900.0f, qv = st[i] * 900.0f;
      pack[i] = ((uint32_t)(int)(short)(int)iv & 0xffffu) | ((uint32_t)(int)(short)(int)qv << 16);
    }
    alloc(h->d_wbpack, 16384);
    if (e == hipSuccess) e = hipMemcpy(h->d_wbpack, pack.data(), sizeof(uint32_t) * 16384, hipMemcpyHostToDevice);
    for (int k = 0; k < 2; k++)
    {
      alloc(h->d_wbtail[k], (size_t)2 * n_channels);
      if (e == hipSuccess) e = hipMemset(h->d_wbtail[k], 0, sizeof(uint32_t) * 2 * n_channels);
    }
    // The phase recurrence runs one workgroup per 16 channels, one per CU, and every step of it is latency: a
    // workgroup of another kernel on the same CU slows it (measured: 276 -> 330..500 us per slice).  When the
    // recurrence needs at most half of the chip its stream gets CUs of its own and the other streams the rest
    // (hipExtStreamCreateWithCUMask; bit i of the mask = CU i, dealt round-robin over the XCDs by the driver).
    if (e == hipSuccess)
    {
      int cus = 0;
      (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
      const uint32_t scan_wgs = (n_channels + 15u) / 16u;
      const uint32_t want = (scan_wgs + 7u) / 8u * 8u;
      bool masked = false;
      if (cus >= 64 && cus <= 1024 && n_channels <= 4096u && want * 2u <= (uint32_t)cus)
      {
        const uint32_t words = ((uint32_t)cus + 31u) / 32u;
        std::vector<uint32_t> scan_mask(words, 0u), rest_mask(words, 0u);
        for (uint32_t i = 0; i < (uint32_t)cus; i++)
        {
          (i < want ? scan_mask : rest_mask)[i / 32] |= 1u << (i % 32);
        }
        hipStream_t a = nullptr, b = nullptr;
        if (hipExtStreamCreateWithCUMask(&a, words, scan_mask.data()) == hipSuccess &&
            hipExtStreamCreateWithCUMask(&b, words, rest_mask.data()) == hipSuccess)
        {
          h->s_scan = a;
          h->s_tail = b;
          masked = true;
        }
        else
        {
          (void)hipGetLastError();
          if (a) (void)hipStreamDestroy(a);
          if (b) (void)hipStreamDestroy(b);
        }
      }
      if (!masked)
      {
        e = hipStreamCreateWithFlags(&h->s_scan, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->s_tail, hipStreamNonBlocking);
      }
      h->cu_masked = masked;
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
    for (int k = 0; k < hrfd_mod::kMaxSlices && e == hipSuccess; k++)
    {
      e = hipEventCreateWithFlags(&h->ev_head[k], hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_scan[k], hipEventDisableTiming);
    }
  }
  if (kind == HRFD_MOD_FM)
  {
    // The FM modulator's 8 kS/s phase recurrence (8192 serial steps per 16-block call: ~0.14 ms whatever the bank) runs
    // slice by slice on a stream of its own BESIDE the x256 cascade of the slice in front (mod_launch_fm).  That
    // stream has the device's highest priority: the recurrence is one wave per workgroup running a dependent chain, and
    // among the cascade's thousands of workgroups it is served last and takes twice its time (measured: 108 us instead of
    // 49 for a 36-tile slice, the cascade then waits for it); with priority it runs at the rate it has alone.  (A
    // priority level also has hardware queues of its own: the stream cannot end up sharing one with the caller's stream,
    // where the two would run in submission order.)
    int lo_prio = 0, hi_prio = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
    if (e == hipSuccess && hipStreamCreateWithPriority(&h->s_scan, hipStreamNonBlocking, hi_prio) != hipSuccess)
    {
      (void)hipGetLastError();
      h->s_scan = nullptr;                                 // (no second stream: the call runs unsliced)
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    for (int k = 0; k < 4 && e == hipSuccess; k++)
    {
      e = hipEventCreateWithFlags(&h->ev_scan[k], hipEventDisableTiming);
    }
  }
  if (e != hipSuccess)
  {
    const int rc = fail(HRFD_ENOMEM, "hrfd_mod_create: %s", hipGetErrorString(e));
    mod_free(h);
    return rc;
  }
  *out = h;
  return HRFD_OK;
}

extern "C" int hrfd_mod_destroy(hrfd_mod *h)
{
  if (h != nullptr)
  {
    mod_free(h);
  }
  return HRFD_OK;
}

extern "C" int hrfd_mod_reset(hrfd_mod *h, uint32_t channel)
{
  if (h == nullptr || (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels))
  {
    return fail(HRFD_EINVAL, "hrfd_mod_reset: bad handle or channel");
  }
  std::lock_guard<std::mutex> g(h->core.mu);
  h->resets.push_back(channel);
  return HRFD_OK;
}

extern "C" int hrfd_mod_set_sideband(hrfd_mod *h, uint32_t channel, int lsb)
{
  if (h == nullptr || (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels))
  {
    return fail(HRFD_EINVAL, "hrfd_mod_set_sideband: bad handle or channel");
  }
  std::lock_guard<std::mutex> g(h->core.mu);
  bank_each_selected(h->n_channels, channel, [&](uint32_t c) { h->h_lsb[c] = lsb ? 1 : 0; });
  h->lsb_dirty = true;
  return HRFD_OK;
}

// AmModulator::setModulationIndex (AmModulator.cc:329-336): accepted when 0 <= index <= 1
extern "C" int hrfd_mod_set_modulation_index(hrfd_mod *h, uint32_t channel, float index)
{
  if (h == nullptr || h->kind != HRFD_MOD_AM || (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels))
  {
    return fail(HRFD_EINVAL, "hrfd_mod_set_modulation_index: needs an AM modulator handle and a valid channel");
  }
  std::lock_guard<std::mutex> g(h->core.mu);
  bank_each_selected(h->n_channels, channel, [&](uint32_t c) {
    if ((index >= 0) && (index <= 1)) h->h_param[c] = index;
  });
  h->param_dirty = true;
  return HRFD_OK;
}

// FmModulator::setFrequencyDeviation (FmModulator.cc:336-346).  As in the reference the range
// test looks at the CURRENT deviation, not at the new one (kept: it is the observable behaviour).
extern "C" int hrfd_mod_set_deviation(hrfd_mod *h, uint32_t channel, float deviation)
{
  if (h == nullptr || (h->kind != HRFD_MOD_FM && h->kind != HRFD_MOD_WBFM) ||
      (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels))
  {
    return fail(HRFD_EINVAL, "hrfd_mod_set_deviation: needs an FM or WBFM modulator handle and a valid channel");
  }
  const float limit = (h->kind == HRFD_MOD_FM) ? 3500.0f : 112000.0f;   // WbFmModulator.cc:313
  std::lock_guard<std::mutex> g(h->core.mu);
  bank_each_selected(h->n_channels, channel, [&](uint32_t c) {
    if ((h->h_param[c] >= 0) && (h->h_param[c] <= limit)) h->h_param[c] = deviation;
  });
  h->param_dirty = true;
  return HRFD_OK;
}

// ------------------------------------------------------------------ the launch
// One call of hrfd_mod_process_device: its arguments, and the handle's host fields as they were under core.mu.
struct ModCall
{
  hrfd_mod *h;
  const int16_t *pcm;
  int8_t *out;
  uint32_t n;                                // samples per channel
  hipStream_t s;
  int cur, sliced, scan_kind, wb_fused;
};

// the cascade's parameters over the whole call, reading `in`
static ModParams mod_params(const ModCall &c, const int16_t *in)
{
  const hrfd_mod *h = c.h;
  ModParams M;
  M.in = in;
  M.out = c.out;
  M.tail_in = h->d_tail[c.cur];
  M.tail_out = h->d_tail[c.cur ^ 1];
  M.lsb = h->d_lsb;
  M.wbstep = h->d_wb;
  M.param = h->d_param;
  M.wbtail = h->d_wbtail[c.cur];
  M.n = c.n;
  M.n_channels = h->n_channels;
  M.libm_fma = libm_variant();
  M.tile0 = 0;
  M.tiles_launch = 0;
  return M;
}

// the baseband passes' parameters over the whole call (a buffer the kind does not have is NULL, and not read)
static BaseParams base_params(const ModCall &c)
{
  const hrfd_mod *h = c.h;
  BaseParams B;
  memset(&B, 0, sizeof(B));
  B.pcm = c.pcm;
  B.rails = h->d_rails;
  B.param = h->d_param;
  B.acc = h->d_acc;
  B.phase = h->d_phase;
  B.wb = h->d_wb;
  B.cos_t = h->d_cos;
  B.sin_t = h->d_sin;
  B.wbpack = h->d_wbpack;
  B.wbtail_out = h->d_wbtail[c.cur ^ 1];
  B.n = c.n;
  B.n_channels = h->n_channels;
  B.libm_fma = libm_variant();
  return B;
}

// k_mod<KIND> over the slice [lo, lo + len) of every channel (len 0: the whole call)
template <int KIND>
static int mod_cascade(const ModParams &M0, uint32_t lo, uint32_t len, hipStream_t s)
{
  ModParams M = M0;
  if (len != 0u)
  {
    M.tile0 = lo / kModTile;
    M.tiles_launch = tx_tiles(len);
  }
  hipLaunchKernelGGL(k_mod<KIND>, dim3(tx_mod_grid(M.n_channels, len != 0u ? len : M.n)), dim3(kModThreads), 0, s, M);
  return bank_launch_ok("k_mod");
}

// a baseband pass, one thread per sample of the whole call
static int base_pass(const char *name, void (*kernel)(const BaseParams), const BaseParams &B, hipStream_t s)
{
  hipLaunchKernelGGL(kernel, dim3(tx_base_grid(B.n_channels, B.n)), dim3(256), 0, s, B);
  return bank_launch_ok(name);
}

// the WBFM modulator's last pass over the slice [lo, lo + len) of every channel (len 0: the whole call): Nco::runFast's
// lookup and stages 6-8 of the cascade in ONE kernel (k_wb_tail, round 6) -- or round 5's two, k_wb_rails in place over the
// phases and k_mod<WB_TAIL> (wb_fused == 0: the A/B and the tests that run both)
static int wb_tail_launch(const ModCall &c, const BaseParams &B0, const ModParams &T, uint32_t lo, uint32_t len, uint32_t max_wgs, hipStream_t s)
{
  const uint32_t C = B0.n_channels, span = (len != 0u) ? len : B0.n;
  if (c.wb_fused != 0)
  {
    WbTailParams P;
    P.cells = c.h->d_wb;
    P.out = T.out;
    P.wbpack = c.h->d_wbpack;
    P.wbtail = T.wbtail;
    P.wbtail_out = B0.wbtail_out;
    P.n = B0.n;
    P.n_channels = C;
    P.lo = lo;
    P.len = len;
    hipLaunchKernelGGL(k_wb_tail, dim3(tx_wb_tail_grid(C, span, max_wgs)), dim3(kWtThreads), 0, s, P);
    return bank_launch_ok("k_wb_tail");
  }
  BaseParams B = B0;
  B.lo = lo;
  B.len = len;
  hipLaunchKernelGGL(k_wb_rails, dim3(tx_wb_rails_grid(C, span, max_wgs)), dim3(kWbRailsThreads), 0, s, B);   // (two workgroups per CU: the 64 KiB table)
  BANK_TRY(bank_launch_ok("k_wb_rails"));
  return mod_cascade<HRFD_MOD_WB_TAIL>(T, lo, len, s);
}

// the Nco phase recurrence over `steps` cells per channel, rows `row_stride` cells apart, on the kernel tx_scan_kernel names
static int phase_scan(const ModCall &c, uint32_t *cells, size_t steps, size_t row_stride, hipStream_t s)
{
  const uint32_t C = c.h->n_channels;
  float *acc = c.h->d_acc;
  const TxScan k = tx_scan_kernel(c.scan_kind, C, steps, row_stride);
  const dim3 grid(tx_scan_grid(k, C));
  switch (k)
  {
  case kTxScanRows8: hipLaunchKernelGGL(k_phase_rows8, grid, dim3(kPrThreads), 0, s, cells, steps, row_stride, acc, C); break;
  case kTxScanRows: hipLaunchKernelGGL(k_phase_rows, grid, dim3(kPrThreads), 0, s, cells, steps, row_stride, acc, C); break;
  case kTxScan64: hipLaunchKernelGGL(k_phase_scan<64>, grid, dim3(kPsThreads), 0, s, cells, steps, row_stride, acc, C, c.h->d_err.p); break;
  default: hipLaunchKernelGGL(k_phase_scan_plain, grid, dim3(64), 0, s, cells, steps, row_stride, acc, C); break;
  }
  return bank_launch_ok("the phase recurrence (k_phase_rows / k_phase_scan)");
}

// WbFmModulator::acceptData (WbFmModulator.cc:341-356): x32 on the PCM, the 256 kS/s Nco, x8
static int mod_launch_wbfm(const ModCall &c)
{
  hrfd_mod *h = c.h;
  const hipStream_t s = c.s;
  const size_t n32 = (size_t)c.n * 32;
  // (Cutting the bank into groups of channels on streams of their own buys nothing: the recurrence's time does not
  // depend on the number of channels, so every group's recurrence runs at the same time and the per-sample passes
  // still queue up in front of and behind it -- measured, 8.8 ms either way for 1024 channels.)
  const BaseParams B = base_params(c);
  const ModParams H = mod_params(c, c.pcm);                  // (k_mod<WB_HEAD> reads the PCM itself)
  const ModParams T = mod_params(c, reinterpret_cast<const int16_t *>(h->d_wb.p));
  // The passes run in TIME SLICES of whole blocks (512 PCM samples), on three streams: the x32 cascade with the Nco
  // steps (k_mod<WB_HEAD>) on the caller's, the phase recurrence -- serial per channel, the same 17 ns per step for
  // 64 channels as for 4096, two thirds of the call -- on one of the handle's, the table lookup and the x8 cascade
  // (k_wb_rails, k_mod<WB_TAIL>) on another: slice t's rails and tail run beside the recurrence of slice t + 1, so
  // the call costs little more than the recurrence alone.  (WbFmModulator.cc:583-637 does the three per sample.)
  // slice boundaries (input samples, multiples of the cascade's tile): a short first slice (the recurrence starts
  // behind its head pass), short last ones (what is left behind the last recurrence is one slice's rails and
  // tail), long ones between (every slice costs the recurrence a launch: ~12 us) -- tx_wbfm_cuts
  uint32_t cuts[hrfd_mod::kMaxSlices];
  const int n_cuts = tx_wbfm_cuts(c.n, hrfd_mod::kMaxSlices, cuts);
  // (only when the recurrence has CUs of its own: beside other kernels on its CUs it loses more than the overlap gains)
  if (!(c.sliced != 0 && n_cuts > 1 && h->s_scan != nullptr && (h->cu_masked || c.sliced > 1)))
  {
    BANK_TRY(mod_cascade<HRFD_MOD_WB_HEAD>(H, 0u, 0u, s));
    BANK_TRY(phase_scan(c, h->d_wb, n32, n32, s));
    return wb_tail_launch(c, B, T, 0u, 0u, 512u, s);
  }
  // Two streams of the handle's own: the recurrences on one (with CUs of its own), every other pass on the second.
  // The caller's stream only forks and joins (it may share its hardware queue with either: when it carried
  // kernels, everything ran in series).  The head passes of all slices go out first -- they depend on nothing but
  // the input -- and the rails and tails of the first slices queue up behind them: those have a millisecond of
  // slack, and every stream with a CU mask is a hardware queue of its own, of which a process should hold few
  // (measured: the same call takes 4.7 ms in a process with five queues and 5.2 with seven).
  HIP_TRY(hipEventRecord(h->ev_fork, s));
  HIP_TRY(hipStreamWaitEvent(h->s_tail, h->ev_fork, 0));
  HIP_TRY(hipStreamWaitEvent(h->s_scan, h->ev_fork, 0));
  for (int k = 0; k < n_cuts; k++)
  {
    const uint32_t lo = (k == 0) ? 0u : cuts[k - 1];
    BANK_TRY(mod_cascade<HRFD_MOD_WB_HEAD>(H, lo, cuts[k] - lo, h->s_tail));
    HIP_TRY(hipEventRecord(h->ev_head[k], h->s_tail));
  }
  for (int k = 0; k < n_cuts; k++)
  {
    const uint32_t lo = (k == 0) ? 0u : cuts[k - 1], len = cuts[k] - lo;
    // (the head passes are through long before the fourth recurrence starts: it waits for the last of them, the
    // ones behind it for nothing -- every wait is a packet the queue takes microseconds over)
    if (k <= 3)
    {
      HIP_TRY(hipStreamWaitEvent(h->s_scan, h->ev_head[k < 3 ? k : n_cuts - 1], 0));
    }
    BANK_TRY(phase_scan(c, h->d_wb + (size_t)lo * 32, (size_t)len * 32, n32, h->s_scan));
    HIP_TRY(hipEventRecord(h->ev_scan[k], h->s_scan));
    HIP_TRY(hipStreamWaitEvent(h->s_tail, h->ev_scan[k], 0));
    BANK_TRY(wb_tail_launch(c, B, T, lo, len, 384u, h->s_tail));
  }
  HIP_TRY(hipEventRecord(h->ev_join, h->s_tail));
  HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
  return HRFD_OK;
}

// FmModulator::modulateSignal (FmModulator.cc:586-627) sets the Nco's frequency and runs it once per PCM sample: the
// step of every sample in parallel (k_fm_step), the phase recurrence (serial per channel: k_phase_scan), cos / sin of
// every phase in parallel (k_fm_rails), then the cascade.  Only the recurrence is serial in time, and it is a quarter
// of the cascade's time per sample: a long call is cut into three TIME SLICES and the recurrence and rails of slice
// k + 1 run on a stream of their own beside the cascade of slice k.  What stays exposed is the first slice's
// recurrence and rails.  (Round 3 ran the four passes one after the other: the recurrence's 0.14 ms and the rails'
// 0.04 sat in front of the cascade's 0.81.)
static int mod_launch_fm(const ModCall &c)
{
  hrfd_mod *h = c.h;
  const hipStream_t s = c.s;
  BaseParams B = base_params(c);
  uint32_t *const phase = reinterpret_cast<uint32_t *>(h->d_phase.p);
  // (round 5, HRFD_FM_FUSED: cos / sin, x 16000 and the narrowing happen in the cascade's stage-0 load -- k_mod<FM_PHASE>
  //  reads the phases; otherwise a pass of its own, k_fm_rails, in front)
  constexpr int kCascade = HRFD_FM_FUSED ? HRFD_MOD_FM_PHASE : HRFD_MOD_RAILS;
  const ModParams M = mod_params(c, HRFD_FM_FUSED ? reinterpret_cast<const int16_t *>(h->d_phase.p) : h->d_rails.p);
  BANK_TRY(base_pass("k_fm_step", k_fm_step, B, s));
  if (!(c.sliced != 0 && tx_fm_sliceable(c.n) && h->s_scan != nullptr))
  {
    BANK_TRY(phase_scan(c, phase, c.n, c.n, s));
#if !HRFD_FM_FUSED
    BANK_TRY(base_pass("k_fm_rails", k_fm_rails, B, s));
#endif
    return mod_cascade<kCascade>(M, 0u, 0u, s);
  }
  // The recurrences and rails of ALL slices follow each other on s_scan; the caller's stream carries the steps and the
  // cascade launches, each behind its slice's event.  Order matters more than priority here: a recurrence workgroup is
  // seven waves, a cascade workgroup four, and once a cascade launch has filled the CUs the slots it frees are retaken four
  // waves at a time -- the recurrence launched BEHIND a cascade launch waits for room and takes twice its time (measured:
  // 108 us for a 36-tile slice instead of 49, whatever the stream's priority).  This way slice k + 1's recurrence is
  // resident before the cascade of slice k starts (its event takes ~13 us to cross queues): timeline of a step in
  // profiles/r4_fmmod_timeline.txt.  Exposed: two event hops, the first slice's recurrence and rails.
  uint32_t cut[4];
  tx_fm_cuts(c.n, cut);
  HIP_TRY(hipEventRecord(h->ev_fork, s));
  HIP_TRY(hipStreamWaitEvent(h->s_scan, h->ev_fork, 0));
  for (int k = 0; k < 3; k++)
  {
    // (the slices' recurrences follow each other in stream order: the accumulators carry over in d_acc)
    B.lo = cut[k];
    B.len = cut[k + 1] - cut[k];
    BANK_TRY(phase_scan(c, phase + B.lo, (size_t)B.len, (size_t)c.n, h->s_scan));
#if !HRFD_FM_FUSED
    hipLaunchKernelGGL(k_fm_rails, dim3(tx_base_grid(B.n_channels, B.len)), dim3(256), 0, h->s_scan, B);
    BANK_TRY(bank_launch_ok("k_fm_rails"));
#endif
    HIP_TRY(hipEventRecord(h->ev_scan[k], h->s_scan));
  }
  for (int k = 0; k < 3; k++)
  {
    HIP_TRY(hipStreamWaitEvent(s, h->ev_scan[k], 0));
    BANK_TRY(mod_cascade<kCascade>(M, cut[k], cut[k + 1] - cut[k], s));
  }
  return HRFD_OK;
}

// AmModulator::modulateSignal: the baseband rails first (k_am_rails), then the shared x256 cascade
static int mod_launch_am(const ModCall &c)
{
  BANK_TRY(base_pass("k_am_rails", k_am_rails, base_params(c), c.s));
  return mod_cascade<HRFD_MOD_RAILS>(mod_params(c, c.h->d_rails), 0u, 0u, c.s);
}

// signals/{am,dsb,pm,fm}.cc | interpolateSignal: baseband pairs, then the x256 cascade with interpolateSignal's own
// stage-1 table
static int mod_launch_sig(const ModCall &c)
{
  const BaseParams B = base_params(c);
  if (c.h->kind == HRFD_MOD_SIG_FM)
  {
    hipLaunchKernelGGL(k_sig_fm, dim3((B.n_channels + 63) / 64), dim3(64), 0, c.s, B);
    BANK_TRY(bank_launch_ok("k_sig_fm"));
  }
  else
  {
    static void (*const rails[3])(const BaseParams) = {k_sig_rails<HRFD_MOD_SIG_AM>, k_sig_rails<HRFD_MOD_SIG_DSB>,
                                                       k_sig_rails<HRFD_MOD_SIG_PM>};
    BANK_TRY(base_pass("k_sig_rails", rails[c.h->kind - HRFD_MOD_SIG_AM], B, c.s));
  }
  return mod_cascade<HRFD_MOD_INTERP>(mod_params(c, c.h->d_rails), 0u, 0u, c.s);
}

// Rule 3 for a launch on `s`: the scratch of a call grows, and a setter's values go up, only when nothing of the handle runs
// any more -- on `s`, on the handle's stream or on the last launch's.  First use and the call behind a setter only.
static int mod_quiesce(hrfd_mod *h, hipStream_t s)
{
  HIP_TRY(hipStreamSynchronize(s));
  return h->core.drain();
}

// under core.mu, in front of the launches on `s`: room for the call's scratch, the setters' values, the resets
static int mod_prepare(hrfd_mod *h, uint32_t n, hipStream_t s)
{
  const size_t bytes = (size_t)n * h->n_channels * 4;      // a 4-byte cell per sample; the WBFM modulator's per 256 kS/s sample
  const bool rails = h->kind == HRFD_MOD_AM || h->kind == HRFD_MOD_FM || h->kind >= HRFD_MOD_SIG_AM;
  const size_t need_wb = h->kind == HRFD_MOD_WBFM ? bytes * 32 : 0, need_rails = rails ? bytes : 0,
               need_phase = h->kind == HRFD_MOD_FM ? bytes : 0;
  const bool grow = need_wb > h->d_wb.cap || need_rails > h->d_rails.cap || need_phase > h->d_phase.cap;
  if (grow || h->lsb_dirty || h->param_dirty)
  {
    BANK_TRY(mod_quiesce(h, s));
  }
  if (need_wb > h->d_wb.cap) BANK_TRY(h->d_wb.grow_bytes(need_wb));
  if (need_rails > h->d_rails.cap) BANK_TRY(h->d_rails.grow_bytes(need_rails));
  if (need_phase > h->d_phase.cap) BANK_TRY(h->d_phase.grow_bytes(need_phase));
  if (h->lsb_dirty)
  {
    HIP_TRY(hipMemcpy(h->d_lsb, h->h_lsb.data(), h->n_channels, hipMemcpyHostToDevice));
    h->lsb_dirty = false;
  }
  if (h->param_dirty)
  {
    HIP_TRY(hipMemcpy(h->d_param, h->h_param.data(), sizeof(float) * h->n_channels, hipMemcpyHostToDevice));
    h->param_dirty = false;
  }
  for (uint32_t ch : h->resets)
  {
    // SsbModulator::resetModulator: every pipeline back to zero
    const size_t first = (ch == HRFD_ALL_CHANNELS) ? 0 : ch, count = (ch == HRFD_ALL_CHANNELS) ? h->n_channels : 1;
    HIP_TRY(hipMemsetAsync(h->d_tail[h->cur] + first * 4 * kModTail, 0, count * 4 * kModTail * sizeof(int16_t), s));
    if (h->kind == HRFD_MOD_WBFM) HIP_TRY(hipMemsetAsync(h->d_wbtail[h->cur] + first * 2, 0, count * 8, s));
    if (h->kind == HRFD_MOD_SIG_FM) HIP_TRY(hipMemsetAsync(h->d_acc + first, 0, count * sizeof(float), s));   // a fresh run of the tool
  }
  h->resets.clear();
  return HRFD_OK;
}

extern "C" int hrfd_mod_process_device(hrfd_mod *h, const int16_t *d_pcm, uint32_t n_per_channel,
                                       int8_t *d_iq_out, void *stream)
{
  if (h == nullptr || d_pcm == nullptr || d_iq_out == nullptr || n_per_channel == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_mod_process_device: NULL argument or n_per_channel == 0");
  }
  BANK_TRY(tx_check_call("hrfd_mod_process_device", h->kind, h->n_channels, n_per_channel));
  HIP_TRY(hipSetDevice(h->core.device));
  ModCall c{h, d_pcm, d_iq_out, n_per_channel, h->core.stream_or_own(stream), 0, 0, 0, 0};
  BANK_TRY(h->core.order_behind_last(c.s));
  {
    std::lock_guard<std::mutex> g(h->core.mu);
    BANK_TRY(mod_prepare(h, n_per_channel, c.s));
    c.cur = h->cur;
    c.sliced = h->sliced;
    c.scan_kind = h->scan_kind;
    c.wb_fused = h->wb_fused;
  }
  switch (h->kind)
  {
  case HRFD_MOD_SSB: BANK_TRY(mod_cascade<HRFD_MOD_SSB>(mod_params(c, d_pcm), 0u, 0u, c.s)); break;
  case HRFD_MOD_INTERP: BANK_TRY(mod_cascade<HRFD_MOD_INTERP>(mod_params(c, d_pcm), 0u, 0u, c.s)); break;
  case HRFD_MOD_AM: BANK_TRY(mod_launch_am(c)); break;
  case HRFD_MOD_FM: BANK_TRY(mod_launch_fm(c)); break;
  case HRFD_MOD_WBFM: BANK_TRY(mod_launch_wbfm(c)); break;
  default: BANK_TRY(mod_launch_sig(c)); break;
  }
  {
    std::lock_guard<std::mutex> g(h->core.mu);
    h->cur ^= 1;
  }
  h->core.launched_on(c.s);
  return HRFD_OK;
}

extern "C" int hrfd_mod_sync(hrfd_mod *h)
{
  if (h == nullptr)
  {
    return fail(HRFD_EINVAL, "NULL handle");
  }
  HIP_TRY(hipSetDevice(h->core.device));
  HIP_TRY(hipStreamSynchronize(h->core.last_stream));
  if (h->kind == HRFD_MOD_FM || h->kind == HRFD_MOD_WBFM)
  {
    uint32_t expired = 0;
    HIP_TRY(hipMemcpy(&expired, h->d_err, sizeof(expired), hipMemcpyDeviceToHost));
    if (expired != 0)
    {
      return fail(HRFD_ESTATE, "hrfd_mod_sync: k_phase_scan gave up waiting %u time(s): the output of this handle is not valid", expired);
    }
  }
  return HRFD_OK;
}

extern "C" int hrfd_mod_process(hrfd_mod *h, const int16_t *pcm, uint32_t n_per_channel, int8_t *iq_out,
                                uint32_t *out_bytes)
{
  if (h == nullptr || pcm == nullptr || iq_out == nullptr || n_per_channel == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_mod_process: NULL argument or n_per_channel == 0");
  }
  BANK_TRY(tx_check_call("hrfd_mod_process", h->kind, h->n_channels, n_per_channel));
  const size_t in_bytes = (size_t)n_per_channel * (h->kind == HRFD_MOD_INTERP ? 2 : 1) * sizeof(int16_t) * h->n_channels;
  const size_t out_total = (size_t)h->n_channels * n_per_channel * 512;
  BankHostCall call(h->core);
  const int16_t *d_in = call.up(h->d_in, pcm, in_bytes);
  int8_t *d_out = call.room(h->d_out, iq_out, out_total);
  BANK_TRY(call.rc);
  BANK_TRY(hrfd_mod_process_device(h, d_in, n_per_channel, d_out, call.st));
  call.down(iq_out, d_out, out_total);
  BANK_TRY(call.finish());
  if (out_bytes != nullptr)
  {
    *out_bytes = n_per_channel << 9;                       // bytes per channel (SsbModulator.cc:512)
  }
  return HRFD_OK;
}

// ------------------------------------------------------------------ Nco
struct hrfd_nco
{
  BankCore core;                       // core.mu guards h_step and step_dirty, and a run as a whole
  uint32_t n_channels = 0;
  float sample_rate = 0;
  DevBuf<float> d_acc, d_step, d_sin, d_cos;
  DevBuf<float> d_i, d_q;              // the outputs of a call: they grow together
  std::vector<float> h_step;
  bool step_dirty = true;
};

// PhaseAccumulator.cc:41 / :105: the step is a double expression stored to float.  The wrap loops of k_nco (and of the
// reference) subtract 2 pi from a FLOAT accumulator: from about 2^27 rad that no longer changes the value and the loop
// never ends, and a NaN or an infinity never passes either compare's way out.  So a step that is not finite or reaches 2^24
// rad (three binades below, many orders of magnitude above every frequency the reference's callers use) is refused on the
// host, before anything is launched.
static bool nco_step(float sample_rate, float frequency, float *step)
{
  *step = (float)((2 * M_PI * frequency) / sample_rate);
  return std::isfinite(*step) && fabsf(*step) < 16777216.0f;
}

extern "C" int hrfd_nco_create(uint32_t n_channels, float sample_rate, float frequency, int device,
                               hrfd_nco **out)
{
  if (out == nullptr || n_channels == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_nco_create: bad arguments");
  }
  *out = nullptr;
  float step0;
  if (!nco_step(sample_rate, frequency, &step0))
  {
    return fail(HRFD_EINVAL, "hrfd_nco_create: the phase step 2 pi f / fs is not finite or is 2^24 rad or more");
  }
  hrfd_nco *h = nullptr;
  BANK_TRY(bank_new("hrfd_nco_create", device, &h));
  h->n_channels = n_channels;
  h->sample_rate = sample_rate;
  // PhaseAccumulator.cc:41: double expression stored to float
  h->h_step.assign(n_channels, step0);
  std::vector<float> st, ct;
  nco_tables(st, ct);
  hipError_t e = hipSuccess;
  if (!(h->d_acc.alloc(n_channels) && h->d_step.alloc(n_channels) && h->d_sin.alloc(16384) && h->d_cos.alloc(16384)))
  {
    e = hipErrorOutOfMemory;
  }
  if (e == hipSuccess) e = hipMemset(h->d_acc, 0, sizeof(float) * n_channels);
  if (e == hipSuccess) e = hipMemcpy(h->d_sin, st.data(), sizeof(float) * 16384, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->d_cos, ct.data(), sizeof(float) * 16384, hipMemcpyHostToDevice);
  if (e != hipSuccess)
  {
    const int rc = fail(HRFD_ENOMEM, "hrfd_nco_create: %s", hipGetErrorString(e));
    bank_free(h);
    return rc;
  }
  *out = h;
  return HRFD_OK;
}

extern "C" int hrfd_nco_destroy(hrfd_nco *h)
{
  if (h != nullptr)
  {
    bank_free(h);
  }
  return HRFD_OK;
}

extern "C" int hrfd_nco_set_frequency(hrfd_nco *h, uint32_t channel, float frequency)
{
  if (h == nullptr || (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels))
  {
    return fail(HRFD_EINVAL, "hrfd_nco_set_frequency: bad handle or channel");
  }
  float step;                                              // PhaseAccumulator.cc:105
  if (!nco_step(h->sample_rate, frequency, &step))
  {
    return fail(HRFD_EINVAL, "hrfd_nco_set_frequency: the phase step 2 pi f / fs is not finite or is 2^24 rad or more (nothing changed)");
  }
  std::lock_guard<std::mutex> g(h->core.mu);
  bank_each_selected(h->n_channels, channel, [&](uint32_t c) { h->h_step[c] = step; });
  h->step_dirty = true;
  return HRFD_OK;
}

extern "C" int hrfd_nco_reset(hrfd_nco *h, uint32_t channel)
{
  if (h == nullptr || (channel != HRFD_ALL_CHANNELS && channel >= h->n_channels))
  {
    return fail(HRFD_EINVAL, "hrfd_nco_reset: bad handle or channel");
  }
  std::lock_guard<std::mutex> g(h->core.mu);
  HIP_TRY(hipSetDevice(h->core.device));
  BANK_TRY(h->core.drain());
  const size_t first = (channel == HRFD_ALL_CHANNELS) ? 0 : channel, count = (channel == HRFD_ALL_CHANNELS) ? h->n_channels : 1;
  HIP_TRY(hipMemset(h->d_acc + first, 0, sizeof(float) * count));
  return HRFD_OK;
}

extern "C" int hrfd_nco_run(hrfd_nco *h, int fast, uint32_t count, float *i_out, float *q_out)
{
  if (h == nullptr || i_out == nullptr || q_out == nullptr || count == 0)
  {
    return fail(HRFD_EINVAL, "hrfd_nco_run: bad arguments");
  }
  const size_t bytes = sizeof(float) * (size_t)h->n_channels * count;
  std::lock_guard<std::mutex> g(h->core.mu);
  BankHostCall call(h->core);
  NcoParams N;
  N.i_out = call.room(h->d_i, i_out, bytes);
  N.q_out = call.room(h->d_q, q_out, bytes);
  BANK_TRY(call.rc);
  if (h->step_dirty)
  {
    HIP_TRY(hipMemcpy(h->d_step, h->h_step.data(), sizeof(float) * h->n_channels, hipMemcpyHostToDevice));
    h->step_dirty = false;
  }
  N.acc = h->d_acc;
  N.step = h->d_step;
  N.sin_t = h->d_sin;
  N.cos_t = h->d_cos;
  N.n_channels = h->n_channels;
  N.count = count;
  N.fast = fast;
  N.libm_fma = libm_variant();
  hipLaunchKernelGGL(k_nco, dim3((h->n_channels + 63) / 64), dim3(64), 0, call.st, N);
  BANK_TRY(bank_launch_ok("k_nco"));
  call.down(i_out, N.i_out, bytes);
  call.down(q_out, N.q_out, bytes);
  return call.finish();
}
