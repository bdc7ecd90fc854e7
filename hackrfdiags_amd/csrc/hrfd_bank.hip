// hackrfdiags_amd/csrc/hrfd_bank.hip -- the host core of the bank handles (hrfd_ddc, hrfd_duc, hrfd_spec, hrfd_cal,
// hrfd_tone, hrfd_audio, hrfd_resamp, hrfd_level, hrfd_tonegen, hrfd_afsk, hrfd_afskgen, hrfd_hdlc) and of the transmit handles (hrfd_mod, hrfd_nco): device and stream ownership with the three ordering rules (BankCore), what stands
// around every launch (the NULL-handle refusal, the launch check, the chunked launch, the loop over the selected channels),
// the blocking host entry (BankHostCall), the history of the PCM banks (BankHistory) with the reset over it, the host part
// of the two generator banks (GenCore: clock, clips, sine table, the process entries), and the setters and argument checks
// the DDC and the DUC share.  DESIGN.md 3.5a states the rules; hrfd_bank.h, hrfd_pcm.h and hrfd_gen.h hold the parts that
// need no HIP, hrfd_buf.h the buffers a handle owns (DevBuf, PinnedBuf: shared with the receive and transmit handles).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "hrfd_buf.h"
#include "hrfd_gen.h"
#include "hrfd_ddc_tables.h"

namespace hrfd {

constexpr int kBankTile = 1024;            // outputs (DDC) or channel samples (DUC) per workgroup
constexpr int kBankThreads = 256;

// Every bank handle embeds one.  The handle's records, history and staging buffers are shared by all its launches, on
// whatever stream each runs, so:
//   1. stream hand-over: a launch on another stream than the last one waits for it on the device (order_behind_last,
//      then launched_on once the launch is accepted)
//   2. staging upload: a pinned staging buffer is rewritten only after the device has read the previous upload out of
//      it (staging_wait before the rewrite, staging_sent behind the copies)
//   3. host-path drain: a blocking host path waits for the handle's stream and the last launch's before it grows or
//      refills the handle's device buffers (drain)
struct BankCore
{
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t last_stream = nullptr;       // the stream of the last accepted launch
  hipEvent_t ev_last = nullptr;            // recorded on last_stream when the next launch runs on another stream
  hipEvent_t ev_upload = nullptr;          // the last upload from the pinned staging buffers has been read
  std::mutex mu;                           // guards the handle's host records (setters may come from another thread)
  uint32_t max_wgs = kBankMaxWgs;          // workgroups of one launch of a chunked call (bank_launch_chunked); under mu

  // `who` is the public create function.  Nothing is left open on failure.
  int open(const char *who, int dev)
  {
    if (hrfd_device_count() <= 0)
    {
      return fail(HRFD_ENODEV, "%s: no HIP device visible (this library has no CPU path)", who);
    }
    if (dev < 0)
    {
      HIP_TRY(hipGetDevice(&dev));
    }
    HIP_TRY(hipSetDevice(dev));
    device = dev;
    if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ev_last, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ev_upload, hipEventDisableTiming) != hipSuccess)
    {
      (void)hipGetLastError();
      close();
      return fail(HRFD_ENOMEM, "%s: device allocation failed", who);
    }
    last_stream = stream;
    return HRFD_OK;
  }

  void close()
  {
    if (stream)
    {
      (void)hipStreamSynchronize(stream);
    }
    if (last_stream && last_stream != stream)
    {
      (void)hipStreamSynchronize(last_stream);
    }
    if (ev_last) (void)hipEventDestroy(ev_last);
    if (ev_upload) (void)hipEventDestroy(ev_upload);
    if (stream) (void)hipStreamDestroy(stream);
    ev_last = ev_upload = nullptr;
    stream = last_stream = nullptr;
  }

  hipStream_t stream_or_own(void *s) const { return s ? (hipStream_t)s : stream; }

  int order_behind_last(hipStream_t s)
  {
    if (s != last_stream)
    {
      HIP_TRY(hipEventRecord(ev_last, last_stream));
      HIP_TRY(hipStreamWaitEvent(s, ev_last, 0));
    }
    return HRFD_OK;
  }

  void launched_on(hipStream_t s) { last_stream = s; }

  int staging_wait() { HIP_TRY(hipEventSynchronize(ev_upload)); return HRFD_OK; }
  int staging_sent(hipStream_t s) { HIP_TRY(hipEventRecord(ev_upload, s)); return HRFD_OK; }

  int drain()
  {
    HIP_TRY(hipStreamSynchronize(stream));
    if (last_stream != stream)
    {
      HIP_TRY(hipStreamSynchronize(last_stream));
    }
    return HRFD_OK;
  }
};

// the refusal of a call without a handle, behind what the call's sizes and addresses decide on their own
static int bank_need_handle(const char *who, const void *handle)
{
  return handle != nullptr ? HRFD_OK : fail(HRFD_EINVAL, "%s: NULL handle", who);
}

// f(i) for item `which` of n, or for every item (HRFD_ALL_CHANNELS); the caller has checked `which`
template <class F>
static void bank_each_selected(uint32_t n, uint32_t which, F f)
{
  for (uint32_t i = 0; i < n; i++)
  {
    if (which == HRFD_ALL_CHANNELS || i == which)
    {
      f(i);
    }
  }
}

// behind every kernel launch
static int bank_launch_ok(const char *kernel)
{
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? HRFD_OK : fail(HRFD_ENODEV, "%s launch failed: %s", kernel, hipGetErrorString(e));
}

// n_wgs workgroups in launches of at most core.max_wgs (bank_each_chunk cuts them): launch(grid) starts one with P.first_wg
// set to its first workgroup
template <class Params, class Launch>
static int bank_launch_chunked(const char *kernel, BankCore &core, uint64_t n_wgs, Params &P, Launch launch)
{
  uint32_t max_wgs;
  {
    std::lock_guard<std::mutex> g(core.mu);
    max_wgs = core.max_wgs;
  }
  return bank_each_chunk<decltype(P.first_wg)>(kernel, n_wgs, max_wgs, [&](decltype(P.first_wg) first, uint32_t count) {
    P.first_wg = first;
    launch(dim3(count));
    return bank_launch_ok(kernel);
  });
}

// test hook of the PCM banks (hrfd_<bank>_debug_set_max_wgs, behind HRFD_HOOK_GATE): with few workgroups per launch a small
// call is cut the way one of more than kBankMaxWgs workgroups is
template <class H>
static int bank_set_max_wgs(const char *who, H *h, uint32_t n)
{
  if (h == nullptr || n < 1 || n > kBankMaxWgs)
  {
    return fail(HRFD_EINVAL, "%s: need a handle and 1..%u workgroups per launch (got %u)", who, kBankMaxWgs, n);
  }
  std::lock_guard<std::mutex> g(h->core.mu);
  h->core.max_wgs = n;
  return HRFD_OK;
}

// A blocking host entry over a handle's own stream: rc holds the first failure, and every step behind one does nothing.
//   BankHostCall call(h->core);                           sets the device and drains (rule 3)
//   d_x = call.up(h->d_x, x, bytes);                      grows the buffer and copies x up; NULL for a NULL x
//   d_y = call.room(h->d_y, y, bytes);                    grows the buffer of an output; NULL for one not asked for
//   BANK_TRY(call.rc); BANK_TRY(x_launch(.., call.st));
//   call.down(y, h->d_y, bytes);                          copies an output back if it was asked for
//   return call.finish();                                 waits for the stream
struct BankHostCall
{
  hipStream_t st;
  int rc;

  explicit BankHostCall(BankCore &core) : st(core.stream), rc(begin(core)) {}

  template <class T>
  T *up(DevBuf<T> &buf, const void *host, size_t bytes)
  {
    T *dev = room(buf, host, bytes);
    if (dev != nullptr)
    {
      rc = copy(dev, host, bytes, hipMemcpyHostToDevice);
    }
    return rc == HRFD_OK ? dev : nullptr;
  }

  template <class T>
  T *room(DevBuf<T> &buf, const void *host, size_t bytes)
  {
    if (rc != HRFD_OK || host == nullptr)
    {
      return nullptr;
    }
    rc = buf.grow_bytes(bytes);
    return rc == HRFD_OK ? buf.p : nullptr;
  }

  void down(void *host, const void *dev, size_t bytes)
  {
    if (rc == HRFD_OK && host != nullptr)
    {
      rc = copy(host, dev, bytes, hipMemcpyDeviceToHost);
    }
  }

  int finish()
  {
    BANK_TRY(rc);
    HIP_TRY(hipStreamSynchronize(st));
    return HRFD_OK;
  }

private:
  static int begin(BankCore &core)
  {
    HIP_TRY(hipSetDevice(core.device));
    return core.drain();
  }

  int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
  {
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, st));
    return HRFD_OK;
  }
};

// The filter history of a PCM bank (hrfd_audio, hrfd_resamp): per channel the last 512 samples as the filter saw them, as
// 256 packed pairs, in a ping-pong of two sides (a launch reads in() and writes out(), flip() turns them over), and the
// channels that start from zeros with the next launch.  hrfd_level keeps its 64 frame peaks per channel the same way, in
// rows of 32 dwords, hrfd_afsk its samples, phase and flags in rows of 18, hrfd_hdlc its
// partial frame in rows of 260.  Host fields under the handle's core.mu.
struct BankHistory
{
  static constexpr size_t kDw = 256;       // dwords per channel, unless alloc is told otherwise
  size_t C = 0;
  size_t dw = kDw;
  std::vector<uint8_t> fresh;              // per channel
  bool any_fresh = false;
  uint32_t side = 0;                       // the side the next launch reads
  DevBuf<uint32_t> d_hist;                 // [2][C][dw]
  DevBuf<uint8_t> d_fresh;                 // [C]

  bool alloc(size_t n_channels, size_t dwords = kDw)
  {
    C = n_channels;
    dw = dwords;
    fresh.assign(C, 0);
    return d_hist.alloc(2 * C * dw) && d_fresh.alloc(C) && hipMemset(d_hist, 0, 4 * 2 * C * dw) == hipSuccess;
  }

  void mark(uint32_t channel)
  {
    bank_each_selected((uint32_t)C, channel, [&](uint32_t c) { fresh[c] = 1; });
    any_fresh = true;
  }

  // the kernel's reset flags for the next launch, or NULL when no channel is marked; read in front of upload
  const uint8_t *reset() const { return any_fresh ? d_fresh.p : nullptr; }

  // between staging_wait and staging_sent: the marks go up through `stage`, C bytes of the handle's pinned staging
  int upload(uint8_t *stage, hipStream_t st)
  {
    if (any_fresh)
    {
      memcpy(stage, fresh.data(), C);
      HIP_TRY(hipMemcpyAsync(d_fresh, stage, C, hipMemcpyHostToDevice, st));
      fresh.assign(C, 0);
      any_fresh = false;
    }
    return HRFD_OK;
  }

  const uint32_t *in() const { return d_hist + side * C * dw; }
  uint32_t *out() const { return d_hist + (side ^ 1u) * C * dw; }
  void flip() { side ^= 1u; }
};

// hrfd_<bank>_reset of a bank whose history is a BankHistory `hist` (level, audio, afsk, hdlc): the channel, or all, starts
// from zeros with the next launch
template <class H>
static int bank_reset_history(H *h, const char *who, uint32_t channel)
{
  BANK_TRY(pcm_check_channel(who, channel, 65536));
  BANK_TRY(bank_need_handle(who, h));
  BANK_TRY(pcm_check_channel(who, channel, h->n_channels));
  std::lock_guard<std::mutex> g(h->core.mu);
  h->hist.mark(channel);
  return HRFD_OK;
}

// What a generator bank (hrfd_tonegen, hrfd_afskgen, hrfd_dcsgen) keeps beside its BankCore: the clock, the watermark of its
// queues, the clip counters with their lazy clear, the rotated sine table and the staging of the blocking host entry.  Host
// fields under the handle's core.mu.  The queues, their copy on the device and the kernel are the bank's own: the gen_*
// functions below take a handle H with core, n_channels and gen, and the bank's launch function
//   int launch(H *, const int16_t *d_pcm, uint64_t stride, uint32_t n_blocks, int16_t *d_out, uint64_t out_stride,
//              uint8_t *d_active, hipStream_t st)
struct GenCore
{
  uint64_t N = 0;                          // the stream time of the next call's first sample
  uint64_t next_end = ~0ull;               // nothing queued ends before this: a call below it has nothing to drop
  bool clear_clips = false;                // reset: the counters are zeroed ahead of the next launch
  DevBuf<int16_t> d_sine;                  // [4096]: sine[i] = COS[(i - 1024) & 4095]
  DevBuf<unsigned long long> d_clips;      // [C]
  DevBuf<int16_t> d_pcm, d_out;            // host-path staging
  DevBuf<uint8_t> d_active;

  bool alloc(size_t C)
  {
    std::vector<int16_t> sine(4096);
    for (uint32_t i = 0; i < 4096; i++)
    {
      sine[i] = Q_DDC_COS[(i - 1024u) & 4095u];
    }
    return d_sine.alloc(4096) && d_clips.alloc(C) &&
           hipMemcpy(d_sine, sine.data(), sizeof(int16_t) * 4096, hipMemcpyHostToDevice) == hipSuccess &&
           hipMemset(d_clips, 0, sizeof(unsigned long long) * C) == hipSuccess;
  }

  // the core's part of a reset, under mu; the bank empties its queues
  void reset()
  {
    N = 0;
    next_end = ~0ull;
    clear_clips = true;
  }

  // the last step of a launch's part under mu, behind the bank's staging on `st`: the counters are zeroed if a reset asked
  // for it, and the clock moves on by the call's n samples
  int advance(uint32_t n_channels, uint64_t n, hipStream_t st)
  {
    if (clear_clips)
    {
      HIP_TRY(hipMemsetAsync(d_clips, 0, sizeof(unsigned long long) * n_channels, st));
      clear_clips = false;
    }
    N += n;
    return HRFD_OK;
  }
};

template <class H>
static int gen_time(H *h, const char *who, uint64_t *N)
{
  if (N == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL result", who);
  }
  BANK_TRY(bank_need_handle(who, h));
  std::lock_guard<std::mutex> g(h->core.mu);
  *N = h->gen.N;
  return HRFD_OK;
}

// the handle and the channel of a getter of one channel (get_clips, pending), behind what its arguments decide on their own
template <class H>
static int gen_check_getter(H *h, const char *who, uint32_t channel)
{
  BANK_TRY(bank_need_handle(who, h));
  return gen_check_one_channel(who, channel, h->n_channels);
}

template <class H>
static int gen_get_clips(H *h, const char *who, uint32_t channel, uint64_t *n)
{
  if (n == nullptr || channel >= 65536)
  {
    return fail(HRFD_EINVAL, "%s: channel %u (one channel) and a result pointer", who, channel);
  }
  BANK_TRY(gen_check_getter(h, who, channel));
  {
    std::lock_guard<std::mutex> g(h->core.mu);
    if (h->gen.clear_clips)
    {
      *n = 0;                              // reset, and no call since
      return HRFD_OK;
    }
  }
  HIP_TRY(hipSetDevice(h->core.device));
  BANK_TRY(h->core.drain());
  unsigned long long v = 0;
  HIP_TRY(hipMemcpy(&v, h->gen.d_clips + channel, sizeof(v), hipMemcpyDeviceToHost));
  *n = v;
  return HRFD_OK;
}

template <class H>
static int gen_check_process(H *h, const char *who, const void *pcm, uint64_t stride, bool device_entry, uint32_t n_blocks,
                             const void *out, uint64_t out_stride)
{
  // what the sizes and addresses decide on their own comes first, so that it is refused with its own text
  BANK_TRY(gen_check_call(who, pcm, stride, device_entry, n_blocks, out, out_stride, 1));
  BANK_TRY(bank_need_handle(who, h));
  BANK_TRY(gen_check_call(who, pcm, stride, device_entry, n_blocks, out, out_stride, h->n_channels));
  std::lock_guard<std::mutex> g(h->core.mu);
  return gen_check_time(who, h->gen.N + (uint64_t)kGenBlock * n_blocks - 1);       // the call's last sample
}

template <class H, class Launch>
static int gen_process_device(H *h, const char *who, Launch launch, const int16_t *d_pcm, uint64_t stride, uint32_t n_blocks,
                              int16_t *d_out, uint64_t out_stride, uint8_t *d_active, void *stream)
{
  BANK_TRY(gen_check_process(h, who, d_pcm, stride, true, n_blocks, d_out, out_stride));
  HIP_TRY(hipSetDevice(h->core.device));
  return launch(h, d_pcm, stride, n_blocks, d_out, out_stride, d_active, h->core.stream_or_own(stream));
}

template <class H, class Launch>
static int gen_process(H *h, const char *who, Launch launch, const int16_t *pcm, uint32_t n_blocks, int16_t *out, uint8_t *active)
{
  BANK_TRY(gen_check_process(h, who, pcm, 0, false, n_blocks, out, 0));
  BankHostCall call(h->core);
  const size_t C = h->n_channels, row = 2 * (size_t)kGenBlock * n_blocks;
  const int16_t *d_pcm = call.up(h->gen.d_pcm, pcm, row * C);
  int16_t *d_out = call.room(h->gen.d_out, out, row * C);
  uint8_t *d_active = call.room(h->gen.d_active, active, C * n_blocks);
  BANK_TRY(call.rc);
  BANK_TRY(launch(h, d_pcm, row, n_blocks, d_out, row, d_active, call.st));
  call.down(out, d_out, row * C);
  call.down(active, d_active, C * n_blocks);
  return call.finish();
}

// The setters and getters of a handle with one tuning record per channel (the DDC and the DUC), under `who`, the public
// function's name.  H has core, n_channels, n_captures, h_chan, N (the absolute wideband sample counter), dirty and
// clear_history.
template <class H>
static int tuned_reset(H *d, const char *who)
{
  BANK_TRY(bank_need_handle(who, d));
  std::lock_guard<std::mutex> g(d->core.mu);
  d->N = 0;
  for (BankTuning &c : d->h_chan)
  {
    bank_reset(c);
  }
  d->clear_history = true;
  d->dirty = true;
  return HRFD_OK;
}

template <class H>
static int tuned_set_tuning(H *d, const char *who, uint32_t channel, uint32_t capture, uint32_t step)
{
  if (d == nullptr || channel >= d->n_channels || capture >= d->n_captures)
  {
    return fail(HRFD_EINVAL, "%s: bad handle, channel or capture", who);
  }
  std::lock_guard<std::mutex> g(d->core.mu);
  bank_retune(d->h_chan[channel], d->N, capture, step);
  d->dirty = true;
  return HRFD_OK;
}

// the bank's own word of one channel, or of all (HRFD_ALL_CHANNELS); the caller has checked its range
template <class H>
static int tuned_set_word(H *d, const char *who, uint32_t channel, uint32_t value)
{
  if (d == nullptr || (channel >= d->n_channels && channel != HRFD_ALL_CHANNELS))
  {
    return fail(HRFD_EINVAL, "%s: bad handle or channel", who);
  }
  std::lock_guard<std::mutex> g(d->core.mu);
  bank_each_selected(d->n_channels, channel, [&](uint32_t c) { d->h_chan[c].word = value; });
  d->dirty = true;
  return HRFD_OK;
}

template <class H>
static int tuned_get_phase(H *d, const char *who, uint32_t channel, uint32_t *theta)
{
  if (d == nullptr || channel >= d->n_channels || theta == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: bad handle, channel or NULL result", who);
  }
  std::lock_guard<std::mutex> g(d->core.mu);
  *theta = bank_phase_at(d->h_chan[channel], d->N);
  return HRFD_OK;
}

// a new handle with its core open, or none
template <class H>
static int bank_new(const char *who, int device, H **h)
{
  *h = new H;
  const int rc = (*h)->core.open(who, device);
  if (rc != HRFD_OK)
  {
    delete *h;
    *h = nullptr;
  }
  return rc;
}

// the one free path of a bank handle, for create's failure path and destroy: the core first (it waits for the handle's
// work), then the handle with the buffers it owns
template <class H>
static void bank_free(H *h)
{
  (void)hipSetDevice(h->core.device);
  h->core.close();
  delete h;
}

// `word` is "decimation" or "interpolation"
static int bank_rate_ok(const char *who, const char *word, uint32_t rate)
{
  if (rate != 1 && rate != 2 && rate != 4 && rate != 8)
  {
    return fail(HRFD_EINVAL, "%s: %s must be 1, 2, 4 or 8 (got %u)", who, word, rate);
  }
  return HRFD_OK;
}

// [4096] (COS[k], COS[(k - 1024) & 4095]) as packed int16, the table both mixers keep in LDS
static bool bank_upload_cos(DevBuf<uint32_t> &d_cs)
{
  std::vector<uint32_t> cs(4096);
  for (int k = 0; k < 4096; k++)
  {
    cs[k] = (uint16_t)Q_DDC_COS[k] | ((uint32_t)(uint16_t)Q_DDC_COS[(k - 1024) & 4095] << 16);
  }
  return d_cs.alloc(4096) && hipMemcpy(d_cs, cs.data(), sizeof(uint32_t) * 4096, hipMemcpyHostToDevice) == hipSuccess;
}

// A call of `bytes` per row at 2.048 MS/s: rows of in_rate * bytes in (in_stride apart, read as 16-bit samples), rows of
// out_rate * bytes out; one of the rates is the handle's R, the other 1.  The launch has one workgroup per (tiled row,
// tile of kBankTile samples) and one per history row.
static int bank_check_call(const char *who, const char *word, uint32_t bytes, const void *in, uint64_t in_stride,
                           uint32_t in_rate, uint64_t out_stride, uint32_t out_rate, uint32_t tiled_rows, uint32_t hist_rows)
{
  if (bytes < 2 || (bytes & 1u) != 0 || bytes > (1u << 25))
  {
    return fail(HRFD_EINVAL, "%s: %s must be even, >= 2 and <= 2^25 (got %u)", who, word, bytes);
  }
  // one launch: gridDim.x * blockDim.x work-items must fit in 32 bits
  if ((uint64_t)tiled_rows * ((bytes / 2u + kBankTile - 1) / kBankTile) + hist_rows > 0xffffffffull / kBankThreads)
  {
    return fail(HRFD_EINVAL, "%s: %u rows x %u bytes need more workgroups than one launch takes", who, tiled_rows, bytes);
  }
  if (in_stride < (uint64_t)in_rate * bytes || out_stride < (uint64_t)out_rate * bytes || (in_stride & 1u) != 0 ||
      ((uintptr_t)in & 1u) != 0)
  {
    return fail(HRFD_EINVAL, "%s: strides shorter than a row, or an odd input stride / address", who);
  }
  return HRFD_OK;
}

} // namespace hrfd
