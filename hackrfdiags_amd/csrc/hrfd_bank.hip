// hackrfdiags_amd/csrc/hrfd_bank.hip -- the host core of the bank handles (hrfd_ddc, hrfd_duc, hrfd_spec, hrfd_cal, hrfd_tone, hrfd_audio, hrfd_resamp): device and
// stream ownership, the three ordering rules, and the argument checks the DDC and the DUC share.  DESIGN.md 3.5a states
// the rules; hrfd_bank.h holds the parts that need no HIP, hrfd_buf.h the buffers a handle owns (DevBuf, PinnedBuf: shared
// with the receive and transmit handles).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "hrfd_bank.h"
#include "hrfd_buf.h"
#include "hrfd_ddc_tables.h"

#define BANK_TRY(expr)                                                                   \
  do                                                                                     \
  {                                                                                      \
    const int rc_ = (expr);                                                              \
    if (rc_ != HRFD_OK) return rc_;                                                      \
  } while (0)

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

// The setters and getters of a handle with one tuning record per channel (the DDC and the DUC), under `who`, the public
// function's name.  H has core, n_channels, n_captures, h_chan, N (the absolute wideband sample counter), dirty and
// clear_history.
template <class H>
static int tuned_reset(H *d, const char *who)
{
  if (d == nullptr)
  {
    return fail(HRFD_EINVAL, "%s: NULL handle", who);
  }
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
  for (uint32_t c = 0; c < d->n_channels; c++)
  {
    if (channel == HRFD_ALL_CHANNELS || c == channel)
    {
      d->h_chan[c].word = value;
    }
  }
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
