// hackrfdiags_amd/csrc/hrfd_buf.h -- device and pinned buffers a handle owns: freed with the handle, whatever members it
// has (hrfd_rx, and hrfd_mod, hrfd_nco and the bank handles on BankCore, hrfd_bank.hip).  Part of the unity translation
// unit hrfd_lib.hip, behind the error helpers of hrfd_api.hip (fail).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

static int grow(void **p, size_t *cap, size_t need)
{
  if (need <= *cap && *p != nullptr)
  {
    return HRFD_OK;
  }
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  hipError_t e = hipMalloc(p, need);
  if (e != hipSuccess)
  {
    *cap = 0;
    return fail(HRFD_ENOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
  }
  *cap = need;
  return HRFD_OK;
}

namespace hrfd {

template <class T>
struct DevBuf
{
  T *p = nullptr;
  size_t cap = 0;                          // bytes
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release()
  {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // n ELEMENTS, at create; false with the text of the failure in hrfd_last_error
  bool alloc(size_t n) { return ::grow((void **)&p, &cap, sizeof(T) * n) == HRFD_OK; }
  // at least `bytes` BYTES: keeps what is large enough, else the contents are lost; HRFD_ENOMEM with its text
  int grow_bytes(size_t bytes) { return ::grow((void **)&p, &cap, bytes); }
  operator T *() const { return p; }
  T *operator->() const { return p; }
};

template <class T>
struct PinnedBuf
{
  T *p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { release(); }
  void release()
  {
    if (p) (void)hipHostFree(p);
    p = nullptr;
  }
  bool alloc(size_t n)
  {
    release();
    return hipHostMalloc((void **)&p, sizeof(T) * n, hipHostMallocDefault) == hipSuccess;
  }
  operator T *() const { return p; }
};

} // namespace hrfd
