// cs_hip_util.h -- small host-side HIP helpers shared by the kernel files and the host stages.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>

#include "../../include/cubeslam_hip.h"

// the calling thread's message behind cs_last_error() (g_cs_err, detect_host.cpp; shared by every path)
void cs_set_error(const std::string& s);

#define CS_HIP_TRY(expr)                                                       \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      cs_set_error(std::string(#expr) + ": " + hipGetErrorString(_e));         \
      return CS_ERR_HIP;                                                       \
    }                                                                          \
  } while (0)

// `call` returns a CS_* code: pass a failure on
#define CS_TRY(call) do { if (int _rc = (call)) return _rc; } while (0)
// grow a DevBuf / PinBuf (below) inside a function that returns a CS_* code
#define CS_ENSURE(buf, n) CS_TRY((buf).ensure(n))

// No C++ exception may cross the C boundary (std::bad_alloc / std::length_error from a host buffer would terminate the caller).
#define CS_GUARD_BEGIN try {
#define CS_GUARD_END(fn_name)                                                                                                \
  } catch (const std::bad_alloc&) { cs_set_error(std::string(fn_name) + ": out of host memory"); return CS_ERR_CAPACITY; }   \
    catch (const std::exception& ex) { cs_set_error(std::string(fn_name) + ": " + ex.what()); return CS_ERR_CAPACITY; }

namespace cs {

// the turn of the persistent solver kernels whose workgroups wait for each other (ba_lm.cpp, pgo_host.cpp): one such kernel at a time per process
inline std::mutex& coop_mutex() { static std::mutex m; return m; }

// the first check of every cs_*_create: a device is visible and `device` names one
inline int check_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { cs_set_error("no HIP device visible; libcubeslam_hip has no CPU fallback"); return CS_ERR_NO_DEVICE; }
  if (device < 0 || device >= n) { cs_set_error("device index out of range"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Grow-only device / pinned buffers.  They free themselves (release() is idempotent: a holder may still call it early) and cannot be copied.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  int ensure(size_t n) {
    if (n <= cap) return CS_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = n + n / 8 + 64;
    CS_HIP_TRY(hipMalloc((void**)&p, want * sizeof(T)));
    cap = want;
    return CS_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
template <class T>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  int ensure(size_t n) {
    if (n <= cap) return CS_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    size_t want = n + n / 8 + 64;
    CS_HIP_TRY(hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault));
    cap = want;
    return CS_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// One stream / one event, destroyed with its holder; not copyable.  Each converts to the raw handle, so the HIP calls take it as written.
// A holder declares its streams BEFORE everything that is queued on them: members die in reverse order, the streams last.
struct Stream {
  hipStream_t s = nullptr;
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  int create(unsigned flags) { CS_HIP_TRY(hipStreamCreateWithFlags(&s, flags)); return CS_OK; }
  int create(unsigned flags, int priority) { CS_HIP_TRY(hipStreamCreateWithPriority(&s, flags, priority)); return CS_OK; }
  operator hipStream_t() const { return s; }
};
struct Event {
  hipEvent_t e = nullptr;
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { if (e) (void)hipEventDestroy(e); }
  int create(unsigned flags = hipEventDefault) { CS_HIP_TRY(hipEventCreateWithFlags(&e, flags)); return CS_OK; }
  operator hipEvent_t() const { return e; }
};

// What a create function has made so far: given back through the handle's own destroy function on every early return, kept by disarm().
template <class H>
struct Guard {
  H* h;
  void (*destroy)(H*);
  Guard(H* h_, void (*destroy_)(H*)) : h(h_), destroy(destroy_) {}
  Guard(const Guard&) = delete;
  Guard& operator=(const Guard&) = delete;
  ~Guard() { if (h) destroy(h); }
  H* disarm() { H* r = h; h = nullptr; return r; }
};

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device's instance of a kernel: a handle on a second GPU of the
// same process (cs_ba_create(device = 1), sharded ranks as threads on several devices) needs its own call.  One table per kernel, a
// slot per device: 0 = not tried, 1 = set, 2 = refused.  Two threads racing on a slot both make the (idempotent) call.
struct DynLdsOnce {
  enum { MAX_DEV = 64 };
  std::atomic<unsigned char> slot[MAX_DEV];
  // true when `fn` may be launched with `bytes` of dynamic LDS on the current device
  bool set(const void* fn, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
    unsigned char s = slot[dev].load(std::memory_order_acquire);
    if (s == 0) {
      s = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess ? 1 : 2;
      if (s == 2) (void)hipGetLastError();     // (the refusal is reported through the return value, not left as the thread's sticky error)
      slot[dev].store(s, std::memory_order_release);
    }
    return s == 1;
  }
};

}  // namespace cs
