// hip/hip_runtime.h -- a counting stand-in for the HIP runtime, for tools/hostonly/owners_check.cpp, ba_proj_edge_check.cpp,
// image_batch_check.cpp and batch_handle_check.cpp alone (its directory goes first on the include path).  Device and pinned memory are malloc, copies are memcpy, streams and events are tokens; everything
// made is kept in a set of what is live and counted (made, dropped), and a free or destroy of something that is not live aborts.  Only what cs_hip_util.h, ba_dbuf.h and
// cs_image_batch.h call exists, and the two handle types that ba_types.h's launcher declarations name.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorUnknown = 999 };
enum { hipHostMallocDefault = 0, hipStreamNonBlocking = 1, hipEventDefault = 0, hipEventBlockingSync = 1, hipEventDisableTiming = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
struct hipStandinToken { int unused; };
typedef hipStandinToken* hipStream_t;
typedef hipStandinToken* hipEvent_t;

namespace hip_standin {
enum Kind { DEVICE, PINNED, STREAM, EVENT, N_KINDS };
inline std::set<void*>& live(int kind) { static std::set<void*> s[N_KINDS]; return s[kind]; }
inline long& made(int kind) { static long n[N_KINDS]; return n[kind]; }
inline long& dropped(int kind) { static long n[N_KINDS]; return n[kind]; }
inline hipError_t make(int kind, void** out, size_t bytes) {
  *out = std::malloc(bytes ? bytes : 1);
  made(kind)++;
  live(kind).insert(*out);
  return hipSuccess;
}
inline hipError_t drop(int kind, void* p) {
  if (!live(kind).erase(p)) { std::fprintf(stderr, "hip stand-in: kind %d: %p given back but not live\n", kind, p); std::abort(); }
  std::free(p);
  dropped(kind)++;
  return hipSuccess;
}
// the knob: the k-th hipEventSynchronize from now (1 = the next) returns an error; 0 = none does
inline int& event_sync_fails_in() { static int k = 0; return k; }
}  // namespace hip_standin

inline const char* hipGetErrorString(hipError_t) { return "stand-in error"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
inline hipError_t hipMalloc(void** p, size_t bytes) { return hip_standin::make(hip_standin::DEVICE, p, bytes); }
inline hipError_t hipFree(void* p) { return hip_standin::drop(hip_standin::DEVICE, p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hip_standin::make(hip_standin::PINNED, p, bytes); }
inline hipError_t hipHostFree(void* p) { return hip_standin::drop(hip_standin::PINNED, p); }
inline hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) { std::memcpy(dst, src, bytes); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t) { std::memcpy(dst, src, bytes); return hipSuccess; }
inline hipError_t hipMemset(void* dst, int v, size_t bytes) { std::memset(dst, v, bytes); return hipSuccess; }
inline hipError_t hipMemsetAsync(void* dst, int v, size_t bytes, hipStream_t) { std::memset(dst, v, bytes); return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hip_standin::make(hip_standin::STREAM, (void**)s, sizeof(hipStandinToken)); }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return hip_standin::make(hip_standin::STREAM, (void**)s, sizeof(hipStandinToken)); }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hip_standin::drop(hip_standin::STREAM, s); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hip_standin::make(hip_standin::EVENT, (void**)e, sizeof(hipStandinToken)); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hip_standin::drop(hip_standin::EVENT, e); }
inline hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDefault); }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { int& k = hip_standin::event_sync_fails_in(); return k > 0 && --k == 0 ? hipErrorUnknown : hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.25f; return hipSuccess; }
