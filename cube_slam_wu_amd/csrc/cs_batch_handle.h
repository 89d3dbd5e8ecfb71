// cs_batch_handle.h -- the host side of a "many small problems, one launch" entry (pose_host.cpp: cs_pose_batch, sim3_pair_host.cpp:
// cs_sim3_pairs): a handle that keeps a stream, two events, one input and one output buffer on the device with their pinned staging, and
// the one round trip every call makes -- upload everything with one copy, launch, download everything with one copy.  Host only.
// What is a path's own stays with it: its argument checks and messages, its records, its launch struct, and when `ran` and host_ms change.
#pragma once
#include <new>
#include <string>

#include "cs_hip_util.h"

namespace cs {

struct BatchHandle {
  int device = 0;
  Stream st;                               // (first: it dies last, after the buffers its copies use)
  Event ev0, ev1;
  DevBuf<unsigned char> d_in, d_out;       // one upload, one download
  PinBuf<unsigned char> h_in, h_out;       // pinned staging of the two
  double kernel_ms = 0, host_ms = 0;
  bool ran = false;
};

// The parts of a buffer, each behind a 256-byte aligned offset: add(bytes) -> the part's offset; `bytes` = the buffer so far.
struct Layout {
  size_t bytes = 0;
  size_t add(size_t n) { const size_t at = bytes; bytes = (at + n + 255) & ~(size_t)255; return at; }
};

// H = the C ABI's handle type, a BatchHandle by another name
template <class H>
void batch_destroy(H* B) {
  if (!B) return;
  (void)hipSetDevice(B->device);
  if (B->st) (void)hipStreamSynchronize(B->st);
  delete B;
}

template <class H>
int batch_create(int device, H** out) {
  if (!out) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  { const int rc = check_device(device); if (rc) return rc; }
  H* B = new (std::nothrow) H();
  if (!B) return CS_ERR_CAPACITY;
  Guard<H> g(B, batch_destroy<H>);
  B->device = device;
  CS_HIP_TRY(hipSetDevice(device));
  CS_TRY(B->st.create(hipStreamNonBlocking));
  CS_TRY(B->ev0.create());
  CS_TRY(B->ev1.create());
  *out = g.disarm();
  return CS_OK;
}

inline int batch_last_timing(const BatchHandle* B, double* kernel_ms, double* host_ms) {
  if (!B) return CS_ERR_INVALID_ARG;
  if (!B->ran) return CS_ERR_NOT_RUN;
  if (kernel_ms) *kernel_ms = B->kernel_ms;
  if (host_ms) *host_ms = B->host_ms;
  return CS_OK;
}

// One call's round trip.  The four buffers are grown to in_bytes / out_bytes; pack() then fills B.h_in.p (and may take addresses inside
// B.d_in.p / B.d_out.p, which hold from there on); h_in is uploaded; launch() enqueues the kernel on B.st; d_out is downloaded into h_out
// and the stream is waited for.  `timed`: the kernel's time between the handle's two events goes to B.kernel_ms.
template <class Pack, class Launch>
int batch_round_trip(BatchHandle& B, size_t in_bytes, size_t out_bytes, bool timed, Pack&& pack, Launch&& launch) {
  CS_HIP_TRY(hipSetDevice(B.device));
  CS_ENSURE(B.d_in, in_bytes);
  CS_ENSURE(B.d_out, out_bytes);
  CS_ENSURE(B.h_in, in_bytes);
  CS_ENSURE(B.h_out, out_bytes);
  pack();
  CS_HIP_TRY(hipMemcpyAsync(B.d_in.p, B.h_in.p, in_bytes, hipMemcpyHostToDevice, B.st));
  if (timed) CS_HIP_TRY(hipEventRecord(B.ev0, B.st));
  launch();
  CS_HIP_TRY(hipGetLastError());
  if (timed) CS_HIP_TRY(hipEventRecord(B.ev1, B.st));
  CS_HIP_TRY(hipMemcpyAsync(B.h_out.p, B.d_out.p, out_bytes, hipMemcpyDeviceToHost, B.st));
  CS_HIP_TRY(hipStreamSynchronize(B.st));
  if (timed) {
    float ms = 0;
    CS_HIP_TRY(hipEventElapsedTime(&ms, B.ev0, B.ev1));
    B.kernel_ms = ms;
  }
  return CS_OK;
}

// The kernels index their records by ptr alone: it must be a non-decreasing partition, ptr[0] = 0.  `what` = "<entry>: <the array's name>".
inline int check_partition(const std::string& what, const int* ptr, int n) {
  if (ptr[0] != 0) { cs_set_error(what + "[0] must be 0"); return CS_ERR_INVALID_ARG; }
  for (int f = 0; f < n; f++)
    if (ptr[f + 1] < ptr[f]) { cs_set_error(what + " must not decrease"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

}  // namespace cs
