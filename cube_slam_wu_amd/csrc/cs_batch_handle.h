// cs_batch_handle.h -- the host side of a "many small problems, one launch" entry: pose_host.cpp (cs_pose_batch), sim3_pair_host.cpp
// (cs_sim3_pairs), sim3_ransac_host.cpp (cs_sim3_ransac), triangulate_host.cpp (cs_triangulate), orb_search_host.cpp (cs_orb_search).
// Host only.  What the five share is here:
//   * the handle -- a stream, two events, one input and one output buffer on the device with their pinned staging -- with its create, destroy
//     and last_timing, and batch_one_shot for an entry that makes a handle for one call;
//   * Layout / Part<T>: the typed parts of a buffer, each behind a 256-byte aligned offset, with copy_in / copy_out to and from the staging;
//   * batch_round_trip: upload everything with one copy, launch, download everything with one copy;
//   * BatchCall: when `ran`, kernel_ms and host_ms change during a call;
//   * the checks of arguments (check_partition, all_finite, none_negative, positive, quaternion_norm_ok) and the refusal (Refuse);
//   * the chunk table of a kernel that gives a wavefront at most `width` items of ONE owner (chunk_count, chunk_fill, count_status).
// What is an entry's own stays with it: which arguments it checks, in which order and with which words, its records, its launch struct.
#pragma once
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "cs_chunk.h"
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

// `count` elements of T at byte `off` of a buffer; at(base) = the part inside the buffer that starts at `base` (h_in.p, d_in.p, ...)
template <class T>
struct Part {
  size_t off = 0, count = 0;
  size_t bytes() const { return count * sizeof(T); }
  T* at(unsigned char* base) const { return reinterpret_cast<T*>(base + off); }
  const T* at(const unsigned char* base) const { return reinterpret_cast<const T*>(base + off); }
};

// The parts of a buffer, each behind a 256-byte aligned offset, in the order they are added; `bytes` = the buffer so far.  An empty part is legal.
struct Layout {
  size_t bytes = 0;
  template <class T>
  Part<T> add(size_t count) {
    const Part<T> part{bytes, count};
    bytes = (bytes + part.bytes() + 255) & ~(size_t)255;
    return part;
  }
};

template <class T>
void copy_in(const Part<T>& part, PinBuf<unsigned char>& h_in, const T* src) { std::memcpy(part.at(h_in.p), src, part.bytes()); }
template <class T>
void copy_out(const Part<T>& part, const PinBuf<unsigned char>& h_out, T* dst) { std::memcpy(dst, part.at(h_out.p), part.bytes()); }

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

// A one-shot entry: a handle of its own for fn(H*), destroyed whatever fn returns.  What the entry refuses without a device it checks before.
template <class H, class Fn>
int batch_one_shot(int device, Fn&& fn) {
  H* B = nullptr;
  CS_TRY(batch_create(device, &B));
  Guard<H> g(B, batch_destroy<H>);         // (never disarmed)
  return fn(B);
}

inline int batch_last_timing(const BatchHandle* B, double* kernel_ms, double* host_ms) {
  if (!B) return CS_ERR_INVALID_ARG;
  if (!B->ran) return CS_ERR_NOT_RUN;
  if (kernel_ms) *kernel_ms = B->kernel_ms;
  if (host_ms) *host_ms = B->host_ms;
  return CS_OK;
}

// What a call does to the handle's `ran`, kernel_ms and host_ms (batch_last_timing): the host clock starts with the object, empty() is the
// answer to a call without a problem, point_of_no_return() withdraws the last run's figures, done() hands out this run's.
// The entries do NOT agree on where the point of no return lies, and each keeps its place:
//   * cs_pose_batch_optimize puts it BEFORE its argument checks (and before empty()): a call it refuses for its arrays leaves
//     cs_pose_batch_last_timing at CS_ERR_NOT_RUN;
//   * every other entry puts it BEHIND its checks: a refused call leaves the last run's timing in place, one that fails later does not.
struct BatchCall {
  BatchHandle& B;
  const double t_begin;
  explicit BatchCall(BatchHandle& b) : B(b), t_begin(now_ms()) {}
  int empty() { B.kernel_ms = B.host_ms = 0; B.ran = true; return CS_OK; }
  void point_of_no_return() { B.ran = false; }
  int done() { B.host_ms = now_ms() - t_begin; B.ran = true; return CS_OK; }
};

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

// ---- what the entries check of their arguments
// The refusal of an argument: `return refuse("NULL argument")` leaves "<who>: NULL argument" behind cs_last_error().  The string is built
// only when it fires.
struct Refuse {
  const char* who;
  int operator()(const char* what) const { cs_set_error(std::string(who) + ": " + what); return CS_ERR_INVALID_ARG; }
};

// The kernels index their records by ptr alone: it must be a non-decreasing partition, ptr[0] = 0.  `what` = "<entry>: <the array's name>".
inline int check_partition(const std::string& what, const int* ptr, int n) {
  if (ptr[0] != 0) { cs_set_error(what + "[0] must be 0"); return CS_ERR_INVALID_ARG; }
  for (int f = 0; f < n; f++)
    if (ptr[f + 1] < ptr[f]) { cs_set_error(what + " must not decrease"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

inline bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

inline bool none_negative(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!(v[i] >= 0)) return false;
  return true;
}

inline bool positive(double x) { return std::isfinite(x) && x > 0; }

// false: the quaternion (four doubles, any order) has zero norm, or its norm overflows or is not a number
inline bool quaternion_norm_ok(const double* q4) { return positive(std::sqrt(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3])); }

// ---- the chunk table (cs_chunk.h) of a partition ptr[0 .. n_owners]: owner f's items ptr[f] .. ptr[f + 1] - 1 in chunks of at most `width`,
// owner after owner, an owner without items without a chunk
inline size_t chunk_count(const int* ptr, size_t n_owners, int width) {
  size_t n = 0;
  for (size_t f = 0; f < n_owners; f++) n += ((size_t)(ptr[f + 1] - ptr[f]) + width - 1) / width;
  return n;
}

inline void chunk_fill(const int* ptr, size_t n_owners, int width, Chunk* chunk) {
  for (size_t f = 0; f < n_owners; f++)
    for (int first = ptr[f]; first < ptr[f + 1]; first += width, chunk++) {
      const int left = ptr[f + 1] - first;
      chunk->owner = (int)f; chunk->first = first; chunk->count = left < width ? left : width; chunk->pad = 0;
    }
}

// out[f] = how many of owner f's items have status `ok`
inline void count_status(const int* ptr, size_t n_owners, const unsigned char* status, int ok, int* out) {
  for (size_t f = 0; f < n_owners; f++) {
    int n = 0;
    for (int i = ptr[f]; i < ptr[f + 1]; i++) n += status[i] == ok ? 1 : 0;
    out[f] = n;
  }
}

}  // namespace cs
