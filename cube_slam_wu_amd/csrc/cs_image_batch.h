// cs_image_batch.h -- the batch driver of the two segment producers (lines_host.cpp: EDLines, lsd_host.cpp: LSD): n images of one size go up in
// one copy, through the producer's kernels and back chunk by chunk, and each image's sequential host stage runs on the detector's worker pool as
// soon as its chunk is in host memory -- the kernels and the copy back of chunk c + 1 run while the pool walks the images of chunk c.  A producer
// supplies its scratch (ImageBatchScratch plus its own buffers), what to launch for a run of images and the host stage of one image; everything
// else -- the order of work on the stream, the gate, the failure rules, the timings -- is run_image_batch, below.
// Plain host C++ over the HIP runtime and the detector's hooks: tools/hostonly/image_batch_check.cpp runs it without a GPU.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <exception>
#include <mutex>
#include <vector>

#include "cs_hip_util.h"
#include "detect_hooks.h"

namespace cs {

enum { BATCH_CHUNK = 4 };      // images per chunk (a chunk's copy back is ~1 ms at KITTI size: the pool starts that long after the call)

// Task 0 of the pool run watches the chunks' events (blocking-sync events: the watcher sleeps) and opens the gate; an image's task sleeps on
// the gate until its chunk has arrived.
struct ChunkGate {
  std::mutex m;
  std::condition_variable cv;
  int ready = 0;               // images [0, ready) are in host memory
  bool failed = false;

  void watch(int device, const hipEvent_t* done, int n_chunks, int chunk, int n_images) {
    (void)hipSetDevice(device);
    for (int c = 0; c < n_chunks; c++) {
      const hipError_t e = hipEventSynchronize(done[c]);
      std::lock_guard<std::mutex> lk(m);
      if (e != hipSuccess) { failed = true; ready = n_images; cv.notify_all(); return; }   // (nobody may wait for ever)
      ready = std::min(n_images, (c + 1) * chunk);
      cv.notify_all();
    }
  }
  bool wait_for(int i) {       // false: a chunk's event reported an error
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return ready > i; });
    return !failed;
  }
};

// grow-only set of events of a producer's scratch: `done` (blocking sync, no timing) and a timed pair per chunk around its kernels.
// Destroyed with the scratch; not copyable.  (Raw handles side by side: ChunkGate::watch walks `done` as an array.)
struct ChunkEvents {
  std::vector<hipEvent_t> done, k0, k1;
  ChunkEvents() = default;
  ChunkEvents(const ChunkEvents&) = delete;
  ChunkEvents& operator=(const ChunkEvents&) = delete;
  ~ChunkEvents() { release(); }
  hipError_t reserve(int n) {
    while ((int)done.size() < n) {
      hipEvent_t a = nullptr, b = nullptr, c = nullptr;
      hipError_t e = hipEventCreateWithFlags(&a, hipEventBlockingSync | hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventCreate(&b);
      if (e == hipSuccess) e = hipEventCreate(&c);
      if (e != hipSuccess) { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); if (c) (void)hipEventDestroy(c); return e; }
      done.push_back(a); k0.push_back(b); k1.push_back(c);
    }
    return hipSuccess;
  }
  void release() {
    for (hipEvent_t e : done) (void)hipEventDestroy(e);
    for (hipEvent_t e : k0) (void)hipEventDestroy(e);
    for (hipEvent_t e : k1) (void)hipEventDestroy(e);
    done.clear(); k0.clear(); k1.clear();
  }
};

// What every producer's resident scratch holds (grow-only; the producer derives from it and adds its own maps and staging).  The producer
// grows d_gray and h_in itself, beside its own buffers, to n_images x in_bytes before it calls run_image_batch.
struct ImageBatchScratch {
  DevBuf<unsigned char> d_gray;     // the batch's images side by side on the device
  PinBuf<unsigned char> h_in;       // ... and in pinned memory (one upload; not used by a one-image call)
  ChunkEvents chunks;
  Event ev0, ev1;                   // around the kernels of a one-image call
  double device_ms = 0, host_ms = 0, total_ms = 0;      // of the last call: the kernels, the host stages (wall), the whole call
};

// the body of a producer's cs_*_last_timing
inline int batch_last_timing(const ImageBatchScratch& S, double* device_ms, double* host_ms, double* total_ms) {
  if (device_ms) *device_ms = S.device_ms;
  if (host_ms) *host_ms = S.host_ms;
  if (total_ms) *total_ms = S.total_ms;
  return CS_OK;
}

// what the pool's tasks of one run_image_batch share (the hooks take a void (*)(int, void*))
template <class Stage>
struct ImageBatchRun {
  const Stage& stage;
  std::vector<int> rc;               // a CS_* code per image
  const unsigned char* const* grays; unsigned char* h_in; size_t in_bytes;
  ChunkGate gate; int device; const hipEvent_t* done; int n_chunks;
  // image i's host stage: the one place it is called from.  Nothing it throws leaves the image's task (it may be running on a pool thread).
  void run_stage(int i) {
    try { rc[i] = stage(i); }
    catch (const std::exception&) { rc[i] = CS_ERR_CAPACITY; }
  }
};

// Upload, launch per chunk, copy back, host stages behind the gate, timings, first error.  The caller holds the producers' lock, has made the
// detector's device current, has grown S.d_gray / S.h_in and the buffers behind d_out / h_out, and has zeroed its per-image outputs.
//   in_bytes               one input image; image i goes to S.d_gray + in_bytes i
//   d_out, h_out           device results and their pinned copy: image i's out_bytes at out_stride i in both
//   launch(i0, ni)         queues the kernels of images [i0, i0 + ni) on the detector's stream (the driver asks hipGetLastError after it)
//   stage(i)               the host stage of image i over its slice of h_out; returns a CS_* code
//   t_begin                now_ms() just after the producer fetched its scratch: where total_ms counts from
// Returns the first non-zero code in image order, after ALL images have had their turn; a HIP error while queueing returns at once (the
// pool has not started then).  S.host_ms counts from the end of the queueing to the return.
template <class Launch, class Stage>
int run_image_batch(cs_detector* d, ImageBatchScratch& S, double t_begin, const unsigned char* const* grays, int n_images, size_t in_bytes, const void* d_out, void* h_out,
                    size_t out_bytes, size_t out_stride, const Launch& launch, const Stage& stage) {
  using Run = ImageBatchRun<Stage>;
  hipStream_t st = (hipStream_t)cs_internal_detector_stream(d);
  if (!S.ev0) { CS_TRY(S.ev0.create()); CS_TRY(S.ev1.create()); }
  Run run{stage, std::vector<int>(n_images, 0), grays, S.h_in.p, in_bytes, {}, cs_internal_detector_device(d), nullptr, 0};
  double t_host;
  if (n_images == 1) {
    // one image (the latency path): straight from the caller's pointer, no pool, no gate, the stage inline
    CS_HIP_TRY(hipMemcpyAsync(S.d_gray.p, grays[0], in_bytes, hipMemcpyHostToDevice, st));
    CS_HIP_TRY(hipEventRecord(S.ev0, st));
    launch(0, 1);
    CS_HIP_TRY(hipGetLastError());
    CS_HIP_TRY(hipEventRecord(S.ev1, st));
    CS_HIP_TRY(hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    CS_HIP_TRY(hipStreamSynchronize(st));
    float ms = 0;
    CS_HIP_TRY(hipEventElapsedTime(&ms, S.ev0, S.ev1));
    S.device_ms = ms;
    t_host = now_ms();
    run.run_stage(0);
  } else {
    // a batch: the images gathered into pinned memory by the pool (the caller's buffers are pageable: one staged copy per image otherwise), one
    // upload, then chunk by chunk [k0 | kernels | k1 | copy back | done] -- ALL of it queued before the pool starts on the first chunk's images
    cs_internal_detector_parallel(d, n_images, [](int i, void* vp) { Run& r = *(Run*)vp; std::memcpy(r.h_in + r.in_bytes * (size_t)i, r.grays[i], r.in_bytes); }, &run);
    const int CH = BATCH_CHUNK, n_chunks = (n_images + CH - 1) / CH;
    CS_HIP_TRY(S.chunks.reserve(n_chunks));
    CS_HIP_TRY(hipMemcpyAsync(S.d_gray.p, S.h_in.p, in_bytes * (size_t)n_images, hipMemcpyHostToDevice, st));
    for (int c = 0; c < n_chunks; c++) {
      const int i0 = c * CH, ni = std::min(CH, n_images - i0);
      CS_HIP_TRY(hipEventRecord(S.chunks.k0[c], st));
      launch(i0, ni);
      CS_HIP_TRY(hipGetLastError());
      CS_HIP_TRY(hipEventRecord(S.chunks.k1[c], st));
      CS_HIP_TRY(hipMemcpyAsync((char*)h_out + out_stride * (size_t)i0, (const char*)d_out + out_stride * (size_t)i0, out_stride * (size_t)(ni - 1) + out_bytes, hipMemcpyDeviceToHost, st));
      CS_HIP_TRY(hipEventRecord(S.chunks.done[c], st));
    }
    run.done = S.chunks.done.data(); run.n_chunks = n_chunks;
    t_host = now_ms();
    // n + 1 tasks, taken in ascending order: task 0 watches the events and never waits for another task, task i + 1 is image i.  A `done` event
    // that reports an error opens the gate for everybody with `failed` set: every image that has not passed the gate by then gets CS_ERR_HIP
    // and its stage does not run (its slice may not have arrived).
    cs_internal_detector_parallel_long(d, n_images + 1, [](int t, void* vp) {
      Run& r = *(Run*)vp;
      if (t == 0) { r.gate.watch(r.device, r.done, r.n_chunks, BATCH_CHUNK, (int)r.rc.size()); return; }
      const int i = t - 1;
      if (!r.gate.wait_for(i)) { r.rc[i] = CS_ERR_HIP; return; }
      r.run_stage(i);
    }, &run);
    CS_HIP_TRY(hipStreamSynchronize(st));          // (every chunk's event has been waited for; this also surfaces a late error)
    double dev = 0;
    for (int c = 0; c < n_chunks; c++) { float ms = 0; CS_HIP_TRY(hipEventElapsedTime(&ms, S.chunks.k0[c], S.chunks.k1[c])); dev += ms; }
    S.device_ms = dev;
  }
  S.host_ms = now_ms() - t_host; S.total_ms = now_ms() - t_begin;
  for (int r : run.rc) if (r) return r;
  return CS_OK;
}

}  // namespace cs
