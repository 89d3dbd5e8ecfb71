// edge_types.h -- what detect_host.cpp hands to edge_kernels.hip (the distance-map front end and the batched table copy).
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

struct EdgeRoi {
  int l, t, w, h;            // ROI inside the gray image
  long long img_off;         // -> first pixel of the ROI's image in the gray pool
  long long cls_off;         // -> class bytes (w * h)
  long long map_off;         // -> output floats (w * h)
};

// A handful of tables between PINNED host memory and device memory in ONE launch (either direction; the host side is addressed through the
// unified address space).  Why not one hipMemcpyAsync each: ten small copies are ten trips through a copy-engine ring (~0.3 ms of latency in
// front of a sweep, ~0.15 ms behind it), and a ring that holds a bulk upload (cs_batch_refill_gray) makes every one of them wait for it.
struct CopySeg { const void* src; void* dst; unsigned long long bytes; };
struct CopySegs { CopySeg s[16]; int n; };
// appends the copy of cnt elements of from's buffer to to's (nothing when cnt is 0)
template <class To, class From> inline void add_copy(CopySegs& cp, const To& to, const From& from, long long cnt) {
  if (cnt > 0) { cp.s[cp.n].src = from.p; cp.s[cp.n].dst = to.p; cp.s[cp.n].bytes = sizeof(*from.p) * (unsigned long long)cnt; cp.n++; }
}

void launch_multi_copy(const CopySegs& segs, hipStream_t st);
void launch_edge_maps(const unsigned char* gray, int W, int H, const EdgeRoi* rois, int n_rois, unsigned char* cls_pool, float* map_pool, int max_w, long long max_px, int low, int high,
                      hipStream_t st);

}  // namespace cs
