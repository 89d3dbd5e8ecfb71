// ba_dbuf.h -- the bundle-adjustment handle's device buffer (DBuf: entries in use beside the capacity, the growing graph's head room) and the
// pinned staging arena of its small uploads (StageArena).  Both free themselves and cannot be copied.  Host only; needs cs_hip_util.h and the
// declaration of cs::BaCopyItem (ba_types.h defines it for whoever calls upload_ptr_deferred).
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "cs_hip_util.h"

namespace cs { struct BaCopyItem; }

// Pinned staging for the structure phase's many small uploads: a blocking hipMemcpy from pageable memory costs ~40 us whatever its
// size, and the phase makes a few dozen; through this arena they are queued on the handle's stream and waited for once.
struct StageArena {
  char* p = nullptr;
  size_t cap = 0, off = 0;
  StageArena() = default;
  StageArena(const StageArena&) = delete;
  StageArena& operator=(const StageArena&) = delete;
  ~StageArena() { release(); }
  void* take(size_t bytes) {          // nullptr: no room (the caller copies directly)
    const size_t at = (off + 63) & ~(size_t)63;
    if (!p || at + bytes > cap) return nullptr;
    off = at + bytes;
    return p + at;
  }
  int begin(size_t want) {            // at the start of a structure phase, the stream idle
    off = 0;
    if (p && cap >= want) return CS_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    CS_HIP_TRY(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
    cap = want;
    return CS_OK;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = off = 0; }
};

inline int g_dbuf_reallocs = 0;     // (diagnostics: device (re)allocations, printed with the structure phase's clock under CS_BA_PROF)
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0, cap = 0;       // entries in use / allocated (grow-only: a graph that is extended frame by frame re-runs the structure phase,
                               // and ~100 hipFree + hipMalloc pairs were a quarter of it at 200 cameras)
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }
  int reserve(size_t count) {
    count = std::max<size_t>(1, count);
    if (p && count <= cap) return CS_OK;
    // (a buffer that has to grow belongs to a graph that is being extended: a quarter of head room, so that the next frames fit --
    // without it every appended frame re-allocated every buffer whose size follows the edges or the points, ~60 of them)
    const size_t want = p ? count + count / 4 + 64 : count;
    g_dbuf_reallocs++;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    CS_HIP_TRY(hipMalloc((void**)&p, want * sizeof(T)));
    cap = want;
    return CS_OK;
  }
  int upload_ptr(const T* h, size_t count) {   // from the caller's memory
    int rc = reserve(count); if (rc) return rc;
    n = count;
    if (n) CS_HIP_TRY(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return CS_OK;
  }
  int append_ptr(const T* h, size_t count) {   // the old contents stay where they are on the device, `count` new entries follow
    if (!count) return CS_OK;
    if (!p || n + count > cap) {               // (with head room: the next frames append in place)
      const size_t want = std::max(n + count, cap + cap / 2 + 16);
      T* q = nullptr;
      CS_HIP_TRY(hipMalloc((void**)&q, want * sizeof(T)));
      if (n) CS_HIP_TRY(hipMemcpy(q, p, n * sizeof(T), hipMemcpyDeviceToDevice));
      if (p) (void)hipFree(p);
      p = q; cap = want;
    }
    CS_HIP_TRY(hipMemcpy(p + n, h, count * sizeof(T), hipMemcpyHostToDevice));
    n += count;
    return CS_OK;
  }
  // the same through a pinned arena, queued on st (a frame's appends: a dozen blocking copies from pageable memory were 0.3-0.5 ms); the
  // arena's contents must stay until st has run (the handle rewinds it after the next structure phase's wait)
  int append_ptr_staged(const T* h, size_t count, StageArena& stage, hipStream_t st) {
    if (!count) return CS_OK;
    const size_t bytes = count * sizeof(T);
    void* pin = (p && n + count <= cap && bytes <= (256u << 10)) ? stage.take(bytes) : nullptr;
    if (!pin) {                                   // growing (the old contents are copied: nothing may still be writing them) or no room
      CS_HIP_TRY(hipStreamSynchronize(st));
      return append_ptr(h, count);
    }
    std::memcpy(pin, h, bytes);
    CS_HIP_TRY(hipMemcpyAsync(p + n, pin, bytes, hipMemcpyHostToDevice, st));
    n += count;
    return CS_OK;
  }
  int upload(const std::vector<T>& h) { return upload_ptr(h.data(), h.size()); }
  int upload_ptr_staged(const T* h, size_t count, StageArena& stage, hipStream_t st) {   // up to 1 MB: through the pinned arena, queued on st (a blocking copy from pageable memory costs 50-100 us)
    const size_t bytes = count * sizeof(T);
    void* pin = (bytes && bytes <= (1u << 20)) ? stage.take(bytes) : nullptr;
    if (!pin) return upload_ptr(h, count);
    int rc = reserve(count); if (rc) return rc;
    n = count;
    std::memcpy(pin, h, bytes);
    CS_HIP_TRY(hipMemcpyAsync(p, pin, bytes, hipMemcpyHostToDevice, st));
    return CS_OK;
  }
  // like upload_ptr_staged, but the copy itself is left to the caller's batched launch (cs::ba_launch_multi_copy): destination, staged
  // source and size are appended to the list.  No room in the arena: a blocking copy now.
  // Tables of more than 64 KB keep their own hipMemcpyAsync (the copy engine moves a large table faster than a kernel reads it over the link:
  // at a million edges the all-kernel form cost the phase 1.5 ms).  (Item is a parameter only so that the declaration above is enough here.)
  template <class Item = cs::BaCopyItem>
  int upload_ptr_deferred(const T* h, size_t count, StageArena& stage, std::vector<Item>& list, hipStream_t st) {
    const size_t bytes = count * sizeof(T);
    if (bytes > (64u << 10)) return upload_ptr_staged(h, count, stage, st);
    void* pin = bytes ? stage.take(bytes) : nullptr;
    if (!pin) return upload_ptr(h, count);
    int rc = reserve(count); if (rc) return rc;
    n = count;
    std::memcpy(pin, h, bytes);
    list.push_back(Item{p, pin, bytes});
    return CS_OK;
  }
  int alloc(size_t count, hipStream_t st = nullptr) {   // zeroed; st: queued on that stream instead of a blocking call per buffer
    int rc = reserve(count); if (rc) return rc;
    n = count;
    if (st) CS_HIP_TRY(hipMemsetAsync(p, 0, std::max<size_t>(1, n) * sizeof(T), st));
    else CS_HIP_TRY(hipMemset(p, 0, std::max<size_t>(1, n) * sizeof(T)));
    return CS_OK;
  }
  // zeroed like alloc(), but the fill is left to the caller's batched launch (cs::ba_launch_multi_zero): ptr / bytes are appended to the list
  int alloc_deferred(size_t count, std::vector<std::pair<void*, size_t>>& zero_list) {
    int rc = reserve(count); if (rc) return rc;
    n = count;
    zero_list.emplace_back((void*)p, std::max<size_t>(1, n) * sizeof(T));
    return CS_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; cap = 0; }
};
