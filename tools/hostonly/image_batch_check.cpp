// image_batch_check.cpp -- the segment producers' batch driver (cube_slam_wu_amd/csrc/cs_image_batch.h: run_image_batch, ChunkGate, ChunkEvents,
// ImageBatchScratch) on its own, without a GPU: compiled against the counting stand-in for <hip/hip_runtime.h> (tools/hostonly/hip_standin, first
// on the include path), where copies are memcpy at the moment they are queued, events are tokens, and one knob makes the k-th hipEventSynchronize
// fail.  The detector's hooks are defined HERE: a null stream, device 0, a real mutex, and a pool of a few std::threads that take task indices in
// ascending order (so task 0, the gate's watcher, runs while the image tasks wait).  A fake launch fills each image's output slice from its input
// slice by a rule that differs per image and per byte; a fake stage checks its own slice against the rule when it runs.
//   * launches cover [0, n) once, in order, in chunks of BATCH_CHUNK, for n in {1, 2, 4, 5, 8, 9}; one image: one launch, the pool untouched
//   * every image's stage runs once and sees its own slice
//   * a failing stage's code comes back (the lowest image's of two) and every other stage still runs; a throwing stage gives CS_ERR_CAPACITY
//   * a failing `done` event: the call returns CS_ERR_HIP and every task returns.  The rule of ChunkGate: the watcher takes the events in chunk
//     order; the first one that fails sets `failed` and opens the gate for ALL images at once, and wait_for reports `failed` as it stands when
//     the waiter gets through.  So with chunk c's event failing, no stage runs for an image >= c * BATCH_CHUNK (its slice was never declared
//     ready with `failed` unset); an image below that ran its stage if it passed the gate before the failure and got CS_ERR_HIP if after --
//     at most once either way.
//   * one scratch over 9 images, 1 larger image, 3 images: right results, `chunks` holds three triples and never shrinks
//   * nothing is live in the stand-in once the scratch is gone
// tests/test_image_batch_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <atomic>
#include <cstdio>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_image_batch.h"

void cs_set_error(const std::string& s) { std::printf("cs_set_error: %s\n", s.c_str()); }

static long g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { g_fail++; std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

// ---- the detector's hooks ----------------------------------------------------------------------------------------------------------------------
struct cs_detector { std::mutex mu; int n_parallel = 0, n_parallel_long = 0; };
static void pool_run(int n, void (*fn)(int, void*), void* ctx) {
  std::atomic<int> next{0};
  auto work = [&] { for (int i; (i = next.fetch_add(1)) < n;) fn(i, ctx); };
  std::thread t[3];
  for (auto& th : t) th = std::thread(work);
  for (auto& th : t) th.join();
}
extern "C" void* cs_internal_detector_stream(cs_detector*) { return nullptr; }
extern "C" int cs_internal_detector_device(cs_detector*) { return 0; }
extern "C" void* cs_internal_detector_lines_mutex(cs_detector* d) { return &d->mu; }
extern "C" void cs_internal_detector_parallel(cs_detector* d, int n, void (*fn)(int, void*), void* ctx) { d->n_parallel++; pool_run(n, fn, ctx); }
extern "C" void cs_internal_detector_parallel_long(cs_detector* d, int n, void (*fn)(int, void*), void* ctx) { d->n_parallel_long++; pool_run(n, fn, ctx); }

// ---- a toy producer ------------------------------------------------------------------------------------------------------------------------------
struct ToyScratch : cs::ImageBatchScratch {
  cs::DevBuf<unsigned char> d_out;
  cs::PinBuf<unsigned char> h_out;
};
enum Behaviour { FINE, FAILS_7, FAILS_9, THROWS_BAD_ALLOC, THROWS_RUNTIME_ERROR };
constexpr size_t kPad = 5;      // out_stride - out_bytes: the slices do not touch
constexpr unsigned char kUntouched = 0xA5;

static unsigned char pixel(int seed, int i, size_t b) { return (unsigned char)(seed * 131 + i * 29 + b * 7 + (b >> 8)); }
static unsigned char rule(unsigned char in, int i, size_t b) { return (unsigned char)(in + 13 * i + 3 * b + 1); }

struct Call {
  int rc = 0;
  std::vector<std::pair<int, int>> launches;
  std::vector<int> staged, wrong;      // per image: times its stage ran, times it did not see its own slice
};
// one producer call as lines_host.cpp / lsd_host.cpp make it: lock, scratch, buffers, the two callables, the driver
static Call toy_call(cs_detector* d, ToyScratch& S, int n, size_t in_bytes, int seed, const std::vector<Behaviour>& how = {}) {
  Call c;
  c.staged.assign(n, 0); c.wrong.assign(n, 0);
  std::vector<std::vector<unsigned char>> img(n, std::vector<unsigned char>(in_bytes));
  std::vector<const unsigned char*> grays(n);
  for (int i = 0; i < n; i++) { for (size_t b = 0; b < in_bytes; b++) img[i][b] = pixel(seed, i, b); grays[i] = img[i].data(); }
  const size_t out_bytes = 2 * in_bytes + 3, stride = out_bytes + kPad;
  std::lock_guard<std::mutex> lk(*(std::mutex*)cs_internal_detector_lines_mutex(d));
  const double t_begin = cs::now_ms();
  CHECK(S.d_gray.ensure(in_bytes * n) == CS_OK && S.h_in.ensure(in_bytes * n) == CS_OK && S.d_out.ensure(stride * n) == CS_OK && S.h_out.ensure(stride * n) == CS_OK);
  std::memset(S.d_out.p, kUntouched, stride * n); std::memset(S.h_out.p, kUntouched, stride * n);
  auto launch = [&](int i0, int ni) {
    c.launches.push_back({i0, ni});
    for (int i = i0; i < i0 + ni; i++)
      for (size_t b = 0; b < out_bytes; b++) S.d_out.p[stride * i + b] = rule(S.d_gray.p[in_bytes * i + b % in_bytes], i, b);
  };
  auto stage = [&](int i) -> int {
    c.staged[i]++;
    for (size_t b = 0; b < out_bytes; b++) if (S.h_out.p[stride * i + b] != rule(img[i][b % in_bytes], i, b)) { c.wrong[i]++; break; }
    switch (how.empty() ? FINE : how[i]) {
      case FAILS_7: return 7;
      case FAILS_9: return 9;
      case THROWS_BAD_ALLOC: throw std::bad_alloc();
      case THROWS_RUNTIME_ERROR: throw std::runtime_error("stage");
      default: return CS_OK;
    }
  };
  c.rc = cs::run_image_batch(d, S, t_begin, grays.data(), n, in_bytes, S.d_out.p, S.h_out.p, out_bytes, stride, launch, stage);
  for (size_t b = stride * n - kPad; b < stride * n; b++) CHECK(S.h_out.p[b] == kUntouched);      // the last copy back ends with the last slice
  return c;
}
static bool all_staged_once(const Call& c) {
  for (size_t i = 0; i < c.staged.size(); i++) if (c.staged[i] != 1 || c.wrong[i]) return false;
  return true;
}
static bool launches_in_chunks(const Call& c, int n) {
  const int CH = cs::BATCH_CHUNK;
  if ((int)c.launches.size() != (n + CH - 1) / CH) return false;
  for (size_t k = 0; k < c.launches.size(); k++)
    if (c.launches[k].first != (int)k * CH || c.launches[k].second != std::min(CH, n - (int)k * CH)) return false;
  return true;
}
static size_t n_live(int kind) { return hip_standin::live(kind).size(); }

int main() {
  {   // launch coverage, every image staged once
    for (int n : {1, 2, 4, 5, 8, 9}) {
      cs_detector d; ToyScratch S;
      const Call c = toy_call(&d, S, n, 301, n);
      CHECK(c.rc == CS_OK && launches_in_chunks(c, n) && all_staged_once(c));
      if (n == 1) CHECK(c.launches.size() == 1 && d.n_parallel == 0 && d.n_parallel_long == 0 && S.chunks.done.empty() && S.device_ms == 0.25);
      else CHECK(d.n_parallel == 1 && d.n_parallel_long == 1 && (int)S.chunks.done.size() == (n + 3) / 4 && S.device_ms == 0.25 * ((n + 3) / 4));
      CHECK(S.host_ms >= 0 && S.total_ms >= S.host_ms);
      double dev = -1, host = -1, total = -1;
      CHECK(cs::batch_last_timing(S, &dev, &host, &total) == CS_OK && dev == S.device_ms && host == S.host_ms && total == S.total_ms);
      CHECK(cs::batch_last_timing(S, nullptr, nullptr, nullptr) == CS_OK);
    }
  }
  {   // failing and throwing stages: in a batch and in the one-image path
    cs_detector d; ToyScratch S;
    std::vector<Behaviour> how(9, FINE);
    how[6] = FAILS_7;
    Call c = toy_call(&d, S, 9, 64, 1, how);
    CHECK(c.rc == 7 && all_staged_once(c));
    how[2] = FAILS_9;      // two failing images: the lower index wins
    c = toy_call(&d, S, 9, 64, 2, how);
    CHECK(c.rc == 9 && all_staged_once(c));
    how[2] = THROWS_BAD_ALLOC;
    c = toy_call(&d, S, 9, 64, 3, how);
    CHECK(c.rc == CS_ERR_CAPACITY && all_staged_once(c));
    how[2] = FINE; how[6] = THROWS_RUNTIME_ERROR;
    c = toy_call(&d, S, 9, 64, 4, how);
    CHECK(c.rc == CS_ERR_CAPACITY && all_staged_once(c));
    for (Behaviour b : {FAILS_7, THROWS_BAD_ALLOC, THROWS_RUNTIME_ERROR}) {
      c = toy_call(&d, S, 1, 64, 5, {b});
      CHECK(c.rc == (b == FAILS_7 ? 7 : CS_ERR_CAPACITY) && all_staged_once(c));
    }
  }
  {   // the second chunk's `done` event fails (the watcher makes the only hipEventSynchronize calls)
    cs_detector d; ToyScratch S;
    hip_standin::event_sync_fails_in() = 2;
    const Call c = toy_call(&d, S, 9, 64, 6);
    CHECK(hip_standin::event_sync_fails_in() == 0);
    CHECK(c.rc == CS_ERR_HIP && launches_in_chunks(c, 9) && d.n_parallel_long == 1);
    for (int i = 0; i < 9; i++) CHECK((i < cs::BATCH_CHUNK ? c.staged[i] <= 1 : c.staged[i] == 0) && !c.wrong[i]);
    // ... and the first chunk's: no stage at all
    hip_standin::event_sync_fails_in() = 1;
    const Call c0 = toy_call(&d, S, 5, 64, 7);
    CHECK(c0.rc == CS_ERR_HIP);
    for (int i = 0; i < 5; i++) CHECK(c0.staged[i] == 0);
    // the scratch serves the next call
    const Call c1 = toy_call(&d, S, 5, 64, 8);
    CHECK(c1.rc == CS_OK && all_staged_once(c1));
  }
  {   // reuse: 9 images, 1 larger image, 3 images of the first size
    cs_detector d;
    {
      ToyScratch S;
      Call c = toy_call(&d, S, 9, 200, 9);
      CHECK(c.rc == CS_OK && launches_in_chunks(c, 9) && all_staged_once(c) && S.chunks.done.size() == 3);
      const std::vector<hipEvent_t> done = S.chunks.done, k0 = S.chunks.k0, k1 = S.chunks.k1;
      c = toy_call(&d, S, 1, 5000, 10);
      CHECK(c.rc == CS_OK && launches_in_chunks(c, 1) && all_staged_once(c) && S.chunks.done == done);
      c = toy_call(&d, S, 3, 200, 11);
      CHECK(c.rc == CS_OK && launches_in_chunks(c, 3) && all_staged_once(c));
      CHECK(S.chunks.done == done && S.chunks.k0 == k0 && S.chunks.k1 == k1);
      CHECK(n_live(hip_standin::EVENT) == 3 * 3 + 2 && n_live(hip_standin::DEVICE) == 2 && n_live(hip_standin::PINNED) == 2);
      CHECK(d.n_parallel == 2 && d.n_parallel_long == 2);
    }
    CHECK(!n_live(hip_standin::DEVICE) && !n_live(hip_standin::PINNED) && !n_live(hip_standin::EVENT) && !n_live(hip_standin::STREAM));
  }
  CHECK(!n_live(hip_standin::DEVICE) && !n_live(hip_standin::PINNED) && !n_live(hip_standin::EVENT) && !n_live(hip_standin::STREAM));

  if (g_fail) { std::printf("image_batch_check: %ld FAILED\n", g_fail); return 1; }
  std::printf("image_batch_check: ok\n");
  return 0;
}
