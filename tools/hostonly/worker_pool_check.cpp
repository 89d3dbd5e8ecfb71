// worker_pool_check.cpp -- cs::WorkerPool (cube_slam_wu_amd/csrc/cs_worker_pool.h) on its own: run(n, fn) calls fn exactly once for every i in
// [0, n), run after run without a lost or doubled item, and max_threads bounds the threads that take items (1: the caller alone).
// tests/test_worker_pool_cpu.py builds it with the host compiler under the thread sanitizer and runs it.
#include <atomic>
#include <cstdio>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_worker_pool.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// every item once: the per-item counters are plain ints on purpose -- two threads taking the same item is a race the sanitizer reports too
static void check_each_once(cs::WorkerPool& pool, int workers, int n) {
  std::vector<int> hits((size_t)(n > 0 ? n : 0), 0);
  std::atomic<int> calls{0};
  pool.run(n, [&](int i) { hits[(size_t)i]++; calls++; });
  int bad = 0;
  for (int h : hits) bad += h != 1;
  CHECK(bad == 0 && calls.load() == (n > 0 ? n : 0), "%d workers, n = %d: %d items not called once, %d calls", workers, n, bad, calls.load());
}

static void check_thread_limit(cs::WorkerPool& pool, int workers, int max_threads) {
  std::mutex mu;
  std::set<std::thread::id> ids;
  std::vector<int> hits(400, 0);
  for (int rep = 0; rep < 50; rep++)
    pool.run(400, [&](int i) {
      hits[(size_t)i]++;
      std::lock_guard<std::mutex> lk(mu);
      ids.insert(std::this_thread::get_id());
    }, max_threads);
  int bad = 0;
  for (int h : hits) bad += h != 50;
  CHECK(bad == 0, "%d workers, max_threads %d: %d items not called once per run", workers, max_threads, bad);
  // (the threads that take items may differ from run to run, so the bound is checked per run below; over all runs the caller is always one of them)
  CHECK(ids.count(std::this_thread::get_id()) == 1, "%d workers, max_threads %d: the caller took no item", workers, max_threads);
  if (max_threads == 1) CHECK(ids.size() == 1, "%d workers, max_threads 1: %d threads took items", workers, (int)ids.size());
  for (int rep = 0; rep < 50; rep++) {
    ids.clear();
    pool.run(400, [&](int) { std::lock_guard<std::mutex> lk(mu); ids.insert(std::this_thread::get_id()); }, max_threads);
    CHECK((int)ids.size() <= max_threads, "%d workers, max_threads %d: %d threads took items in one run", workers, max_threads, (int)ids.size());
  }
}

int main() {
  for (int workers : {0, 1, 5}) {
    cs::WorkerPool pool(workers);
    for (int n : {0, 1, 2, 7, 1000}) check_each_once(pool, workers, n);
    // a thousand runs back to back: the generation / pending handshake must neither lose a run's items nor hand one out twice
    std::vector<int> hits(7, 0);
    for (int rep = 0; rep < 1000; rep++) pool.run(7, [&](int i) { hits[(size_t)i]++; });
    int bad = 0;
    for (int h : hits) bad += h != 1000;
    CHECK(bad == 0, "%d workers: %d of 7 items not called 1000 times in 1000 runs", workers, bad);
    check_thread_limit(pool, workers, 1);
    check_thread_limit(pool, workers, 2);
  }
  if (g_fail) { std::printf("worker_pool_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("worker_pool_check: ok\n");
  return 0;
}
