// cs_worker_pool.h -- the persistent worker pool of the detector's host stages (one per detector; the calling thread takes part).
// Plain C++: tests/test_worker_pool_cpu.py builds tools/hostonly/worker_pool_check.cpp against it under the thread sanitizer.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace cs {

// run() publishes (fn, n) under the lock and bumps the generation; every worker wakes once per generation, takes items off the shared
// counter unless `limit` threads have joined already, and reports back; run() returns when all workers have reported (so fn outlives its use).
// The caller's place among the `limit` is taken before the workers are woken: it always takes items, and with a limit of 1 it alone does.
class WorkerPool {
 public:
  explicit WorkerPool(int n_workers) {
    for (int i = 0; i < n_workers; i++) th_.emplace_back([this]() { loop(); });
  }
  ~WorkerPool() {
    { std::lock_guard<std::mutex> lk(m_); stop_ = true; gen_++; }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // max_threads: at most this many threads (the caller included) take items -- for items that run for milliseconds, where more
  // runnable threads than the CPU quota tolerates only get the process throttled
  void run(int n, const std::function<void(int)>& fn, int max_threads = 0x7fffffff) {
    if (n <= 0) return;
    if (th_.empty() || n == 1) { for (int i = 0; i < n; i++) fn(i); return; }
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn; n_ = n; next_.store(0); joined_.store(1); limit_ = std::max(1, max_threads); pending_ = (int)th_.size(); gen_++;
    }
    cv_.notify_all();
    work(true);
    std::unique_lock<std::mutex> lk(m_);
    done_.wait(lk, [this]() { return pending_ == 0; });
    fn_ = nullptr;
  }
 private:
  void work(bool caller) {
    if (!caller && joined_.fetch_add(1) >= limit_) return;
    for (;;) {
      int i = next_.fetch_add(1);
      if (i >= n_) break;
      (*fn_)(i);
    }
  }
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&]() { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
      }
      work(false);
      {
        std::lock_guard<std::mutex> lk(m_);
        if (--pending_ == 0) done_.notify_all();
      }
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int)>* fn_ = nullptr;
  std::atomic<int> next_{0}, joined_{0};
  int n_ = 0, pending_ = 0, limit_ = 0x7fffffff;
  unsigned long long gen_ = 0;
  bool stop_ = false;
};

}  // namespace cs
