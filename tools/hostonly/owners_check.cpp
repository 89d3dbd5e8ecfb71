// owners_check.cpp -- the types that own device resources (cube_slam_wu_amd/csrc/cs_hip_util.h: DevBuf, PinBuf, Stream, Event, Guard;
// ba_dbuf.h: DBuf, StageArena) on their own, without a GPU: compiled against a counting stand-in for <hip/hip_runtime.h>
// (tools/hostonly/hip_standin, first on the include path), in which a free or destroy of something that is not live aborts.
//   * After every scenario nothing is live: device memory, pinned memory, streams, events.
//   * The capacities follow the three growth rules, restated HERE; DBuf::append_ptr keeps the old contents across a regrow.
//   * None of the types can be copied.
// tests/test_owners_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/ba_dbuf.h"

void cs_set_error(const std::string& s) { std::printf("cs_set_error: %s\n", s.c_str()); }
namespace cs { struct BaCopyItem { void* dst; const void* src; size_t bytes; }; }      // (ba_types.h's, for upload_ptr_deferred)

static_assert(!std::is_copy_constructible<cs::DevBuf<int>>::value && !std::is_copy_assignable<cs::DevBuf<int>>::value, "DevBuf");
static_assert(!std::is_copy_constructible<cs::PinBuf<int>>::value && !std::is_copy_assignable<cs::PinBuf<int>>::value, "PinBuf");
static_assert(!std::is_copy_constructible<DBuf<int>>::value && !std::is_copy_assignable<DBuf<int>>::value, "DBuf");
static_assert(!std::is_copy_constructible<StageArena>::value && !std::is_copy_assignable<StageArena>::value, "StageArena");
static_assert(!std::is_copy_constructible<cs::Stream>::value && !std::is_copy_assignable<cs::Stream>::value, "Stream");
static_assert(!std::is_copy_constructible<cs::Event>::value && !std::is_copy_assignable<cs::Event>::value, "Event");
static_assert(!std::is_copy_constructible<cs::Guard<int>>::value, "Guard");

static long g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { g_fail++; std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

static size_t n_live(int kind) { return hip_standin::live(kind).size(); }
static void nothing_live(const char* scenario) {
  const size_t n[4] = {n_live(hip_standin::DEVICE), n_live(hip_standin::PINNED), n_live(hip_standin::STREAM), n_live(hip_standin::EVENT)};
  if (n[0] || n[1] || n[2] || n[3]) { g_fail++; std::printf("FAIL after '%s': live device %zu pinned %zu streams %zu events %zu\n", scenario, n[0], n[1], n[2], n[3]); }
}

// the three growth rules, restated (never taken from the headers)
static size_t rule_ensure(size_t n) { return n + n / 8 + 64; }                                               // DevBuf / PinBuf
static size_t rule_reserve(bool first, size_t count) { return first ? count : count + count / 4 + 64; }      // DBuf::reserve
static size_t rule_append(size_t n, size_t count, size_t cap) { return std::max(n + count, cap + cap / 2 + 16); }

// a handle as the library's create functions make them: streams first, then what is queued on them
struct Toy {
  cs::Stream st, side;
  cs::Event ev[4];
  cs::DevBuf<double> d;
  cs::PinBuf<int> h;
  DBuf<int> g;
  StageArena arena;
};
static int g_toy_destroyed = 0;
static void toy_destroy(Toy* t) { g_toy_destroyed++; delete t; }
static int toy_create(bool fail_half_way, Toy** out) {
  *out = nullptr;
  cs::Guard<Toy> g(new Toy(), toy_destroy);
  Toy* t = g.h;
  CS_TRY(t->st.create(hipStreamNonBlocking));
  CS_TRY(t->side.create(hipStreamNonBlocking, -1));
  CS_TRY(t->ev[0].create());
  CS_TRY(t->ev[1].create(hipEventDisableTiming));
  CS_ENSURE(t->d, 100);
  CS_ENSURE(t->h, 4);
  CS_TRY(t->g.alloc(7, t->st));
  CS_TRY(t->arena.begin(1 << 12));
  if (fail_half_way) return CS_ERR_INVALID_ARG;      // (what a refused rocBLAS handle or a bad parameter does in a create function)
  *out = g.disarm();
  return CS_OK;
}

int main() {
  {   // default-constructed and never used
    cs::DevBuf<double> a; cs::PinBuf<int> b; DBuf<float> c; StageArena d; cs::Stream s; cs::Event e, arr[8]; cs::Guard<Toy> g(nullptr, toy_destroy);
    CHECK(!a.p && !b.p && !c.p && !d.p && !s && !e && !arr[7] && !g.h);
  }
  nothing_live("default-constructed");
  CHECK(g_toy_destroyed == 0);

  {   // grown three times, each by its own rule
    cs::DevBuf<double> a; cs::PinBuf<int> b; DBuf<float> c; StageArena d;
    const size_t steps[3] = {10, 100, 1000};
    for (int i = 0; i < 3; i++) {
      CHECK(a.ensure(steps[i]) == CS_OK && a.cap == rule_ensure(steps[i]));
      CHECK(b.ensure(steps[i]) == CS_OK && b.cap == rule_ensure(steps[i]));
      CHECK(c.reserve(steps[i]) == CS_OK && c.cap == rule_reserve(i == 0, steps[i]));
      CHECK(d.begin(64 * steps[i]) == CS_OK && d.cap == 64 * steps[i] && d.off == 0);
      CHECK(n_live(hip_standin::DEVICE) == 2 && n_live(hip_standin::PINNED) == 2);       // (the old allocation went when the new one came)
    }
    CHECK(a.ensure(5) == CS_OK && a.cap == rule_ensure(1000) && c.reserve(5) == CS_OK && c.cap == rule_reserve(false, 1000));      // grow-only
    CHECK(c.reserve(0) == CS_OK);
    DBuf<int> one; CHECK(one.reserve(0) == CS_OK && one.cap == 1);       // (an empty table still has an address)
    // the pinned scalars of the bundle adjustment: grown only below `need`, then to need + need / 4 + 256 through ensure()
    cs::PinBuf<double> h; size_t need = 16;
    if (h.cap < need) CHECK(h.ensure(need + need / 4 + 256) == CS_OK);
    const size_t cap0 = h.cap; CHECK(cap0 == rule_ensure(16 + 4 + 256));
    need = cap0; if (h.cap < need) CHECK(h.ensure(need + need / 4 + 256) == CS_OK);
    CHECK(h.cap == cap0);
  }
  nothing_live("grown three times");

  {   // release() early, then the scope's end: the second time does nothing
    cs::DevBuf<double> a; cs::PinBuf<int> b; DBuf<float> c; StageArena d;
    CHECK(a.ensure(3) == CS_OK && b.ensure(3) == CS_OK && c.alloc(3) == CS_OK && d.begin(256) == CS_OK);
    a.release(); b.release(); c.release(); d.release();
    nothing_live("release()");
    CHECK(!a.p && !a.cap && !b.p && !b.cap && !c.p && !c.cap && !c.n && !d.p && !d.cap);
    a.release(); c.release();
    CHECK(a.ensure(3) == CS_OK && c.reserve(3) == CS_OK && c.cap == 3);      // (and they can be used again: the first allocation's rule)
  }
  nothing_live("release() and scope exit");

  {   // an array of events of which only some were created; streams with and without a priority
    cs::Event ev[8]; cs::Stream st[3];
    for (int i = 0; i < 3; i++) CHECK(ev[i].create(i ? hipEventDisableTiming : hipEventDefault) == CS_OK);
    CHECK(st[0].create(hipStreamNonBlocking) == CS_OK && st[2].create(hipStreamNonBlocking, -1) == CS_OK);
    CHECK(n_live(hip_standin::EVENT) == 3 && n_live(hip_standin::STREAM) == 2);
    hipEvent_t raw = ev[1]; hipStream_t raw_st = st[2];       // (the conversions the HIP calls rely on)
    CHECK(raw == ev[1].e && raw_st == st[2].s && !ev[5] && !st[1]);
  }
  nothing_live("events partly created");

  {   // a creation guard that fires gives everything back through the destroy function, once
    Toy* t = (Toy*)1;
    CHECK(toy_create(true, &t) == CS_ERR_INVALID_ARG && t == nullptr && g_toy_destroyed == 1);
  }
  nothing_live("guard fired");

  {   // ... and a disarmed one leaves the handle to its caller
    Toy* t = nullptr;
    CHECK(toy_create(false, &t) == CS_OK && t != nullptr && g_toy_destroyed == 1);
    CHECK(n_live(hip_standin::STREAM) == 2 && n_live(hip_standin::EVENT) == 2 && n_live(hip_standin::DEVICE) == 2 && n_live(hip_standin::PINNED) == 2);
    CHECK(t->g.n == 7 && t->g.cap == 7);
    toy_destroy(t);
    CHECK(g_toy_destroyed == 2);
  }
  nothing_live("guard disarmed");

  {   // append_ptr: the capacities of a stated series of calls, and the contents across every regrow
    DBuf<int> d;
    const size_t counts[5] = {5, 11, 1, 100, 0};
    std::vector<int> all;
    size_t n = 0, cap = 0;
    for (size_t count : counts) {
      std::vector<int> rows(count);
      for (size_t i = 0; i < count; i++) rows[i] = (int)(1000 * (all.size() + 1) + i);
      if (count && (cap == 0 || n + count > cap)) cap = rule_append(n, count, cap);
      n += count;
      CHECK(d.append_ptr(rows.data(), count) == CS_OK && d.n == n && d.cap == cap);
      all.insert(all.end(), rows.begin(), rows.end());
      CHECK(n_live(hip_standin::DEVICE) == 1);
      CHECK(std::equal(all.begin(), all.end(), d.p));       // (the stand-in's device memory is the host's)
    }
    CHECK(cap == 117 && n == 117);       // 16, 16, 40, 117, 117 by hand
    // the staged and deferred forms through an arena, beside it
    StageArena arena; cs::Stream st; DBuf<int> e; std::vector<cs::BaCopyItem> list;
    CHECK(arena.begin(1 << 12) == CS_OK && st.create(hipStreamNonBlocking) == CS_OK);
    CHECK(e.upload_ptr_deferred(all.data(), 10, arena, list, st) == CS_OK && list.size() == 1 && list[0].dst == e.p && list[0].bytes == 40 && e.cap == 10);
    CHECK(e.append_ptr_staged(all.data(), 20, arena, st) == CS_OK && e.n == 30 && e.cap == rule_append(10, 20, 10));     // (no room: the plain append)
    const size_t off = arena.off;
    CHECK(e.append_ptr_staged(all.data(), 1, arena, st) == CS_OK && e.n == 31 && e.cap == 31 && arena.off > off);       // (room: in place, through the arena)
  }
  nothing_live("append_ptr");

  if (g_fail) { std::printf("owners_check: %ld FAILED\n", g_fail); return 1; }
  std::printf("owners_check: ok\n");
  return 0;
}
