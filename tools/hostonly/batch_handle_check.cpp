// batch_handle_check.cpp -- what the five batched entries share on the host (cube_slam_wu_amd/csrc/cs_batch_handle.h) on its own, without a GPU
// and without the library: compiled against the counting stand-in for <hip/hip_runtime.h> (tools/hostonly/hip_standin, first on the include
// path), where device and pinned memory are malloc, copies are memcpy and everything made is counted.
//   * Layout / Part: every offset a multiple of 256, no two parts overlap, an empty part is legal, and for the five entries' layouts -- the
//     same element types and counts as pose_host.cpp, sim3_pair_host.cpp, sim3_ransac_host.cpp, triangulate_host.cpp and orb_search_host.cpp
//     give Layout::add -- every offset and the total equal the sums those files multiplied out by hand before there was a Part, restated
//     below as plain arithmetic (`Bytes`), at n = 0, n = 1 and an odd n
//   * chunk_count / chunk_fill against an enumeration item by item: owner sizes 0, 1, 63, 64, 65, 128, 129, empty owners first, last and
//     two in a row, no owner at all; every item once and in order, every count in 1 .. 64, no chunk over two owners, pad 0, and as many
//     chunks as there are items that begin one; count_status on the same partitions
//   * BatchCall: ran, kernel_ms and host_ms after empty(), after a refusal before the point of no return, after a failure behind it and
//     after done(), for an entry that puts the point behind its checks and for one that puts it before them
//   * a round trip through copy_in, batch_round_trip and copy_out hands back what the fake kernel made of the input
//   * Refuse and the argument predicates
//   * batch_one_shot: fn's code comes back, and whatever it returns as much is freed as was made -- nothing is live afterwards
// tests/test_batch_handle_cpu.py builds it with the host compiler, plain and with the address and undefined-behaviour sanitizers, and runs it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_batch_handle.h"
#include "../../cube_slam_wu_amd/csrc/orb_search_types.h"
#include "../../cube_slam_wu_amd/csrc/pose_types.h"
#include "../../cube_slam_wu_amd/csrc/sim3_pair_types.h"
#include "../../cube_slam_wu_amd/csrc/sim3_ransac_types.h"
#include "../../cube_slam_wu_amd/csrc/triangulate_types.h"

static std::string g_last_error;
void cs_set_error(const std::string& s) { g_last_error = s; }

static long g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { g_fail++; std::printf("FAIL line %d: %s\n", __LINE__, #cond); } } while (0)

// ---- Layout / Part ------------------------------------------------------------------------------------------------------------------------------
// the layout as it was written before Part: add(bytes) -> the offset, behind 256-byte alignment
struct Bytes {
  size_t bytes = 0;
  std::vector<size_t> off, len;
  void add(size_t n) { off.push_back(bytes); len.push_back(n); bytes = (bytes + n + 255) & ~(size_t)255; }
};
struct Typed {
  cs::Layout l;
  std::vector<size_t> off, len;
  template <class T>
  void add(size_t count) {
    const cs::Part<T> p = l.add<T>(count);
    unsigned char* base = nullptr;
    CHECK(p.count == count && p.bytes() == count * sizeof(T));
    CHECK(reinterpret_cast<unsigned char*>(p.at(base)) - base == (std::ptrdiff_t)p.off);
    off.push_back(p.off); len.push_back(p.bytes());
  }
};
static void same(const Typed& t, const Bytes& b) {
  CHECK(t.l.bytes == b.bytes && t.off == b.off && t.len == b.len);
  CHECK(t.l.bytes % 256 == 0);
  for (size_t k = 0; k < t.off.size(); k++) {
    CHECK(t.off[k] % 256 == 0);
    CHECK(t.off[k] + t.len[k] <= (k + 1 < t.off.size() ? t.off[k + 1] : t.l.bytes));      // (offsets ascend: no part reaches the next one)
  }
}

// nf owners (frames, pairs, jobs), n items, R rounds / hypotheses, c chunks
static void check_layouts(size_t nf, size_t n, size_t R, size_t c, bool inspect) {
  { Typed t; Bytes b;      // cs_pose_batch_optimize: d_in, d_out; cs_pose_linearize_batch: d_out
    t.add<double>(7 * nf); t.add<double>(5 * nf); t.add<double>(n * cs::POSE_OBS_DOUBLES); t.add<int>(nf + 1);
    b.add(7 * nf * 8); b.add(5 * nf * 8); b.add(n * cs::POSE_OBS_DOUBLES * 8); b.add((nf + 1) * 4);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<double>(7 * nf); t.add<double>(nf * R); t.add<int>(nf * R); t.add<unsigned char>(n);
    b.add(7 * nf * 8); b.add(nf * R * 8); b.add(nf * R * 4); b.add(n);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<double>(nf * cs::POSE_SYSTEM_DOUBLES); t.add<unsigned char>(n);
    b.add(nf * cs::POSE_SYSTEM_DOUBLES * 8); b.add(n);
    same(t, b); }
  { Typed t; Bytes b;      // cs_sim3_pairs_optimize: d_in, d_out; cs_sim3_pairs_linearize: d_out
    t.add<double>(8 * nf); t.add<double>(8 * nf); t.add<double>(n * cs::SIM3_PAIR_MATCH_DOUBLES); t.add<int>(nf + 1); t.add<unsigned char>(nf);
    b.add(8 * nf * 8); b.add(8 * nf * 8); b.add(n * cs::SIM3_PAIR_MATCH_DOUBLES * 8); b.add((nf + 1) * 4); b.add(nf);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<double>(8 * nf); t.add<double>(2 * nf); t.add<int>(2 * nf); t.add<int>(nf); t.add<unsigned char>(n);
    b.add(8 * nf * 8); b.add(2 * nf * 8); b.add(2 * nf * 4); b.add(nf * 4); b.add(n);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<double>(4 * n); t.add<double>(28 * n);
    b.add(4 * n * 8); b.add(28 * n * 8);
    same(t, b); }
  { Typed t; Bytes b;      // cs_sim3_ransac_run: d_in, d_out; cs_sim3_ransac_hypotheses: d_out
    t.add<double>(8 * nf); t.add<double>(n * cs::SIM3_RANSAC_MATCH_DOUBLES); t.add<int>(nf + 1); t.add<int>(nf); t.add<unsigned long long>(nf); t.add<unsigned char>(nf);
    b.add(8 * nf * 8); b.add(n * cs::SIM3_RANSAC_MATCH_DOUBLES * 8); b.add((nf + 1) * 4); b.add(nf * 4); b.add(nf * 8); b.add(nf);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<double>(8 * nf); t.add<int>(nf); t.add<int>(nf); t.add<int>(nf); t.add<int>(nf); t.add<unsigned char>(n);
    b.add(8 * nf * 8); b.add(nf * 4); b.add(nf * 4); b.add(nf * 4); b.add(nf * 4); b.add(n);
    same(t, b); }
  { Typed t; Bytes b;
    const size_t each = nf * R;
    t.add<double>(8 * each); t.add<int>(each);
    b.add(8 * each * 8); b.add(each * 4);
    same(t, b); }
  { Typed t; Bytes b;      // cs_triangulate_run / _inspect: d_in, d_out
    t.add<cs::TriPair>(nf); t.add<double>(n * cs::TRI_MATCH_DOUBLES); t.add<cs::Chunk>(c);
    b.add(nf * sizeof(cs::TriPair)); b.add(n * cs::TRI_MATCH_DOUBLES * 8); b.add(c * 16);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<double>(n * cs::TRI_OUT_DOUBLES); t.add<unsigned char>(n); t.add<unsigned char>(n); t.add<double>(inspect ? n * 3 : 0); t.add<unsigned char>(16);
    b.add(n * cs::TRI_OUT_DOUBLES * 8); b.add(n); b.add(n); b.add(inspect ? n * 3 * 8 : 0); b.add(16);
    same(t, b);
    CHECK(t.l.bytes >= 256); }
  { Typed t; Bytes b;      // cs_orb_search_set_frames: d_set (nf frames, n keypoints, R cells); cs_orb_search_run / _inspect: d_in, d_out
    t.add<cs::OrbFrame>(nf); t.add<int>(nf * (R + 1)); t.add<double>(n * cs::ORB_KP_DOUBLES); t.add<int>(n); t.add<unsigned>(n * cs::ORB_DESC_WORDS); t.add<unsigned char>(16);
    b.add(nf * sizeof(cs::OrbFrame)); b.add(nf * (R + 1) * sizeof(int)); b.add(n * cs::ORB_KP_DOUBLES * 8); b.add(n * sizeof(int)); b.add(n * cs::ORB_DESC_WORDS * sizeof(unsigned)); b.add(16);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<cs::OrbJob>(nf); t.add<double>(n * cs::ORB_QUERY_DOUBLES); t.add<unsigned>(n * cs::ORB_DESC_WORDS); t.add<unsigned char>(n); t.add<cs::Chunk>(c);
    b.add(nf * sizeof(cs::OrbJob)); b.add(n * cs::ORB_QUERY_DOUBLES * 8); b.add(n * cs::ORB_DESC_WORDS * sizeof(unsigned)); b.add(n); b.add(c * 16);
    same(t, b); }
  { Typed t; Bytes b;
    t.add<int>(n); t.add<int>(n); t.add<unsigned char>(n); t.add<unsigned char>(n); t.add<double>(inspect ? n * cs::ORB_INSPECT_DOUBLES : 0); t.add<int>(inspect ? n : 0);
    t.add<int>(inspect ? n : 0); t.add<unsigned char>(16);
    b.add(n * sizeof(int)); b.add(n * sizeof(int)); b.add(n); b.add(n); b.add(inspect ? n * cs::ORB_INSPECT_DOUBLES * 8 : 0); b.add(inspect ? n * sizeof(int) : 0);
    b.add(inspect ? n * sizeof(int) : 0); b.add(16);
    same(t, b); }
}

static void check_parts() {
  static_assert(sizeof(cs::Chunk) == 16, "the chunk record");
  cs::Layout l;
  const auto a = l.add<double>(0);                     // an empty part: legal, takes no room, and the next part starts where it does
  const auto b = l.add<int>(3);
  const auto c = l.add<unsigned char>(257);
  CHECK(a.off == 0 && a.bytes() == 0 && b.off == 0 && b.bytes() == 12 && c.off == 256 && c.bytes() == 257 && l.bytes == 768);
  for (int inspect = 0; inspect < 2; inspect++) {
    check_layouts(0, 0, 1, 0, inspect != 0);
    check_layouts(1, 0, 1, 0, inspect != 0);           // an owner without an item
    check_layouts(1, 1, 1, 1, inspect != 0);
    check_layouts(7, 451, 4, 11, inspect != 0);
    check_layouts(33, 2001, 3, 49, inspect != 0);
  }
}

// ---- the chunk table -----------------------------------------------------------------------------------------------------------------------------
static void check_chunks(const std::vector<int>& sizes) {
  const size_t nf = sizes.size();
  std::vector<int> ptr(1, 0), owner_of;
  for (size_t f = 0; f < nf; f++) {
    ptr.push_back(ptr.back() + sizes[f]);
    owner_of.insert(owner_of.end(), (size_t)sizes[f], (int)f);
  }
  const size_t n = owner_of.size();
  size_t begins = 0;                                   // the items that begin a chunk: an owner's first, and every 64th after it
  for (size_t i = 0; i < n; i++) begins += (i - (size_t)ptr[owner_of[i]]) % 64 == 0 ? 1 : 0;
  const size_t n_chunks = cs::chunk_count(ptr.data(), nf, 64);
  CHECK(n_chunks == begins);
  const cs::Chunk untouched = {-7, -7, -7, -7};
  std::vector<cs::Chunk> chunk(n_chunks + 1, untouched);
  cs::chunk_fill(ptr.data(), nf, 64, chunk.data());
  size_t next = 0;
  for (size_t c = 0; c < n_chunks; c++) {
    const cs::Chunk& ch = chunk[c];
    CHECK(ch.count >= 1 && ch.count <= 64 && ch.pad == 0);
    CHECK((size_t)ch.first == next);
    for (int k = 0; k < ch.count && next < n; k++, next++) CHECK(owner_of[next] == ch.owner);
    CHECK(next == (size_t)ch.first + (size_t)ch.count);
  }
  CHECK(next == n);
  CHECK(chunk[n_chunks].owner == -7 && chunk[n_chunks].first == -7 && chunk[n_chunks].count == -7 && chunk[n_chunks].pad == -7);

  std::vector<unsigned char> status(n + 1);
  std::vector<int> want(nf + 1, 0), got(nf + 1, -7);
  for (size_t i = 0; i < n; i++) {
    status[i] = (unsigned char)((i * 7 + i / 5) % 3);
    want[owner_of[i]] += status[i] == 2 ? 1 : 0;
  }
  want[nf] = -7;
  cs::count_status(ptr.data(), nf, status.data(), 2, got.data());
  CHECK(got == want);
}

// ---- BatchCall, the round trip and the one-shot ----------------------------------------------------------------------------------------------------
struct TestHandle : cs::BatchHandle {};
enum What { EMPTY, REFUSED_EARLY, FAILS_LATE, RUNS };

// an entry of either order: `point_first` = the point of no return before the checks (cs_pose_batch_optimize), else behind them
static int entry(TestHandle* B, bool point_first, What what, const std::vector<double>& in, std::vector<double>* out) {
  const cs::Refuse refuse{"entry"};
  cs::BatchCall call(*B);
  if (point_first) call.point_of_no_return();
  if (what == EMPTY) return call.empty();
  if (what == REFUSED_EARLY) return refuse("an argument");
  if (!point_first) call.point_of_no_return();
  if (what == FAILS_LATE) return CS_ERR_HIP;
  cs::Layout li, lo;
  const auto in_v = li.add<double>(in.size());
  const auto out_v = lo.add<double>(in.size());
  const auto out_n = lo.add<int>(1);
  auto launch = [&] {                                  // (the stand-in's device memory is the host's)
    for (size_t i = 0; i < in.size(); i++) out_v.at(B->d_out.p)[i] = 2.0 * in_v.at(B->d_in.p)[i] + 1.0;
    *out_n.at(B->d_out.p) = (int)in.size();
  };
  if (int rc = cs::batch_round_trip(*B, li.bytes, lo.bytes, true, [&] { cs::copy_in(in_v, B->h_in, in.data()); }, launch)) return rc;
  int n = -1;
  out->assign(in.size(), 0.0);
  cs::copy_out(out_v, B->h_out, out->data());
  cs::copy_out(out_n, B->h_out, &n);
  CHECK(n == (int)in.size());
  return call.done();
}

static void check_calls(bool point_first) {
  TestHandle* B = nullptr;
  CHECK(cs::batch_create(0, &B) == CS_OK && B);
  if (!B) return;
  double k = -1, h = -1;
  CHECK(cs::batch_last_timing(B, &k, &h) == CS_ERR_NOT_RUN);
  std::vector<double> in(301), out;
  for (size_t i = 0; i < in.size(); i++) in[i] = 0.5 * (double)i - 7.0;

  CHECK(entry(B, point_first, EMPTY, in, &out) == CS_OK);
  CHECK(B->ran && cs::batch_last_timing(B, &k, &h) == CS_OK && k == 0.0 && h == 0.0);

  CHECK(entry(B, point_first, RUNS, in, &out) == CS_OK);
  CHECK(B->ran && cs::batch_last_timing(B, &k, &h) == CS_OK && k == 0.25 && h >= 0.0);      // (0.25: the stand-in's hipEventElapsedTime)
  CHECK(out.size() == in.size());
  for (size_t i = 0; i < out.size(); i++) CHECK(out[i] == 2.0 * in[i] + 1.0);
  const double h_run = h;

  g_last_error.clear();
  CHECK(entry(B, point_first, REFUSED_EARLY, in, &out) == CS_ERR_INVALID_ARG && g_last_error == "entry: an argument");
  if (point_first) {
    CHECK(!B->ran && cs::batch_last_timing(B, &k, &h) == CS_ERR_NOT_RUN);
  } else {                                             // the last run's timing stays in place
    CHECK(B->ran && cs::batch_last_timing(B, &k, &h) == CS_OK && k == 0.25 && h == h_run);
  }

  CHECK(entry(B, point_first, RUNS, in, &out) == CS_OK && B->ran);
  CHECK(entry(B, point_first, FAILS_LATE, in, &out) == CS_ERR_HIP);
  CHECK(!B->ran && cs::batch_last_timing(B, &k, &h) == CS_ERR_NOT_RUN);

  CHECK(entry(B, point_first, EMPTY, in, &out) == CS_OK);
  CHECK(B->ran && cs::batch_last_timing(B, &k, &h) == CS_OK && k == 0.0 && h == 0.0);
  in.resize(5);                                        // a smaller batch on the grown buffers
  CHECK(entry(B, point_first, RUNS, in, &out) == CS_OK && B->ran && out.size() == 5 && out[4] == 2.0 * in[4] + 1.0);
  cs::batch_destroy(B);
}

static bool nothing_live() {
  bool ok = true;
  for (int kind = 0; kind < hip_standin::N_KINDS; kind++) ok = ok && hip_standin::live(kind).empty() && hip_standin::made(kind) == hip_standin::dropped(kind);
  return ok;
}

static void check_one_shot() {
  CHECK(nothing_live());
  const long streams = hip_standin::made(hip_standin::STREAM), events = hip_standin::made(hip_standin::EVENT);
  std::vector<double> in(17, 1.5), out;
  int calls = 0;
  CHECK(cs::batch_one_shot<TestHandle>(0, [&](TestHandle* B) -> int { calls++; return entry(B, false, RUNS, in, &out); }) == CS_OK);
  CHECK(calls == 1 && out.size() == 17 && out[16] == 4.0 && nothing_live());
  // fn fails after the handle's buffers have been made: its code comes back and the destroy still runs
  CHECK(cs::batch_one_shot<TestHandle>(0, [&](TestHandle* B) -> int {
          calls++;
          CHECK(entry(B, false, RUNS, in, &out) == CS_OK);
          CHECK(!hip_standin::live(hip_standin::DEVICE).empty() && !hip_standin::live(hip_standin::PINNED).empty());
          return CS_ERR_CAPACITY;
        }) == CS_ERR_CAPACITY);
  CHECK(calls == 2 && nothing_live());
  CHECK(cs::batch_one_shot<TestHandle>(0, [&](TestHandle* B) -> int { calls++; return entry(B, true, REFUSED_EARLY, in, &out); }) == CS_ERR_INVALID_ARG);
  CHECK(calls == 3 && nothing_live());
  CHECK(hip_standin::made(hip_standin::STREAM) == streams + 3 && hip_standin::made(hip_standin::EVENT) == events + 6);
  // a device the stand-in does not have: refused before anything is made, fn never runs
  CHECK(cs::batch_one_shot<TestHandle>(3, [&](TestHandle*) -> int { calls++; return CS_OK; }) == CS_ERR_INVALID_ARG);
  CHECK(calls == 3 && hip_standin::made(hip_standin::STREAM) == streams + 3 && nothing_live());
}

// ---- the refusal and the predicates ----------------------------------------------------------------------------------------------------------------
static void check_arguments() {
  g_last_error = "before";
  const cs::Refuse refuse{"cs_some_entry"};
  CHECK(g_last_error == "before");                     // (nothing happens until it fires)
  CHECK(refuse("NULL argument") == CS_ERR_INVALID_ARG && g_last_error == "cs_some_entry: NULL argument");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double fine[4] = {0.0, -1.5, 1e308, -0.0}, with_inf[3] = {1.0, -inf, 2.0}, with_nan[3] = {1.0, 2.0, nan};
  CHECK(cs::all_finite(fine, 4) && !cs::all_finite(with_inf, 3) && !cs::all_finite(with_nan, 3) && cs::all_finite(with_nan, 2) && cs::all_finite(nullptr, 0));
  const double some[3] = {0.0, -0.0, inf}, neg[2] = {1.0, -1e-300};
  CHECK(cs::none_negative(some, 3) && !cs::none_negative(neg, 2) && !cs::none_negative(with_nan, 3) && cs::none_negative(nullptr, 0));
  CHECK(cs::positive(1e-300) && !cs::positive(0.0) && !cs::positive(-1.0) && !cs::positive(inf) && !cs::positive(nan));
  const double unit[4] = {0.0, 0.0, 0.0, 1.0}, scaled[4] = {0.1, -0.2, 0.3, -0.4}, zero[4] = {0.0, 0.0, 0.0, 0.0}, huge[4] = {1e200, 0.0, 0.0, 1e200}, bad[4] = {0.0, nan, 0.0, 1.0};
  CHECK(cs::quaternion_norm_ok(unit) && cs::quaternion_norm_ok(scaled) && !cs::quaternion_norm_ok(zero) && !cs::quaternion_norm_ok(huge) && !cs::quaternion_norm_ok(bad));
  const int ok_ptr[4] = {0, 0, 5, 5}, late[2] = {1, 2}, down[3] = {0, 4, 3};
  CHECK(cs::check_partition("e: ptr", ok_ptr, 3) == CS_OK && cs::check_partition("e: ptr", ok_ptr, 0) == CS_OK);
  CHECK(cs::check_partition("e: ptr", late, 1) == CS_ERR_INVALID_ARG && g_last_error == "e: ptr[0] must be 0");
  CHECK(cs::check_partition("e: ptr", down, 2) == CS_ERR_INVALID_ARG && g_last_error == "e: ptr must not decrease");
}

int main() {
  check_parts();
  check_chunks({0, 1, 63, 64, 65, 128, 129});
  check_chunks({0, 0, 5, 0, 0, 64, 0});
  check_chunks({129, 0, 0, 1, 0, 0});
  check_chunks({0});
  check_chunks({});
  check_calls(false);
  check_calls(true);
  check_one_shot();
  check_arguments();
  CHECK(nothing_live());
  if (g_fail) { std::printf("batch_handle_check: %ld FAILED\n", g_fail); return 1; }
  std::printf("batch_handle_check: ok\n");
  return 0;
}
