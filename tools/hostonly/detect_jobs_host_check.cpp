// detect_jobs_host_check.cpp -- the detector host's job-table rules (cube_slam_wu_amd/csrc/detect_jobs_host.h) on their own, without a GPU, each
// against the reference's rule restated HERE (never against the header's own output): the top-edge samples of a box, the yaw list of a camera
// yaw, the three slot / vanishing-point span rules, the launch order of the line setup, the layout of a small call's merged I/O block.
// tests/test_detect_jobs_host_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/detect_jobs_host.h"

using namespace cs_dh;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// ---- top-edge samples: box_proposal_detail.cpp:212-219 ---------------------------------------------------------------------------------
static void check_top(double left_d, double w_d) {
  const double box[5] = {left_d, 40.0, w_d, 80.0, 0.9};
  // the reference: int truncations of left and w, right from the double sum, the step rounded from an integer quotient capped at 20
  int left = box[0], w = box[2];
  int right = left + box[2];
  int res = (int)std::round(std::min(20, w / 10));
  std::vector<int> want;
  if (res >= 1) linespace<int>(left + 5, right - 5, res, want);
  CHECK(top_sample_step(box) == res, "box (%g, %g): step %d, want %d", left_d, w_d, top_sample_step(box), res);
  std::vector<int> got(LINESPACE_MAX + 1, -12345);
  const int n = top_samples(box, got.data());
  CHECK(n == (int)want.size(), "box (%g, %g): %d samples, want %d", left_d, w_d, n, (int)want.size());
  for (int i = 0; i < n && i < (int)want.size(); i++) CHECK(got[i] == want[i], "box (%g, %g): sample %d is %d, want %d", left_d, w_d, i, got[i], want[i]);
  CHECK(got[n] == -12345, "box (%g, %g): wrote past its count", left_d, w_d);
  // the capacity the batch layout reserves for the box is the count-only call
  CHECK(top_samples(box, nullptr) == (int)want.size(), "box (%g, %g): the count-only call gives %d", left_d, w_d, top_samples(box, nullptr));
}
static void check_top_samples() {
  { const double skipped[5] = {100, 40, 9, 80, 0.9}; CHECK(top_sample_step(skipped) < 1 && top_samples(skipped, nullptr) == 0, "a box of width 9 is not skipped"); }
  { const double one[5] = {100, 40, 10, 80, 0.9}; CHECK(top_samples(one, nullptr) == 1, "a box of width 10 has %d samples, not 1", top_samples(one, nullptr)); }
  { const double wide[5] = {3, 40, 1000, 80, 0.9}; CHECK(top_sample_step(wide) == 20, "width 1000: step %d, not capped at 20", top_sample_step(wide)); }
  for (double w : {9.0, 10.0, 19.0, 20.0, 105.0, 200.0, 209.0, 1000.0}) check_top(100.0, w);
  check_top(10.7, 30.6);      // left 10, w 30, but right = (int)(10 + 30.6) = 40
  check_top(0.0, 25000.0);    // more samples than linespace ever returns
}

// ---- yaw lists: :180-184 ---------------------------------------------------------------------------------------------------------------
static void check_yaw(double cam_yaw, double range, double step) {
  const double yaw_init = cam_yaw - 90.0 / 180.0 * CS_PI;
  std::vector<double> want;
  linespace<double>(yaw_init - range / 180.0 * CS_PI, yaw_init + range / 180.0 * CS_PI, step / 180.0 * CS_PI, want);
  const int cap = yaw_list_capacity(range, step);
  CHECK(cap == (int)(2.0 * range / std::max(1e-9, step)) + 3, "capacity of (%g, %g) is %d", range, step, cap);
  CHECK((int)want.size() <= cap, "(%g, %g) at %g: %d entries do not fit the capacity %d", range, step, cam_yaw, (int)want.size(), cap);
  std::vector<double> y(cap + 1, -7.0), c(cap + 1, -7.0), s(cap + 1, -7.0);
  const int n = fill_yaw_list(cam_yaw, range, step, cap, y.data(), c.data(), s.data());
  CHECK(n == (int)want.size(), "(%g, %g) at %g: %d entries, want %d", range, step, cam_yaw, n, (int)want.size());
  for (int i = 0; i < n && i < (int)want.size(); i++) {
    CHECK(y[i] == want[i], "(%g, %g) at %g: entry %d is %.17g, want %.17g", range, step, cam_yaw, i, y[i], want[i]);
    CHECK(c[i] == h_cos(want[i]) && s[i] == h_sin(want[i]), "(%g, %g) at %g: cos / sin of entry %d", range, step, cam_yaw, i);
  }
  CHECK(y[cap] == -7.0 && c[cap] == -7.0 && s[cap] == -7.0, "(%g, %g) at %g: wrote past the capacity", range, step, cam_yaw);
  // a capacity that is too small: reported, and nothing written past it
  if (want.size() >= 2) {
    const int small = (int)want.size() - 1;
    std::vector<double> y2(want.size() + 2, -7.0), c2(want.size() + 2, -7.0), s2(want.size() + 2, -7.0);
    CHECK(fill_yaw_list(cam_yaw, range, step, small, y2.data(), c2.data(), s2.data()) < 0, "(%g, %g) at %g: overflow of %d entries not reported", range, step, cam_yaw, small);
    for (size_t i = small; i < y2.size(); i++) CHECK(y2[i] == -7.0 && c2[i] == -7.0 && s2[i] == -7.0, "(%g, %g) at %g: overflow wrote entry %d", range, step, cam_yaw, (int)i);
  }
}
static void check_yaw_lists() {
  const double rs[3][2] = {{30, 6}, {45, 0.5}, {45, 3}};
  for (const auto& p : rs)
    for (double cam_yaw : {0.0, CS_PI, -CS_PI, 1e-3}) check_yaw(cam_yaw, p[0], p[1]);
}

// ---- span rules --------------------------------------------------------------------------------------------------------------------------
static void check_spans() {
  std::vector<cs::JobDesc> jobs;
  for (int rp : {1, 3})
    for (int y : {0, 1, 5, 181})
      for (int t : {0, 1, 4}) { cs::JobDesc jd{}; jd.RP = rp; jd.Y = y; jd.T = t; jobs.push_back(jd); }
  const int ycap = 181;      // the frame's longest list (lean rule)
  for (int rule = 0; rule < 3; rule++) {
    const char* name = rule == 0 ? "exact" : rule == 1 ? "padded" : "longest list";
    long long end_slot = 0, end_vp = 0;      // the running totals a job builder keeps
    for (cs::JobDesc jd : jobs) {
      const JobSpan s = rule == 0 ? span_exact(jd) : rule == 1 ? span_padded(jd) : span_longest_list(jd, ycap);
      const long long need_slots = (long long)jd.RP * jd.Y * jd.T * 2, need_vps = (long long)jd.RP * jd.Y;
      jd.slot_off = end_slot; jd.vp_off = (int)end_vp;
      CHECK(s.slots >= 0 && s.vps >= 0, "%s: job (%d, %d, %d) has a negative span (%lld, %lld)", name, jd.RP, jd.Y, jd.T, s.slots, s.vps);
      CHECK(s.slots >= need_slots && s.vps >= need_vps, "%s: job (%d, %d, %d) gets (%lld, %lld), needs (%lld, %lld)", name, jd.RP, jd.Y, jd.T, s.slots, s.vps, need_slots, need_vps);
      end_slot = jd.slot_off + s.slots; end_vp = jd.vp_off + s.vps;
      if (rule == 0) CHECK(s.slots == need_slots && s.vps == need_vps, "exact: job (%d, %d, %d) gets (%lld, %lld)", jd.RP, jd.Y, jd.T, s.slots, s.vps);
      if (rule == 1) CHECK(jd.slot_off % 256 == 0 && jd.vp_off % 64 == 0 && s.slots % 256 == 0 && s.vps % 64 == 0, "padded: job (%d, %d, %d) at (%lld, %d)", jd.RP, jd.Y, jd.T, jd.slot_off, jd.vp_off);
      if (rule == 1 && need_slots == 0 && jd.Y == 0) CHECK(s.slots == 0 && s.vps == 0, "padded: a null job owns (%lld, %lld)", s.slots, s.vps);
      if (need_slots > 0) {
        const SlotRef a = decode_slot(jd, jd.slot_off), z = decode_slot(jd, jd.slot_off + need_slots - 1);
        CHECK(a.cfg == 1 && a.t == 0 && a.rp == 0 && a.y == 0, "%s: first slot of (%d, %d, %d) decodes to (%d, %d, %d, %d)", name, jd.RP, jd.Y, jd.T, a.cfg, a.t, a.rp, a.y);
        CHECK(z.cfg == 2 && z.t == jd.T - 1 && z.rp == jd.RP - 1 && z.y == jd.Y - 1, "%s: last slot of (%d, %d, %d) decodes to (%d, %d, %d, %d)", name, jd.RP, jd.Y, jd.T, z.cfg, z.t,
              z.rp, z.y);
      }
    }
  }
}

// ---- launch order of the line setup ------------------------------------------------------------------------------------------------------
static unsigned long long g_seed = 4711;
static int rnd(int n) { g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL; return (int)((g_seed >> 33) % (unsigned long long)n); }
static void check_order(size_t nj, bool equal_work) {
  std::vector<FrameIn> frames(3);
  frames[0].n_lines = 400; frames[1].n_lines = 37; frames[2].n_lines = equal_work ? 400 : 0;
  std::vector<cs::JobDesc> jobs(nj);
  for (auto& jd : jobs) {
    jd = cs::JobDesc{};
    jd.frame = equal_work ? 0 : rnd(3);
    jd.g.el = 10; jd.g.et = 20; jd.g.er = 10 + (equal_work ? 100 : 1 + rnd(600)); jd.g.eb = 20 + (equal_work ? 100 : 1 + rnd(300));
  }
  std::vector<int> order(nj + 1, -1);
  line_setup_order(jobs.data(), nj, frames, order.data());
  CHECK(order[nj] == -1, "order of %d jobs: wrote past the end", (int)nj);
  std::vector<int> seen(nj, 0);
  long long wmax = 1;
  auto work = [&](int j) { return (long long)(jobs[j].g.er - jobs[j].g.el) * (jobs[j].g.eb - jobs[j].g.et) * frames[jobs[j].frame].n_lines; };
  for (size_t j = 0; j < nj; j++) wmax = std::max(wmax, work((int)j));
  long long prev = 64;
  for (size_t i = 0; i < nj; i++) {
    const int j = order[i];
    CHECK(j >= 0 && j < (int)nj && !seen[j], "order of %d jobs: entry %d is %d", (int)nj, (int)i, j);
    if (j < 0 || j >= (int)nj) continue;
    seen[j] = 1;
    const long long bucket = work(j) * 63 / wmax;      // 64 buckets of the work, the largest first
    CHECK(bucket <= prev, "order of %d jobs: bucket %lld after %lld at entry %d", (int)nj, bucket, prev, (int)i);
    prev = bucket;
  }
}

// ---- merged I/O block of a small call -----------------------------------------------------------------------------------------------------
static void check_arena(size_t nj, size_t nb, int kmax) {
  const size_t n_yaw = 184, n_top = 5 * nb + 3;
  const SmallCallArena A(nj, n_yaw, n_top, nb, kmax);
  // every piece with the bytes it has to hold, in order
  const size_t off[17] = {A.o_ls, A.o_sp, A.o_vp, A.o_y, A.o_yc, A.o_ys, A.o_tx, A.o_b0, A.o_bn, A.o_jobs, A.o_rec, A.o_wc, A.o_fb, A.o_jv, A.o_cb, A.o_end, 0};
  const size_t bytes[15] = {sizeof(int) * nj, sizeof(long long) * (nj + 1), sizeof(int) * (nj + 1), 8 * n_yaw, 8 * n_yaw, 8 * n_yaw, sizeof(int) * n_top, sizeof(int) * nb, sizeof(int) * nb,
                            sizeof(cs::JobDesc) * nj, sizeof(cs_cuboid) * nb * kmax, sizeof(int) * nb, sizeof(int) * nb, sizeof(int) * nj, sizeof(long long) * (nj + 1)};
  CHECK(off[0] == 0, "arena (%d, %d): starts at %d", (int)nj, (int)nb, (int)off[0]);
  for (int i = 0; i < 15; i++) {
    CHECK(off[i] % 256 == 0, "arena (%d, %d): piece %d at %d", (int)nj, (int)nb, i, (int)off[i]);
    CHECK(off[i + 1] >= off[i] + bytes[i], "arena (%d, %d): piece %d [%d, +%d) overlaps the next at %d", (int)nj, (int)nb, i, (int)off[i], (int)bytes[i], (int)off[i + 1]);
    CHECK(off[i + 1] < off[i] + bytes[i] + 256, "arena (%d, %d): more than padding after piece %d", (int)nj, (int)nb, i);
  }
  CHECK(A.o_end % 256 == 0, "arena (%d, %d): ends at %d", (int)nj, (int)nb, (int)A.o_end);
  // what goes up ends where the job table ends; what comes back starts with the job table
  CHECK(A.in_end == A.o_rec && A.in_end >= A.o_jobs + sizeof(cs::JobDesc) * nj && A.in_end < A.o_jobs + sizeof(cs::JobDesc) * nj + 256, "arena (%d, %d): inputs end at %d, job table [%d, +%d)",
        (int)nj, (int)nb, (int)A.in_end, (int)A.o_jobs, (int)(sizeof(cs::JobDesc) * nj));
}

int main() {
  check_top_samples();
  check_yaw_lists();
  check_spans();
  check_order(1, false); check_order(7, true); check_order(300, false); check_order(5000, false);
  for (size_t nj : {(size_t)1, (size_t)SMALL_CALL_JOBS})
    for (size_t nb : {(size_t)0, (size_t)1, nj}) check_arena(nj, nb, 2);
  if (g_fail) { std::printf("detect_jobs_host_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("detect_jobs_host_check: ok\n");
  return 0;
}
