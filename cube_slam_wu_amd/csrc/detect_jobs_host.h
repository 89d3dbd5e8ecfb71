// detect_jobs_host.h -- the rules in FRONT of the sweep kernels that every job builder of detect_host.cpp shares, once each (detect_rank_host.h
// holds those BEHIND the kernels).  Plain C++, no HIP call: tests/test_detect_jobs_host_cpu.py builds it with the host compiler.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "detect_rank_host.h"

namespace cs_dh {

enum { LINESPACE_MAX = 1001 };   // the most entries linespace produces
template <class T>
void linespace(T a, T b, T step, std::vector<T>& out) {  // matrix_utils.cpp:368-380
  for (; a <= b && out.size() <= 1000; a += step) out.push_back(a);
}

// Top-edge samples of a box (box_proposal_detail.cpp:212-219; a step below 1: the box is skipped, :215) into `out` (null: count only)
inline int top_sample_step(const double* box5) { int w = box5[2]; return (int)std::round(std::min(20, w / 10)); }
inline int top_samples(const double* box5, int* out) {
  const int res = top_sample_step(box5);
  int left = box5[0], n = 0;
  int right = left + box5[2];
  for (int x = left + 5; res >= 1 && x <= right - 5; x += res) {
    if (out) out[n] = x;
    if (++n > 1000) break;
  }
  return n;
}

// Yaw list of a camera yaw (:180-184) and the capacity the pools are sized by; returns the count, -1 when it exceeds `cap`.  No allocation.
inline int yaw_list_capacity(double range_deg, double step_deg) { return (int)(2.0 * range_deg / std::max(1e-9, step_deg)) + 3; }
inline int fill_yaw_list(double cam_yaw, double range_deg, double step_deg, int cap, double* yaw, double* c, double* s) {
  const double yaw_init = cam_yaw - 90.0 / 180.0 * CS_PI;
  double a = yaw_init - range_deg / 180.0 * CS_PI;
  const double b = yaw_init + range_deg / 180.0 * CS_PI, step = step_deg / 180.0 * CS_PI;
  int n = 0;
  for (; a <= b && n <= 1000; a += step) {      // linespace<double>
    if (n == cap) return -1;
    yaw[n++] = a;
  }
  for (int y = 0; y < n; y++) { c[y] = h_cos(yaw[y]); s[y] = h_sin(yaw[y]); }
  return n;
}

// The slots and vanishing-point entries a job owns.  exact: round path.  padded: production path -- whole 256-slot blocks (a scorer workgroup
// never straddles two jobs), whole waves (a wave of the VP kernels reads one job).  longest_list: lean roll/pitch path -- room for the
// longest yaw list the frame can carry to the job (ycap >= jd.Y).
struct JobSpan { long long slots, vps; };
inline long long whole_blocks(long long n) { return (n + 255) & ~255LL; }
inline long long whole_waves(long long n) { return (n + 63) & ~63LL; }
inline JobSpan span_exact(const cs::JobDesc& jd) { return JobSpan{(long long)jd.RP * jd.Y * jd.T * 2, (long long)jd.RP * jd.Y}; }
inline JobSpan span_padded(const cs::JobDesc& jd) { return JobSpan{whole_blocks(span_exact(jd).slots), whole_waves(span_exact(jd).vps)}; }
inline JobSpan span_longest_list(const cs::JobDesc& jd, int ycap) { return JobSpan{(long long)jd.RP * ycap * jd.T * 2, whole_waves((long long)jd.RP * ycap)}; }

// Launch order of the line setup: largest ROI area x segment count first (counting sort), so that the kernel's tail is not a late-started long job
inline void line_setup_order(const cs::JobDesc* jobs, size_t nj, const std::vector<FrameIn>& frames, int* order) {
  enum { NBK = 64 };
  auto work = [&](const cs::JobDesc& jd) { return (long long)(jd.g.er - jd.g.el) * (jd.g.eb - jd.g.et) * frames[jd.frame].n_lines; };
  long long wmax = 1;
  for (size_t j = 0; j < nj; j++) wmax = std::max(wmax, work(jobs[j]));
  int cnt[NBK + 1] = {0};
  auto bucket = [&](const cs::JobDesc& jd) { return NBK - 1 - (int)(work(jd) * (NBK - 1) / wmax); };
  for (size_t j = 0; j < nj; j++) cnt[bucket(jobs[j]) + 1]++;
  for (int q = 0; q < NBK; q++) cnt[q + 1] += cnt[q];
  for (size_t j = 0; j < nj; j++) order[cnt[bucket(jobs[j])]++] = (int)j;
}

// Merged I/O block of a small call: [inputs | the job table (in and out) | outputs] in 256-byte pieces; [0, in_end) goes up, [o_jobs, o_end) comes back
enum { SMALL_CALL_JOBS = 256 };
struct SmallCallArena {
  size_t o_ls = 0, o_sp = 0, o_vp = 0, o_y = 0, o_yc = 0, o_ys = 0, o_tx = 0, o_b0 = 0, o_bn = 0;   // in: launch order, prefixes, yaw tables, top samples, box table
  size_t o_jobs = 0, in_end = 0, o_rec = 0, o_wc = 0, o_fb = 0, o_jv = 0, o_cb = 0, o_end = 0;      // out: records, winner counts, tie flags, valid counts, compact bases
  SmallCallArena() = default;
  SmallCallArena(size_t nj, size_t n_yaw, size_t n_top, size_t nb, int kmax) {
    auto room = [&](size_t bytes) { const size_t at = o_end; o_end += (size_t)whole_blocks((long long)bytes); return at; };
    o_ls = room(sizeof(int) * nj); o_sp = room(sizeof(long long) * (nj + 1)); o_vp = room(sizeof(int) * (nj + 1));
    o_y = room(8 * n_yaw); o_yc = room(8 * n_yaw); o_ys = room(8 * n_yaw); o_tx = room(sizeof(int) * n_top); o_b0 = room(sizeof(int) * nb); o_bn = room(sizeof(int) * nb);
    o_jobs = room(sizeof(cs::JobDesc) * nj); in_end = o_end;
    o_rec = room(sizeof(cs_cuboid) * nb * kmax); o_wc = room(sizeof(int) * nb); o_fb = room(sizeof(int) * nb); o_jv = room(sizeof(int) * nj);
    o_cb = room(sizeof(long long) * (nj + 1));
  }
};

}  // namespace cs_dh
