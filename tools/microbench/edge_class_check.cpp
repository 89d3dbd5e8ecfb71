// edge_class_check -- host-only run of the pose-edge class record (csrc/ba_edge_class.h) through the calls cs_ba_set_edges_* / cs_ba_append_edges_* make
// of it: set, append, append with kernels present, set again, for all three classes; checks sizes, contents, padding and the quaternion's norm.
// Meant for the sanitizers (plain host code, nothing of it runs on a device):
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tools/microbench/edge_class_check.cpp -o build_tmp/edge_class_check && build_tmp/edge_class_check
// tests/test_ba_host_cpu.py builds it without them and runs it.
#include "../../cube_slam_wu_amd/csrc/ba_edge_class.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "edge_class_check: %s failed (line %d)\n", #c, __LINE__); exit(1); } } while (0)

namespace {

// n edges with recognisable values: endpoint k + base, payload entry j of edge k = base + k + j / 1000
struct Edges {
  std::vector<int> a, b;
  std::vector<double> m, i, x;
  Edges(const cs::EdgeClassDims& d, int n, int base) {
    for (int k = 0; k < n; k++) {
      a.push_back(base + k); b.push_back(base + k + 1);
      for (int j = 0; j < d.meas; j++) m.push_back(base + k + j / 1000.0);
      for (int j = 0; j < d.info; j++) i.push_back(base + k + j / 1000.0);
      for (int j = 0; j < d.extra; j++) x.push_back(base + k + j / 1000.0);
    }
  }
};

void check_class(const cs::EdgeClassDims& d) {
  cs::EdgeClassHost c{d};
  auto add = [&](bool replace, const Edges& e) { return c.add(replace, (int)e.a.size(), e.a.data(), e.b.data(), e.m.data(), e.i.data(), d.extra ? e.x.data() : nullptr); };
  auto consistent = [&](int n) {
    CHECK(c.size() == n && (int)c.b.size() == n && (int)c.meas.size() == d.meas * n && (int)c.info.size() == d.info * n && (int)c.extra.size() == d.extra * n);
    CHECK(c.rk.size() == c.rd.size() && (c.rk.empty() || (int)c.rk.size() == n) && (int)c.lvl.size() <= n);
    for (int k = 0; k < n && d.meas_is_pose; k++) {
      const double* q = &c.meas[7 * (size_t)k + 3];
      CHECK(std::fabs(std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) - 1.0) < 1e-14);
    }
  };
  const Edges e5(d, 5, 100), e3(d, 3, 200), e1(d, 1, 300), e4(d, 4, 400), e0(d, 0, 0);
  // set
  CHECK(add(true, e5)); consistent(5);
  CHECK(c.a[4] == 104 && c.b[4] == 105 && c.info[d.info * 4 + 1] == 104.001 && (d.meas_is_pose || c.meas[d.meas * 4 + 2] == 104.002));
  // append without kernels: none appear; levels set by the caller stay as they are (shorter than the class)
  c.lvl.assign(5, 1);
  CHECK(add(false, e3)); consistent(8);
  CHECK(c.rk.empty() && c.lvl.size() == 5 && c.a[5] == 200 && c.info[d.info * 7] == 202.0);
  // append with kernels present: the new edges get RK_NONE / 0, the old ones keep theirs
  c.rk.assign(8, 3); c.rd.assign(8, 1.5);
  CHECK(add(false, e1)); consistent(9);
  CHECK(c.rk[7] == 3 && c.rd[7] == 1.5 && c.rk[8] == 0 && c.rd[8] == 0.0 && c.lvl.size() == 5);
  CHECK(add(false, e0)); consistent(9);
  CHECK(c.add(false, 0, nullptr, nullptr, nullptr, nullptr, nullptr)); consistent(9);
  if (d.extra) CHECK(c.extra[d.extra * 8 + 1] == 300.001);
  // bad arguments change nothing
  CHECK(!c.add(false, -1, e1.a.data(), e1.b.data(), e1.m.data(), e1.i.data(), e1.x.data()));
  CHECK(!c.add(true, 1, e1.a.data(), nullptr, e1.m.data(), e1.i.data(), e1.x.data()));
  CHECK(!c.add(true, 1, e1.a.data(), e1.b.data(), e1.m.data(), nullptr, e1.x.data()));
  if (d.extra) CHECK(!c.add(true, 1, e1.a.data(), e1.b.data(), e1.m.data(), e1.i.data(), nullptr));
  consistent(9); CHECK(c.rk.size() == 9);
  // set again: a new list, without kernels and levels
  CHECK(add(true, e4)); consistent(4);
  CHECK(c.rk.empty() && c.rd.empty() && c.lvl.empty() && c.a[0] == 400 && c.b[3] == 404);
  CHECK(add(true, e0)); consistent(0);
}

}  // namespace

int main() {
  for (const cs::EdgeClassDims& d : cs::kPoseEdgeDims) check_class(d);
  printf("edge_class_check: ok\n");
  return 0;
}
