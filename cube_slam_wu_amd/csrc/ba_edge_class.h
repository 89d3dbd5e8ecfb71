// ba_edge_class.h -- the caller's description of one pose-edge class of the bundle adjustment, on the host: EdgeSE3Cuboid, EdgeSE3CuboidProj or
// EdgeSE3Expmap (odometry).  cs_ba holds one record per class; cs_ba_set_edges_* / cs_ba_append_edges_* fill it, the structure phase reads it,
// cs_ba_dump / cs_ba_load write and read it.  Plain host C++ (tools/microbench/edge_class_check.cpp runs it on its own).
#pragma once
#include <vector>
#include "cs_se3.h"

namespace cs {

// doubles per edge of each payload array; meas_is_pose: the measurement is an SE3Quat (t, q) whose quaternion is normalised on entry
struct EdgeClassDims { int meas, info, extra; bool meas_is_pose; };
constexpr EdgeClassDims kPoseEdgeDims[3] = {{10, 81, 0, false}, {4, 16, 9, false}, {7, 36, 0, true}};      // cs_edge_class - CS_EDGE_CUBOID: Cuboid, CuboidProj (extra = K), odometry

struct EdgeClassHost {
  EdgeClassDims d;
  std::vector<int> a, b;                    // the two endpoints in the caller's edge order: (camera, cuboid), odometry (camera i, camera j)
  std::vector<double> meas, info, extra;
  std::vector<int> rk;                      // robust kernels (cs_ba_set_robust_kernels): kind and delta per edge; empty = no edge of the class has one
  std::vector<double> rd;
  std::vector<unsigned char> lvl;           // edge levels (cs_ba_set_edge_levels); empty, or shorter than the class (appended edges) = level 0
  int size() const { return (int)a.size(); }
  // n edges behind the class's list, or (replace) in its place.  A new list has no kernels and no levels; appended edges get no kernel
  // (RK_NONE, delta 0) where the class has kernels, and leave the levels as they are.  false: bad arguments, nothing changed.
  bool add(bool replace, int n, const int* ea, const int* eb, const double* m, const double* inf, const double* ext) {
    if (n < 0 || (n && (!ea || !eb || !m || !inf || (d.extra && !ext)))) return false;
    if (replace) { a.clear(); b.clear(); meas.clear(); info.clear(); extra.clear(); rk.clear(); rd.clear(); lvl.clear(); }
    const size_t m0 = meas.size();
    a.insert(a.end(), ea, ea + n); b.insert(b.end(), eb, eb + n);
    meas.insert(meas.end(), m, m + d.meas * (size_t)n); info.insert(info.end(), inf, inf + d.info * (size_t)n);
    if (d.extra) extra.insert(extra.end(), ext, ext + d.extra * (size_t)n);
    if (d.meas_is_pose) for (size_t k = m0; k < meas.size(); k += 7) { Pose p = pose_load(&meas[k]); pose_normalize(p); pose_store(p, &meas[k]); }
    if (!rk.empty()) { rk.resize(a.size(), 0); rd.resize(a.size(), 0.0); }
    return true;
  }
};

}  // namespace cs
