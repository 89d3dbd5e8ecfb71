// detect_cam_host.h -- the camera cache of a frame (set_cam_pose, box_proposal_detail.cpp:45-56) and its roll/pitch sample poses
// (:344-355, :368-377).  Plain C++, no HIP call: tools/hostonly/detect_rank_host_check.cpp checks it with the host compiler.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "detect_jobs_host.h"

namespace cs_dh {

inline double cof3(const double* a, int i, int j) {
  int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return a[3 * i1 + j1] * a[3 * i2 + j2] - a[3 * i1 + j2] * a[3 * i2 + j1];
}
// 3x3 inverse in cofactor form, the algorithm Eigen's Matrix3d::inverse() uses.
inline void inv3(const double* a, double* r) {
  double c0 = cof3(a, 0, 0), c1 = cof3(a, 1, 0), c2 = cof3(a, 2, 0);
  double det = (c0 * a[0] + c1 * a[3]) + c2 * a[6];
  double id = 1.0 / det;
  r[0] = c0 * id; r[1] = c1 * id; r[2] = c2 * id;
  r[3] = cof3(a, 0, 1) * id; r[4] = cof3(a, 1, 1) * id; r[5] = cof3(a, 2, 1) * id;
  r[6] = cof3(a, 0, 2) * id; r[7] = cof3(a, 1, 2) * id; r[8] = cof3(a, 2, 2) * id;
}
inline void mul3(const double* a, const double* b, double* r) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) r[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
// Rotation matrix -> quaternion (Shoemake, as Eigen::Quaterniond(Matrix3d)) -> ZYX Euler angles
// (matrix_utils.cpp:38-49).
inline void rot_to_euler(const double* R, double e[3]) {
  double w, q[3];
  double t = R[0] + R[4] + R[8];
  if (t > 0.0) {
    t = std::sqrt(t + 1.0);
    w = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    w = (R[3 * k + j] - R[3 * j + k]) * t;
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
  }
  double qx = q[0], qy = q[1], qz = q[2];
  e[0] = std::atan2(2 * (w * qx + qy * qz), 1 - 2 * (qx * qx + qy * qy));
  e[1] = std::asin(2 * (w * qy - qz * qx));
  e[2] = std::atan2(2 * (w * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz));
}
// matrix_utils.cpp:81-96
inline void euler_to_rot(double roll, double pitch, double yaw, double* R) {
  double cp = h_cos(pitch), sp = h_sin(pitch), sr = h_sin(roll), cr = h_cos(roll), sy = h_sin(yaw), cy = h_cos(yaw);
  R[0] = cp * cy; R[1] = (sr * sp * cy) - (cr * sy); R[2] = (cr * sp * cy) + (sr * sy);
  R[3] = cp * sy; R[4] = (sr * sp * sy) + (cr * cy); R[5] = (cr * sp * sy) - (sr * cy);
  R[6] = -sp; R[7] = sr * cp; R[8] = cr * cp;
}

struct CamCache {
  cs::RpPose pose;  // KinvR, R, t, ground plane, roll, pitch
  double euler[3];
  double cam_yaw;
};
// set_cam_pose (box_proposal_detail.cpp:45-56) for rotation R (row-major 3x3) and position t.
inline void make_cam(const double* K, const double* R, const double* t, CamCache& c) {
  std::memcpy(c.pose.R, R, 9 * sizeof(double));
  std::memcpy(c.pose.t, t, 3 * sizeof(double));
  rot_to_euler(R, c.euler);
  double invR[9];
  inv3(R, invR);
  mul3(K, invR, c.pose.KinvR);
  c.cam_yaw = c.euler[2];
  // ground plane in the sensor frame: T_wc^T (0,0,1,0)  (:130-131)
  for (int i = 0; i < 3; i++) c.pose.plane[i] = ((R[0 + i] * 0.0 + R[3 + i] * 0.0) + R[6 + i] * 1.0) + 0.0 * 0.0;
  c.pose.plane[3] = ((t[0] * 0.0 + t[1] * 0.0) + t[2] * 1.0) + 1.0 * 0.0;
  c.pose.roll = c.euler[0];
  c.pose.pitch = c.euler[1];
}

// The roll/pitch sample poses of a frame (:344-355): raw roll and pitch -6 .. +6 degrees in steps of 3, roll-major, at the raw yaw; appended to `out`
inline void sample_rp_poses(const double* K, const double* t, const CamCache& raw, std::vector<CamCache>& out) {
  std::vector<double> rolls, pitches;
  linespace<double>(raw.euler[0] - 6.0 / 180.0 * CS_PI, raw.euler[0] + 6.0 / 180.0 * CS_PI, 3.0 / 180.0 * CS_PI, rolls);
  linespace<double>(raw.euler[1] - 6.0 / 180.0 * CS_PI, raw.euler[1] + 6.0 / 180.0 * CS_PI, 3.0 / 180.0 * CS_PI, pitches);
  for (double r : rolls)
    for (double p : pitches) {
      double Rn[9];
      euler_to_rot(r, p, raw.euler[2], Rn);
      CamCache c;
      make_cam(K, Rn, t, c);
      c.pose.roll = r; c.pose.pitch = p;  // the row stores the *sample* angles (:686)
      out.push_back(c);
    }
}

}  // namespace cs_dh
