// triangulate_host.cpp -- the C ABI of the batched two-view triangulation of new map points (include/cubeslam_hip.h: cs_triangulate_*).
//
// What an ORB-SLAM2-derived local mapper does on every keyframe in LocalMapping::CreateNewMapPoints -- for the current keyframe and each
// covisible neighbour, over every match: the parallax decision, linear triangulation or a stereo back-projection, the depth tests, the
// reprojection gates and the scale-consistency test -- for all neighbours in ONE kernel launch (triangulate_kernels.hip).  The host checks
// every argument, makes each pair's record (cs_triangulate.h: triangulate_pair_record), packs the matches into 96-byte records, cuts the
// pairs into chunks of at most 64 matches, uploads everything with one copy, launches, downloads everything with one copy and counts each
// pair's accepted matches.  There is no CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/cubeslam_hip.h"
#include "cs_batch_handle.h"
#include "triangulate_types.h"

static_assert((int)CS_TRI_OK == cs::TRI_OK && (int)CS_TRI_PAIR_NOT_RUN == cs::TRI_PAIR_NOT_RUN && (int)CS_TRI_LOW_PARALLAX == cs::TRI_LOW_PARALLAX &&
              (int)CS_TRI_W_ZERO == cs::TRI_W_ZERO && (int)CS_TRI_DEPTH1 == cs::TRI_DEPTH1 && (int)CS_TRI_DEPTH2 == cs::TRI_DEPTH2 &&
              (int)CS_TRI_REPROJ1 == cs::TRI_REPROJ1 && (int)CS_TRI_REPROJ2 == cs::TRI_REPROJ2 && (int)CS_TRI_ZERO_DIST == cs::TRI_ZERO_DIST &&
              (int)CS_TRI_SCALE == cs::TRI_SCALE, "cs_triangulate_status is cs_triangulate.h's");
static_assert((int)CS_TRI_ROUTE_NONE == cs::TRI_ROUTE_NONE && (int)CS_TRI_ROUTE_TRIANGULATED == cs::TRI_ROUTE_TRIANGULATED &&
              (int)CS_TRI_ROUTE_STEREO1 == cs::TRI_ROUTE_STEREO1 && (int)CS_TRI_ROUTE_STEREO2 == cs::TRI_ROUTE_STEREO2, "cs_triangulate_route is cs_triangulate.h's");

// d_in = [pair records | match records | chunks], d_out = [out8 | status | route | cos3]
struct cs_triangulate : cs::BatchHandle {};

namespace {

using cs::all_finite;
using cs::positive;

int check_params(const cs_triangulate_params* p) {
  const cs::Refuse refuse{"cs_triangulate"};
  if (!p) return refuse("NULL parameters");
  if (!positive(p->min_baseline_ratio) || !positive(p->max_cos_parallax) || !positive(p->chi2_mono) || !positive(p->chi2_stereo) || !positive(p->ratio_factor) ||
      !positive(p->scale_range)) return refuse("every parameter must be finite and positive");
  return CS_OK;
}

struct Inputs {
  const double *Tcw1, *Tcw2, *cam1, *cam2, *median_depth2;
  const int* match_ptr;
  const double *kp1, *kp2;
};

// What every entry checks before anything is launched.  *n_matches = match_ptr[n_pairs].
int check_pairs(const char* who, int n_pairs, const Inputs& in, size_t* n_matches) {
  const cs::Refuse refuse{who};
  if (!in.Tcw1 || !in.Tcw2 || !in.cam1 || !in.cam2 || !in.median_depth2 || !in.match_ptr) return refuse("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": match_ptr", in.match_ptr, n_pairs)) return rc;
  const size_t np = (size_t)n_pairs, n = (size_t)in.match_ptr[n_pairs];
  if (n > (size_t)INT_MAX / cs::TRI_MATCH_DOUBLES) return refuse("too many matches for one call");
  if (n > 0 && (!in.kp1 || !in.kp2)) return refuse("NULL match array");
  if (!all_finite(in.Tcw1, 7 * np) || !all_finite(in.Tcw2, 7 * np)) return refuse("a pose is not finite");
  for (size_t f = 0; f < np; f++)
    for (const double* T : {in.Tcw1 + 7 * f, in.Tcw2 + 7 * f})
      if (!cs::quaternion_norm_ok(T + 3)) return refuse("a quaternion has zero norm or overflows");
  if (!all_finite(in.cam1, 6 * np) || !all_finite(in.cam2, 6 * np) || !all_finite(in.median_depth2, np)) return refuse("an intrinsic or a median depth is not finite");
  for (size_t f = 0; f < np; f++)
    for (const double* c : {in.cam1 + 6 * f, in.cam2 + 6 * f})
      if (!(c[0] > 0 && c[1] > 0)) return refuse("fx and fy must be positive");
  for (const double* kp : {in.kp1, in.kp2})
    for (size_t i = 0; i < n; i++) {
      const double* k = kp + 6 * i;
      if (!std::isfinite(k[0]) || !std::isfinite(k[1]) || !std::isfinite(k[2])) return refuse("a keypoint coordinate is not finite");
      if (k[2] >= 0 && !positive(k[3])) return refuse("a depth beside a right-image coordinate must be finite and positive");
      if (!positive(k[4]) || !positive(k[5])) return refuse("sigma2 and scale must be finite and positive");
    }
  *n_matches = n;
  return CS_OK;
}

int run(cs_triangulate* B, const char* who, const cs_triangulate_params* p, int n_pairs, const Inputs& in, double* X3_out, double* normal3_out, double* min_distance_out,
        double* max_distance_out, unsigned char* status_out, unsigned char* route_out, unsigned char* ran_out, int* n_accepted_out, double* cos3_out, bool inspect) {
  const cs::Refuse refuse{who};
  if (!B || n_pairs < 0) return refuse("no handle or a negative pair count");
  int rc = check_params(p); if (rc) return rc;
  cs::BatchCall call(*B);
  if (n_pairs == 0) return call.empty();
  size_t n = 0;
  rc = check_pairs(who, n_pairs, in, &n); if (rc) return rc;
  if (!ran_out || !n_accepted_out) return refuse("NULL output");
  if (n > 0 && (!X3_out || !normal3_out || !min_distance_out || !max_distance_out || !status_out || !route_out || (inspect && !cos3_out))) return refuse("NULL output");
  call.point_of_no_return();                           // (behind the checks: cs_batch_handle.h, BatchCall)
  const size_t np = (size_t)n_pairs, n_chunks = cs::chunk_count(in.match_ptr, np, cs::TRI_CHUNK);

  cs::Layout li, lo;
  const auto in_pair = li.add<cs::TriPair>(np);
  const auto in_rec = li.add<double>(n * cs::TRI_MATCH_DOUBLES);
  const auto in_chunk = li.add<cs::Chunk>(n_chunks);
  const auto out_8 = lo.add<double>(n * cs::TRI_OUT_DOUBLES);
  const auto out_st = lo.add<unsigned char>(n), out_rt = lo.add<unsigned char>(n);
  const auto out_cos = lo.add<double>(inspect ? n * 3 : 0);
  lo.add<unsigned char>(16);                           // (a batch without a match still has an output buffer)

  cs::TriLaunch a;
  auto pack = [&] {
    cs::TriPair* pair = in_pair.at(B->h_in.p);
    for (size_t f = 0; f < np; f++)
      cs::triangulate_pair_record(in.Tcw1 + 7 * f, in.Tcw2 + 7 * f, in.cam1 + 6 * f, in.cam2 + 6 * f, in.median_depth2[f], p->min_baseline_ratio, pair[f]);
    cs::chunk_fill(in.match_ptr, np, cs::TRI_CHUNK, in_chunk.at(B->h_in.p));
    double* rec = in_rec.at(B->h_in.p);
    for (size_t i = 0; i < n; i++, rec += cs::TRI_MATCH_DOUBLES) {
      std::memcpy(rec, in.kp1 + 6 * i, 6 * 8);
      std::memcpy(rec + 6, in.kp2 + 6 * i, 6 * 8);
    }
    std::memset(&a, 0, sizeof(a));
    a.n_chunks = (int)n_chunks;
    a.prm.min_baseline_ratio = p->min_baseline_ratio; a.prm.max_cos_parallax = p->max_cos_parallax; a.prm.chi2_mono = p->chi2_mono;
    a.prm.chi2_stereo = p->chi2_stereo; a.prm.ratio_factor = p->ratio_factor; a.prm.scale_range = p->scale_range;
    a.chunk = in_chunk.at(B->d_in.p); a.pair = in_pair.at(B->d_in.p); a.rec = in_rec.at(B->d_in.p);
    a.out8 = out_8.at(B->d_out.p); a.status = out_st.at(B->d_out.p); a.route = out_rt.at(B->d_out.p);
    a.cos3 = inspect ? out_cos.at(B->d_out.p) : nullptr;
  };
  rc = cs::batch_round_trip(*B, li.bytes, lo.bytes, true, pack, [&] { cs::triangulate_launch(a, inspect, B->st); }); if (rc) return rc;

  const double* o8 = out_8.at(B->h_out.p);
  for (size_t i = 0; i < n; i++, o8 += cs::TRI_OUT_DOUBLES) {
    for (int k = 0; k < 3; k++) { X3_out[3 * i + k] = o8[k]; normal3_out[3 * i + k] = o8[3 + k]; }
    min_distance_out[i] = o8[6];
    max_distance_out[i] = o8[7];
  }
  if (n) {
    cs::copy_out(out_st, B->h_out, status_out);
    cs::copy_out(out_rt, B->h_out, route_out);
    if (inspect) cs::copy_out(out_cos, B->h_out, cos3_out);
  }
  const cs::TriPair* pair = in_pair.at(B->h_in.p);
  for (size_t f = 0; f < np; f++) ran_out[f] = pair[f].ran != 0.0 ? 1 : 0;
  cs::count_status(in.match_ptr, np, status_out, CS_TRI_OK, n_accepted_out);
  return call.done();
}

}  // namespace

extern "C" {

void cs_triangulate_default_params(cs_triangulate_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_baseline_ratio = 0.01;
  p->max_cos_parallax = 0.9998;
  p->chi2_mono = 5.991;
  p->chi2_stereo = 7.8;
  p->ratio_factor = 1.5 * 1.2;
  p->scale_range = 1.2 * 1.2 * 1.2 * 1.2 * 1.2 * 1.2 * 1.2;
}

int cs_triangulate_create(int device, cs_triangulate** out) { return cs::batch_create(device, out); }

void cs_triangulate_destroy(cs_triangulate* B) { cs::batch_destroy(B); }

int cs_triangulate_run(cs_triangulate* B, const cs_triangulate_params* p, int n_pairs, const double* Tcw1, const double* Tcw2, const double* cam1, const double* cam2,
                       const double* median_depth2, const int* match_ptr, const double* kp1, const double* kp2, double* X3_out, double* normal3_out,
                       double* min_distance_out, double* max_distance_out, unsigned char* status_out, unsigned char* route_out, unsigned char* ran_out, int* n_accepted_out) {
  const Inputs in = {Tcw1, Tcw2, cam1, cam2, median_depth2, match_ptr, kp1, kp2};
  return run(B, "cs_triangulate_run", p, n_pairs, in, X3_out, normal3_out, min_distance_out, max_distance_out, status_out, route_out, ran_out, n_accepted_out, nullptr, false);
}

int cs_triangulate_last_timing(const cs_triangulate* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_triangulate_pairs(int device, const cs_triangulate_params* p, int n_pairs, const double* Tcw1, const double* Tcw2, const double* cam1, const double* cam2,
                         const double* median_depth2, const int* match_ptr, const double* kp1, const double* kp2, double* X3_out, double* normal3_out,
                         double* min_distance_out, double* max_distance_out, unsigned char* status_out, unsigned char* route_out, unsigned char* ran_out, int* n_accepted_out) {
  if (n_pairs < 0) return cs::Refuse{"cs_triangulate_pairs"}("a negative pair count");
  const Inputs in = {Tcw1, Tcw2, cam1, cam2, median_depth2, match_ptr, kp1, kp2};
  return cs::batch_one_shot<cs_triangulate>(device, [&](cs_triangulate* B) -> int {
    return run(B, "cs_triangulate_pairs", p, n_pairs, in, X3_out, normal3_out, min_distance_out, max_distance_out, status_out, route_out, ran_out, n_accepted_out, nullptr, false);
  });
}

int cs_triangulate_inspect(int device, const cs_triangulate_params* p, int n_pairs, const double* Tcw1, const double* Tcw2, const double* cam1, const double* cam2,
                           const double* median_depth2, const int* match_ptr, const double* kp1, const double* kp2, double* X3_out, double* normal3_out,
                           double* min_distance_out, double* max_distance_out, unsigned char* status_out, unsigned char* route_out, unsigned char* ran_out,
                           int* n_accepted_out, double* cos3_out) {
  if (n_pairs < 0) return cs::Refuse{"cs_triangulate_inspect"}("a negative pair count");
  const Inputs in = {Tcw1, Tcw2, cam1, cam2, median_depth2, match_ptr, kp1, kp2};
  return cs::batch_one_shot<cs_triangulate>(device, [&](cs_triangulate* B) -> int {
    return run(B, "cs_triangulate_inspect", p, n_pairs, in, X3_out, normal3_out, min_distance_out, max_distance_out, status_out, route_out, ran_out, n_accepted_out, cos3_out, true);
  });
}

}  // extern "C"
