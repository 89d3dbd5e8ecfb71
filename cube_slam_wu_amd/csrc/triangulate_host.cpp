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

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

bool positive(double x) { return std::isfinite(x) && x > 0; }

int check_params(const cs_triangulate_params* p) {
  if (!p) { cs_set_error("cs_triangulate: NULL parameters"); return CS_ERR_INVALID_ARG; }
  if (!positive(p->min_baseline_ratio) || !positive(p->max_cos_parallax) || !positive(p->chi2_mono) || !positive(p->chi2_stereo) || !positive(p->ratio_factor) ||
      !positive(p->scale_range)) { cs_set_error("cs_triangulate: every parameter must be finite and positive"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

struct Inputs {
  const double *Tcw1, *Tcw2, *cam1, *cam2, *median_depth2;
  const int* match_ptr;
  const double *kp1, *kp2;
};

// What every entry checks before anything is launched.  *n_matches = match_ptr[n_pairs].
int check_pairs(const char* who, int n_pairs, const Inputs& in, size_t* n_matches) {
  auto fail = [&](const char* what) { cs_set_error((std::string(who) + ": " + what).c_str()); return CS_ERR_INVALID_ARG; };
  if (!in.Tcw1 || !in.Tcw2 || !in.cam1 || !in.cam2 || !in.median_depth2 || !in.match_ptr) return fail("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": match_ptr", in.match_ptr, n_pairs)) return rc;
  const size_t np = (size_t)n_pairs, n = (size_t)in.match_ptr[n_pairs];
  if (n > (size_t)INT_MAX / cs::TRI_MATCH_DOUBLES) return fail("too many matches for one call");
  if (n > 0 && (!in.kp1 || !in.kp2)) return fail("NULL match array");
  if (!all_finite(in.Tcw1, 7 * np) || !all_finite(in.Tcw2, 7 * np)) return fail("a pose is not finite");
  for (size_t f = 0; f < np; f++)
    for (const double* T : {in.Tcw1 + 7 * f, in.Tcw2 + 7 * f})
      if (!positive(std::sqrt(T[3] * T[3] + T[4] * T[4] + T[5] * T[5] + T[6] * T[6]))) return fail("a quaternion has zero norm or overflows");
  if (!all_finite(in.cam1, 6 * np) || !all_finite(in.cam2, 6 * np) || !all_finite(in.median_depth2, np)) return fail("an intrinsic or a median depth is not finite");
  for (size_t f = 0; f < np; f++)
    for (const double* c : {in.cam1 + 6 * f, in.cam2 + 6 * f})
      if (!(c[0] > 0 && c[1] > 0)) return fail("fx and fy must be positive");
  for (const double* kp : {in.kp1, in.kp2})
    for (size_t i = 0; i < n; i++) {
      const double* k = kp + 6 * i;
      if (!std::isfinite(k[0]) || !std::isfinite(k[1]) || !std::isfinite(k[2])) return fail("a keypoint coordinate is not finite");
      if (k[2] >= 0 && !positive(k[3])) return fail("a depth beside a right-image coordinate must be finite and positive");
      if (!positive(k[4]) || !positive(k[5])) return fail("sigma2 and scale must be finite and positive");
    }
  *n_matches = n;
  return CS_OK;
}

int run(cs_triangulate* B, const char* who, const cs_triangulate_params* p, int n_pairs, const Inputs& in, double* X3_out, double* normal3_out, double* min_distance_out,
        double* max_distance_out, unsigned char* status_out, unsigned char* route_out, unsigned char* ran_out, int* n_accepted_out, double* cos3_out, bool inspect) {
  auto fail = [&](const char* what) { cs_set_error((std::string(who) + ": " + what).c_str()); return CS_ERR_INVALID_ARG; };
  if (!B || n_pairs < 0) return fail("no handle or a negative pair count");
  int rc = check_params(p); if (rc) return rc;
  if (n_pairs == 0) { B->kernel_ms = B->host_ms = 0; B->ran = true; return CS_OK; }
  const double t_begin = cs::now_ms();
  size_t n = 0;
  rc = check_pairs(who, n_pairs, in, &n); if (rc) return rc;
  if (!ran_out || !n_accepted_out) return fail("NULL output");
  if (n > 0 && (!X3_out || !normal3_out || !min_distance_out || !max_distance_out || !status_out || !route_out || (inspect && !cos3_out))) return fail("NULL output");
  B->ran = false;                                      // (a refused call leaves the last run's timing in place; one that fails from here on does not)
  const size_t np = (size_t)n_pairs;
  size_t n_chunks = 0;
  for (size_t f = 0; f < np; f++) n_chunks += ((size_t)(in.match_ptr[f + 1] - in.match_ptr[f]) + cs::TRI_CHUNK - 1) / cs::TRI_CHUNK;

  cs::Layout li, lo;
  const size_t in_pair = li.add(np * sizeof(cs::TriPair)), in_rec = li.add(n * cs::TRI_MATCH_DOUBLES * 8), in_chunk = li.add(n_chunks * sizeof(cs::TriChunk));
  const size_t out_8 = lo.add(n * cs::TRI_OUT_DOUBLES * 8), out_st = lo.add(n), out_rt = lo.add(n), out_cos = lo.add(inspect ? n * 3 * 8 : 0);
  lo.add(16);                                          // (a batch without a match still has an output buffer)

  cs::TriLaunch a;
  auto pack = [&] {
    unsigned char* h = B->h_in.p;
    cs::TriPair* pair = reinterpret_cast<cs::TriPair*>(h + in_pair);
    cs::TriChunk* chunk = reinterpret_cast<cs::TriChunk*>(h + in_chunk);
    size_t c = 0;
    for (size_t f = 0; f < np; f++) {
      cs::triangulate_pair_record(in.Tcw1 + 7 * f, in.Tcw2 + 7 * f, in.cam1 + 6 * f, in.cam2 + 6 * f, in.median_depth2[f], p->min_baseline_ratio, pair[f]);
      for (int first = in.match_ptr[f]; first < in.match_ptr[f + 1]; first += cs::TRI_CHUNK, c++) {
        const int left = in.match_ptr[f + 1] - first;
        chunk[c].pair = (int)f; chunk[c].first = first; chunk[c].count = left < cs::TRI_CHUNK ? left : (int)cs::TRI_CHUNK; chunk[c].pad = 0;
      }
    }
    double* rec = reinterpret_cast<double*>(h + in_rec);
    for (size_t i = 0; i < n; i++, rec += cs::TRI_MATCH_DOUBLES) {
      std::memcpy(rec, in.kp1 + 6 * i, 6 * 8);
      std::memcpy(rec + 6, in.kp2 + 6 * i, 6 * 8);
    }
    std::memset(&a, 0, sizeof(a));
    a.n_chunks = (int)n_chunks;
    a.prm.min_baseline_ratio = p->min_baseline_ratio; a.prm.max_cos_parallax = p->max_cos_parallax; a.prm.chi2_mono = p->chi2_mono;
    a.prm.chi2_stereo = p->chi2_stereo; a.prm.ratio_factor = p->ratio_factor; a.prm.scale_range = p->scale_range;
    a.chunk = reinterpret_cast<const cs::TriChunk*>(B->d_in.p + in_chunk);
    a.pair = reinterpret_cast<const cs::TriPair*>(B->d_in.p + in_pair);
    a.rec = reinterpret_cast<const double*>(B->d_in.p + in_rec);
    a.out8 = reinterpret_cast<double*>(B->d_out.p + out_8);
    a.status = B->d_out.p + out_st;
    a.route = B->d_out.p + out_rt;
    a.cos3 = inspect ? reinterpret_cast<double*>(B->d_out.p + out_cos) : nullptr;
  };
  rc = cs::batch_round_trip(*B, li.bytes, lo.bytes, true, pack, [&] { cs::triangulate_launch(a, inspect, B->st); }); if (rc) return rc;

  const double* o8 = reinterpret_cast<const double*>(B->h_out.p + out_8);
  for (size_t i = 0; i < n; i++, o8 += cs::TRI_OUT_DOUBLES) {
    for (int k = 0; k < 3; k++) { X3_out[3 * i + k] = o8[k]; normal3_out[3 * i + k] = o8[3 + k]; }
    min_distance_out[i] = o8[6];
    max_distance_out[i] = o8[7];
  }
  if (n) {
    std::memcpy(status_out, B->h_out.p + out_st, n);
    std::memcpy(route_out, B->h_out.p + out_rt, n);
    if (inspect) std::memcpy(cos3_out, B->h_out.p + out_cos, n * 3 * 8);
  }
  const cs::TriPair* pair = reinterpret_cast<const cs::TriPair*>(B->h_in.p + in_pair);
  for (size_t f = 0; f < np; f++) {
    ran_out[f] = pair[f].ran != 0.0 ? 1 : 0;
    int acc = 0;
    for (int i = in.match_ptr[f]; i < in.match_ptr[f + 1]; i++) acc += status_out[i] == CS_TRI_OK ? 1 : 0;
    n_accepted_out[f] = acc;
  }
  B->host_ms = cs::now_ms() - t_begin;
  B->ran = true;
  return CS_OK;
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
  if (n_pairs < 0) { cs_set_error("cs_triangulate_pairs: a negative pair count"); return CS_ERR_INVALID_ARG; }
  cs_triangulate* B = nullptr;
  int rc = cs_triangulate_create(device, &B);
  if (rc) return rc;
  const Inputs in = {Tcw1, Tcw2, cam1, cam2, median_depth2, match_ptr, kp1, kp2};
  rc = run(B, "cs_triangulate_pairs", p, n_pairs, in, X3_out, normal3_out, min_distance_out, max_distance_out, status_out, route_out, ran_out, n_accepted_out, nullptr, false);
  cs_triangulate_destroy(B);
  return rc;
}

int cs_triangulate_inspect(int device, const cs_triangulate_params* p, int n_pairs, const double* Tcw1, const double* Tcw2, const double* cam1, const double* cam2,
                           const double* median_depth2, const int* match_ptr, const double* kp1, const double* kp2, double* X3_out, double* normal3_out,
                           double* min_distance_out, double* max_distance_out, unsigned char* status_out, unsigned char* route_out, unsigned char* ran_out,
                           int* n_accepted_out, double* cos3_out) {
  if (n_pairs < 0) { cs_set_error("cs_triangulate_inspect: a negative pair count"); return CS_ERR_INVALID_ARG; }
  cs_triangulate* B = nullptr;
  int rc = cs_triangulate_create(device, &B);
  if (rc) return rc;
  const Inputs in = {Tcw1, Tcw2, cam1, cam2, median_depth2, match_ptr, kp1, kp2};
  rc = run(B, "cs_triangulate_inspect", p, n_pairs, in, X3_out, normal3_out, min_distance_out, max_distance_out, status_out, route_out, ran_out, n_accepted_out, cos3_out, true);
  cs_triangulate_destroy(B);
  return rc;
}

}  // extern "C"
