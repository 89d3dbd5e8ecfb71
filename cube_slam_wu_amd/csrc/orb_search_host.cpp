// orb_search_host.cpp -- the C ABI of the batched guided ORB matcher (include/cubeslam_hip.h: cs_orb_search_*).
//
// What an ORB-SLAM2-derived back end does between its geometric steps in ORBmatcher::Fuse (both forms) and ORBmatcher::SearchBySim3 -- per
// map point: project into a keyframe, gate by depth range and viewing angle, predict the pyramid level, collect the keypoints of the grid
// cells around the projection, and keep the nearest descriptor -- for all jobs of a call in ONE kernel launch (orb_search_kernels.hip).
// The handle keeps a SET OF FRAMES on the device: cs_orb_search_set_frames checks every argument, makes each frame's record and its grid
// (cs_orb_search.h: orb_frame_record, orb_pack_frame -- the stable counting sort by cell happens while the keypoints are copied into the
// pinned staging buffer anyway) and uploads once; cs_orb_search_run then ships only job records, queries and the chunk table.  There is no
// CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/cubeslam_hip.h"
#include "cs_batch_handle.h"
#include "orb_search_types.h"

static_assert((int)CS_ORB_OK == cs::ORB_OK && (int)CS_ORB_SKIPPED == cs::ORB_SKIPPED && (int)CS_ORB_BEHIND == cs::ORB_BEHIND &&
              (int)CS_ORB_OUT_OF_IMAGE == cs::ORB_OUT_OF_IMAGE && (int)CS_ORB_OUT_OF_RANGE == cs::ORB_OUT_OF_RANGE && (int)CS_ORB_VIEW_ANGLE == cs::ORB_VIEW_ANGLE &&
              (int)CS_ORB_NO_CANDIDATE == cs::ORB_NO_CANDIDATE && (int)CS_ORB_TOO_FAR == cs::ORB_TOO_FAR, "cs_orb_search_status is cs_orb_search.h's");
static_assert((int)CS_ORB_CHECK_VIEW == cs::ORB_CHECK_VIEW && (int)CS_ORB_CHECK_REPROJ == cs::ORB_CHECK_REPROJ, "cs_orb_search_flags is cs_orb_search.h's");

// d_set = [frame records | cell starts | sorted keypoints | their indices | their descriptors], resident between calls;
// d_in = [job records | queries | query descriptors | skip | chunks], d_out = [best_idx | best_dist | status | level | insp5 | n_window | n_candidates]
struct cs_orb_search : cs::BatchHandle {
  cs::DevBuf<unsigned char> d_set;
  cs::PinBuf<unsigned char> h_set;
  bool has_frames = false;
  int n_frames = 0;
  cs::OrbParams prm = {};
  cs::Part<cs::OrbFrame> set_frame;        // the parts of d_set
  cs::Part<int> set_start, set_orig;
  cs::Part<double> set_kp4;
  cs::Part<unsigned> set_desc;
};

namespace {

using cs::all_finite;
using cs::positive;

int check_params(const char* who, const cs_orb_search_params* p) {
  const cs::Refuse refuse{who};
  if (!p) return refuse("NULL parameters");
  if (!positive(p->min_dist_factor) || !positive(p->max_dist_factor) || !std::isfinite(p->view_cos) || !positive(p->chi2_mono) || !positive(p->chi2_stereo))
    return refuse("the distance factors and chi2 gates must be finite and positive, view_cos finite");
  if (p->grid_cols < 1 || p->grid_cols > cs::ORB_MAX_GRID || p->grid_rows < 1 || p->grid_rows > cs::ORB_MAX_GRID) return refuse("grid_cols and grid_rows must be in 1 .. 128");
  return CS_OK;
}

struct Frames {
  const int* kp_ptr;
  const double* kp;
  const int* octave;
  const unsigned char* desc;
  const double *cam, *bounds, *scale_factor;
  const int* n_levels;
};

struct Jobs {
  const int* frame_of_job;
  const double *pose8, *th;
  const int *max_hamming, *flags, *query_ptr;
  const double *X, *normal, *dist_range;
  const unsigned char *qdesc, *skip;
};

struct Outputs {
  unsigned char* status;
  int *best_idx, *best_dist;
  unsigned char* level;
  int* n_ok;
  double* insp5;
  int *n_window, *n_candidates;
};

// What cs_orb_search_set_frames checks before anything is packed.  *n_keypoints = kp_ptr[n_frames].
int check_frames(const char* who, const cs_orb_search_params* p, int n_frames, const Frames& in, size_t* n_keypoints) {
  const cs::Refuse refuse{who};
  *n_keypoints = 0;
  if (n_frames == 0) return CS_OK;
  if (!in.kp_ptr || !in.cam || !in.bounds || !in.scale_factor || !in.n_levels) return refuse("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": kp_ptr", in.kp_ptr, n_frames)) return rc;
  const size_t nf = (size_t)n_frames, n = (size_t)in.kp_ptr[n_frames];
  if (n > (size_t)INT_MAX / 8 || nf * ((size_t)p->grid_cols * p->grid_rows + 1) > (size_t)INT_MAX / 4) return refuse("too many keypoints or frames for one set");
  if (n > 0 && (!in.kp || !in.octave || !in.desc)) return refuse("NULL keypoint array");
  if (!all_finite(in.cam, 5 * nf) || !all_finite(in.bounds, 4 * nf) || !all_finite(in.scale_factor, nf)) return refuse("an intrinsic, a bound or a scale factor is not finite");
  for (size_t f = 0; f < nf; f++) {
    const double *c = in.cam + 5 * f, *b = in.bounds + 4 * f;
    if (!(c[0] > 0 && c[1] > 0)) return refuse("fx and fy must be positive");
    if (!(b[1] > b[0] && b[3] > b[2])) return refuse("max_x > min_x and max_y > min_y are required");
    if (!std::isfinite(p->grid_cols / (b[1] - b[0])) || !std::isfinite(p->grid_rows / (b[3] - b[2]))) return refuse("the image bounds are too narrow for the grid");
    if (!(in.scale_factor[f] > 1)) return refuse("scale_factor must be greater than 1");
    if (in.n_levels[f] < 1 || in.n_levels[f] > cs::ORB_MAX_LEVELS) return refuse("n_levels must be in 1 .. 16");
    double sc = 1.0;
    for (int l = 1; l < in.n_levels[f]; l++) sc = sc * in.scale_factor[f];
    if (!std::isfinite(sc * sc)) return refuse("the level table overflows");
    for (int i = in.kp_ptr[f]; i < in.kp_ptr[f + 1]; i++)
      if (in.octave[i] < 0 || in.octave[i] >= in.n_levels[f]) return refuse("an octave is outside 0 .. n_levels - 1");
  }
  if (!all_finite(in.kp, 3 * n)) return refuse("a keypoint coordinate is not finite");
  *n_keypoints = n;
  return CS_OK;
}

// What cs_orb_search_run checks before anything is launched.  *n_queries = query_ptr[n_jobs].
int check_jobs(const char* who, int n_frames, int n_jobs, const Jobs& in, size_t* n_queries) {
  const cs::Refuse refuse{who};
  if (!in.frame_of_job || !in.pose8 || !in.th || !in.max_hamming || !in.flags || !in.query_ptr) return refuse("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": query_ptr", in.query_ptr, n_jobs)) return rc;
  const size_t nj = (size_t)n_jobs, n = (size_t)in.query_ptr[n_jobs];
  if (n > (size_t)INT_MAX / 8) return refuse("too many queries for one call");
  if (n > 0 && (!in.X || !in.normal || !in.dist_range || !in.qdesc || !in.skip)) return refuse("NULL query array");
  if (!all_finite(in.pose8, 8 * nj)) return refuse("a pose is not finite");
  for (size_t j = 0; j < nj; j++) {
    const double* T = in.pose8 + 8 * j;
    if (in.frame_of_job[j] < 0 || in.frame_of_job[j] >= n_frames) return refuse("a frame index is outside the handle's frame set");
    if (!cs::quaternion_norm_ok(T + 3)) return refuse("a quaternion has zero norm or overflows");
    if (!(T[7] > 0)) return refuse("the scale s must be positive");
    if (!positive(in.th[j])) return refuse("th must be finite and positive");
    if (in.max_hamming[j] < 0 || in.max_hamming[j] > 256) return refuse("max_hamming must be in 0 .. 256");
    if (in.flags[j] & ~(cs::ORB_CHECK_VIEW | cs::ORB_CHECK_REPROJ)) return refuse("unknown flag bits");
  }
  if (!all_finite(in.X, 3 * n) || !all_finite(in.normal, 3 * n)) return refuse("a point or a normal is not finite");
  for (size_t i = 0; i < n; i++) {
    const double lo = in.dist_range[2 * i], hi = in.dist_range[2 * i + 1];
    if (!(positive(lo) && std::isfinite(hi) && lo <= hi)) return refuse("0 < min_distance <= max_distance, both finite, are required");
  }
  *n_queries = n;
  return CS_OK;
}

int set_frames(cs_orb_search* B, const char* who, const cs_orb_search_params* p, int n_frames, const Frames& in) {
  const cs::Refuse refuse{who};
  if (!B || n_frames < 0) return refuse("no handle or a negative frame count");
  int rc = check_params(who, p); if (rc) return rc;
  size_t n = 0;
  rc = check_frames(who, p, n_frames, in, &n); if (rc) return rc;
  const size_t nf = (size_t)n_frames, cells = (size_t)p->grid_cols * p->grid_rows;

  cs::Layout l;
  const auto at_frame = l.add<cs::OrbFrame>(nf);
  const auto at_start = l.add<int>(nf * (cells + 1));
  const auto at_kp4 = l.add<double>(n * cs::ORB_KP_DOUBLES);
  const auto at_orig = l.add<int>(n);
  const auto at_desc = l.add<unsigned>(n * cs::ORB_DESC_WORDS);
  l.add<unsigned char>(16);                            // (a set without a frame still has a buffer)
  CS_HIP_TRY(hipSetDevice(B->device));
  B->has_frames = false;                               // (from here on the set the handle held is gone)
  CS_ENSURE(B->d_set, l.bytes);
  CS_ENSURE(B->h_set, l.bytes);
  unsigned char* h = B->h_set.p;
  cs::OrbFrame* frame = at_frame.at(h);
  for (size_t f = 0; f < nf; f++) {
    const int first = in.kp_ptr[f], count = in.kp_ptr[f + 1] - first;
    cs::orb_frame_record(in.cam + 5 * f, in.bounds + 4 * f, in.scale_factor[f], in.n_levels[f], p->grid_cols, p->grid_rows, first, (int)(f * (cells + 1)), frame[f]);
    frame[f].n_sorted = cs::orb_pack_frame(frame[f], count, in.kp + 3 * (size_t)first, in.octave + first, in.desc + 32 * (size_t)first,
                                           at_start.at(h) + f * (cells + 1), at_kp4.at(h) + cs::ORB_KP_DOUBLES * (size_t)first, at_orig.at(h) + first,
                                           at_desc.at(h) + cs::ORB_DESC_WORDS * (size_t)first);
  }
  CS_HIP_TRY(hipMemcpyAsync(B->d_set.p, h, l.bytes, hipMemcpyHostToDevice, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  B->prm.min_dist_factor = p->min_dist_factor; B->prm.max_dist_factor = p->max_dist_factor; B->prm.view_cos = p->view_cos; B->prm.chi2_mono = p->chi2_mono;
  B->prm.chi2_stereo = p->chi2_stereo; B->prm.grid_cols = p->grid_cols; B->prm.grid_rows = p->grid_rows;
  B->set_frame = at_frame; B->set_start = at_start; B->set_kp4 = at_kp4; B->set_orig = at_orig; B->set_desc = at_desc;
  B->n_frames = n_frames;
  B->has_frames = true;
  return CS_OK;
}

int run(cs_orb_search* B, const char* who, int n_jobs, const Jobs& in, const Outputs& out, bool inspect) {
  const cs::Refuse refuse{who};
  if (!B || n_jobs < 0) return refuse("no handle or a negative job count");
  if (!B->has_frames) return refuse("the handle holds no frame set (cs_orb_search_set_frames)");
  cs::BatchCall call(*B);
  if (n_jobs == 0) return call.empty();
  size_t n = 0;
  int rc = check_jobs(who, B->n_frames, n_jobs, in, &n); if (rc) return rc;
  if (!out.n_ok) return refuse("NULL output");
  if (n > 0 && (!out.status || !out.best_idx || !out.best_dist || !out.level || (inspect && (!out.insp5 || !out.n_window || !out.n_candidates)))) return refuse("NULL output");
  call.point_of_no_return();                           // (behind the checks: cs_batch_handle.h, BatchCall)
  const size_t nj = (size_t)n_jobs, n_chunks = cs::chunk_count(in.query_ptr, nj, cs::ORB_CHUNK);

  cs::Layout li, lo;
  const auto in_job = li.add<cs::OrbJob>(nj);
  const auto in_q = li.add<double>(n * cs::ORB_QUERY_DOUBLES);
  const auto in_qd = li.add<unsigned>(n * cs::ORB_DESC_WORDS);
  const auto in_skip = li.add<unsigned char>(n);
  const auto in_chunk = li.add<cs::Chunk>(n_chunks);
  const auto out_idx = lo.add<int>(n), out_dist = lo.add<int>(n);
  const auto out_st = lo.add<unsigned char>(n), out_lv = lo.add<unsigned char>(n);
  const auto out_insp = lo.add<double>(inspect ? n * cs::ORB_INSPECT_DOUBLES : 0);
  const auto out_nw = lo.add<int>(inspect ? n : 0), out_nc = lo.add<int>(inspect ? n : 0);
  lo.add<unsigned char>(16);                           // (a batch without a query still has an output buffer)

  cs::OrbLaunch a;
  auto pack = [&] {
    cs::OrbJob* job = in_job.at(B->h_in.p);
    for (size_t j = 0; j < nj; j++) cs::orb_job_record(in.pose8 + 8 * j, in.th[j], in.frame_of_job[j], in.max_hamming[j], in.flags[j], job[j]);
    cs::chunk_fill(in.query_ptr, nj, cs::ORB_CHUNK, in_chunk.at(B->h_in.p));
    double* q = in_q.at(B->h_in.p);
    unsigned* qd = in_qd.at(B->h_in.p);
    for (size_t i = 0; i < n; i++, q += cs::ORB_QUERY_DOUBLES, qd += cs::ORB_DESC_WORDS) {
      std::memcpy(q, in.X + 3 * i, 3 * 8);
      std::memcpy(q + 3, in.normal + 3 * i, 3 * 8);
      std::memcpy(q + 6, in.dist_range + 2 * i, 2 * 8);
      cs::orb_pack_descriptor(in.qdesc + 32 * i, qd);
    }
    if (n) cs::copy_in(in_skip, B->h_in, in.skip);
    std::memset(&a, 0, sizeof(a));
    a.n_chunks = (int)n_chunks;
    a.prm = B->prm;
    unsigned char *ds = B->d_set.p, *di = B->d_in.p, *dout = B->d_out.p;
    a.frame = B->set_frame.at(ds); a.start = B->set_start.at(ds); a.kp4 = B->set_kp4.at(ds); a.orig = B->set_orig.at(ds); a.desc = B->set_desc.at(ds);
    a.chunk = in_chunk.at(di); a.job = in_job.at(di); a.q8 = in_q.at(di); a.qdesc = in_qd.at(di); a.skip = in_skip.at(di);
    a.status = out_st.at(dout); a.level = out_lv.at(dout); a.best_idx = out_idx.at(dout); a.best_dist = out_dist.at(dout);
    a.insp5 = inspect ? out_insp.at(dout) : nullptr;
    a.n_window = inspect ? out_nw.at(dout) : nullptr;
    a.n_candidates = inspect ? out_nc.at(dout) : nullptr;
  };
  rc = cs::batch_round_trip(*B, li.bytes, lo.bytes, true, pack, [&] { cs::orb_search_launch(a, inspect, B->st); }); if (rc) return rc;

  if (n) {
    cs::copy_out(out_st, B->h_out, out.status);
    cs::copy_out(out_lv, B->h_out, out.level);
    cs::copy_out(out_idx, B->h_out, out.best_idx);
    cs::copy_out(out_dist, B->h_out, out.best_dist);
    if (inspect) {
      cs::copy_out(out_insp, B->h_out, out.insp5);
      cs::copy_out(out_nw, B->h_out, out.n_window);
      cs::copy_out(out_nc, B->h_out, out.n_candidates);
    }
  }
  cs::count_status(in.query_ptr, nj, out.status, CS_ORB_OK, out.n_ok);
  return call.done();
}

int one_shot(const char* who, int device, const cs_orb_search_params* p, int n_frames, const Frames& fr, int n_jobs, const Jobs& jb, const Outputs& out, bool inspect) {
  if (n_frames < 0 || n_jobs < 0) return cs::Refuse{who}("a negative frame or job count");
  return cs::batch_one_shot<cs_orb_search>(device, [&](cs_orb_search* B) -> int {
    if (int rc = set_frames(B, who, p, n_frames, fr)) return rc;
    return run(B, who, n_jobs, jb, out, inspect);
  });
}

}  // namespace

extern "C" {

void cs_orb_search_default_params(cs_orb_search_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_dist_factor = 0.8;
  p->max_dist_factor = 1.2;
  p->view_cos = 0.5;
  p->chi2_mono = 5.99;
  p->chi2_stereo = 7.8;
  p->grid_cols = 64;
  p->grid_rows = 48;
}

int cs_orb_search_create(int device, cs_orb_search** out) { return cs::batch_create(device, out); }

void cs_orb_search_destroy(cs_orb_search* B) { cs::batch_destroy(B); }

int cs_orb_search_set_frames(cs_orb_search* B, const cs_orb_search_params* p, int n_frames, const int* kp_ptr, const double* kp, const int* octave, const unsigned char* desc,
                             const double* cam, const double* bounds, const double* scale_factor, const int* n_levels) {
  const Frames fr = {kp_ptr, kp, octave, desc, cam, bounds, scale_factor, n_levels};
  return set_frames(B, "cs_orb_search_set_frames", p, n_frames, fr);
}

int cs_orb_search_run(cs_orb_search* B, int n_jobs, const int* frame_of_job, const double* pose8, const double* th, const int* max_hamming, const int* flags, const int* query_ptr,
                      const double* X, const double* normal, const double* dist_range, const unsigned char* qdesc, const unsigned char* skip, unsigned char* status_out,
                      int* best_idx_out, int* best_dist_out, unsigned char* level_out, int* n_ok_out) {
  const Jobs jb = {frame_of_job, pose8, th, max_hamming, flags, query_ptr, X, normal, dist_range, qdesc, skip};
  const Outputs out = {status_out, best_idx_out, best_dist_out, level_out, n_ok_out, nullptr, nullptr, nullptr};
  return run(B, "cs_orb_search_run", n_jobs, jb, out, false);
}

int cs_orb_search_last_timing(const cs_orb_search* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_orb_search_jobs(int device, const cs_orb_search_params* p, int n_frames, const int* kp_ptr, const double* kp, const int* octave, const unsigned char* desc, const double* cam,
                       const double* bounds, const double* scale_factor, const int* n_levels, int n_jobs, const int* frame_of_job, const double* pose8, const double* th,
                       const int* max_hamming, const int* flags, const int* query_ptr, const double* X, const double* normal, const double* dist_range, const unsigned char* qdesc,
                       const unsigned char* skip, unsigned char* status_out, int* best_idx_out, int* best_dist_out, unsigned char* level_out, int* n_ok_out) {
  const Frames fr = {kp_ptr, kp, octave, desc, cam, bounds, scale_factor, n_levels};
  const Jobs jb = {frame_of_job, pose8, th, max_hamming, flags, query_ptr, X, normal, dist_range, qdesc, skip};
  const Outputs out = {status_out, best_idx_out, best_dist_out, level_out, n_ok_out, nullptr, nullptr, nullptr};
  return one_shot("cs_orb_search_jobs", device, p, n_frames, fr, n_jobs, jb, out, false);
}

int cs_orb_search_inspect(int device, const cs_orb_search_params* p, int n_frames, const int* kp_ptr, const double* kp, const int* octave, const unsigned char* desc,
                          const double* cam, const double* bounds, const double* scale_factor, const int* n_levels, int n_jobs, const int* frame_of_job, const double* pose8,
                          const double* th, const int* max_hamming, const int* flags, const int* query_ptr, const double* X, const double* normal, const double* dist_range,
                          const unsigned char* qdesc, const unsigned char* skip, unsigned char* status_out, int* best_idx_out, int* best_dist_out, unsigned char* level_out,
                          int* n_ok_out, double* insp5_out, int* n_window_out, int* n_candidates_out) {
  const Frames fr = {kp_ptr, kp, octave, desc, cam, bounds, scale_factor, n_levels};
  const Jobs jb = {frame_of_job, pose8, th, max_hamming, flags, query_ptr, X, normal, dist_range, qdesc, skip};
  const Outputs out = {status_out, best_idx_out, best_dist_out, level_out, n_ok_out, insp5_out, n_window_out, n_candidates_out};
  return one_shot("cs_orb_search_inspect", device, p, n_frames, fr, n_jobs, jb, out, true);
}

int cs_orb_search_mutual(int n1, const int* best12, const unsigned char* status12, int n2, const int* best21, const unsigned char* status21, int* match12_out, int* n_out) {
  if (n1 < 0 || n2 < 0 || !n_out || (n1 > 0 && (!best12 || !status12 || !match12_out)) || (n2 > 0 && (!best21 || !status21)))
    return cs::Refuse{"cs_orb_search_mutual"}("a negative count or a NULL argument");
  int n = 0;
  for (int i = 0; i < n1; i++) {
    const int j = best12[i];
    const bool both = status12[i] == CS_ORB_OK && j >= 0 && j < n2 && status21[j] == CS_ORB_OK && best21[j] == i;
    match12_out[i] = both ? j : -1;
    n += both ? 1 : 0;
  }
  *n_out = n;
  return CS_OK;
}

}  // extern "C"
