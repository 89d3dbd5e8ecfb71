// ba_host.cpp -- host side of path B (g2o bundle adjustment) behind the C ABI of include/cubeslam_hip.h: the handle's life, graph input, the
// structure phase and its uploads, edge levels and classification, inspection, dump / load.  The numeric steps and the LM loop are ba_lm.cpp's.
//
// Mirrors, step for step, what g2o's BlockSolver + OptimizationAlgorithmLevenberg do
// (object_slam/Thirdparty/g2o/g2o/core/block_solver.hpp, optimization_algorithm_levenberg.cpp): the
// structure phase (index mapping, edge orderings, Schur pattern) runs once on the host when the edges are
// set; every numeric step is a HIP kernel on resident data; the LM control flow (lambda schedule, accept /
// reject, termination) is scalar host code fed by one chi2 read-back per trial.  There is no CPU fallback.
#include "ba_handle.h"

namespace {

using cs::now_ms;
using cs::cam_rank;
using cs::landmark_owners;
using cs::run_items;
using cs::struct_threads;

// The per-landmark camera lists of the last structure phase (st_cams_of / st_edge_of, st_cam_cnt) stay valid only while the projection edges
// [0, st_lists_edges) and the landmark count they were built for are untouched -- cs_ba_append_* only adds behind them.  EVERY entry point that
// rewrites e_pt / e_cam or the vertex arrays calls this, so that the next phase checks every edge's indices again and rebuilds the lists.
inline void proj_edge_lists_invalidate(cs_ba* B) { B->st_lists_edges = 0; B->st_cam_cnt.clear(); }

// the host's level vectors from the device's bytes, after a classification there (the layout is that of the structure phase that filled d_lvl)
int refresh_levels_host(cs_ba* B) {
  if (!B->lvl_host_stale) return CS_OK;
  const size_t nM = (size_t)B->lvl_nM, nS = (size_t)B->lvl_nS;
  std::vector<unsigned char> all(nM + nS);
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (!all.empty()) CS_HIP_TRY(hipMemcpy(all.data(), B->d_lvl.p, all.size(), hipMemcpyDeviceToHost));
  B->lvl_mono.assign(all.begin(), all.begin() + nM);
  B->lvl_stereo.assign(all.begin() + nM, all.end());
  B->lvl_host_stale = false;
  return CS_OK;
}
bool any_level(const std::vector<unsigned char>& l) { for (unsigned char c : l) if (c) return true; return false; }
// the projection edges' levels in e_pt's order (nM mono, nS stereo; a class's vector may be shorter -- appended edges are at level 0 -- or empty)
bool combined_proj_levels(const cs_ba* B, int nM, int nS, std::vector<unsigned char>& out) {
  if (!any_level(B->lvl_mono) && !any_level(B->lvl_stereo)) return false;
  out.assign((size_t)nM + nS, 0);
  std::copy(B->lvl_mono.begin(), B->lvl_mono.begin() + std::min<size_t>(B->lvl_mono.size(), nM), out.begin());
  std::copy(B->lvl_stereo.begin(), B->lvl_stereo.begin() + std::min<size_t>(B->lvl_stereo.size(), nS), out.begin() + nM);
  return true;
}
// One per-edge attribute (level, kernel kind, kernel delta) of the camera-cuboid edges in ce_cam's order -- the EdgeSE3Cuboid list, then the
// EdgeSE3CuboidProj list -- from the two classes' vectors; zero where a class's vector is empty or shorter than its list.  At least n_min entries.
template <class T>
std::vector<T> combined_cuboid(const cs_ba* B, std::vector<T> cs::EdgeClassHost::*attr, size_t n_min = 0) {
  const size_t n3 = (size_t)B->n_cub3, np = (size_t)B->n_cub - n3;
  const std::vector<T>&v3 = B->pose_class(CS_EDGE_CUBOID).*attr, &vp = B->pose_class(CS_EDGE_CUBOID_PROJ).*attr;
  std::vector<T> out(std::max(n3 + np, n_min), T(0));
  std::copy_n(v3.begin(), std::min(v3.size(), n3), out.begin());
  std::copy_n(vp.begin(), std::min(vp.size(), np), out.begin() + n3);
  return out;
}
// d_ce_active / d_oe_active = the sharding's words with the levels folded in
void fold_pose_levels(const cs_ba* B, std::vector<int>& ca, std::vector<int>& oa) {
  ca = B->h_ce_shard; oa = B->h_oe_shard;
  const std::vector<unsigned char> lc = combined_cuboid(B, &cs::EdgeClassHost::lvl), &lo = B->pose_class(CS_EDGE_ODOM).lvl;
  for (size_t k = 0; k < ca.size(); k++) if (lc[k]) ca[k] = 0;
  for (size_t k = 0; k < oa.size(); k++) if (k < lo.size() && lo[k]) oa[k] = 0;
}

// diagnostics (CS_BA_PROF): host phase clock of the structure phase, with the device allocations so far
struct PhaseMarks {
  const bool on = [] { static const bool prof = getenv("CS_BA_PROF") != nullptr; return prof; }();
  double t_ph = now_ms();
  void operator()(const char* what) { if (on) { double t = now_ms(); fprintf(stderr, "[ba structure] %-28s %8.2f ms   (%d device allocations so far)\n", what, t - t_ph, g_dbuf_reallocs); t_ph = t; } }
};

// The structure phase's uploads and zero fills, queued on the handle's stream.
// (the ~80 small uploads of a structure phase: staged in the pinned arena, copied by one kernel per group of up to 48 tables at
// the end of the phase -- nothing launched inside the phase reads them.  CS_BA_UPLOAD_KERNEL=0: one hipMemcpyAsync per table, as before.)
// (the ~50 zero fills of a structure phase -- one hipMemsetAsync each, 4-6 us of host time apiece, a third of an appended frame's phase --
// are collected and go out as one kernel per group of up to 48 buffers: zflush() where the order against other device work matters)
struct StructureUploads {
  cs_ba* B;
  std::vector<cs::BaCopyItem> copy_list;
  std::vector<std::pair<void*, size_t>> zero_list;
  const bool upload_kernel = [] { const char* e = getenv("CS_BA_UPLOAD_KERNEL"); return !e || atoi(e) != 0; }();
  explicit StructureUploads(cs_ba* b) : B(b) {}
  template <class T>
  int up(DBuf<T>& buf, const T* h, size_t n) {
    CS_TRY(upload_kernel ? buf.upload_ptr_deferred(h, n, B->stage, copy_list, B->st) : buf.upload_ptr_staged(h, n, B->stage, B->st));
    return flush(false);
  }
  template <class T>
  int up(DBuf<T>& buf, const std::vector<T>& v) { return up(buf, v.data(), v.size()); }
  template <class T>
  int alloc_zeroed(DBuf<T>& buf, size_t n) { return buf.alloc_deferred(n, zero_list); }
  int zflush() {
    for (size_t i = 0; i < zero_list.size(); i += 48) cs::ba_launch_multi_zero(zero_list.data() + i, (int)std::min<size_t>(48, zero_list.size() - i), B->st);
    zero_list.clear();
    CS_HIP_TRY(hipGetLastError());
    return CS_OK;
  }
  // (a launch per 24 tables or 2 MB staged, so that a large graph's transfers run beside the host work that follows them)
  int flush(bool all) {
    size_t bytes = 0;
    for (const cs::BaCopyItem& c : copy_list) bytes += c.bytes;
    if (!all && copy_list.size() < 24 && bytes < ((size_t)2 << 20)) return CS_OK;
    for (size_t i = 0; i < copy_list.size(); i += 48) cs::ba_launch_multi_copy(copy_list.data() + i, (int)std::min<size_t>(48, copy_list.size() - i), B->st);
    copy_list.clear();
    CS_HIP_TRY(hipGetLastError());
    return CS_OK;
  }
};

// ---- index mapping (sparse_optimizer.cpp:166-190): non-marginalised vertices by id, then the points
void reference_columns(cs_ba* B) {
  const int nc = B->nc, no = B->no;
  B->cam_col_ref.assign(nc, -1); B->cub_col_ref.assign(no, -1); B->pt_lm.assign(B->np, -1);
  int col = 0;
  auto do_cams = [&]() { for (int i = 0; i < nc; i++) if (!B->cam_fixed[i]) { B->cam_col_ref[i] = col; col += 6; } };
  auto do_cubs = [&]() { for (int i = 0; i < no; i++) if (!B->cub_fixed[i]) { B->cub_col_ref[i] = col; col += 9; } };
  if (B->cuboids_first) { do_cubs(); do_cams(); } else { do_cams(); do_cubs(); }
  B->n_pose = col;
}

// external (host-evaluated) edges: indices, and what their pattern means for the solver choice
int check_external_edges(const cs_ba* B, bool& binary_on_cuboid) {
  const int nc = B->nc, no = B->no, np = B->np;
  binary_on_cuboid = false;
  for (int k = 0; k < B->ext_n; k++) {
    const int ci = B->ext_e4[4 * k], ii = B->ext_e4[4 * k + 1], cj = B->ext_e4[4 * k + 2], ij = B->ext_e4[4 * k + 3];
    auto bad = [&](int c, int i) { return c < 0 || c > 2 || i < 0 || i >= (c == 0 ? nc : c == 1 ? no : np); };
    if (bad(ci, ii) || (ij >= 0 && bad(cj, ij))) { cs_set_error("external edge: vertex class / index out of range"); return CS_ERR_INVALID_ARG; }
    if (ij >= 0 && (ci == 2 || cj == 2)) { cs_set_error("external edge: a binary edge may join cameras and cuboids only (a marginalised point takes unary terms only: its coupling to a pose would change the Schur structure)"); return CS_ERR_INVALID_ARG; }
    if (ij >= 0 && ci == cj && ii == ij) { cs_set_error("external edge: both ends are the same vertex"); return CS_ERR_INVALID_ARG; }
    if (ij >= 0 && (ci == 1 || cj == 1)) binary_on_cuboid = true;
  }
  if (B->shard_n > 1 && (B->ext_n > 0 || B->ext_fn || B->ext_terms_set)) { cs_set_error("external (host-evaluated) edges are not supported on a sharded handle"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}
// ... their records, and the binary ones grouped by the unordered pair of vertices they join (stable: the caller's order inside a group)
int upload_external_edges(cs_ba* B, StructureUploads& U) {
  { std::vector<int> e4(B->ext_e4); if (e4.empty()) e4.assign(4, 0); CS_TRY(U.up(B->d_ext_e4, e4)); }
  std::vector<int> order, gptr(1, 0);
  auto key = [&](int k) {
    const long long a = ((long long)B->ext_e4[4 * k] << 32) | (unsigned)B->ext_e4[4 * k + 1], b = ((long long)B->ext_e4[4 * k + 2] << 32) | (unsigned)B->ext_e4[4 * k + 3];
    return std::make_pair(std::min(a, b), std::max(a, b));
  };
  for (int k = 0; k < B->ext_n; k++) if (B->ext_e4[4 * k + 3] >= 0) order.push_back(k);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key(x) < key(y); });
  for (size_t q = 0; q < order.size(); q++) if (q + 1 == order.size() || key(order[q]) != key(order[q + 1])) gptr.push_back((int)q + 1);
  B->ext_groups = (int)gptr.size() - 1;
  if (order.empty()) order.push_back(0);
  CS_TRY(U.up(B->d_ext_order, order)); CS_TRY(U.up(B->d_ext_gptr, gptr));
  return CS_OK;
}

// The elimination / band / BCR / sparse decision between two candidate systems.  (a) g2o's: cameras and cuboids (only the points are
// marginalised).  (b) The cuboids eliminated as
// well: a cuboid is coupled to the cameras that observe it and to nothing else, exactly like a landmark with a 9 x 9 block, so
// S_cc -= H_co D_oo^-1 H_co^T is the same exact block elimination -- a different elimination order of one Cholesky
// factorisation, not a different system -- and the reduced system shrinks to the cameras (C4: 10 494 -> 5 994 unknowns,
// bandwidth 182 -> 119: a cuboid couples the ~20 consecutive cameras that see it, which the landmarks' band nearly contains).
// The one with the cheaper banded factorisation (n bw^2) is taken; (b) needs the fused Schur schedule and at most
// BA_ELIM_MAX_SLOTS cameras per cuboid; sharded, a cuboid's edges then all live on ONE rank (that of its lowest-index observing
// camera) so that its block is complete where it is eliminated, and the cuboids' increments are summed over the ranks after the
// back-substitution (zero on every rank but the owner).  CS_BA_KEEP_CUBOIDS=1 forces (a).
// The ordering only permutes the linear system; g2o's order is kept for x/b inspection (cam_col_ref).
void choose_reduced_solver(cs_ba* B, const cs::Ordering& keep_o, const cs::Ordering& elim_o, bool try_elim, PhaseMarks& mark) {
  const int nc = B->nc, no = B->no;
  // banded path only where the persistent kernel's team is guaranteed to be resident on THIS device (occupancy query x CUs:
  // 256 CUs admit bandwidths up to ~1900; a partitioned or smaller device proportionally less); dense rocSOLVER otherwise
  auto band_ok = [&](const cs::Ordering& O) { return !B->force_dense && O.n_red > 128 && O.bw + 1 <= O.n_red / 2 && cs::ba_band_fits_device(O.n_red, O.bw + 1); };
  auto cost = [&](const cs::Ordering& O) { return band_ok(O) ? (double)O.n_red * (O.bw + 1.0) * (O.bw + 1.0) : (double)O.n_red * O.n_red * O.n_red / 3.0; };
  // (an ordering without unknowns -- every camera fixed, the driver's frame-0 graph -- is not a candidate: nothing would be
  // factorised and the cuboids' elimination / back-substitution hang off the reduced solve)
  B->elim = try_elim && elim_o.n_red > 0 && cost(elim_o) < cost(keep_o);
  const cs::Ordering& O = B->elim ? elim_o : keep_o;
  B->cam_col = O.cam_col; B->cub_col = O.cub_col; B->n_red = O.n_red;
  B->band_ld = band_ok(O) ? O.bw + 1 : 0;
  // A general sparse factorisation (fill-reducing order of the block graph, ba_sparse.h) where it is the fastest of the three.  The
  // estimates are fits to measurements on MI355X (tools/ba_mesh_quick.py): banded -- 1.15 n / 64 dependent steps of
  // (10 + 0.043 bw) us; dense rocSOLVER potrf -- n^3 / 3 at 11 Tflop/s + 1 ms; sparse -- 25 us per level of the elimination tree +
  // 1.5 ms per Gflop + the dense tail's n^3 / 3 at 3 Tflop/s (rocSOLVER at 1-2 k unknowns) + the dense assembly's extra cost (1 ms + the
  // n x n fill).  The plan (an O(N^2) minimum-degree sweep) is only built when the alternative costs more than 5 ms.  CS_BA_SPARSE=0 never, =1 whenever the plan fits.
  mark("  band fits device");
  B->sparse = false; B->S_clean = false;
  const char* e = getenv("CS_BA_SPARSE");
  const int mode = e ? atoi(e) : -1;
  const double nn = (double)O.n_red;
  double est_band = B->band_ld ? 1.15 * nn / 64.0 * (10.0 + 0.043 * (B->band_ld - 1)) * 1e-3 : 1e30;
  // (wide bands: the line above was fitted on bandwidths of 100-200; the 1 920-camera survey mesh -- 11 514 unknowns, bandwidth 1 121 -- takes the banded
  // kernels 14.2 ms where it says 12.0 (bench.py, ba.solver_paths: 17.2 ms per damped solve against 14.8 through the sparse path, ~3 ms of either the reduce))
  if (B->band_ld > 128) est_band *= 1.0 + 0.00018 * (B->band_ld - 128);
  const double est_dense = nn * nn * nn / 3.0 / 11e12 * 1e3 + 1.0;
  // block cyclic reduction where the band is narrow enough for 128-unknown blocks and its few levels beat the banded kernels' chain of steps
  B->use_bcr = false;
  if (B->band_ld && cs::ba_bcr_ok(O.n_red, B->band_ld)) {
    const double est_bcr = cs::ba_bcr_estimate_ms(O.n_red);
    const char* eb = getenv("CS_BAND_BCR");
    if (est_bcr < est_band || (eb && atoi(eb) == 2)) { B->use_bcr = true; est_band = est_bcr; }
  }
  const double est_other = std::min(est_band, est_dense);
  const bool consider = mode != 0 && !B->force_dense && B->shard_n == 1 && O.n_red >= 256 && (mode == 1 || est_other > 5.0);
  if (!consider) return;
  std::vector<int> dim(nc + no, 0), col(nc + no, 0);
  for (int v : O.free_ids) { dim[v] = v < nc ? 6 : 9; col[v] = v < nc ? O.cam_col[v] : O.cub_col[v - nc]; }
  const bool fits = B->solver.build(O.adj, O.free_ids, dim, col, 0.35, getenv("CS_BA_SPARSE_NO_TAIL") ? 0 : (getenv("CS_BA_SPARSE_TAIL_MAX") ? atoi(getenv("CS_BA_SPARSE_TAIL_MAX")) : 9000));
  const cs::SparsePlan& plan = B->solver.plan;      // (the handle's own: a plan that is not taken is not uploaded, and B->sparse stays false)
  const double nt = (double)plan.n_tail;
  const double est_sparse = 0.025 * plan.levels + 1.5 * plan.flops * 2e-9 + (nt > 0 ? nt * nt * nt / 3.0 / 3e12 * 1e3 + 1.0 : 0.0) + 1.0 + nn * nn * 8.0 / 2e12 * 1e3
                            + 0.3;   // (the sparse solve is not deferrable: its trials take cs_ba_optimize's synchronising flow -- four more host round trips than the stream flow of the band)
  if (mark.on && fits) fprintf(stderr, "[ba structure] sparse plan: %d vertices, %d levels, %lld values (%.1f%% of the dense triangle), largest panel %d, %.2f Gflop + a dense tail of %d unknowns; estimates ms: sparse %.1f, band %.1f, dense %.1f\n",
                               plan.N, plan.levels, plan.nvals, 100.0 * plan.nvals / (0.5 * nn * nn), plan.max_panel, plan.flops * 2e-9, plan.n_tail, est_sparse, est_band < 1e29 ? est_band : -1.0, est_dense);
  if (fits && (mode == 1 || est_sparse < est_other)) { B->sparse = true; B->band_ld = 0; B->use_bcr = false; }
}

// ---- sharded: the column cut (separator mode) where the band admits one and the device holds the kernels' teams
void choose_sharding(cs_ba* B) {
  B->sep_mode = false; B->cut.clear(); B->sepw.clear(); B->sep_off.clear(); B->n_sep = 0; B->w_max = 0; B->msg_doubles = 0;
  B->int_c = B->int_n = B->zl = B->wl = B->zr = B->wr = 0;
  const int R = B->shard_n;
  if (R <= 1 || B->band_ld <= 0 || getenv("CS_BA_SHARD_ALLREDUCE") != nullptr) return;
  std::vector<int> cut, sepw;
  if (!cs::separator_cut(B->cam_col, B->cub_col, B->n_red, B->band_ld, R, cut, sepw)) return;
  // the separator system (block tridiagonal, blocks <= w_max: a band of 2 w_max) goes through the same persistent kernels
  int wm = 0, nsep = 0;
  for (int k = 1; k < R; k++) { wm = std::max(wm, sepw[k]); nsep += sepw[k]; }
  // the interiors go through the ONE-SIDED kernel (grid = team + 1), whose residency depends on LD only: every rank decides alike
  int ni_max = 0;
  for (int r = 0; r < R; r++) ni_max = std::max(ni_max, cut[r + 1] - cut[r] - sepw[r]);
  if (!cs::ba_band_fits_device(nsep, 2 * wm) || !cs::ba_band_fits_device(ni_max, B->band_ld, true)) return;
  B->sep_mode = true; B->cut = cut; B->sepw = sepw;
  B->sep_off.assign(R + 1, 0);
  for (int k = 1; k < R; k++) { B->sep_off[k + 1] = B->sep_off[k] + sepw[k]; B->w_max = std::max(B->w_max, sepw[k]); }
  B->n_sep = B->sep_off[R];
  B->msg_doubles = 3 * (size_t)B->w_max * B->w_max + 2 * (size_t)B->w_max;
  const int r = B->shard_rank;
  B->zl = cut[r]; B->wl = sepw[r]; B->int_c = cut[r] + sepw[r]; B->int_n = cut[r + 1] - B->int_c;
  B->zr = cut[r + 1]; B->wr = (r + 1 < R) ? sepw[r + 1] : 0;
}

// stereo edges: which records are the same for every edge (the structure is unsharded here: cs_ba_set_shard refuses a stereo graph, so E = n_proj)
int decide_stereo_uniform(cs_ba* B, int E, int nM, int nS) {
  if (nS <= 0) return CS_OK;
  if (B->shard_n > 1 || E != B->n_proj) { cs_set_error("stereo projection edges are not supported on a sharded handle"); return CS_ERR_INVALID_ARG; }
  const char* env = getenv("CS_BA_UNIFORM");
  const bool on = !env || atoi(env) != 0;
  if (nM == 0) std::memcpy(B->uni8 + 4, B->h_se_intr.data(), 32);      // (no mono edge: the first stereo edge's intrinsics are the reference record)
  B->intr_uniform_all = nM > 0 ? B->intr_uniform : on;
  B->sinfo_uniform = on;
  for (int s = 0; s < nS && (B->intr_uniform_all || B->sinfo_uniform); s++) {
    if (B->intr_uniform_all && std::memcmp(&B->h_se_intr[4 * (size_t)s], B->uni8 + 4, 32) != 0) B->intr_uniform_all = false;
    if (B->sinfo_uniform && std::memcmp(&B->h_se_sinfo[10 * (size_t)s], B->h_se_sinfo.data(), 80) != 0) B->sinfo_uniform = false;
  }
  return CS_OK;
}

// The edge tables go to the device from a second host thread while the caller's builds the Schur schedule (host work only): five
// arrays of E ints through blocking copies (0.3-0.4 ms each at a million edges, from pageable memory), the zero-fills and the eight
// gathers that put the caller's measurement rows into both edge orders.  Everything is queued on B->st; the phase's one wait is
// at its end.  (The staging arena is the caller's thread's: this one copies directly.)
int upload_edge_tables(cs_ba* B, const cs::EdgeOrders& O, int nM, int nS) {
  CS_HIP_TRY(hipSetDevice(B->device));
  const int E = O.E;
  const size_t Ez = (size_t)E;
  CS_TRY(B->cm_pm.upload_ptr(O.cm_pm, Ez)); CS_TRY(B->d_src.upload_ptr(O.src_of_slot, Ez));
  // (the information / intrinsics records in the two edge orders only when they differ between edges: BaView::info_u / intr_u otherwise)
  bool per_info = !B->info_uniform, per_intr = !B->intr_uniform, have_hub = B->have_huber;
  const double* src_uv = B->raw_uv.p; const double* src_info = B->raw_info.p; const double* src_intr = B->raw_intr.p; const double* src_huber = B->raw_huber.p;
  if (nS > 0) {
    // A stereo graph: the gathers below index rows in e_pt's order -- the mono edges' rows (on the device since they were set), then the stereo
    // edges' (on the host) -- so the two are put behind each other first.  A mono edge's slot of a stereo-only field stays zero and the reverse.
    const size_t Mz = (size_t)nM, Sz = (size_t)nS;
    auto rows = [&](DBuf<double>& comb, int w, const double* mono_dev, const double* mono_rec4, const double* st_host) -> int {
      CS_TRY(comb.reserve((size_t)w * (Mz + Sz)));
      comb.n = (size_t)w * (Mz + Sz);
      if (Mz && mono_dev) CS_HIP_TRY(hipMemcpyAsync(comb.p, mono_dev, 8 * (size_t)w * Mz, hipMemcpyDeviceToDevice, B->st));
      else if (Mz && mono_rec4) cs::ba_launch_fill_rows4(comb.p, mono_rec4, nM, B->st);
      else if (Mz) CS_HIP_TRY(hipMemsetAsync(comb.p, 0, 8 * (size_t)w * Mz, B->st));
      if (st_host) CS_HIP_TRY(hipMemcpy(comb.p + (size_t)w * Mz, st_host, 8 * (size_t)w * Sz, hipMemcpyHostToDevice));
      else CS_HIP_TRY(hipMemsetAsync(comb.p + (size_t)w * Mz, 0, 8 * (size_t)w * Sz, B->st));
      return CS_OK;
    };
    per_info = nM > 0 && !B->info_uniform; per_intr = !B->intr_uniform_all; have_hub = B->have_huber || !B->h_se_huber.empty();
    CS_TRY(rows(B->comb_uv, 2, B->raw_uv.p, nullptr, B->h_se_uv.data())); src_uv = B->comb_uv.p;
    if (per_info) { CS_TRY(rows(B->comb_info, 4, B->raw_info.p, nullptr, nullptr)); src_info = B->comb_info.p; }
    if (per_intr) { CS_TRY(rows(B->comb_intr, 4, B->raw_intr_virtual ? nullptr : B->raw_intr.p, B->uni8 + 4, B->h_se_intr.data())); src_intr = B->comb_intr.p; }
    if (have_hub) { CS_TRY(rows(B->comb_huber, 1, B->have_huber ? B->raw_huber.p : nullptr, nullptr, B->h_se_huber.empty() ? nullptr : B->h_se_huber.data())); src_huber = B->comb_huber.p; }
    // the stereo-only fields in both orders, built here from the host rows
    const bool per_sinfo = !B->sinfo_uniform;
    std::vector<int> pk(Ez), ck(Ez);
    std::vector<double> pu(Ez), cu(Ez), ps(per_sinfo ? 10 * Ez : 0), cs10(per_sinfo ? 10 * Ez : 0);
    for (size_t sl = 0; sl < Ez; sl++) {
      const int s = O.src_of_slot[sl] - nM;
      pk[sl] = s >= 0; pu[sl] = s >= 0 ? B->h_se_ur[s] : 0.0;
      if (per_sinfo) { if (s >= 0) std::memcpy(&ps[10 * sl], &B->h_se_sinfo[10 * (size_t)s], 80); else std::memset(&ps[10 * sl], 0, 80); }
    }
    for (size_t q = 0; q < Ez; q++) {
      const size_t sl = (size_t)O.cm_pm[q];
      ck[q] = pk[sl]; cu[q] = pu[sl];
      if (per_sinfo) std::memcpy(&cs10[10 * q], &ps[10 * sl], 80);
    }
    CS_TRY(B->d_pm_kind.upload(pk)); CS_TRY(B->d_cm_kind.upload(ck)); CS_TRY(B->d_pm_ur.upload(pu)); CS_TRY(B->d_cm_ur.upload(cu));
    if (per_sinfo) { CS_TRY(B->d_pm_sinfo.upload(ps)); CS_TRY(B->d_cm_sinfo.upload(cs10)); }
  }
  CS_TRY(B->pm_uv.alloc(2 * Ez, B->st)); CS_TRY(B->pm_huber.alloc(Ez, B->st)); CS_TRY(B->cm_uv.alloc(2 * Ez, B->st)); CS_TRY(B->cm_huber.alloc(Ez, B->st));
  if (per_info) { CS_TRY(B->pm_info.alloc(4 * Ez, B->st)); CS_TRY(B->cm_info.alloc(4 * Ez, B->st)); }
  if (per_intr) { CS_TRY(B->pm_intr.alloc(4 * Ez, B->st)); CS_TRY(B->cm_intr.alloc(4 * Ez, B->st)); }
  cs::ba_launch_gather_rows(src_uv, B->d_src.p, E, 2, B->pm_uv.p, B->st);
  if (per_info) cs::ba_launch_gather_rows(src_info, B->d_src.p, E, 4, B->pm_info.p, B->st);
  if (per_intr) cs::ba_launch_gather_rows(src_intr, B->d_src.p, E, 4, B->pm_intr.p, B->st);
  // the width records: widths <= 0 (no kernel) as +0.0, the sign bit = the edge's level (ba_kernels.hip: edge_off); levels exist -> their
  // bytes in e_pt's order go up first (the only per-edge upload a level costs, and only here)
  const unsigned char* lvl_dev = nullptr;
  {
    std::vector<unsigned char> lv;
    B->lvl_on_device = combined_proj_levels(B, nM, nS, lv);
    if (B->lvl_on_device) { CS_TRY(B->d_lvl.upload(lv)); lvl_dev = B->d_lvl.p; B->lvl_nM = nM; B->lvl_nS = nS; }
  }
  if (have_hub || lvl_dev) cs::ba_launch_gather_widths(have_hub ? src_huber : nullptr, B->d_src.p, lvl_dev, E, B->pm_huber.p, B->st);   // (else: zeros from the allocation)
  cs::ba_launch_gather_rows(B->pm_uv.p, B->cm_pm.p, E, 2, B->cm_uv.p, B->st);
  if (per_info) cs::ba_launch_gather_rows(B->pm_info.p, B->cm_pm.p, E, 4, B->cm_info.p, B->st);
  if (per_intr) cs::ba_launch_gather_rows(B->pm_intr.p, B->cm_pm.p, E, 4, B->cm_intr.p, B->st);
  cs::ba_launch_gather_rows(B->pm_huber.p, B->cm_pm.p, E, 1, B->cm_huber.p, B->st);
  CS_HIP_TRY(hipGetLastError());
  CS_TRY(B->pm_pt.upload_ptr(O.pm_pt, Ez)); CS_TRY(B->pm_cam.upload_ptr(O.pm_cam, Ez)); CS_TRY(B->cm_pt.upload_ptr(O.cm_pt, Ez));
  return CS_OK;
}

// kernel kinds of the projection edges in both orders -- only if some edge has a kernel other than Huber
int upload_proj_kinds(cs_ba* B, StructureUploads& U, const cs::EdgeOrders& O, int nM) {
  bool generic = false;
  for (int kd : B->rk_proj) if (kd != cs::RK_NONE && kd != cs::RK_HUBER) { generic = true; break; }
  for (int kd : B->rk_stereo) if (kd != cs::RK_NONE && kd != cs::RK_HUBER) { generic = true; break; }
  if (!generic) { B->d_pm_rk.release(); B->d_cm_rk.release(); return CS_OK; }
  // (a class without a kind list has Huber wherever its delta is positive: with a kind array on the device every edge is looked up in it)
  std::vector<double> hub_m;
  if (B->rk_proj.empty() && B->have_huber && nM > 0) { hub_m.resize((size_t)nM); CS_HIP_TRY(hipMemcpy(hub_m.data(), B->raw_huber.p, 8 * (size_t)nM, hipMemcpyDeviceToHost)); }
  std::vector<int> pk, ck;
  cs::proj_kind_tables(O, [&](int src) -> int {
    if (src < nM) return !B->rk_proj.empty() ? B->rk_proj[src] : (!hub_m.empty() && hub_m[src] > 0 ? cs::RK_HUBER : cs::RK_NONE);
    const int s2 = src - nM;
    return !B->rk_stereo.empty() ? B->rk_stereo[s2] : (!B->h_se_huber.empty() && B->h_se_huber[s2] > 0 ? cs::RK_HUBER : cs::RK_NONE);
  }, pk, ck);
  CS_TRY(U.up(B->d_pm_rk, pk)); CS_TRY(U.up(B->d_cm_rk, ck));
  return CS_OK;
}

// The Schur schedules' tables, each group written once; a schedule that is not in use goes up as constructed (its placeholder).
int upload_elim_tables(cs_ba* B, StructureUploads& U, const cs::FusedSchedule& F) {
  CS_TRY(U.up(B->d_slotE_ptr, F.slotE_ptr)); CS_TRY(U.up(B->d_slotE_idx, F.slotE_idx));
  CS_TRY(U.up(B->d_cubS_ptr, F.cubS_ptr)); CS_TRY(U.up(B->d_cubS_cam, F.cubS_cam)); CS_TRY(U.up(B->d_ce_slot, F.ce_slot)); CS_TRY(U.up(B->d_cub_tile, F.cub_tile)); CS_TRY(U.up(B->d_cub_coef, F.cub_coef));
  CS_TRY(U.alloc_zeroed(B->cub_M, B->fused ? 54 * F.cubS_cam.size() : 1)); CS_TRY(U.alloc_zeroed(B->cub_Dinv, B->fused ? 81 * (size_t)std::max(1, B->no) : 1)); CS_TRY(U.alloc_zeroed(B->d_elim_fail, 1));
  return U.zflush();
}
int upload_segment_tables(cs_ba* B, StructureUploads& U, const cs::FusedSchedule& F) {
  CS_TRY(U.up(B->d_run_lm, F.run_lm)); CS_TRY(U.up(B->d_seg_ptr, F.seg_ptr)); CS_TRY(U.up(B->d_seg_k, F.seg_k)); CS_TRY(U.up(B->d_seg_tile, F.seg_tile)); CS_TRY(U.up(B->d_seg_slot, F.seg_slot));
  CS_TRY(U.up(B->d_run_e0, F.run_e0)); CS_TRY(U.up(B->d_seg_cam, F.seg_cam));
  CS_TRY(U.up(B->d_gp_ptr, F.gp_ptr)); CS_TRY(U.up(B->d_gp_i1, F.gp_i1)); CS_TRY(U.up(B->d_gp_i2, F.gp_i2)); CS_TRY(U.up(B->d_gtile, F.gtile)); CS_TRY(U.up(B->d_gcam_ptr, F.gcam_ptr)); CS_TRY(U.up(B->d_gslot, F.gslot));
  CS_TRY(U.alloc_zeroed(B->part_tiles, B->fused ? 36 * (size_t)F.n_tiles : 1)); CS_TRY(U.alloc_zeroed(B->part_coef, B->fused ? 6 * (size_t)F.n_slots : 1));
  return U.zflush();
}
int upload_pair_tables(cs_ba* B, StructureUploads& U, const cs::PairSchedule& Q) {
  CS_TRY(U.up(B->pair_ptr, Q.pair_ptr)); CS_TRY(U.up(B->pair_i1, Q.pair_i1)); CS_TRY(U.up(B->pair_i2, Q.pair_i2)); CS_TRY(U.up(B->ent_a, Q.ent_a)); CS_TRY(U.up(B->ent_b, Q.ent_b));
  return CS_OK;
}

// ---- cuboid / odometry edges: their vertex adjacency, ends, owners (with the levels folded in) and kernels
int upload_pose_edge_lists(cs_ba* B, StructureUploads& U, const cs::PoseEdgeEnds& P, cs::PoseEdgeOwners& W) {
  const cs::EdgeClassHost& od = B->pose_class(CS_EDGE_ODOM);
  const cs::VertexEdges c1 = cs::vertex_edge_csr(B->nc, P.ce_cam, P.n_cub), c2 = cs::vertex_edge_csr(B->nc, P.oe_i, P.n_odom),
                        c3 = cs::vertex_edge_csr(B->nc, P.oe_j, P.n_odom), c4 = cs::vertex_edge_csr(B->no, P.ce_cub, P.n_cub);
  CS_TRY(U.up(B->cam_ce_ptr, c1.ptr)); CS_TRY(U.up(B->cam_ce_idx, c1.idx)); CS_TRY(U.up(B->cam_oei_ptr, c2.ptr)); CS_TRY(U.up(B->cam_oei_idx, c2.idx));
  CS_TRY(U.up(B->cam_oej_ptr, c3.ptr)); CS_TRY(U.up(B->cam_oej_idx, c3.idx)); CS_TRY(U.up(B->cub_ce_ptr, c4.ptr)); CS_TRY(U.up(B->cub_ce_idx, c4.idx));
  CS_TRY(U.up(B->d_ce_cam, B->ce_cam)); CS_TRY(U.up(B->d_ce_cub, B->ce_cub)); CS_TRY(U.up(B->d_oe_i, od.a)); CS_TRY(U.up(B->d_oe_j, od.b));
  {
    std::vector<int> mine(std::max(1, B->no), 0);
    for (int o = 0; o < B->no; o++) mine[o] = W.cub_owner[o] == B->shard_rank;
    CS_TRY(U.up(B->d_cub_mine, mine));
  }
  B->h_ce_shard = W.ca; B->h_oe_shard = W.oa;
  for (cs::EdgeClassHost& c : B->ec) c.lvl.resize(any_level(c.lvl) ? (size_t)c.size() : 0);
  fold_pose_levels(B, W.ca, W.oa);      // (a level-1 edge gives zero blocks and no chi2, like an edge of another rank)
  CS_TRY(U.up(B->d_ce_active, W.ca)); CS_TRY(U.up(B->d_oe_active, W.oa));
  // kernels of the camera-cuboid edges (EdgeSE3Cuboid list, then EdgeSE3CuboidProj list) and of the odometry edges
  auto any_kernel = [](const std::vector<int>& kinds) { for (int kd : kinds) if (kd != 0) return true; return false; };
  const std::vector<int> kc = combined_cuboid(B, &cs::EdgeClassHost::rk, 1);
  if (any_kernel(kc)) {
    const std::vector<double> dc = combined_cuboid(B, &cs::EdgeClassHost::rd, 1);
    CS_TRY(U.up(B->d_ce_rk, kc)); CS_TRY(U.up(B->d_ce_rdelta, dc));
  } else { B->d_ce_rk.release(); B->d_ce_rdelta.release(); }
  if (any_kernel(od.rk)) {
    std::vector<int> kk(od.rk); std::vector<double> dd(od.rd);
    kk.resize(std::max(1, B->n_odom), 0); dd.resize(std::max(1, B->n_odom), 0.0);
    CS_TRY(U.up(B->d_oe_rk, kk)); CS_TRY(U.up(B->d_oe_rdelta, dd));
  } else { B->d_oe_rk.release(); B->d_oe_rdelta.release(); }
  return CS_OK;
}
// ... their measurements, and the blocks their kernels write
int upload_pose_edge_payload(cs_ba* B, StructureUploads& U) {
  const cs::EdgeClassHost &c3 = B->pose_class(CS_EDGE_CUBOID), &cp = B->pose_class(CS_EDGE_CUBOID_PROJ), &od = B->pose_class(CS_EDGE_ODOM);
  const size_t n_cub = (size_t)B->n_cub, n_odom = (size_t)B->n_odom;
  CS_TRY(U.up(B->ce_meas, c3.meas)); CS_TRY(U.up(B->ce_info, c3.info)); CS_TRY(U.up(B->oe_meas, od.meas)); CS_TRY(U.up(B->oe_info, od.info));
  CS_TRY(U.up(B->pe_meas, cp.meas)); CS_TRY(U.up(B->pe_info, cp.info)); CS_TRY(U.up(B->pe_K, cp.extra));
  CS_TRY(U.alloc_zeroed(B->ce_Hcc, 36 * n_cub)); CS_TRY(U.alloc_zeroed(B->ce_Hoo, 81 * n_cub)); CS_TRY(U.alloc_zeroed(B->ce_Hco, 54 * n_cub)); CS_TRY(U.alloc_zeroed(B->ce_bc, 6 * n_cub)); CS_TRY(U.alloc_zeroed(B->ce_bo, 9 * n_cub));
  CS_TRY(U.alloc_zeroed(B->oe_Hii, 36 * n_odom)); CS_TRY(U.alloc_zeroed(B->oe_Hjj, 36 * n_odom)); CS_TRY(U.alloc_zeroed(B->oe_Hij, 36 * n_odom)); CS_TRY(U.alloc_zeroed(B->oe_bi, 6 * n_odom)); CS_TRY(U.alloc_zeroed(B->oe_bj, 6 * n_odom));
  return CS_OK;
}

// ---- linear system storage (E: this rank's projection edges)
int allocate_system_storage(cs_ba* B, int E, StructureUploads& U) {
  const size_t nc = (size_t)B->nc, no = (size_t)B->no, np = (size_t)B->np;
  const int R = B->shard_n;
  CS_TRY(U.alloc_zeroed(B->Hcam, 36 * nc)); CS_TRY(U.alloc_zeroed(B->bcam, 6 * nc)); CS_TRY(U.alloc_zeroed(B->Hcub, 81 * no)); CS_TRY(U.alloc_zeroed(B->bcub, 9 * no));
  CS_TRY(U.alloc_zeroed(B->Hll, 9 * np)); CS_TRY(U.alloc_zeroed(B->bl, 3 * np)); CS_TRY(U.alloc_zeroed(B->W, 18 * (size_t)E)); CS_TRY(U.alloc_zeroed(B->WD, 18 * (size_t)E));
  CS_TRY(U.alloc_zeroed(B->Dinv, 9 * np)); CS_TRY(U.alloc_zeroed(B->dbl, 3 * np));
  B->s_doubles = (size_t)B->n_red * (B->band_ld ? B->band_ld : B->n_red);
  CS_TRY(U.alloc_zeroed(B->S, B->s_doubles + B->n_pose));   // [S | rhs]: one buffer, one all-reduce in the sharded solve
  CS_TRY(U.alloc_zeroed(B->xl, 3 * np));
  CS_TRY(U.alloc_zeroed(B->d_band_info, cs::BAND_INFO_WORDS));  // the solver's status words (band_solver.h)
  CS_TRY(U.alloc_zeroed(B->band_linv, B->band_ld ? std::max(cs::ba_band_workspace_doubles(B->n_red, B->band_ld), B->use_bcr ? cs::ba_bcr_workspace_doubles(B->n_red, 128) : (size_t)1) : 1));   // inverted diagonal blocks (+ the separator's rows in the nested order)
  B->nb_chi = cs::ba_chi2_blocks(E);
  B->n_chi_partials = B->nb_chi + (B->n_cub + B->n_odom + 63) / 64;
  CS_TRY(U.alloc_zeroed(B->chi_partial, B->n_chi_partials));
  CS_TRY(U.alloc_zeroed(B->scale_partial, (size_t)cs::ba_scale_blocks()));
  CS_TRY(U.alloc_zeroed(B->d_info, 1));
  if (B->sparse) CS_TRY(B->solver.upload(B->st));      // (one queued copy; this phase's closing wait is the one it asks for)
  if (B->sep_mode) {
    CS_TRY(U.alloc_zeroed(B->sepY, (size_t)(B->wl + B->wr) * B->int_n));
    CS_TRY(U.alloc_zeroed(B->sep_msgs, B->msg_doubles * (size_t)R));
    CS_TRY(U.alloc_zeroed(B->sepS, (size_t)B->n_sep * 2 * B->w_max + B->n_sep));   // [S_sep (band of 2 w_max) | rhs_sep]
    CS_TRY(U.alloc_zeroed(B->sep_work, std::max(cs::ba_band_workspace_doubles(B->n_sep, 2 * B->w_max), cs::ba_bcr_sep_ok(B->w_max, B->shard_n) ? cs::ba_bcr_sep_workspace_doubles(B->shard_n) : (size_t)1)));
    CS_TRY(U.alloc_zeroed(B->d_sep_info, cs::BAND_INFO_WORDS));
    CS_TRY(U.alloc_zeroed(B->int_work, cs::ba_band_workspace_doubles(B->int_n, B->band_ld)));
    CS_TRY(U.alloc_zeroed(B->d_int_info, cs::BAND_INFO_WORDS));
    std::vector<int> sep_col(R + 1, 0);
    for (int k = 1; k < R; k++) sep_col[k] = B->cut[k];
    CS_TRY(U.up(B->d_sep_off, B->sep_off)); CS_TRY(U.up(B->d_sep_col, sep_col));
    // what this rank contributes to the collectives of one LM trial: its separator message, the solution vector, three scalars
    B->bytes_per_trial = 8 * ((long long)B->msg_doubles + B->n_pose + 3);
  } else {
    CS_TRY(U.alloc_zeroed(B->sepY, 1)); CS_TRY(U.alloc_zeroed(B->sep_msgs, 1)); CS_TRY(U.alloc_zeroed(B->sepS, 1)); CS_TRY(U.alloc_zeroed(B->int_work, 1));
    CS_TRY(U.alloc_zeroed(B->d_int_info, cs::BAND_INFO_WORDS)); CS_TRY(U.alloc_zeroed(B->sep_work, 1)); CS_TRY(U.alloc_zeroed(B->d_sep_info, cs::BAND_INFO_WORDS));
    std::vector<int> none1(1, 0);
    CS_TRY(U.up(B->d_sep_off, none1)); CS_TRY(U.up(B->d_sep_col, none1));
    B->bytes_per_trial = R > 1 ? 8 * ((long long)B->s_doubles + B->n_pose + 3 + (B->elim ? B->n_pose - B->n_red : 0)) : 0;
  }
  B->bytes_per_trial_allreduce = 8 * ((long long)B->s_doubles + B->n_pose + 3 + (B->elim ? B->n_pose - B->n_red : 0));
  {
    const size_t need = std::max<size_t>(16, (size_t)B->n_pose + 2);
    CS_TRY(U.alloc_zeroed(B->d_scalars, need));
    if (B->h_scalars.cap < need) CS_ENSURE(B->h_scalars, need + need / 4 + 256);     // (with head room: a graph that grows by a camera per frame would re-pin this buffer every frame, ~0.1 ms)
  }
  CS_TRY(U.alloc_zeroed(B->cams_bak, 7 * nc)); CS_TRY(U.alloc_zeroed(B->points_bak, 3 * np)); CS_TRY(U.alloc_zeroed(B->cubes_bak, 10 * no));
  std::vector<double> u8(B->uni8, B->uni8 + 8);
  if (B->n_stereo > 0) u8.insert(u8.end(), B->h_se_sinfo.begin(), B->h_se_sinfo.begin() + 10);      // (a stereo graph: the stereo edges' reference record behind the mono one)
  return U.up(B->d_uni, u8);
}

// the kernels' view of the handle (every table is in place: the edge tables' helper thread has been joined)
void fill_view(cs_ba* B, int E, int nM, int nS) {
  cs::BaView& v = B->view;
  v.cams = B->cams.p; v.points = B->points.p; v.cubes = B->cubes.p; v.cam_col = B->d_cam_col.p; v.cub_col = B->d_cub_col.p; v.pt_free = B->d_pt_free.p;
  v.nc = B->nc; v.np = B->np; v.no = B->no; v.n_pose = B->n_pose; v.n_red = B->n_red; v.elim = B->elim ? 1 : 0; v.elim_max_slots = B->elim_max_slots;
  v.cubS_ptr = B->d_cubS_ptr.p; v.cubS_cam = B->d_cubS_cam.p; v.ce_slot = B->d_ce_slot.p; v.cub_tile = B->d_cub_tile.p; v.cub_coef = B->d_cub_coef.p;
  v.cub_mine = B->d_cub_mine.p;
  v.cub_M = B->cub_M.p; v.cub_Dinv = B->cub_Dinv.p; v.elim_fail = B->d_elim_fail.p; v.slotE_ptr = B->d_slotE_ptr.p; v.slotE_idx = B->d_slotE_idx.p;
  v.n_proj = E; v.pm_pt = B->pm_pt.p; v.pm_cam = B->pm_cam.p; v.pm_uv = B->pm_uv.p; v.pm_info = B->pm_info.p; v.pm_intr = B->pm_intr.p; v.pm_huber = B->pm_huber.p;
  v.rk_off = B->rk_off;
  v.pm_rk = B->d_pm_rk.p; v.cm_rk = B->d_cm_rk.p; v.ce_rk = B->d_ce_rk.p; v.ce_rdelta = B->d_ce_rdelta.p; v.oe_rk = B->d_oe_rk.p; v.oe_rdelta = B->d_oe_rdelta.p;
  v.pt_ptr = B->pt_ptr.p; v.cm_pm = B->cm_pm.p; v.cm_pt = B->cm_pt.p; v.cm_uv = B->cm_uv.p; v.cm_info = B->cm_info.p; v.cm_intr = B->cm_intr.p; v.cm_huber = B->cm_huber.p; v.cam_ptr = B->cam_ptr.p;
  v.n_cub3 = B->n_cub3; v.pe_meas = B->pe_meas.p; v.pe_info = B->pe_info.p; v.pe_K = B->pe_K.p;
  v.n_cub = B->n_cub; v.ce_cam = B->d_ce_cam.p; v.ce_cub = B->d_ce_cub.p; v.ce_meas = B->ce_meas.p; v.ce_info = B->ce_info.p; v.ce_active = B->d_ce_active.p;
  v.ce_Hcc = B->ce_Hcc.p; v.ce_Hoo = B->ce_Hoo.p; v.ce_Hco = B->ce_Hco.p; v.ce_bc = B->ce_bc.p; v.ce_bo = B->ce_bo.p;
  v.n_odom = B->n_odom; v.oe_i = B->d_oe_i.p; v.oe_j = B->d_oe_j.p; v.oe_meas = B->oe_meas.p; v.oe_info = B->oe_info.p; v.oe_active = B->d_oe_active.p;
  v.oe_Hii = B->oe_Hii.p; v.oe_Hjj = B->oe_Hjj.p; v.oe_Hij = B->oe_Hij.p; v.oe_bi = B->oe_bi.p; v.oe_bj = B->oe_bj.p;
  v.cam_ce_ptr = B->cam_ce_ptr.p; v.cam_ce_idx = B->cam_ce_idx.p; v.cam_oei_ptr = B->cam_oei_ptr.p; v.cam_oei_idx = B->cam_oei_idx.p;
  v.cam_oej_ptr = B->cam_oej_ptr.p; v.cam_oej_idx = B->cam_oej_idx.p; v.cub_ce_ptr = B->cub_ce_ptr.p; v.cub_ce_idx = B->cub_ce_idx.p;
  v.Hcam = B->Hcam.p; v.bcam = B->bcam.p; v.Hcub = B->Hcub.p; v.bcub = B->bcub.p; v.Hll = B->Hll.p; v.bl = B->bl.p; v.W = B->W.p; v.WD = B->WD.p;
  v.fuse_lin = 0;
  {
    v.info_u = B->info_uniform && E > 0 ? B->d_uni.p : nullptr;
    v.intr_u = B->intr_uniform && E > 0 ? B->d_uni.p + 4 : nullptr;
    v.pm_kind = v.cm_kind = nullptr; v.pm_ur = v.cm_ur = v.pm_sinfo = v.cm_sinfo = v.sinfo_u = nullptr;
    if (nS > 0) {
      v.info_u = (B->info_uniform || nM == 0) ? B->d_uni.p : nullptr;
      v.intr_u = B->intr_uniform_all ? B->d_uni.p + 4 : nullptr;
      v.pm_kind = B->d_pm_kind.p; v.cm_kind = B->d_cm_kind.p; v.pm_ur = B->d_pm_ur.p; v.cm_ur = B->d_cm_ur.p;
      if (B->sinfo_uniform) v.sinfo_u = B->d_uni.p + 8; else { v.pm_sinfo = B->d_pm_sinfo.p; v.cm_sinfo = B->d_cm_sinfo.p; }
    }
  }
  v.Dinv = B->Dinv.p; v.dbl = B->dbl.p; v.S = B->S.p; v.band_ld = B->band_ld; v.lam_lo = B->sep_mode ? B->cut[B->shard_rank] : 0; v.lam_hi = B->sep_mode ? B->cut[B->shard_rank + 1] : (B->shard_rank == 0 ? 0x7fffffff : 0); v.rhs = B->S.p + B->s_doubles; v.xl = B->xl.p;
  v.n_pairs = B->n_pairs; v.pair_ptr = B->pair_ptr.p; v.pair_i1 = B->pair_i1.p; v.pair_i2 = B->pair_i2.p; v.ent_a = B->ent_a.p; v.ent_b = B->ent_b.p;
  v.fused = B->fused ? 1 : 0; v.n_seg = B->n_seg; for (int q = 0; q < 5; q++) v.seg_class[q] = B->seg_class[q];
  v.seg_ptr = B->d_seg_ptr.p; v.seg_k = B->d_seg_k.p; v.seg_tile = B->d_seg_tile.p; v.seg_slot = B->d_seg_slot.p; v.run_lm = B->d_run_lm.p; v.run_e0 = B->d_run_e0.p; v.seg_cam = B->d_seg_cam.p;
  v.part_tiles = B->part_tiles.p; v.part_coef = B->part_coef.p;
  v.n_gpairs = B->n_gpairs; v.gpair_ptr = B->d_gp_ptr.p; v.gpair_i1 = B->d_gp_i1.p; v.gpair_i2 = B->d_gp_i2.p; v.gtile = B->d_gtile.p;
  v.gcam_ptr = B->d_gcam_ptr.p; v.gslot = B->d_gslot.p;
  v.chi_partial = B->chi_partial.p;
}

}  // namespace

// The structure phase: the passes of ba_structure.h in order, everything for the device queued on B->st, one wait at the end.
int finalize_structure(cs_ba* B) {
  if (!B->structure_dirty) return CS_OK;
  struct Clock { cs_ba* b; double t0; ~Clock() { b->tm.structure_ms += now_ms() - t0; } } clock{B, now_ms()};
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));             // nothing of an earlier call may still read the buffers (or the staging arena) reused below
  CS_TRY(refresh_levels_host(B));                      // (levels a classification left on the device survive this phase through the host's copy)
  B->pm_cm_valid = false;
  CS_TRY(B->stage.begin((size_t)8 << 20));
  PhaseMarks mark;
  const int nc = B->nc, no = B->no, np = B->np;
  // ---- checks.  Camera-cuboid edges of both kinds as one list: EdgeSE3Cuboid first, then EdgeSE3CuboidProj
  const cs::EdgeClassHost &c3 = B->pose_class(CS_EDGE_CUBOID), &cp = B->pose_class(CS_EDGE_CUBOID_PROJ), &od = B->pose_class(CS_EDGE_ODOM);
  B->ce_cam = c3.a; B->ce_cam.insert(B->ce_cam.end(), cp.a.begin(), cp.a.end());
  B->ce_cub = c3.b; B->ce_cub.insert(B->ce_cub.end(), cp.b.begin(), cp.b.end());
  B->n_cub3 = c3.size();
  B->n_cub = (int)B->ce_cam.size();
  B->n_odom = od.size();
  reference_columns(B);
  // (edges that an earlier phase of this handle has seen were checked then, and append only raises nc / np)
  for (int k = std::min(B->st_lists_edges, B->n_proj); k < B->n_proj; k++)
    if (B->e_pt[k] < 0 || B->e_pt[k] >= np || B->e_cam[k] < 0 || B->e_cam[k] >= nc) { cs_set_error("projection edge index out of range"); return CS_ERR_INVALID_ARG; }
  mark("  checks, index mapping");
  // ---- lists: every landmark's cameras (the lists of the last phase are kept on the handle: a graph that was only appended to extends them)
  const int st_nb = 1 - B->st_cur;
  cs::CameraLists L;
  B->st_cams_of[st_nb].ensure((size_t)B->n_proj); B->st_edge_of[st_nb].ensure((size_t)B->n_proj);
  L.cams_of = B->st_cams_of[st_nb].data(); L.edge_of = B->st_edge_of[st_nb].data();
  {
    const int E0 = B->st_lists_edges, np0 = (int)B->st_cam_cnt.size() - 1;
    const bool grown = E0 > 0 && np0 >= 0 && np0 <= np && E0 <= B->n_proj && (B->n_proj - E0) <= E0 / 4 && B->st_cams_of[B->st_cur].size() == (size_t)E0 && B->st_edge_of[B->st_cur].size() == (size_t)E0;
    const cs::PrevLists prev{E0, &B->st_cam_cnt, B->st_cams_of[B->st_cur].data(), B->st_edge_of[B->st_cur].data()};
    cs::landmark_camera_lists(np, B->n_proj, B->e_pt.data(), B->e_cam.data(), grown ? &prev : nullptr, B->n_proj > 20000 ? struct_threads() : 1, L);   // (200 cameras / 100 k edges: 0.67 -> 0.35 ms)
  }
  mark("  camera lists (count, fill, sort)");
  std::vector<int> seen;
  if (!cs::check_lists_collect_seen(L, np, B->pt_fixed.data(), seen)) { cs_set_error("two projection edges between the same point and camera"); return CS_ERR_INVALID_ARG; }
  mark("  duplicate check");
  // ---- sets: the free landmarks grouped by the set of cameras that see them
  const cs::CameraSets S = cs::group_by_camera_set(L, seen, seen.size() > 5000 ? struct_threads() : 1);
  mark("  group by camera set");
  mark("camera sets");
  // ---- cuboid / odometry edge indices are used below: check them first
  for (int k = 0; k < B->n_cub; k++)
    if (B->ce_cam[k] < 0 || B->ce_cam[k] >= nc || B->ce_cub[k] < 0 || B->ce_cub[k] >= no) { cs_set_error("cuboid edge index out of range"); return CS_ERR_INVALID_ARG; }
  for (int k = 0; k < B->n_odom; k++)
    if (od.a[k] < 0 || od.a[k] >= nc || od.b[k] < 0 || od.b[k] >= nc) { cs_set_error("odometry edge index out of range"); return CS_ERR_INVALID_ARG; }
  B->cam_col.assign(nc, -1); B->cub_col.assign(no, -1);
  bool ext_binary_on_cuboid = false;
  CS_TRY(check_external_edges(B, ext_binary_on_cuboid));
  const cs::Vertices V{nc, no, np, B->cam_fixed.data(), B->cub_fixed.data(), B->pt_fixed.data()};
  const cs::PoseEdgeEnds P{B->n_cub, B->ce_cam.data(), B->ce_cub.data(), B->n_odom, od.a.data(), od.b.data(), B->ext_n, B->ext_e4.data()};
  const std::vector<std::vector<int>> cub_cams = cs::cuboid_camera_lists(V, P);
  int max_slots = 0, n_free_cub = 0;
  for (int o = 0; o < no; o++) { max_slots = std::max(max_slots, (int)cub_cams[o].size()); if (!B->cub_fixed[o]) n_free_cub++; }
  bool fused_ok = getenv("CS_BA_SCHUR_PAIRS") == nullptr;
  {
    // (tracks of more than BA_FUSED_KMAX views go through the segments' plain multiply-add kernel: meant for the tail of a map -- when a
    // quarter of the landmarks are such tracks the pair-major path is the faster build again, measured at C4's size with 20 views each)
    size_t n_long = 0;
    for (int p : S.gorder) {
      const int kk = L.count(p);
      if (kk > cs::BA_LONG_KMAX) { fused_ok = false; break; }
      if (kk > cs::BA_FUSED_KMAX) n_long++;
    }
    if (4 * n_long > S.gorder.size()) fused_ok = false;
  }
  mark("  cuboid cameras, track lengths");
  // ---- orderings and the solver choice
  {
    // (an external binary edge on a cuboid couples it to something besides its observing cameras: the cuboids then stay in the system)
    B->elim_max_slots = std::max(1, std::min(max_slots, (int)cs::BA_ELIM_MAX_SLOTS));
    const bool try_elim = fused_ok && n_free_cub > 0 && max_slots <= cs::BA_ELIM_MAX_SLOTS && getenv("CS_BA_KEEP_CUBOIDS") == nullptr && !ext_binary_on_cuboid;
    cs::PoseGraph G; G.V = V; G.L = &L; G.S = &S; G.P = P; G.cub_cams = &cub_cams;
    // (the two candidate orderings only read shared data: g2o's system on a second thread while this one orders the cameras-only system)
    cs::Ordering keep_o, elim_o;
    if (try_elim && nc + no > 64) {
      run_items(2, [&](int t) { if (t == 0) elim_o = cs::rcm_ordering(G, true); else keep_o = cs::rcm_ordering(G, false); });
    } else {
      keep_o = cs::rcm_ordering(G, false);
      if (try_elim) elim_o = cs::rcm_ordering(G, true);
    }
    mark("  two orderings");
    choose_reduced_solver(B, keep_o, elim_o, try_elim, mark);
  }
  mark("ordering (RCM)");
  // ---- sharding: the column cut (separator mode) and who owns what
  choose_sharding(B);
  const cs::Sharding sh{B->shard_rank, B->shard_n, &B->cut};
  std::vector<int> owner;
  if (B->sep_mode) owner = cs::landmark_owners_by_column(L, np, B->cam_col, B->cut);   // the rank that owns the lowest column among its free cameras (none: rank 0)
  else if (B->shard_n > 1) landmark_owners(B->shard_n, nc, np, B->n_proj, B->e_pt.data(), B->e_cam.data(), owner);
  else owner.assign(np, 0);
  B->lm_owner = owner;
  int nl = 0;
  std::vector<int> pt_free(np);
  for (int i = 0; i < np; i++) { pt_free[i] = B->pt_fixed[i] ? 0 : 1; if (pt_free[i]) B->pt_lm[i] = nl++; }
  B->n_lm = nl;
  StructureUploads U(B);
  CS_TRY(U.up(B->d_cam_col, B->cam_col)); CS_TRY(U.up(B->d_cub_col, B->cub_col)); CS_TRY(U.up(B->d_pt_free, pt_free));
  CS_TRY(upload_external_edges(B, U));
  // ---- orders: the projection edges point-major and camera-major (host scratch kept on the handle for its memory only)
  cs::EdgeOrders O;
  cs::landmark_slot_ranges(L, np, owner, B->shard_rank, O);
  const int E = O.E;   // local edges
  if (B->slot_src_cap < (size_t)E) { B->slot_src_cap = (size_t)E + (B->slot_src ? (size_t)E / 4 : 0) + 1; B->slot_src.reset(new int[B->slot_src_cap]); }
  B->slot_src_n = E;
  B->st_pm_pt.ensure((size_t)E); B->st_pm_cam.ensure((size_t)E); B->st_cm_pm.ensure((size_t)E); B->st_cm_pt.ensure((size_t)E);
  O.src_of_slot = B->slot_src.get(); O.pm_pt = B->st_pm_pt.data(); O.pm_cam = B->st_pm_cam.data(); O.cm_pm = B->st_cm_pm.data(); O.cm_pt = B->st_cm_pt.data();
  const int NTH = (E > 20000) ? struct_threads() : 1;
  cs::point_major_order(L, np, owner, B->shard_rank, B->cam_col, NTH, O);
  mark("  point-major order");
  cs::camera_major_order(nc, NTH, O);
  mark("  index arrays (point-major, camera-major)");
  const int nS = B->n_stereo, nM = B->n_proj - nS;
  CS_TRY(decide_stereo_uniform(B, E, nM, nS));
  int edge_rc = CS_OK;
  std::thread edge_th([&]() { edge_rc = upload_edge_tables(B, O, nM, nS); });
  struct JoinEdge { std::thread& t; ~JoinEdge() { if (t.joinable()) t.join(); } } join_edge{edge_th};
  CS_TRY(U.up(B->pt_ptr, O.pt_ptr));
  CS_TRY(upload_proj_kinds(B, U, O, nM));
  CS_TRY(U.up(B->cam_ptr, O.cam_ptr));
  mark("edge orderings + upload");
  // ---- schedule: the Schur pattern.  Fused path: it needs every landmark to be seen by <= BA_LONG_KMAX cameras; otherwise
  // (or with CS_BA_SCHUR_PAIRS=1, diagnostics) the pair-major path.
  B->fused = fused_ok;        // (CS_BA_SCHUR_PAIRS unset, no track beyond BA_LONG_KMAX views, long tracks a minority: decided with the orderings above)
  for (int p : S.gorder) if (owner[p] == B->shard_rank && L.count(p) > cs::BA_LONG_KMAX) { B->fused = false; break; }
  B->schur_entries = 0;
  for (int p : S.gorder) if (owner[p] == B->shard_rank) { const long long k = L.count(p); B->schur_entries += k * (k + 1) / 2; }
  cs::FusedSchedule F(no);
  cs::PairSchedule Q;
  if (B->fused) {
    cs::SchurInput in;
    in.V = V; in.L = &L; in.S = &S; in.owner = &owner; in.rank = B->shard_rank; in.cam_col = &B->cam_col; in.pt_ptr = &O.pt_ptr; in.n_pose = B->n_pose;
    in.elim = B->elim; in.cub_cams = &cub_cams; in.P = P; in.seg_lm = cs::BA_SEG_LM; in.fused_kmax = cs::BA_FUSED_KMAX;
    cs::fused_segments(in, S.runs() > 256 ? struct_threads() : 1, F);
    mark("  segments of the runs");
    cs::fused_cuboid_slots(in, F);
    CS_TRY(upload_elim_tables(B, U, F));
    mark("  cuboid slots");
    cs::fused_destination_sort(in, F);
    mark("  destination sort");
    cs::fused_destination_lists(in, F);
    mark("  destination lists");
    CS_TRY(upload_segment_tables(B, U, F));
    CS_TRY(upload_pair_tables(B, U, Q));
  } else {
    Q = cs::schur_pairs(np, pt_free, O, B->cam_col, B->n_pose);
    CS_TRY(upload_pair_tables(B, U, Q));
    CS_TRY(upload_segment_tables(B, U, F));
    CS_TRY(upload_elim_tables(B, U, F));
  }
  B->n_seg = F.n_seg; B->n_gpairs = F.n_gpairs; B->n_pairs = Q.n_pairs;
  for (int q = 0; q < 5; q++) B->seg_class[q] = F.seg_class[q];
  mark("Schur schedule");
  // ---- pose edges
  cs::PoseEdgeOwners W = cs::pose_edge_owners(V, P, cub_cams, B->cam_col, B->cub_col, B->n_red, B->elim, sh);
  CS_TRY(upload_pose_edge_lists(B, U, P, W));
  mark("  pose edge lists");
  CS_TRY(upload_pose_edge_payload(B, U));
  mark("  pose edge measurements");
  // ---- storage
  CS_TRY(allocate_system_storage(B, E, U));
  // (the helper thread allocates the edge tables' device buffers: their addresses are final only once it is done)
  mark("  pose edge tables staged");
  edge_th.join();
  mark("  edge-table thread joined");
  if (edge_rc) return edge_rc;
  fill_view(B, E, nM, nS);
  // the allocations above are zeroed on B->st (one batched fill, one wait here); uploads went through blocking copies
  CS_TRY(U.zflush());
  CS_TRY(U.flush(true));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  B->append_stage.off = 0;           // (the appended rows have arrived)
  B->st_lists_edges = B->n_proj; B->st_cam_cnt = std::move(L.cam_cnt); B->st_cur = st_nb;   // (for a grown graph's next phase)
  mark("pose edges + allocations");
  B->structure_dirty = false;
  B->have_system = false;
  B->backup_live = false;
  return CS_OK;
}

// The persistent solver kernels' turn (ba_lm.cpp) is held across the collectives of a trial when they are queued on the stream (RCCL): two communicator handles in one
// process would wait for each other (one holds the turn inside a collective, the other needs the turn to enqueue its side).  One
// process per GPU is the contract; cs_ba_comm_init enforces it.
static std::atomic<int> g_comm_handles{0};

extern "C" {

int cs_ba_create(int device, cs_ba** out) {
  if (!out) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  { const int rc = cs::check_device(device); if (rc) return rc; }
  CS_GUARD_BEGIN
  cs::Guard<cs_ba> g(new cs_ba(), cs_ba_destroy);   // freed on every early return
  cs_ba* B = g.h;
  B->device = device;
  { const char* e = getenv("CS_BA_FORCE_DENSE"); B->force_dense = (e && atoi(e)) ? 1 : 0; }  // diagnostics: rocSOLVER dense path
  CS_HIP_TRY(hipSetDevice(device));
  CS_TRY(B->st.create(hipStreamNonBlocking));
  CS_TRY(B->st2.create(hipStreamNonBlocking));   // (a high-priority side stream was measured in round 5: no effect on the kernels that run beside a device-filling one)
  CS_TRY(B->st3.create(hipStreamNonBlocking));
  for (cs::Event* e : {&B->ev_fork, &B->ev_join, &B->ev_join3, &B->ev_upd}) CS_TRY(e->create(hipEventDisableTiming));
  for (auto& e : B->ev) CS_TRY(e.create());
  for (auto& e : B->sev) CS_TRY(e.create());
  CS_ENSURE(B->h_lam, 2); CS_ENSURE(B->h_trial, 8); CS_ENSURE(B->h_status, 4);
  std::fill_n(B->h_lam.p, 2, 0.0); std::fill_n(B->h_trial.p, 8, 0.0); std::fill_n(B->h_status.p, 4, 0);
  CS_TRY(B->d_lam.alloc(2));
  CS_TRY(B->blas.create(B->st));
  *out = g.disarm();
  return CS_OK;
  CS_GUARD_END("cs_ba_create")
}

// (every member gives itself back, the streams last: see the head of struct cs_ba)
void cs_ba_destroy(cs_ba* B) {
  if (!B) return;
  (void)hipSetDevice(B->device);
  for (const cs::Stream* s : {&B->st, &B->st2, &B->st3}) if (s->s) (void)hipStreamSynchronize(*s);
  if (B->comm) { (void)ncclCommDestroy(B->comm); g_comm_handles--; }
  delete B;
}

int cs_ba_set_vertices(cs_ba* B, const double* cams7, const int* cam_fixed, int nc, const double* cuboids10, const int* cub_fixed, int no,
                       const double* points3, const int* pt_fixed, int np, int cuboids_first) {
  CS_GUARD_BEGIN
  if (!B || nc < 0 || no < 0 || np < 0 || (nc && (!cams7 || !cam_fixed)) || (no && (!cuboids10 || !cub_fixed)) || (np && (!points3 || !pt_fixed))) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));       // (appended rows may still be on their way: cs_ba_append_* queues them on st)
  B->nc = nc; B->no = no; B->np = np; B->cuboids_first = cuboids_first;
  proj_edge_lists_invalidate(B);
  B->cam_fixed.assign(cam_fixed, cam_fixed + nc); B->cub_fixed.assign(cub_fixed, cub_fixed + no); B->pt_fixed.assign(pt_fixed, pt_fixed + np);
  // SE3Quat(Vector7d) normalises the rotation and makes w >= 0 (se3quat.h:68-71); cuboid::fromVector does not.
  std::vector<double> c(cams7, cams7 + 7 * (size_t)nc);
  for (int i = 0; i < nc; i++) { cs::Pose p = cs::pose_load(&c[7 * (size_t)i]); cs::pose_normalize(p); cs::pose_store(p, &c[7 * (size_t)i]); }
  int rc = B->cams.upload(c); if (rc) return rc;
  rc = B->cubes.upload(std::vector<double>(cuboids10, cuboids10 + 10 * (size_t)no)); if (rc) return rc;
  rc = B->points.upload(std::vector<double>(points3, points3 + 3 * (size_t)np)); if (rc) return rc;
  B->structure_dirty = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_set_vertices")
}

// ---- growing graphs (the reference's pattern: main_obj.cpp:802-803 adds a frame and calls optimize(5); g2o's seam is
// Solver::updateStructure, core/solver.h:62, core/block_solver.hpp:297-350).  New vertices and edges are appended behind the existing
// ones; the estimates that live on the device (possibly optimised there) stay untouched; the structure phase runs again on the
// next solve (49 ms at C4, a few ms at C3 -- DESIGN.md section 3).
// the appends' pinned staging arena (1 MB, made by the first append; rewound once the structure phase has waited for the stream)
static int append_arena(cs_ba* B) {
  if (B->append_stage.p) return CS_OK;
  return B->append_stage.begin((size_t)1 << 20);
}
int cs_ba_append_vertices(cs_ba* B, const double* cams7, const int* cam_fixed, int n_cams, const double* cuboids10, const int* cub_fixed, int n_cub,
                          const double* points3, const int* pt_fixed, int n_pts) {
  CS_GUARD_BEGIN
  if (!B || n_cams < 0 || n_cub < 0 || n_pts < 0 || (n_cams && (!cams7 || !cam_fixed)) || (n_cub && (!cuboids10 || !cub_fixed)) || (n_pts && (!points3 || !pt_fixed))) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  std::vector<double> c(cams7, cams7 + 7 * (size_t)n_cams);
  for (int i = 0; i < n_cams; i++) { cs::Pose p = cs::pose_load(&c[7 * (size_t)i]); cs::pose_normalize(p); cs::pose_store(p, &c[7 * (size_t)i]); }
  int rc;
  if ((rc = append_arena(B))) return rc;
  if ((rc = B->cams.append_ptr_staged(c.data(), 7 * (size_t)n_cams, B->append_stage, B->st)) || (rc = B->cubes.append_ptr_staged(cuboids10, 10 * (size_t)n_cub, B->append_stage, B->st)) ||
      (rc = B->points.append_ptr_staged(points3, 3 * (size_t)n_pts, B->append_stage, B->st))) return rc;
  B->cam_fixed.insert(B->cam_fixed.end(), cam_fixed, cam_fixed + n_cams);
  B->cub_fixed.insert(B->cub_fixed.end(), cub_fixed, cub_fixed + n_cub);
  B->pt_fixed.insert(B->pt_fixed.end(), pt_fixed, pt_fixed + n_pts);
  B->nc += n_cams; B->no += n_cub; B->np += n_pts;
  B->structure_dirty = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_append_vertices")
}
// are the n new records all equal to the handle's reference record (the first record ever set)?  A few threads over the caller's arrays.
static void scan_uniform_records(cs_ba* B, bool first, const double* info4, const double* intr4, int n) {
  if (first) {
    const char* env = getenv("CS_BA_UNIFORM");   // (read per call: the parity test sets the same graph up both ways in one process)
    const bool on = !env || atoi(env) != 0;
    B->info_uniform = B->intr_uniform = on && n > 0;
    if (n > 0) { std::memcpy(B->uni8, info4, 32); std::memcpy(B->uni8 + 4, intr4, 32); }
  }
  if (!(B->info_uniform || B->intr_uniform) || n <= 0) return;
  const double t_scan = now_ms();
  const int nt = n > (1 << 16) ? 8 : 1;
  std::vector<char> ok_i(nt, 1), ok_k(nt, 1);
  auto work = [&](int t) {
    const size_t lo = (size_t)n * t / nt, hi = (size_t)n * (t + 1) / nt;
    bool a = B->info_uniform, b = B->intr_uniform;
    for (size_t k = lo; k < hi && (a || b); k++) {
      if (a && std::memcmp(info4 + 4 * k, B->uni8, 32) != 0) a = false;
      if (b && std::memcmp(intr4 + 4 * k, B->uni8 + 4, 32) != 0) b = false;
    }
    ok_i[t] = a; ok_k[t] = b;
  };
  if (nt == 1) work(0);
  else { std::vector<std::thread> th; for (int t = 0; t < nt; t++) th.emplace_back(work, t); for (auto& x : th) x.join(); }
  for (int t = 0; t < nt; t++) { B->info_uniform = B->info_uniform && ok_i[t]; B->intr_uniform = B->intr_uniform && ok_k[t]; }
  if (getenv("CS_BA_PROF")) fprintf(stderr, "[ba set edges] uniform-record scan of %d edges: %.2f ms\n", n, now_ms() - t_scan);
}
int cs_ba_append_edges_proj(cs_ba* B, int n, const int* pt, const int* cam, const double* uv, const double* info4, const double* intr4, const double* huber) {
  if (!B || n < 0 || (n && (!pt || !cam || !uv || !info4 || !intr4))) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  if (n == 0) return CS_OK;
  const int n_mono = B->n_proj - B->n_stereo;      // (the stereo edges keep their place behind the mono ones)
  if (n_mono > 0 && (huber != nullptr) != B->have_huber) { cs_set_error("cs_ba_append_edges_proj: Huber deltas must be given for all projection edges or for none"); return CS_ERR_INVALID_ARG; }
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  int rc;
  const bool first_edges = n_mono == 0;
  scan_uniform_records(B, first_edges, info4, intr4, n);
  if (first_edges) { B->raw_info_virtual = B->info_uniform; B->raw_intr_virtual = B->intr_uniform; B->raw_info.n = 0; B->raw_intr.n = 0; }
  // an appended edge with another record: the records of the edges so far are written out from the reference record, then kept per edge
  auto write_out = [&](DBuf<double>& raw, const double* rec4, bool& is_virtual) -> int {
    int r = raw.reserve(4 * (size_t)(n_mono + n));
    if (r) return r;
    cs::ba_launch_fill_rows4(raw.p, rec4, n_mono, B->st);
    CS_HIP_TRY(hipGetLastError());
    raw.n = 4 * (size_t)n_mono;
    is_virtual = false;
    return CS_OK;
  };
  if (B->raw_info_virtual && !B->info_uniform && (rc = write_out(B->raw_info, B->uni8, B->raw_info_virtual))) return rc;
  if (B->raw_intr_virtual && !B->intr_uniform && (rc = write_out(B->raw_intr, B->uni8 + 4, B->raw_intr_virtual))) return rc;
  if ((rc = append_arena(B))) return rc;
  if ((rc = B->raw_uv.append_ptr_staged(uv, 2 * (size_t)n, B->append_stage, B->st))) return rc;
  if (!B->raw_info_virtual && (rc = B->raw_info.append_ptr_staged(info4, 4 * (size_t)n, B->append_stage, B->st))) return rc;
  if (!B->raw_intr_virtual && (rc = B->raw_intr.append_ptr_staged(intr4, 4 * (size_t)n, B->append_stage, B->st))) return rc;
  if (huber) { rc = B->raw_huber.append_ptr_staged(huber, (size_t)n, B->append_stage, B->st); if (rc) return rc; }
  B->have_huber = huber != nullptr;
  B->e_pt.insert(B->e_pt.end() - B->n_stereo, pt, pt + n); B->e_cam.insert(B->e_cam.end() - B->n_stereo, cam, cam + n);
  if (B->n_stereo > 0) proj_edge_lists_invalidate(B);      // (the stereo edges' indices moved)
  if (!B->rk_proj.empty()) for (int k = 0; k < n; k++) B->rk_proj.push_back((huber && huber[k] > 0) ? cs::RK_HUBER : cs::RK_NONE);
  B->n_proj += n;
  B->structure_dirty = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_append_edges_proj")
}
// The six entry points of the pose-edge classes: cs_ba_set_edges_* replaces the class's list (its kernels and levels go with it), cs_ba_append_edges_*
// extends it (cs::EdgeClassHost::add).
static int pose_edges_add(cs_ba* B, int edge_class, bool replace, int n, const int* a, const int* b, const double* meas, const double* info, const double* extra) {
  if (!B || !B->pose_class(edge_class).add(replace, n, a, b, meas, info, extra)) return CS_ERR_INVALID_ARG;
  B->structure_dirty = true;
  return CS_OK;
}
int cs_ba_append_edges_cuboid(cs_ba* B, int n, const int* cam, const int* cub, const double* meas10, const double* info81) {
  CS_GUARD_BEGIN
  return pose_edges_add(B, CS_EDGE_CUBOID, false, n, cam, cub, meas10, info81, nullptr);
  CS_GUARD_END("cs_ba_append_edges_cuboid")
}
int cs_ba_append_edges_cuboid_proj(cs_ba* B, int n, const int* cam, const int* cub, const double* meas4, const double* info16, const double* K9) {
  CS_GUARD_BEGIN
  return pose_edges_add(B, CS_EDGE_CUBOID_PROJ, false, n, cam, cub, meas4, info16, K9);
  CS_GUARD_END("cs_ba_append_edges_cuboid_proj")
}
int cs_ba_append_edges_odom(cs_ba* B, int n, const int* ci, const int* cj, const double* meas7, const double* info36) {
  CS_GUARD_BEGIN
  return pose_edges_add(B, CS_EDGE_ODOM, false, n, ci, cj, meas7, info36, nullptr);
  CS_GUARD_END("cs_ba_append_edges_odom")
}

int cs_ba_set_estimates(cs_ba* B, const double* cams7, const double* cuboids10, const double* points3) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));       // (appended rows may still be on their way)
  if (cams7 && B->nc) {
    std::vector<double> c(cams7, cams7 + 7 * (size_t)B->nc);
    for (int i = 0; i < B->nc; i++) { cs::Pose p = cs::pose_load(&c[7 * (size_t)i]); cs::pose_normalize(p); cs::pose_store(p, &c[7 * (size_t)i]); }
    CS_HIP_TRY(hipMemcpy(B->cams.p, c.data(), 56 * (size_t)B->nc, hipMemcpyHostToDevice));
  }
  if (cuboids10 && B->no) CS_HIP_TRY(hipMemcpy(B->cubes.p, cuboids10, 80 * (size_t)B->no, hipMemcpyHostToDevice));
  if (points3 && B->np) CS_HIP_TRY(hipMemcpy(B->points.p, points3, 24 * (size_t)B->np, hipMemcpyHostToDevice));
  B->have_system = false;
  B->backup_live = false;
  return CS_OK;
  CS_GUARD_END("cs_ba_set_estimates")
}

int cs_ba_set_edges_proj(cs_ba* B, int n, const int* pt, const int* cam, const double* uv, const double* info4, const double* intr4, const double* huber) {
  CS_GUARD_BEGIN
  if (!B || n < 0 || (n && (!pt || !cam || !uv || !info4 || !intr4))) return CS_ERR_INVALID_ARG;
  {   // the mono edges are replaced; the stereo edges behind them stay
    const std::vector<int> sp(B->e_pt.end() - B->n_stereo, B->e_pt.end()), sc(B->e_cam.end() - B->n_stereo, B->e_cam.end());
    B->e_pt.assign(pt, pt + n); B->e_cam.assign(cam, cam + n);
    B->e_pt.insert(B->e_pt.end(), sp.begin(), sp.end()); B->e_cam.insert(B->e_cam.end(), sc.begin(), sc.end());
  }
  B->n_proj = n + B->n_stereo;
  proj_edge_lists_invalidate(B);
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));       // (appended rows may still be on their way)
  int rc;
  if ((rc = refresh_levels_host(B))) return rc;
  B->lvl_mono.clear();                            // (a new list: every edge at level 0; the stereo edges keep theirs)
  scan_uniform_records(B, true, info4, intr4, n);
  if ((rc = B->raw_uv.upload_ptr(uv, 2 * (size_t)n))) return rc;
  B->raw_info_virtual = B->info_uniform; B->raw_intr_virtual = B->intr_uniform;
  if (B->raw_info_virtual) B->raw_info.n = 0; else if ((rc = B->raw_info.upload_ptr(info4, 4 * (size_t)n))) return rc;
  if (B->raw_intr_virtual) B->raw_intr.n = 0; else if ((rc = B->raw_intr.upload_ptr(intr4, 4 * (size_t)n))) return rc;
  B->have_huber = huber != nullptr;
  B->rk_proj.clear();
  if (huber) { rc = B->raw_huber.upload_ptr(huber, (size_t)n); if (rc) return rc; } else B->raw_huber.release();
  B->structure_dirty = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_set_edges_proj")
}

// EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.h:178-206): uvr3 = (u_left, v, u_right), info9 row-major, intr5 = fx fy cx cy bf, huber as
// cs_ba_set_edges_proj's.  The edges follow the mono projection edges in g2o's edge order and join the same device lists.
static int stereo_edges_add(cs_ba* B, bool replace, int n, const int* pt, const int* cam, const double* uvr3, const double* info9, const double* intr5, const double* huber) {
  if (!B || n < 0 || (n && (!pt || !cam || !uvr3 || !info9 || !intr5))) return CS_ERR_INVALID_ARG;
  if (n > 0 && B->shard_n > 1) { cs_set_error("stereo projection edges are not supported on a sharded handle"); return CS_ERR_INVALID_ARG; }
  if (!replace && n == 0) return CS_OK;
  if (!replace && B->n_stereo > 0 && (huber != nullptr) != !B->h_se_huber.empty()) { cs_set_error("cs_ba_append_edges_proj_stereo: Huber deltas must be given for all stereo edges or for none"); return CS_ERR_INVALID_ARG; }
  if (replace) {
    if (int rl = refresh_levels_host(B)) return rl;
    B->lvl_stereo.clear();
    B->e_pt.resize(B->e_pt.size() - B->n_stereo); B->e_cam.resize(B->e_cam.size() - B->n_stereo);
    B->n_proj -= B->n_stereo; B->n_stereo = 0;
    B->h_se_uv.clear(); B->h_se_ur.clear(); B->h_se_intr.clear(); B->h_se_sinfo.clear(); B->h_se_huber.clear(); B->rk_stereo.clear();
    proj_edge_lists_invalidate(B);
  }
  B->e_pt.insert(B->e_pt.end(), pt, pt + n); B->e_cam.insert(B->e_cam.end(), cam, cam + n);
  for (int k = 0; k < n; k++) {
    B->h_se_uv.push_back(uvr3[3 * (size_t)k]); B->h_se_uv.push_back(uvr3[3 * (size_t)k + 1]); B->h_se_ur.push_back(uvr3[3 * (size_t)k + 2]);
    B->h_se_intr.insert(B->h_se_intr.end(), intr5 + 5 * (size_t)k, intr5 + 5 * (size_t)k + 4);
    B->h_se_sinfo.insert(B->h_se_sinfo.end(), info9 + 9 * (size_t)k, info9 + 9 * (size_t)k + 9); B->h_se_sinfo.push_back(intr5[5 * (size_t)k + 4]);
    if (huber) B->h_se_huber.push_back(huber[k]);
    if (!B->rk_stereo.empty()) B->rk_stereo.push_back((huber && huber[k] > 0) ? cs::RK_HUBER : cs::RK_NONE);
  }
  B->n_stereo += n; B->n_proj += n;
  B->structure_dirty = true;
  return CS_OK;
}
int cs_ba_set_edges_proj_stereo(cs_ba* B, int n, const int* pt, const int* cam, const double* uvr3, const double* info9, const double* intr5, const double* huber) {
  CS_GUARD_BEGIN
  return stereo_edges_add(B, true, n, pt, cam, uvr3, info9, intr5, huber);
  CS_GUARD_END("cs_ba_set_edges_proj_stereo")
}
int cs_ba_append_edges_proj_stereo(cs_ba* B, int n, const int* pt, const int* cam, const double* uvr3, const double* info9, const double* intr5, const double* huber) {
  CS_GUARD_BEGIN
  return stereo_edges_add(B, false, n, pt, cam, uvr3, info9, intr5, huber);
  CS_GUARD_END("cs_ba_append_edges_proj_stereo")
}

int cs_ba_set_edges_cuboid(cs_ba* B, int n, const int* cam, const int* cub, const double* meas10, const double* info81) {
  CS_GUARD_BEGIN
  return pose_edges_add(B, CS_EDGE_CUBOID, true, n, cam, cub, meas10, info81, nullptr);
  CS_GUARD_END("cs_ba_set_edges_cuboid")
}
int cs_ba_set_edges_cuboid_proj(cs_ba* B, int n, const int* cam, const int* cub, const double* meas4, const double* info16, const double* K9) {
  CS_GUARD_BEGIN
  return pose_edges_add(B, CS_EDGE_CUBOID_PROJ, true, n, cam, cub, meas4, info16, K9);
  CS_GUARD_END("cs_ba_set_edges_cuboid_proj")
}
int cs_ba_set_edges_odom(cs_ba* B, int n, const int* ci, const int* cj, const double* meas7, const double* info36) {
  CS_GUARD_BEGIN
  return pose_edges_add(B, CS_EDGE_ODOM, true, n, ci, cj, meas7, info36, nullptr);
  CS_GUARD_END("cs_ba_set_edges_odom")
}

// ---- external (host-evaluated) edges: the CPU path for edge types the library does not evaluate.  The caller runs such an edge through
// its own virtuals -- computeError, linearizeOplus, constructQuadraticForm (core/optimizable_graph.h:394-454, base_binary_edge.hpp:54-205,
// base_unary_edge.hpp:42-123) -- and hands over what they accumulate.
int cs_ba_set_external_edges(cs_ba* B, int n, const int* class_i, const int* idx_i, const int* class_j, const int* idx_j) {
  if (!B || n < 0 || (n && (!class_i || !idx_i || !class_j || !idx_j))) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  // an edge whose two ends are the same vertex has no off-diagonal block (its whole quadratic form belongs to the vertex's diagonal terms,
  // cs_ba_set_external_terms' cam36 / cub81 / pt9): the off-diagonal kernel would address the upper triangle of a diagonal block
  for (int k = 0; k < n; k++)
    if (class_i[k] == class_j[k] && idx_i[k] == idx_j[k]) { cs_set_error("cs_ba_set_external_edges: edge " + std::to_string(k) + " joins a vertex to itself; add its terms to the vertex's diagonal block instead"); return CS_ERR_INVALID_ARG; }
  B->ext_n = n;
  B->ext_e4.resize(4 * (size_t)n);
  for (int k = 0; k < n; k++) { B->ext_e4[4 * k] = class_i[k]; B->ext_e4[4 * k + 1] = idx_i[k]; B->ext_e4[4 * k + 2] = class_j[k]; B->ext_e4[4 * k + 3] = idx_j[k]; }
  B->ext_terms_set = false;
  B->structure_dirty = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_set_external_edges")
}
int cs_ba_set_external_terms(cs_ba* B, const double* cam36, const double* cam6, const double* cub81, const double* cub9, const double* pt9, const double* pt3,
                             const double* Hij81, double chi2) {
  CS_GUARD_BEGIN
  if (!B || (cam36 && !cam6) || (cub81 && !cub9) || (pt9 && !pt3) || (B->ext_n > 0 && !Hij81)) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));     // the previous linearisation may still read the buffers
  int rc;
  auto put = [&](DBuf<double>& d, const double* h, size_t n) -> int { return h ? d.upload_ptr(h, n) : d.alloc(n, B->st); };
  if ((rc = put(B->ext_cam36, cam36, 36 * (size_t)B->nc)) || (rc = put(B->ext_cam6, cam6, 6 * (size_t)B->nc)) || (rc = put(B->ext_cub81, cub81, 81 * (size_t)B->no)) ||
      (rc = put(B->ext_cub9, cub9, 9 * (size_t)B->no)) || (rc = put(B->ext_pt9, pt9, 9 * (size_t)B->np)) || (rc = put(B->ext_pt3, pt3, 3 * (size_t)B->np)) ||
      (rc = put(B->ext_Hij, Hij81, 81 * (size_t)B->ext_n))) return rc;
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  B->ext_has_cam = cam36 != nullptr; B->ext_has_cub = cub81 != nullptr; B->ext_has_pt = pt9 != nullptr;
  if (Hij81) B->h_ext_Hij.assign(Hij81, Hij81 + 81 * (size_t)B->ext_n); else B->h_ext_Hij.clear();
  B->ext_chi2 = chi2;
  B->ext_terms_set = true;
  B->have_system = false;
  return CS_OK;
  CS_GUARD_END("cs_ba_set_external_terms")
}
int cs_ba_set_external_chi2(cs_ba* B, double chi2) {
  if (!B) return CS_ERR_INVALID_ARG;
  if (!B->ext_terms_set) { cs_set_error("cs_ba_set_external_chi2: call cs_ba_set_external_terms first"); return CS_ERR_NOT_RUN; }
  B->ext_chi2 = chi2;
  return CS_OK;
}
int cs_ba_set_external_callback(cs_ba* B, cs_external_fn fn, void* ctx) {
  if (!B) return CS_ERR_INVALID_ARG;
  B->ext_fn = fn; B->ext_ctx = ctx;
  return CS_OK;
}

// What the handle keeps per edge class, whichever way the class stores it: the caller's edge count (-1: no such class), the levels, the kernel
// kinds and the kernel deltas (nullptr: the mono projection edges', which live on the device in raw_huber).
struct EdgeClassRef { int count; std::vector<unsigned char>* levels; std::vector<int>* kinds; std::vector<double>* deltas; };
static EdgeClassRef edge_class_ref(cs_ba* B, int edge_class) {
  switch (edge_class) {
    case CS_EDGE_PROJ: return {B->n_proj - B->n_stereo, &B->lvl_mono, &B->rk_proj, nullptr};
    case CS_EDGE_PROJ_STEREO: return {B->n_stereo, &B->lvl_stereo, &B->rk_stereo, &B->h_se_huber};
    case CS_EDGE_CUBOID: case CS_EDGE_CUBOID_PROJ: case CS_EDGE_ODOM: { cs::EdgeClassHost& c = B->pose_class(edge_class); return {c.size(), &c.lvl, &c.rk, &c.rd}; }
    default: return {-1, nullptr, nullptr, nullptr};
  }
}
static const int kEdgeClasses[5] = {CS_EDGE_PROJ, CS_EDGE_PROJ_STEREO, CS_EDGE_CUBOID, CS_EDGE_CUBOID_PROJ, CS_EDGE_ODOM};      // (in the order of the dump's level trailer)
static bool any_class_level(cs_ba* B) { for (int c : kEdgeClasses) if (any_level(*edge_class_ref(B, c).levels)) return true; return false; }

// Robust kernels of one edge class (OptimizableGraph::Edge::setRobustKernel, core/optimizable_graph.h:419-423; the kernels:
// core/robust_kernel_impl.cpp:78-165).  Replaces the class's kernels; n = the class's edge count.
int cs_ba_set_robust_kernels(cs_ba* B, int edge_class, int n, const int* kind, const double* delta) {
  CS_GUARD_BEGIN
  if (!B || n < 0 || (n && kind && !delta)) return CS_ERR_INVALID_ARG;
  const EdgeClassRef cls = edge_class_ref(B, edge_class);
  if (cls.count < 0) { cs_set_error("cs_ba_set_robust_kernels: unknown edge class"); return CS_ERR_INVALID_ARG; }
  if (!kind) n = cls.count;         // removing the class's kernels: the count is the library's own (n is ignored)
  if (n != cls.count) { cs_set_error("cs_ba_set_robust_kernels: n must equal the number of edges of the class (set the edges first)"); return CS_ERR_INVALID_ARG; }
  std::vector<int> kk(n, 0); std::vector<double> dd(n, 0.0);
  for (int k = 0; k < n && kind; k++) {
    if (kind[k] < 0 || kind[k] >= cs::RK_KINDS) { cs_set_error("cs_ba_set_robust_kernels: unknown kernel kind"); return CS_ERR_INVALID_ARG; }
    if (kind[k] != cs::RK_NONE && !(delta[k] > 0)) { cs_set_error("cs_ba_set_robust_kernels: a kernel needs delta > 0"); return CS_ERR_INVALID_ARG; }
    kk[k] = kind[k]; dd[k] = kind[k] != cs::RK_NONE ? delta[k] : 0.0;
  }
  if (edge_class == CS_EDGE_PROJ) {      // the mono projection edges' deltas live on the device
    CS_HIP_TRY(hipSetDevice(B->device));
    CS_HIP_TRY(hipStreamSynchronize(B->st));
    int rc = B->raw_huber.upload_ptr(dd.data(), (size_t)n); if (rc) return rc;    // delta per edge, 0 = none
    B->have_huber = true;
  } else *cls.deltas = dd;
  *cls.kinds = kk;
  B->structure_dirty = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_set_robust_kernels")
}

// ---- edge levels, kernels switched in place, classification, rounds: ORB-SLAM2's LocalBundleAdjustment / BundleAdjustment on the device ----------
static int levels_refuse_shard(const cs_ba* B, const char* who) {
  if (B->shard_n <= 1) return CS_OK;
  cs_set_error(std::string(who) + ": edge levels are not supported on a sharded handle");
  return CS_ERR_INVALID_ARG;
}
// the host's projection levels into a finished structure: the bytes in e_pt's order, the signs of the width records in both edge orders
static int push_proj_levels(cs_ba* B) {
  const int nS = B->n_stereo, nM = B->n_proj - nS, E = B->slot_src_n;
  std::vector<unsigned char> lv;
  const bool any = combined_proj_levels(B, nM, nS, lv);
  if (!any && !B->lvl_on_device) return CS_OK;       // (nothing on the device to take back)
  if (!any) lv.assign((size_t)nM + nS, 0);
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  int rc = B->d_lvl.upload(lv); if (rc) return rc;
  B->lvl_nM = nM; B->lvl_nS = nS;
  cs::ba_launch_relabel_widths(B->pm_huber.p, B->d_src.p, B->d_lvl.p, E, B->st);
  cs::ba_launch_gather_rows(B->pm_huber.p, B->cm_pm.p, E, 1, B->cm_huber.p, B->st);
  CS_HIP_TRY(hipGetLastError());
  B->lvl_on_device = any;
  return CS_OK;
}
static int push_pose_levels(cs_ba* B) {
  std::vector<int> ca, oa;
  fold_pose_levels(B, ca, oa);
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (!ca.empty()) CS_HIP_TRY(hipMemcpy(B->d_ce_active.p, ca.data(), sizeof(int) * ca.size(), hipMemcpyHostToDevice));
  if (!oa.empty()) CS_HIP_TRY(hipMemcpy(B->d_oe_active.p, oa.data(), sizeof(int) * oa.size(), hipMemcpyHostToDevice));
  return CS_OK;
}
int cs_ba_set_edge_levels(cs_ba* B, int edge_class, int n, const unsigned char* level) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  if (int rs = levels_refuse_shard(B, "cs_ba_set_edge_levels")) return rs;
  const EdgeClassRef cls = edge_class_ref(B, edge_class);
  if (cls.count < 0) { cs_set_error("cs_ba_set_edge_levels: unknown edge class"); return CS_ERR_INVALID_ARG; }
  if (n != cls.count) { cs_set_error("cs_ba_set_edge_levels: n must equal the number of edges of the class"); return CS_ERR_INVALID_ARG; }
  for (int k = 0; k < n && level; k++) if (level[k] > 1) { cs_set_error("cs_ba_set_edge_levels: a level is 0 or 1"); return CS_ERR_INVALID_ARG; }
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = refresh_levels_host(B); if (rc) return rc;
  std::vector<unsigned char>& l = *cls.levels;
  if (level) l.assign(level, level + n); else l.clear();
  B->have_system = false;          // (the system on the device is the old active set's)
  if (B->structure_dirty) return CS_OK;      // (the structure phase that is due applies them)
  return (edge_class == CS_EDGE_PROJ || edge_class == CS_EDGE_PROJ_STEREO) ? push_proj_levels(B) : push_pose_levels(B);
  CS_GUARD_END("cs_ba_set_edge_levels")
}
int cs_ba_get_edge_levels(cs_ba* B, int edge_class, int n, unsigned char* level) {
  CS_GUARD_BEGIN
  if (!B || (n && !level)) return CS_ERR_INVALID_ARG;
  const EdgeClassRef cls = edge_class_ref(B, edge_class);
  if (cls.count < 0) { cs_set_error("cs_ba_get_edge_levels: unknown edge class"); return CS_ERR_INVALID_ARG; }
  if (n != cls.count) { cs_set_error("cs_ba_get_edge_levels: n must equal the number of edges of the class"); return CS_ERR_INVALID_ARG; }
  int rc = refresh_levels_host(B); if (rc) return rc;
  const std::vector<unsigned char>& l = *cls.levels;
  for (int k = 0; k < n; k++) level[k] = (size_t)k < l.size() ? l[k] : 0;
  return CS_OK;
  CS_GUARD_END("cs_ba_get_edge_levels")
}
int cs_ba_set_kernels_enabled(cs_ba* B, int edge_class, int enabled) {
  if (!B || edge_class_ref(B, edge_class).count < 0) return CS_ERR_INVALID_ARG;
  const int bit = 1 << edge_class, now = enabled ? (B->rk_off & ~bit) : (B->rk_off | bit);
  if (now != B->rk_off) B->have_system = false;
  B->rk_off = now;
  B->view.rk_off = now;            // (a scalar of the kernels' argument block: no upload, no structure phase)
  return CS_OK;
}
static int cs_ba_classify_edges_impl(cs_ba* B, const cs_ba_classify* p, int n_outliers[2], double* chi2_mono, double* chi2_stereo) {
  if (!B || !p) return CS_ERR_INVALID_ARG;
  if (int rs = levels_refuse_shard(B, "cs_ba_classify_edges")) return rs;
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = finalize_structure(B); if (rc) return rc;
  const int nS = B->n_stereo, nM = B->n_proj - nS, E = B->slot_src_n;
  const bool want_chi = chi2_mono || chi2_stereo;
  if (!B->lvl_on_device) {      // the first level of this structure: its bytes, all 0
    if ((rc = B->d_lvl.alloc((size_t)nM + nS, B->st))) return rc;
    B->lvl_nM = nM; B->lvl_nS = nS; B->lvl_on_device = true;
  }
  if (!B->pm_cm_valid) {
    if ((rc = B->d_pm_cm.reserve((size_t)E))) return rc;
    B->d_pm_cm.n = (size_t)E;
    cs::ba_launch_invert_perm(B->cm_pm.p, E, B->d_pm_cm.p, B->st);
    B->pm_cm_valid = true;
  }
  if ((rc = B->d_cls_counts.alloc(2, B->st))) return rc;
  if (want_chi && (rc = B->d_cls_chi.alloc((size_t)nM + nS, B->st))) return rc;
  cs::BaClassify a{};
  a.thr_mono = p->chi2_mono; a.thr_stereo = p->chi2_stereo; a.depth_positive = p->depth_positive; a.sticky = p->sticky;
  a.pm_huber = B->pm_huber.p; a.cm_huber = B->cm_huber.p; a.pm_cm = B->d_pm_cm.p; a.src = B->d_src.p; a.lvl = B->d_lvl.p; a.n_mono = nM;
  a.counts = B->d_cls_counts.p; a.chi_out = want_chi ? B->d_cls_chi.p : nullptr;
  cs::ba_launch_classify(B->view, a, B->st);
  CS_HIP_TRY(hipGetLastError());
  int cnt[2] = {0, 0};
  CS_HIP_TRY(hipMemcpyAsync(cnt, B->d_cls_counts.p, sizeof(cnt), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (chi2_mono && nM) CS_HIP_TRY(hipMemcpy(chi2_mono, B->d_cls_chi.p, 8 * (size_t)nM, hipMemcpyDeviceToHost));
  if (chi2_stereo && nS) CS_HIP_TRY(hipMemcpy(chi2_stereo, B->d_cls_chi.p + nM, 8 * (size_t)nS, hipMemcpyDeviceToHost));
  if (n_outliers) { n_outliers[0] = cnt[0]; n_outliers[1] = cnt[1]; }
  if (p->chi2_mono > 0 || p->chi2_stereo > 0) { B->lvl_host_stale = true; B->have_system = false; }
  return CS_OK;
}
int cs_ba_classify_edges(cs_ba* B, const cs_ba_classify* p, int n_outliers[2], double* chi2_mono, double* chi2_stereo) {
  CS_GUARD_BEGIN
  return cs_ba_classify_edges_impl(B, p, n_outliers, chi2_mono, chi2_stereo);
  CS_GUARD_END("cs_ba_classify_edges")
}
int cs_ba_optimize_rounds(cs_ba* B, const cs_ba_round* rounds, int n_rounds, int* iterations_done, int* n_outliers, double* chi2_hist, double* lambda_hist, int* trials_hist, int hist_cap) {
  CS_GUARD_BEGIN
  if (!B || n_rounds < 0 || (n_rounds && !rounds) || hist_cap < 0) return CS_ERR_INVALID_ARG;
  if (int rs = levels_refuse_shard(B, "cs_ba_optimize_rounds")) return rs;
  for (int r = 0; r < n_rounds; r++) if (rounds[r].iterations < 0) return CS_ERR_INVALID_ARG;
  for (int r = 0; r < n_rounds; r++) {
    int rc = cs_ba_set_kernels_enabled(B, CS_EDGE_PROJ, rounds[r].kernels_enabled); if (rc) return rc;
    if ((rc = cs_ba_set_kernels_enabled(B, CS_EDGE_PROJ_STEREO, rounds[r].kernels_enabled))) return rc;
    const size_t off = (size_t)r * hist_cap;
    int done = 0;
    rc = cs_ba_optimize_sharded_impl(B, rounds[r].iterations, nullptr, nullptr, &done, chi2_hist ? chi2_hist + off : nullptr, lambda_hist ? lambda_hist + off : nullptr,
                                     trials_hist ? trials_hist + off : nullptr, hist_cap);
    if (rc) return rc;
    if (iterations_done) iterations_done[r] = done;
    int cnt[2] = {-1, -1};
    if (rounds[r].classify.chi2_mono > 0 || rounds[r].classify.chi2_stereo > 0) { rc = cs_ba_classify_edges_impl(B, &rounds[r].classify, cnt, nullptr, nullptr); if (rc) return rc; }
    if (n_outliers) { n_outliers[2 * r] = cnt[0]; n_outliers[2 * r + 1] = cnt[1]; }
  }
  return CS_OK;
  CS_GUARD_END("cs_ba_optimize_rounds")
}

int cs_ba_set_shard(cs_ba* B, int rank, int n_ranks) {
  if (!B || n_ranks < 1 || rank < 0 || rank >= n_ranks) return CS_ERR_INVALID_ARG;
  if (B->n_stereo > 0 && n_ranks > 1) { cs_set_error("cs_ba_set_shard: stereo projection edges are not supported on a sharded handle"); return CS_ERR_INVALID_ARG; }
  if (n_ranks > 1 && (B->lvl_host_stale || any_class_level(B))) {
    cs_set_error("cs_ba_set_shard: edge levels are not supported on a sharded handle"); return CS_ERR_INVALID_ARG;
  }
  B->shard_rank = rank; B->shard_n = n_ranks;
  B->structure_dirty = true;
  return CS_OK;
}

int cs_ba_shard_landmark_owners(int n_ranks, int n_cams, int n_points, int n_proj, const int* e_pt, const int* e_cam, int* owner_out) {
  if (n_ranks < 1 || n_cams < 0 || n_points < 0 || n_proj < 0 || (n_proj && (!e_pt || !e_cam)) || (n_points && !owner_out)) return CS_ERR_INVALID_ARG;
  std::vector<int> owner;
  landmark_owners(n_ranks, n_cams, n_points, n_proj, e_pt, e_cam, owner);
  std::copy(owner.begin(), owner.end(), owner_out);
  return CS_OK;
}

// ---- RCCL: one process per GPU, the library issues the collectives itself (ncclAllReduce on the handle's stream)
int cs_ba_comm_unique_id(unsigned char id128[128]) {
  if (!id128) return CS_ERR_INVALID_ARG;
  ncclUniqueId id;
  BA_NCCL(ncclGetUniqueId(&id));
  static_assert(sizeof(id.internal) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id128, id.internal, 128);
  return CS_OK;
}

int cs_ba_comm_init(cs_ba* B, int rank, int n_ranks, const unsigned char id128[128]) {
  if (!B || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  if (B->comm) { (void)ncclCommDestroy(B->comm); B->comm = nullptr; g_comm_handles--; }
  if (g_comm_handles.load() > 0) { cs_set_error("cs_ba_comm_init: this process already holds a communicator handle (one process per GPU)"); return CS_ERR_INVALID_ARG; }
  ncclUniqueId id;
  std::memcpy(id.internal, id128, 128);
  BA_NCCL(ncclCommInitRank(&B->comm, n_ranks, id, rank));
  g_comm_handles++;
  return cs_ba_set_shard(B, rank, n_ranks);
}

// How the sharded solve is organised (after the structure phase): separator mode or the all-reduce of the whole [S | b]; the size of
// the separator system; the bytes this rank contributes to the collectives of one LM trial, and what the all-reduce would be.
int cs_ba_shard_info(cs_ba* B, int* sep_mode, int* n_sep, int* w_max, long long* bytes_per_trial, long long* bytes_per_trial_allreduce, int* interior_n) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  if (sep_mode) *sep_mode = B->sep_mode ? 1 : 0;
  if (n_sep) *n_sep = B->n_sep;
  if (w_max) *w_max = B->w_max;
  if (bytes_per_trial) *bytes_per_trial = B->bytes_per_trial;
  if (bytes_per_trial_allreduce) *bytes_per_trial_allreduce = B->bytes_per_trial_allreduce;
  if (interior_n) *interior_n = B->sep_mode ? B->int_n : B->n_red;
  return CS_OK;
  CS_GUARD_END("cs_ba_shard_info")
}
// Accumulated stage times of the separator-mode solves (ms; divide by cs_ba_timing::n_solves): interior factorisation, separator
// message (Y = B L^-T, T, t), gather of the messages (through a callback this includes the host round trip), separator system
// (assembly + dense Cholesky + solve), interior back-substitution.  They partition cs_ba_timing::factor_ms.
int cs_ba_shard_timing(cs_ba* B, double out5[5]) {
  if (!B || !out5) return CS_ERR_INVALID_ARG;
  for (int i = 0; i < 5; i++) out5[i] = B->sep_ms[i];
  return CS_OK;
}
// The rank that owns each landmark under the rule in force (separator mode: by the lowest column of its free cameras).
int cs_ba_get_landmark_owners(cs_ba* B, int* owner_out) {
  if (!B || (B->np && !owner_out)) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  std::copy(B->lm_owner.begin(), B->lm_owner.end(), owner_out);
  return CS_OK;
  CS_GUARD_END("cs_ba_get_landmark_owners")
}

int cs_ba_get_state(cs_ba* B, double* cams7, double* cuboids10, double* points3) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (cams7 && B->nc) CS_HIP_TRY(hipMemcpy(cams7, B->cams.p, 56 * (size_t)B->nc, hipMemcpyDeviceToHost));
  if (cuboids10 && B->no) CS_HIP_TRY(hipMemcpy(cuboids10, B->cubes.p, 80 * (size_t)B->no, hipMemcpyDeviceToHost));
  if (points3 && B->np) CS_HIP_TRY(hipMemcpy(points3, B->points.p, 24 * (size_t)B->np, hipMemcpyDeviceToHost));
  return CS_OK;
  CS_GUARD_END("cs_ba_get_state")
}

int cs_ba_sizes(cs_ba* B, int* size_pose, int* size_lm) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  int rc = finalize_structure(B); if (rc) return rc;
  if (size_pose) *size_pose = B->n_pose;
  if (size_lm) *size_lm = 3 * B->n_lm;
  return CS_OK;
  CS_GUARD_END("cs_ba_sizes")
}

int cs_ba_solver_layout(cs_ba* B, int* band_ld, int* team) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  int rc = finalize_structure(B); if (rc) return rc;
  int rw = 0;
  if (band_ld) *band_ld = B->band_ld;
  if (team) *team = B->band_ld ? cs::ba_band_team(B->band_ld, &rw) : 0;
  return CS_OK;
  CS_GUARD_END("cs_ba_solver_layout")
}

static int cs_ba_get_system_impl(cs_ba* B, double* Hpp, double* Hll9, double* Hpl18, double* b, double* x) {
  if (!B) return CS_ERR_INVALID_ARG;
  if (int rn = need_system(B, "cs_ba_get_system")) return rn;
  CS_HIP_TRY(hipSetDevice(B->device));
  const int n = B->n_pose;
  if (Hpp) {
    std::memset(Hpp, 0, sizeof(double) * (size_t)n * n);
    std::vector<double> hc(36 * (size_t)B->nc), ho(81 * (size_t)B->no), hco(54 * (size_t)B->n_cub), hij(36 * (size_t)B->n_odom);
    if (B->nc) CS_HIP_TRY(hipMemcpy(hc.data(), B->Hcam.p, 8 * hc.size(), hipMemcpyDeviceToHost));
    if (B->no) CS_HIP_TRY(hipMemcpy(ho.data(), B->Hcub.p, 8 * ho.size(), hipMemcpyDeviceToHost));
    if (B->n_cub) CS_HIP_TRY(hipMemcpy(hco.data(), B->ce_Hco.p, 8 * hco.size(), hipMemcpyDeviceToHost));
    if (B->n_odom) CS_HIP_TRY(hipMemcpy(hij.data(), B->oe_Hij.p, 8 * hij.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < B->nc; i++) { int c = B->cam_col_ref[i]; if (c < 0) continue; for (int r = 0; r < 6; r++) for (int q = 0; q < 6; q++) Hpp[(size_t)(c + r) * n + c + q] = hc[36 * (size_t)i + 6 * r + q]; }
    for (int i = 0; i < B->no; i++) { int c = B->cub_col_ref[i]; if (c < 0) continue; for (int r = 0; r < 9; r++) for (int q = 0; q < 9; q++) Hpp[(size_t)(c + r) * n + c + q] = ho[81 * (size_t)i + 9 * r + q]; }
    for (int k = 0; k < B->n_cub; k++) {
      int ca = B->cam_col_ref[B->ce_cam[k]], cb = B->cub_col_ref[B->ce_cub[k]];
      if (ca < 0 || cb < 0) continue;
      for (int r = 0; r < 6; r++) for (int q = 0; q < 9; q++) { double val = hco[54 * (size_t)k + 9 * r + q]; Hpp[(size_t)(ca + r) * n + cb + q] += val; Hpp[(size_t)(cb + q) * n + ca + r] += val; }
    }
    const cs::EdgeClassHost& od = B->pose_class(CS_EDGE_ODOM);
    for (int k = 0; k < B->n_odom; k++) {
      int ca = B->cam_col_ref[od.a[k]], cb = B->cam_col_ref[od.b[k]];
      if (ca < 0 || cb < 0) continue;
      for (int r = 0; r < 6; r++) for (int q = 0; q < 6; q++) { double val = hij[36 * (size_t)k + 6 * r + q]; Hpp[(size_t)(ca + r) * n + cb + q] += val; Hpp[(size_t)(cb + q) * n + ca + r] += val; }
    }
    for (int k = 0; k < B->ext_n && B->ext_terms_set; k++) {     // the host-evaluated binary edges' blocks
      const int ci = B->ext_e4[4 * k], ii = B->ext_e4[4 * k + 1], cj = B->ext_e4[4 * k + 2], ij = B->ext_e4[4 * k + 3];
      if (ij < 0) continue;
      const int ca = ci ? B->cub_col_ref[ii] : B->cam_col_ref[ii], cb = cj ? B->cub_col_ref[ij] : B->cam_col_ref[ij], di = ci ? 9 : 6, dj = cj ? 9 : 6;
      if (ca < 0 || cb < 0) continue;
      for (int r = 0; r < di; r++) for (int q = 0; q < dj; q++) { const double val = B->h_ext_Hij[81 * (size_t)k + dj * r + q]; Hpp[(size_t)(ca + r) * n + cb + q] += val; Hpp[(size_t)(cb + q) * n + ca + r] += val; }
    }
  }
  if (Hll9) {
    std::vector<double> hl(9 * (size_t)B->np);
    if (B->np) CS_HIP_TRY(hipMemcpy(hl.data(), B->Hll.p, 8 * hl.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < B->np; i++) if (B->pt_lm[i] >= 0) std::memcpy(Hll9 + 9 * (size_t)B->pt_lm[i], &hl[9 * (size_t)i], 72);
  }
  if (Hpl18) {
    std::vector<double> w(18 * (size_t)B->slot_src_n);
    if (!w.empty()) CS_HIP_TRY(hipMemcpy(w.data(), B->W.p, 8 * w.size(), hipMemcpyDeviceToHost));
    std::memset(Hpl18, 0, 144 * (size_t)B->n_proj);      // (an edge owned by another rank stays zero)
    for (int sl = 0; sl < B->slot_src_n; sl++) std::memcpy(Hpl18 + 18 * (size_t)B->slot_src[sl], &w[18 * (size_t)sl], 144);
  }
  auto to_ref = [&](const std::vector<double>& src, double* dst) {  // solver order -> g2o's order
    for (int i = 0; i < B->nc; i++) if (B->cam_col[i] >= 0) std::memcpy(dst + B->cam_col_ref[i], &src[B->cam_col[i]], 48);
    for (int i = 0; i < B->no; i++) if (B->cub_col[i] >= 0) std::memcpy(dst + B->cub_col_ref[i], &src[B->cub_col[i]], 72);
    std::memcpy(dst + B->n_pose, &src[B->n_pose], 8 * (src.size() - B->n_pose));
  };
  if (b) to_ref(B->h_b, b);
  if (x && !B->h_x.empty()) to_ref(B->h_x, x);
  return CS_OK;
}
int cs_ba_get_system(cs_ba* B, double* Hpp, double* Hll9, double* Hpl18, double* b, double* x) {
  CS_GUARD_BEGIN
  return cs_ba_get_system_impl(B, Hpp, Hll9, Hpl18, b, x);
  CS_GUARD_END("cs_ba_get_system")
}

// Solver::computeMarginals (core/block_solver.hpp:488-499): LinearSolver::solvePattern(spinv, blockIndices, *_Hpp) -- blocks of the INVERSE of
// the pose-pose Hessian H_pp as buildSystem left it (no lambda: restoreDiagonal has run; no Schur complement: the reference's call factorises
// _Hpp itself, core/marginal_covariance_cholesky.cpp:154-222).  Block k = rows of vertex (class_i[k], idx_i[k]) x columns of vertex
// (class_j[k], idx_j[k]), row-major, d_i x d_j doubles (6 per camera, 9 per cuboid), one after the other in `out`.  H_pp is assembled dense in
// g2o's index order (as cs_ba_get_system), factorised by rocSOLVER, and the columns of the requested j-vertices are solved for: a call for
// inspection and for covariance queries of a handful of vertices, not a per-iteration path.  Returns CS_ERR_NOT_RUN before cs_ba_build_system,
// CS_ERR_INVALID_ARG for a fixed vertex or a point, *positive_definite = 0 (and CS_OK) when the factorisation fails (g2o: false).
int cs_ba_pose_marginals(cs_ba* B, int n_pairs, const int* class_i, const int* idx_i, const int* class_j, const int* idx_j, double* out, int* positive_definite) {
  CS_GUARD_BEGIN
  if (!B || n_pairs < 0 || (n_pairs && (!class_i || !idx_i || !class_j || !idx_j || !out))) return CS_ERR_INVALID_ARG;
  if (positive_definite) *positive_definite = 1;
  if (int rn = need_system(B, "cs_ba_pose_marginals")) return rn;
  if (B->shard_n > 1) { cs_set_error("cs_ba_pose_marginals: not on a sharded handle (a rank holds a partial system)"); return CS_ERR_INVALID_ARG; }
  if (n_pairs == 0) return CS_OK;
  const int n = B->n_pose;
  if (n <= 0) { cs_set_error("cs_ba_pose_marginals: the graph has no free camera or cuboid"); return CS_ERR_INVALID_ARG; }
  if ((long long)n * n > (1ll << 28)) { cs_set_error("cs_ba_pose_marginals: the dense pose Hessian would exceed 2 GB"); return CS_ERR_CAPACITY; }
  auto col_of = [&](int cls, int idx, int& dim) -> int {
    if (cls == CS_VERTEX_CAM) { dim = 6; return (idx >= 0 && idx < B->nc) ? B->cam_col_ref[idx] : -1; }
    if (cls == CS_VERTEX_CUBOID) { dim = 9; return (idx >= 0 && idx < B->no) ? B->cub_col_ref[idx] : -1; }
    dim = 0; return -1;
  };
  // the distinct column vertices: one block column of right-hand sides each
  std::vector<int> col_base, col_dim, rhs_of_pair(n_pairs);
  std::map<int, int> rhs_at;            // pose column -> first right-hand-side column
  int m = 0;
  for (int k = 0; k < n_pairs; k++) {
    int di, dj;
    const int ci = col_of(class_i[k], idx_i[k], di), cj = col_of(class_j[k], idx_j[k], dj);
    if (ci < 0 || cj < 0) { cs_set_error("cs_ba_pose_marginals: pair " + std::to_string(k) + " names a fixed vertex, a point or an index out of range"); return CS_ERR_INVALID_ARG; }
    auto it = rhs_at.find(cj);
    if (it == rhs_at.end()) { it = rhs_at.emplace(cj, m).first; col_base.push_back(cj); col_dim.push_back(dj); m += dj; }
    rhs_of_pair[k] = it->second;
  }
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  std::vector<double> H((size_t)n * n);
  { const int rc = cs_ba_get_system_impl(B, H.data(), nullptr, nullptr, nullptr, nullptr); if (rc) return rc; }
  std::vector<double> E((size_t)n * m, 0.0);      // column-major n x m: unit vectors
  for (size_t q = 0, c0 = 0; q < col_base.size(); c0 += col_dim[q], q++)
    for (int d = 0; d < col_dim[q]; d++) E[(c0 + d) * (size_t)n + col_base[q] + d] = 1.0;
  DBuf<double> dH, dE;
  DBuf<int> dinfo;
  int rc;
  if ((rc = dH.reserve((size_t)n * n)) || (rc = dE.reserve((size_t)n * m)) || (rc = dinfo.reserve(1))) return rc;
  CS_HIP_TRY(hipMemcpyAsync(dH.p, H.data(), 8 * H.size(), hipMemcpyHostToDevice, B->st));
  CS_HIP_TRY(hipMemcpyAsync(dE.p, E.data(), 8 * E.size(), hipMemcpyHostToDevice, B->st));
  CS_ROC_TRY(rocblas_set_stream(B->blas, B->st));
  CS_ROC_TRY(rocsolver_dpotrf(B->blas, rocblas_fill_upper, n, dH.p, n, dinfo.p));      // (symmetric: row- and column-major are the same matrix)
  int info = 0;
  CS_HIP_TRY(hipMemcpyAsync(&info, dinfo.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (info != 0) { if (positive_definite) *positive_definite = 0; return CS_OK; }
  CS_ROC_TRY(rocsolver_dpotrs(B->blas, rocblas_fill_upper, n, m, dH.p, n, dE.p, n));
  CS_HIP_TRY(hipMemcpyAsync(E.data(), dE.p, 8 * E.size(), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  size_t o = 0;
  for (int k = 0; k < n_pairs; k++) {
    int di, dj;
    const int ci = col_of(class_i[k], idx_i[k], di);
    (void)col_of(class_j[k], idx_j[k], dj);
    for (int r = 0; r < di; r++) for (int c = 0; c < dj; c++) out[o++] = E[(size_t)(rhs_of_pair[k] + c) * n + ci + r];
  }
  return CS_OK;
  CS_GUARD_END("cs_ba_pose_marginals")
}

// Inspection for parity tests: the damped reduced system exactly as the solver is about to factorise it -- dense symmetric n_red x n_red
// (n_red = cs_ba_reduced_size), its right-hand side, and the column of every camera / cuboid in it (solver order = reverse
// Cuthill-McKee; -1: fixed; a cuboid column >= n_red: the cuboid was eliminated and is not part of S).  Runs the Schur-complement build
// (block_solver.hpp:373-439) at `lambda` on the current linearisation; no factorisation.
int cs_ba_get_reduced_system(cs_ba* B, double lambda, double* S_dense, double* rhs, int* cam_col, int* cub_col) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  if (int rn = need_system(B, "cs_ba_get_reduced_system")) return rn;
  if (B->shard_n > 1) { cs_set_error("cs_ba_get_reduced_system: not on a sharded handle (a rank holds a partial system)"); return CS_ERR_INVALID_ARG; }
  CS_HIP_TRY(hipSetDevice(B->device));
  const int n = B->n_red;
  if (cam_col) std::copy(B->cam_col.begin(), B->cam_col.end(), cam_col);
  if (cub_col) std::copy(B->cub_col.begin(), B->cub_col.end(), cub_col);
  if (n <= 0) return CS_OK;
  { int rcl = put_lambda(B, lambda); if (rcl) return rcl; }
  CS_HIP_TRY(hipMemsetAsync(B->S.p, 0, sizeof(double) * (B->s_doubles + B->n_pose), B->st));
  CS_HIP_TRY(hipMemsetAsync(B->d_elim_fail.p, 0, sizeof(int), B->st));
  cs::ba_launch_reduce(B->view, B->d_lam.p, B->st, B->st2, B->ev_fork, B->ev_join);
  if (B->ext_n > 0 && B->ext_terms_set) cs::ba_launch_ext_offdiag(B->view, B->ext_groups, B->d_ext_gptr.p, B->d_ext_order.p, B->d_ext_e4.p, B->ext_Hij.p, B->st);
  CS_HIP_TRY(hipGetLastError());
  std::vector<double> h(B->s_doubles + B->n_pose);
  CS_HIP_TRY(hipMemcpyAsync(h.data(), B->S.p, 8 * h.size(), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (rhs) std::copy(h.begin() + B->s_doubles, h.begin() + B->s_doubles + n, rhs);
  if (S_dense) {
    std::memset(S_dense, 0, sizeof(double) * (size_t)n * n);
    if (B->band_ld) {
      for (int c = 0; c < n; c++)
        for (int d = 0; d < B->band_ld && c + d < n; d++) { const double v = h[(size_t)c * B->band_ld + d]; S_dense[(size_t)(c + d) * n + c] = v; S_dense[(size_t)c * n + c + d] = v; }
    } else {
      for (int r = 0; r < n; r++) for (int c = 0; c <= r; c++) { const double v = h[(size_t)r * n + c]; S_dense[(size_t)r * n + c] = v; S_dense[(size_t)c * n + r] = v; }
    }
  }
  return CS_OK;
  CS_GUARD_END("cs_ba_get_reduced_system")
}

int cs_ba_reduced_size(cs_ba* B, int* n_reduced, int* cuboids_eliminated) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  if (n_reduced) *n_reduced = B->n_red;
  if (cuboids_eliminated) *cuboids_eliminated = B->elim ? 1 : 0;
  return CS_OK;
  CS_GUARD_END("cs_ba_reduced_size")
}

int cs_ba_band_order(cs_ba* B, int* block_cyclic_reduction, int* levels) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  const bool bcr = B->band_ld > 0 && B->use_bcr;
  if (block_cyclic_reduction) *block_cyclic_reduction = bcr ? 1 : 0;
  if (levels) { int L = 0; for (int N = (B->n_red + 127) / 128; bcr && N >= 1; N /= 2) L++; *levels = L; }
  return CS_OK;
  CS_GUARD_END("cs_ba_band_order")
}
int cs_ba_solver_path(cs_ba* B, int* path, int* bandwidth, double* sparse_fill) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  if (path) *path = B->band_ld ? CS_BA_PATH_BAND : (B->sparse ? CS_BA_PATH_SPARSE : CS_BA_PATH_DENSE);
  if (bandwidth) *bandwidth = B->band_ld ? B->band_ld - 1 : 0;
  if (sparse_fill) *sparse_fill = B->sparse ? B->solver.fill(B->n_red) : 0.0;
  return CS_OK;
  CS_GUARD_END("cs_ba_solver_path")
}

int cs_ba_schur_layout(cs_ba* B, int* fused, int* n_segments, int* n_partial_blocks, int* n_blocks) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  if (fused) *fused = B->fused ? 1 : 0;
  if (n_segments) *n_segments = B->n_seg;
  if (n_partial_blocks) *n_partial_blocks = (int)(B->part_tiles.n / 36);
  if (n_blocks) *n_blocks = B->fused ? B->n_gpairs : B->n_pairs;
  return CS_OK;
  CS_GUARD_END("cs_ba_schur_layout")
}

// Inspection for tests: a fingerprint of every index table the structure phase leaves on the device (edge orders, per-vertex lists,
// the Schur schedule, the solver's column maps), one 64-bit FNV-1a hash per table in a fixed order.  Two builds of one graph -- the
// threaded loops and CS_BA_STRUCT_THREADS=1, an appended graph and the same graph set up at once -- must agree table by table.
int cs_ba_structure_digest(cs_ba* B, unsigned long long* out, int cap, int* n_tables) {
  if (!B || !n_tables || cap < 0 || (cap && !out)) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  int rc = finalize_structure(B); if (rc) return rc;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  const DBuf<int>* tabs[] = {&B->d_cam_col, &B->d_cub_col, &B->d_pt_free, &B->pm_pt, &B->pm_cam, &B->pt_ptr, &B->cm_pm, &B->cm_pt, &B->cam_ptr, &B->d_src,
                             &B->d_run_lm, &B->d_seg_ptr, &B->d_seg_k, &B->d_seg_tile, &B->d_seg_slot, &B->d_gp_ptr, &B->d_gp_i1, &B->d_gp_i2, &B->d_gtile, &B->d_gcam_ptr, &B->d_gslot,
                             &B->pair_ptr, &B->pair_i1, &B->pair_i2, &B->ent_a, &B->ent_b, &B->d_cubS_ptr, &B->d_cubS_cam, &B->d_ce_slot, &B->d_cub_tile, &B->d_cub_coef,
                             &B->d_slotE_ptr, &B->d_slotE_idx, &B->cam_ce_ptr, &B->cam_ce_idx, &B->cam_oei_ptr, &B->cam_oei_idx, &B->cam_oej_ptr, &B->cam_oej_idx, &B->cub_ce_ptr, &B->cub_ce_idx,
                             &B->d_ce_active, &B->d_oe_active};
  const int nt = (int)(sizeof(tabs) / sizeof(tabs[0]));
  *n_tables = nt;
  std::vector<int> h;
  for (int t = 0; t < nt && t < cap; t++) {
    h.resize(tabs[t]->n);
    if (tabs[t]->n) CS_HIP_TRY(hipMemcpy(h.data(), tabs[t]->p, sizeof(int) * tabs[t]->n, hipMemcpyDeviceToHost));
    // (the last two tables are the sharding's activity words: an edge's level is folded into the device's copy and is no part of the structure)
    if (t >= nt - 2) { const std::vector<int>& sh = t == nt - 2 ? B->h_ce_shard : B->h_oe_shard; std::copy(sh.begin(), sh.begin() + std::min(sh.size(), h.size()), h.begin()); }
    unsigned long long f = 1469598103934665603ull ^ (unsigned long long)tabs[t]->n;
    for (int v : h) { f ^= (unsigned)v; f *= 1099511628211ull; }
    out[t] = f;
  }
  return CS_OK;
  CS_GUARD_END("cs_ba_structure_digest")
}

// The diagonal Hessian blocks g2o keeps mapped into its vertices (BaseVertex::_hessian, core/base_vertex.hpp:30,52-54; mapped by
// BlockSolver::buildStructure, block_solver.hpp:185,191) and that OptimizationAlgorithmLevenberg::computeLambdaInit reads
// (optimization_algorithm_levenberg.cpp:166-180): A_ii of every vertex, caller's vertex order, zeros for fixed vertices.
int cs_ba_get_vertex_hessians(cs_ba* B, double* cam36, double* cub81, double* pt9) {
  if (!B) return CS_ERR_INVALID_ARG;
  if (int rn = need_system(B, "cs_ba_get_vertex_hessians")) return rn;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (cam36 && B->nc) {
    CS_HIP_TRY(hipMemcpy(cam36, B->Hcam.p, 8 * 36 * (size_t)B->nc, hipMemcpyDeviceToHost));
    for (int i = 0; i < B->nc; i++) if (B->cam_fixed[i]) std::memset(cam36 + 36 * (size_t)i, 0, 288);
  }
  if (cub81 && B->no) {
    CS_HIP_TRY(hipMemcpy(cub81, B->Hcub.p, 8 * 81 * (size_t)B->no, hipMemcpyDeviceToHost));
    for (int i = 0; i < B->no; i++) if (B->cub_fixed[i]) std::memset(cub81 + 81 * (size_t)i, 0, 648);
  }
  if (pt9 && B->np) {
    CS_HIP_TRY(hipMemcpy(pt9, B->Hll.p, 8 * 9 * (size_t)B->np, hipMemcpyDeviceToHost));
    for (int i = 0; i < B->np; i++) if (B->pt_fixed[i]) std::memset(pt9 + 9 * (size_t)i, 0, 72);
  }
  return CS_OK;
}


int cs_ba_set_lm_params(cs_ba* B, double user_lambda_init, int max_trials_after_failure) {
  if (!B || !(user_lambda_init == user_lambda_init) || max_trials_after_failure < 1) return CS_ERR_INVALID_ARG;
  B->user_lambda_init = user_lambda_init > 0 ? user_lambda_init : 0.0;
  B->max_trials_after_failure = max_trials_after_failure;
  return CS_OK;
}
int cs_ba_set_stage_timing(cs_ba* B, int on) {
  if (!B) return CS_ERR_INVALID_ARG;
  B->stage_timing = on != 0;
  B->lin_pending = false;
  return CS_OK;
}
int cs_ba_last_timing(cs_ba* B, cs_ba_timing* t) {
  if (!B || !t) return CS_ERR_INVALID_ARG;
  *t = B->tm;
  t->schur_entries = B->schur_entries;
  // algorithmic bytes per linearisation + Schur build: per projection edge 136 B read
  // + 144 B Hpl written, re-read once by the Schur stage; per camera 336 B; per point 96 B written, 96 B read,
  // 72 B Dinv written; per cuboid edge 864 B read + 432 B written.
  t->linearize_bytes = (long long)B->slot_src_n * (136 + 144 + 144) + (long long)B->nc * 336 + (long long)B->np * 264 + (long long)B->n_cub3 * (864 + 432) + (long long)(B->n_cub - B->n_cub3) * (368 + 1400);
  return CS_OK;
}

}  // extern "C"

// ---- debug / repro aids --------------------------------------------------------------------------------------------------------------
// cs_ba_check_finite: the stand-in for the NaN checks of g2o's debug builds (errors: sparse_optimizer.cpp:78-86; Jacobians:
// block_solver.hpp:533-544) -- see ba_scan_finite_kernel.  CS_BA_DEBUG_NAN=1 runs it after every linearisation, solve and update and
// prints what it finds to stderr.
static int check_finite_impl(cs_ba* B, char* report, int report_cap, int* n_bad_out) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = finalize_structure(B); if (rc) return rc;
  const cs::BaView& v = B->view;
  const int E = v.n_proj, n_edges = E + B->n_cub + B->n_odom;
  DBuf<double> chi; DBuf<int> out;
  if ((rc = chi.alloc(std::max(1, n_edges), B->st))) return rc;
  // (level-0 edges only: a level-1 edge is outside the active set and may well be non-finite)
  DBuf<unsigned char> lce, loe;
  { const std::vector<unsigned char> l = combined_cuboid(B, &cs::EdgeClassHost::lvl); if (any_level(l) && (rc = lce.upload(l))) return rc; }
  if (any_level(B->pose_class(CS_EDGE_ODOM).lvl)) { std::vector<unsigned char> l(B->pose_class(CS_EDGE_ODOM).lvl); l.resize((size_t)B->n_odom, 0); if ((rc = loe.upload(l))) return rc; }
  cs::ba_launch_edge_chi(v, chi.p, B->st, lce.p, loe.p);
  struct Arr { const char* name; const double* p; long long n; int per; const char* owner; };
  std::vector<Arr> arrs = {
    {"squared error of a projection edge", chi.p, E, 1, "projection edge (caller's index)"},
    {"squared error of a camera-cuboid edge", chi.p + E, B->n_cub, 1, "camera-cuboid edge (EdgeSE3Cuboid list, then EdgeSE3CuboidProj list)"},
    {"squared error of an odometry edge", chi.p + E + B->n_cub, B->n_odom, 1, "odometry edge"},
    {"camera estimates", v.cams, 7LL * B->nc, 7, "camera"}, {"cuboid estimates", v.cubes, 10LL * B->no, 10, "cuboid"}, {"point estimates", v.points, 3LL * B->np, 3, "point"},
  };
  if (B->have_system) {
    const Arr sys[] = {
      {"A_ii of a camera", v.Hcam, 36LL * B->nc, 36, "camera"}, {"b_i of a camera", v.bcam, 6LL * B->nc, 6, "camera"},
      {"A_ii of a cuboid", v.Hcub, 81LL * B->no, 81, "cuboid"}, {"b_i of a cuboid", v.bcub, 9LL * B->no, 9, "cuboid"},
      {"A_jj of a point", v.Hll, 9LL * B->np, 9, "point"}, {"b_j of a point", v.bl, 3LL * B->np, 3, "point"},
      {"H_pl block of a projection edge (J_cam^T Omega J_point)", v.W, 18LL * E, 18, "projection edge (caller's index)"},
      {"J^T Omega J block of a camera-cuboid edge", v.ce_Hco, 54LL * B->n_cub, 54, "camera-cuboid edge"},
      {"J^T Omega J block of an odometry edge", v.oe_Hij, 36LL * B->n_odom, 36, "odometry edge"},
    };
    arrs.insert(arrs.end(), std::begin(sys), std::end(sys));
  }
  if (B->have_system && B->tm.n_solves > 0) {      // (an increment belongs to the system it solved)
    arrs.push_back({"pose increment x_p (solver order)", v.rhs, B->n_pose, 1, "column"});
    arrs.push_back({"landmark increment", v.xl, 3LL * B->np, 3, "point"});
  }
  std::vector<int> h(2 * arrs.size());
  for (size_t t = 0; t < arrs.size(); t++) { h[2 * t] = 0; h[2 * t + 1] = 0x7fffffff; }
  if ((rc = out.upload(h))) return rc;
  for (size_t t = 0; t < arrs.size(); t++) cs::ba_launch_scan_finite(arrs[t].p, arrs[t].n, out.p + 2 * t, B->st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipMemcpyAsync(h.data(), out.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  long long total = 0;
  std::string rep;
  for (size_t t = 0; t < arrs.size(); t++) {
    if (!h[2 * t]) continue;
    total += h[2 * t];
    long long owner = (h[2 * t + 1] - 1) / arrs[t].per;
    if (arrs[t].per == 18 || (arrs[t].per == 1 && t == 0)) {      // projection edges: point-major slot -> the caller's edge index
      owner = (owner >= 0 && owner < B->slot_src_n) ? B->slot_src[(size_t)owner] : -1;
    }
    rep += std::string(arrs[t].name) + ": " + std::to_string(h[2 * t]) + " non-finite value(s), first in " + arrs[t].owner + " " + std::to_string(owner) + "\n";
  }
  if (report && report_cap > 0) { const size_t n = std::min(rep.size(), (size_t)report_cap - 1); std::memcpy(report, rep.data(), n); report[n] = 0; }
  if (n_bad_out) *n_bad_out = (int)std::min<long long>(total, 0x7fffffff);
  return CS_OK;
}
int cs_ba_check_finite(cs_ba* B, int* n_bad, char* report, int report_cap) {
  CS_GUARD_BEGIN
  return check_finite_impl(B, report, report_cap, n_bad);
  CS_GUARD_END("cs_ba_check_finite")
}
bool debug_nan_enabled() { static const bool on = [] { const char* e = getenv("CS_BA_DEBUG_NAN"); return e && atoi(e) != 0; }(); return on; }
void debug_nan_scan(cs_ba* B, const char* where) {
  if (!debug_nan_enabled()) return;
  char rep[2048]; int n = 0;
  if (check_finite_impl(B, rep, (int)sizeof(rep), &n) == CS_OK && n > 0) fprintf(stderr, "[cs_ba CS_BA_DEBUG_NAN] %s:\n%s", where, rep);
}

// cs_ba_dump / cs_ba_load: the whole problem description (current estimates included) as one flat binary file, so that a failing field
// case becomes a fixture -- the stand-in for OptimizableGraph::save / load (core/optimizable_graph.h:594-606), which the reference's own
// graph cannot use (its vendored g2o registers none of its types with the Factory).  Layout: magic "CSBA0002", 16 int32 counts / flags,
// then the arrays in the order written below, each raw little-endian.  Shard settings and external edges are not part of it.
namespace {
struct DumpHeader { char magic[8]; int v[16]; };
constexpr int kDumpPoseCounts = 7, kDumpStereoCounts = 13;      // v[7 + 2 i], v[8 + 2 i]: edges and kernels of pose-edge class i (cs_ba::ec); v[13 .. 15]: the stereo class
struct LevelTrailer { char magic[8]; int rk_off; int n[5]; };      // optional, behind the arrays: levels of CS_EDGE_PROJ, _PROJ_STEREO, _CUBOID, _CUBOID_PROJ, _ODOM (n[i] = 0: all at level 0)
template <class T> bool wr(FILE* f, const std::vector<T>& a) { return a.empty() || fwrite(a.data(), sizeof(T), a.size(), f) == a.size(); }
template <class T> bool rd(FILE* f, std::vector<T>& a, size_t n) { a.resize(n); return n == 0 || fread(a.data(), sizeof(T), n, f) == n; }
}  // namespace
int cs_ba_dump(cs_ba* B, const char* path) {
  CS_GUARD_BEGIN
  if (!B || !path) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  { const int rl = refresh_levels_host(B); if (rl) return rl; }
  const int nst = B->n_stereo, np_e = B->n_proj - nst;
  std::vector<double> cams(7 * (size_t)B->nc), cubs(10 * (size_t)B->no), pts(3 * (size_t)B->np), uv(2 * (size_t)np_e), info(4 * (size_t)np_e), intr(4 * (size_t)np_e), hub(B->have_huber ? np_e : 0);
  auto d2h = [&](std::vector<double>& h, const double* d) -> int { if (!h.empty()) CS_HIP_TRY(hipMemcpy(h.data(), d, 8 * h.size(), hipMemcpyDeviceToHost)); return CS_OK; };
  int rc;
  if ((rc = d2h(cams, B->cams.p)) || (rc = d2h(cubs, B->cubes.p)) || (rc = d2h(pts, B->points.p)) || (rc = d2h(uv, B->raw_uv.p)) || (rc = d2h(hub, B->raw_huber.p))) return rc;
  // (records that were never stored -- every edge carries the reference record -- are written out here)
  if (B->raw_info_virtual) { for (int k = 0; k < np_e; k++) std::memcpy(&info[4 * (size_t)k], B->uni8, 32); } else if ((rc = d2h(info, B->raw_info.p))) return rc;
  if (B->raw_intr_virtual) { for (int k = 0; k < np_e; k++) std::memcpy(&intr[4 * (size_t)k], B->uni8 + 4, 32); } else if ((rc = d2h(intr, B->raw_intr.p))) return rc;
  FILE* f = fopen(path, "wb");
  if (!f) { cs_set_error(std::string("cs_ba_dump: cannot open ") + path); return CS_ERR_INVALID_ARG; }
  DumpHeader H{};
  std::memcpy(H.magic, "CSBA0002", 8);
  const int head[7] = {B->nc, B->no, B->np, B->cuboids_first, np_e, B->have_huber ? 1 : 0, (int)B->rk_proj.size()}, tail[3] = {nst, B->h_se_huber.empty() ? 0 : 1, (int)B->rk_stereo.size()};
  std::memcpy(H.v, head, sizeof(head)); std::memcpy(H.v + kDumpStereoCounts, tail, sizeof(tail));
  for (int i = 0; i < 3; i++) { H.v[kDumpPoseCounts + 2 * i] = B->ec[i].size(); H.v[kDumpPoseCounts + 2 * i + 1] = (int)B->ec[i].rk.size(); }
  bool ok = fwrite(&H, sizeof(H), 1, f) == 1;
  ok = ok && wr(f, cams) && wr(f, B->cam_fixed) && wr(f, cubs) && wr(f, B->cub_fixed) && wr(f, pts) && wr(f, B->pt_fixed);
  const std::vector<int> m_pt(B->e_pt.begin(), B->e_pt.begin() + np_e), m_cam(B->e_cam.begin(), B->e_cam.begin() + np_e), s_pt(B->e_pt.begin() + np_e, B->e_pt.end()), s_cam(B->e_cam.begin() + np_e, B->e_cam.end());
  ok = ok && wr(f, m_pt) && wr(f, m_cam) && wr(f, uv) && wr(f, info) && wr(f, intr) && wr(f, hub) && wr(f, B->rk_proj);
  for (const cs::EdgeClassHost& c : B->ec) ok = ok && wr(f, c.a) && wr(f, c.b) && wr(f, c.meas) && wr(f, c.info) && wr(f, c.extra) && wr(f, c.rk) && wr(f, c.rd);
  // (the stereo projection edges last: a graph without one dumps the bytes it always did)
  ok = ok && wr(f, s_pt) && wr(f, s_cam) && wr(f, B->h_se_uv) && wr(f, B->h_se_ur) && wr(f, B->h_se_intr) && wr(f, B->h_se_sinfo) && wr(f, B->h_se_huber) && wr(f, B->rk_stereo);
  // (edge levels and kernel switches behind everything else, and only when there is one: a handle without them dumps the bytes it always did)
  if (B->rk_off != 0 || any_class_level(B)) {
    LevelTrailer T{};
    std::memcpy(T.magic, "CSLV0001", 8);
    T.rk_off = B->rk_off;
    std::vector<unsigned char> lv[5];
    for (int i = 0; i < 5; i++) {
      const EdgeClassRef c = edge_class_ref(B, kEdgeClasses[i]);
      if (any_level(*c.levels)) { lv[i] = *c.levels; lv[i].resize((size_t)c.count, 0); }
      T.n[i] = (int)lv[i].size();
    }
    ok = ok && fwrite(&T, sizeof(T), 1, f) == 1;
    for (int i = 0; i < 5; i++) ok = ok && wr(f, lv[i]);
  }
  ok = (fclose(f) == 0) && ok;
  if (!ok) { cs_set_error(std::string("cs_ba_dump: write to ") + path + " failed"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
  CS_GUARD_END("cs_ba_dump")
}
int cs_ba_load(const char* path, int device, cs_ba** out) {
  CS_GUARD_BEGIN
  if (!path || !out) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) { cs_set_error(std::string("cs_ba_load: cannot open ") + path); return CS_ERR_INVALID_ARG; }
  struct Close { FILE* f; ~Close() { fclose(f); } } cl{f};
  DumpHeader H;
  if (fread(&H, sizeof(H), 1, f) != 1 || std::memcmp(H.magic, "CSBA0002", 8) != 0) { cs_set_error("cs_ba_load: not a cs_ba dump (magic CSBA0002)"); return CS_ERR_INVALID_ARG; }
  for (int i = 0; i < 16; i++) if (H.v[i] < 0) { cs_set_error("cs_ba_load: corrupt header"); return CS_ERR_INVALID_ARG; }
  const int nc = H.v[0], no = H.v[1], np = H.v[2], cf = H.v[3], npe = H.v[4], hh = H.v[5], nrk = H.v[6], nst = H.v[13], sth = H.v[14], nrks = H.v[15];
  std::vector<double> cams, cubs, pts, uv, info, intr, hub;
  std::vector<int> camf, cubf, ptf, ept, ecam, rkp;
  cs::EdgeClassHost pe[3] = {{cs::kPoseEdgeDims[0]}, {cs::kPoseEdgeDims[1]}, {cs::kPoseEdgeDims[2]}};      // the pose-edge classes as the file has them
  bool ok = rd(f, cams, 7 * (size_t)nc) && rd(f, camf, nc) && rd(f, cubs, 10 * (size_t)no) && rd(f, cubf, no) && rd(f, pts, 3 * (size_t)np) && rd(f, ptf, np);
  ok = ok && rd(f, ept, npe) && rd(f, ecam, npe) && rd(f, uv, 2 * (size_t)npe) && rd(f, info, 4 * (size_t)npe) && rd(f, intr, 4 * (size_t)npe) && rd(f, hub, hh ? npe : 0) && rd(f, rkp, nrk);
  for (int i = 0; i < 3; i++) {
    cs::EdgeClassHost& c = pe[i];
    const size_t n = (size_t)H.v[kDumpPoseCounts + 2 * i], nk = (size_t)H.v[kDumpPoseCounts + 2 * i + 1];
    ok = ok && rd(f, c.a, n) && rd(f, c.b, n) && rd(f, c.meas, c.d.meas * n) && rd(f, c.info, c.d.info * n) && rd(f, c.extra, c.d.extra * n) && rd(f, c.rk, nk) && rd(f, c.rd, nk) && (nk == 0 || nk == n);
  }
  std::vector<int> spt, scam, rks; std::vector<double> suv, sur, sintr, ssinfo, shub;
  ok = ok && rd(f, spt, nst) && rd(f, scam, nst) && rd(f, suv, 2 * (size_t)nst) && rd(f, sur, nst) && rd(f, sintr, 4 * (size_t)nst) && rd(f, ssinfo, 10 * (size_t)nst) && rd(f, shub, sth ? nst : 0) && rd(f, rks, nrks);
  LevelTrailer LT{};
  std::vector<unsigned char> lv[5];
  bool have_levels = false;
  if (ok && fread(&LT, sizeof(LT), 1, f) == 1) {
    have_levels = true;
    const int cnt5[5] = {npe, nst, H.v[kDumpPoseCounts], H.v[kDumpPoseCounts + 2], H.v[kDumpPoseCounts + 4]};
    ok = std::memcmp(LT.magic, "CSLV0001", 8) == 0;
    for (int i = 0; i < 5 && ok; i++) ok = (LT.n[i] == 0 || LT.n[i] == cnt5[i]) && rd(f, lv[i], (size_t)LT.n[i]);
  }
  if (!ok || (nrks && nrks != nst) || (nrk && nrk != npe)) { cs_set_error("cs_ba_load: truncated or inconsistent file"); return CS_ERR_INVALID_ARG; }
  cs_ba* B = nullptr;
  int rc = cs_ba_create(device, &B); if (rc) return rc;
  cs::Guard<cs_ba> g(B, cs_ba_destroy);
  if ((rc = cs_ba_set_vertices(B, cams.data(), camf.data(), nc, cubs.data(), cubf.data(), no, pts.data(), ptf.data(), np, cf))) return rc;
  // (the setters normalise quaternions; the dumped ones are normalised already and must come back with their exact bits)
  if (nc) CS_HIP_TRY(hipMemcpy(B->cams.p, cams.data(), 56 * (size_t)nc, hipMemcpyHostToDevice));
  if (npe && (rc = cs_ba_set_edges_proj(B, npe, ept.data(), ecam.data(), uv.data(), info.data(), intr.data(), hh ? hub.data() : nullptr))) return rc;
  if (nrk && (rc = cs_ba_set_robust_kernels(B, CS_EDGE_PROJ, npe, rkp.data(), hub.data()))) return rc;
  if (nst) {
    std::vector<double> uvr(3 * (size_t)nst), i9(9 * (size_t)nst), k5(5 * (size_t)nst);
    for (int k = 0; k < nst; k++) {
      uvr[3 * (size_t)k] = suv[2 * (size_t)k]; uvr[3 * (size_t)k + 1] = suv[2 * (size_t)k + 1]; uvr[3 * (size_t)k + 2] = sur[k];
      std::memcpy(&i9[9 * (size_t)k], &ssinfo[10 * (size_t)k], 72); std::memcpy(&k5[5 * (size_t)k], &sintr[4 * (size_t)k], 32); k5[5 * (size_t)k + 4] = ssinfo[10 * (size_t)k + 9];
    }
    if ((rc = cs_ba_set_edges_proj_stereo(B, nst, spt.data(), scam.data(), uvr.data(), i9.data(), k5.data(), sth ? shub.data() : nullptr))) return rc;
    if (nrks && (rc = cs_ba_set_robust_kernels(B, CS_EDGE_PROJ_STEREO, nst, rks.data(), shub.data()))) return rc;
  }
  for (int i = 0; i < 3; i++) {
    const cs::EdgeClassHost& c = pe[i];
    if (c.size() && (rc = pose_edges_add(B, CS_EDGE_CUBOID + i, true, c.size(), c.a.data(), c.b.data(), c.meas.data(), c.info.data(), c.extra.data()))) return rc;
    if (c.size() && c.d.meas_is_pose) B->ec[i].meas = c.meas;      // (the dumped quaternions come back with their exact bits, as the cameras' above)
    if (!c.rk.empty() && (rc = cs_ba_set_robust_kernels(B, CS_EDGE_CUBOID + i, c.size(), c.rk.data(), c.rd.data()))) return rc;
  }
  if (have_levels) {
    for (int i = 0; i < 5; i++) {
      if (LT.n[i] && (rc = cs_ba_set_edge_levels(B, kEdgeClasses[i], LT.n[i], lv[i].data()))) return rc;
      if ((LT.rk_off >> kEdgeClasses[i]) & 1) { if ((rc = cs_ba_set_kernels_enabled(B, kEdgeClasses[i], 0))) return rc; }
    }
  }
  *out = g.disarm();
  return CS_OK;
  CS_GUARD_END("cs_ba_load")
}
