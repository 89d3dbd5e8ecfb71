// ba_handle.h -- the bundle-adjustment handle (struct cs_ba; its buffer types are ba_dbuf.h's), the two macros of its host
// code, and the few functions that cross between ba_host.cpp (graph input, structure phase, inspection, dump / load) and ba_lm.cpp (the
// stepwise calls, the damped solve, the LM loop).  Host code only: included by those two files and nothing else.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <mutex>
#include <thread>
#include <map>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "ba_dbuf.h"
#include "ba_edge_class.h"
#include "ba_structure.h"
#include "ba_types.h"
#include "band_solver.h"
#include "cs_hip_util.h"
#include "cs_lm.h"
#include "cs_sparse_solver.h"

// (nothing below is part of the library's ABI: none of it is exported)
#pragma GCC visibility push(hidden)

// a phase mark on the handle's stream -- only while the stage split is asked for (cs_ba_set_stage_timing)
#define BA_MARK(B, e) do { if ((B)->stage_timing) CS_HIP_TRY(hipEventRecord((e), (B)->st)); } while (0)
#define BA_NCCL(expr)                                                          \
  do {                                                                         \
    ncclResult_t _r = (expr);                                                  \
    if (_r != ncclSuccess) {                                                   \
      cs_set_error(std::string(#expr) + ": " + ncclGetErrorString(_r));     \
      return CS_ERR_HIP;                                                       \
    }                                                                          \
  } while (0)

using cs::UBuf;    // (host scratch of the structure phase: ba_structure.h)

struct cs_ba {
  // Every device resource below is an owner type that gives itself back, and members die in reverse declaration order.  So: the three
  // streams first -- they die last, after everything that was queued on them -- the BLAS handle behind its stream, then buffers, events and
  // pinned words in any order.  cs_ba_destroy waits for the streams, closes the communicator and deletes: nothing is named there.
  int device = 0;
  cs::Stream st;
  cs::Stream st2;                            // side stream of the reduce phase (cuboid elimination beside the landmark segments)
  cs::Stream st3;                            // third stream of the linearisation: the landmark kernel beside the camera kernel (which fills a fraction of the CUs)
  cs::BlasHandle blas;
  StageArena stage;                          // pinned staging of the structure phase's small uploads
  // the landmarks' camera lists of the last structure phase (host): a graph that is only appended to extends them instead of re-sorting all edges
  int st_lists_edges = 0, st_cur = 0; std::vector<int> st_cam_cnt; UBuf<int> st_cams_of[2], st_edge_of[2];   // (two sets: a phase reads the last one's and fills the other)
  UBuf<int> st_pm_pt, st_pm_cam, st_cm_pm, st_cm_pt;   // host scratch of the edge orders, kept for its memory only
  StageArena append_stage;                   // ... and of cs_ba_append_*'s rows (queued on st, rewound by the structure phase)
  cs::Event ev_fork, ev_join, ev_join3;      // the side streams' fork and their two joins
  cs::Event ev[8];   // phase marks on the stream (linearise: 0-1; solve: 2 reduce 3 factor 4 back-substitution 5)
  cs::Event sev[4];  // separator mode, inside [3, 4]: interior factorised, separator message formed, messages gathered, separator system solved
  double sep_ms[5] = {0, 0, 0, 0, 0};   // accumulated: interior factorisation, message (Y, T, t), gather, separator solve, interior back-substitution
  bool lin_pending = false;  // ev[0..1] recorded but not yet read
  cs::PinBuf<int> h_status;  // pinned: [status of the (interior's) factorisation, a cuboid block failed, status of the separator system's factorisation -- sparse: [2], [3] are the solver's two words]
  // sharded BA over RCCL (cs_ba_comm_init): the collectives are issued from here, on this handle's stream
  ncclComm_t comm = nullptr;
  DBuf<double> d_scalars;    // [chi2, LM scale term] of a trial; lambda_0's diagonal on iteration 0
  // lambda of the current trial lives in device memory (d_lam: [lambda, lambda of the pose diagonals in LM's scale term]), copied from
  // the pinned h_lam at the head of a trial's launch sequence: the sequence itself never changes
  cs::PinBuf<double> h_lam;
  DBuf<double> d_lam;
  cs::PinBuf<double> h_scalars;  // pinned mirror
  // the trial's [chi2, scale term, failure flag, sequence number], written by the trial's last kernel itself (ba_sum2_flag_kernel) and polled by
  // cs_ba_optimize: pinned, device-visible
  cs::PinBuf<double> h_trial;
  double trial_seq = 0.0;
  // G2OBatchStatistics-like stage split (core/batch_stats.h:48-62): like g2o's setComputeBatchStatistics it is OFF unless asked for
  // (cs_ba_set_stage_timing) -- every phase mark is an event on the stream, ~6 us of dispatch gap each, eight per LM trial
  bool stage_timing = false;
  // OptimizationAlgorithmLevenberg's two properties (optimization_algorithm_levenberg.cpp:50-51, setters :191-199): cs_ba_set_lm_params
  double user_lambda_init = 0.0;      // "initialLambda": > 0 replaces tau * max |H_jj| (computeLambdaInit :168-169)
  int max_trials_after_failure = 10;  // "maxTrialsAfterFailure": trials of one iteration (:149-151)
  cs::Event ev_upd;                // recorded behind a trial's update kernel when the next linearisation is speculated: its side streams fork there
  // host copy of the problem description
  int nc = 0, no = 0, np = 0, cuboids_first = 0;
  std::vector<int> cam_fixed, cub_fixed, pt_fixed, cam_col, cub_col, pt_lm;  // pt_lm: landmark index among free points or -1
  std::vector<int> cam_col_ref, cub_col_ref;  // columns in g2o's sort-by-id order (inspection only); cam_col / cub_col are in solver (RCM) order
  int band_ld = 0;                            // 0 = dense reduced system
  bool use_bcr = false;
  int force_dense = 0;
  // sharded BA: landmarks (with all their projection edges) are dealt to ranks by the camera subsequence of their
  // first observation; cuboid / odometry edges follow their camera.  Every rank keeps all vertices.
  int shard_rank = 0, shard_n = 1;
  // Separator mode of the sharded solve (shard_n > 1, banded system, every rank's interior wide enough): rank r owns the columns
  // [cut[r], cut[r + 1]) of the band -- its first sepw[r] >= bandwidth columns are the separator Z_r (sepw[0] = 0), the rest its interior
  // -- and everything whose lowest column falls into that range (landmarks with their projection edges, cuboids, odometry edges).
  // What a rank builds then lies in its own columns and in the diagonal block of the next separator; it factorises its interior only,
  // the ranks exchange the separators' Schur complements (3 w^2 + 2 w doubles each) and the interiors' solutions.  Otherwise
  // (sep_mode == false) the whole [S | b] is summed over the ranks and every rank factorises it.
  bool sep_mode = false;
  std::vector<int> cut, sepw, sep_off, lm_owner;   // sep_off[k]: row of separator k in the separator system (k = 1 .. R - 1; sep_off[R] = n_sep)
  int n_sep = 0, w_max = 0;
  size_t msg_doubles = 0;                          // one rank's message: [LL | RL | RR | tL | tR]
  int int_c = 0, int_n = 0, zl = 0, wl = 0, zr = 0, wr = 0;   // this rank's interior and its two separators
  DBuf<double> sepY, sep_msgs, sepS, int_work, sep_work;
  DBuf<int> d_sep_off, d_sep_col, d_int_info, d_sep_info;
  long long bytes_per_trial = 0, bytes_per_trial_allreduce = 0;   // payload this rank contributes to the collectives of one LM trial; what the all-reduce of [S | b] would be
  size_t s_doubles = 0;                       // size of S; rhs follows it in the same allocation (one all-reduce)
  int n_pose = 0, n_lm = 0;
  int n_red = 0;            // dimension of the system the solver factorises: n_pose, or the cameras' part when the cuboids are eliminated too
  bool elim = false;        // free cuboids eliminated like landmarks (single rank, fused Schur schedule)
  int elim_max_slots = 1;   // observing cameras of the widest free cuboid
  // general sparse Cholesky of the reduced system (cs_sparse_solver.h): graphs the ordering cannot band
  bool sparse = false;         // this structure's solves go through `solver` (its plan was built, accepted and uploaded)
  bool S_clean = false;        // sparse: S holds nothing outside the plan's pattern (set by the first trial's full clear)
  cs::SparseSolver solver;
  DBuf<int> d_cub_mine;     // sharded + eliminated cuboids: 1 = this rank owns the cuboid (holds all its edges)
  DBuf<int> d_cubS_ptr, d_cubS_cam, d_ce_slot, d_cub_tile, d_cub_coef, d_elim_fail, d_slotE_ptr, d_slotE_idx;
  DBuf<double> cub_M, cub_Dinv;
  // The three pose-edge classes as the caller gave them (ba_edge_class.h): endpoints, payload, kernels and levels of EdgeSE3Cuboid,
  // EdgeSE3CuboidProj and EdgeSE3Expmap, kept until the structure phase puts them on the device.
  cs::EdgeClassHost ec[3] = {{cs::kPoseEdgeDims[0]}, {cs::kPoseEdgeDims[1]}, {cs::kPoseEdgeDims[2]}};
  cs::EdgeClassHost& pose_class(int edge_class) { return ec[edge_class - CS_EDGE_CUBOID]; }
  const cs::EdgeClassHost& pose_class(int edge_class) const { return ec[edge_class - CS_EDGE_CUBOID]; }
  int n_proj = 0, n_cub = 0, n_odom = 0;   // n_cub = EdgeSE3Cuboid + EdgeSE3CuboidProj edges (the combined list ce_cam / ce_cub); n_cub, n_cub3 and n_odom are written by finalize_structure only
  int n_cub3 = 0;                          // of which EdgeSE3Cuboid (they come first)
  DBuf<double> pe_meas, pe_info, pe_K;
  std::vector<int> e_pt, e_cam;      // projection edges, caller order: the mono edges [0, n_proj - n_stereo), the stereo edges behind them (g2o's edge order)
  // stereo projection edges (EdgeStereoSE3ProjectXYZ; cs_ba_set_edges_proj_stereo): counted in n_proj, their payload in the caller's order on the
  // host until the structure phase puts it beside the mono edges' in the two edge orders
  int n_stereo = 0;
  std::vector<double> h_se_uv, h_se_ur, h_se_intr, h_se_sinfo, h_se_huber;   // 2, 1, 4 (fx fy cx cy), 10 (information 3 x 3, bf), 1 (empty: no kernel) per edge
  std::vector<int> rk_stereo;                                                // kernel kinds (cs_ba_set_robust_kernels), empty: Huber from the deltas
  bool intr_uniform_all = false, sinfo_uniform = false;                      // decided by the structure phase: BaView::intr_u over both classes, sinfo_u
  DBuf<double> comb_uv, comb_info, comb_intr, comb_huber;                    // a stereo graph's rows of both classes in e_pt's order (the gathers' source)
  DBuf<double> d_pm_ur, d_cm_ur, d_pm_sinfo, d_cm_sinfo;
  DBuf<int> d_pm_kind, d_cm_kind;
  DBuf<int> d_src;                   // device copy of slot_src (the gathers of the structure phase)
  std::unique_ptr<int[]> slot_src;   // point-major slot -> caller edge (uninitialised storage with head room: kept across structure phases)
  size_t slot_src_cap = 0; int slot_src_n = 0;
  std::vector<int> ce_cam, ce_cub;
  bool structure_dirty = true;
  // device buffers
  DBuf<double> cams, points, cubes, cams_bak, points_bak, cubes_bak;
  DBuf<int> d_cam_col, d_cub_col, d_pt_free;
  DBuf<int> pm_pt, pm_cam, pt_ptr, cm_pm, cm_pt, cam_ptr;
  DBuf<double> pm_uv, pm_info, pm_intr, pm_huber, cm_uv, cm_info, cm_intr, cm_huber;
  DBuf<int> d_ce_cam, d_ce_cub, d_oe_i, d_oe_j, d_ce_active, d_oe_active;
  DBuf<double> ce_meas, ce_info, ce_Hcc, ce_Hoo, ce_Hco, ce_bc, ce_bo, oe_meas, oe_info, oe_Hii, oe_Hjj, oe_Hij, oe_bi, oe_bj;
  DBuf<int> cam_ce_ptr, cam_ce_idx, cam_oei_ptr, cam_oei_idx, cam_oej_ptr, cam_oej_idx, cub_ce_ptr, cub_ce_idx;
  DBuf<double> Hcam, bcam, Hcub, bcub, Hll, bl, W, WD, Dinv, dbl, S, rhs, xl, chi_partial, band_linv, scale_partial;
  DBuf<int> pair_ptr, pair_i1, pair_i2, ent_a, ent_b;
  // fused Schur schedule (BaView::fused)
  bool fused = false;
  int n_seg = 0, n_gpairs = 0, seg_class[5] = {0, 0, 0, 0, 0};
  DBuf<int> d_run_lm, d_seg_ptr, d_seg_k, d_seg_tile, d_seg_slot, d_gp_ptr, d_gp_i1, d_gp_i2, d_gtile, d_gcam_ptr, d_gslot;
  DBuf<int> d_run_e0, d_seg_cam;     // round 6: a run entry's first point-major edge (= pt_ptr[run_lm]) and a segment slot's camera (= pm_cam of the segment's first landmark): two dependent loads less at the head of ba_lin_schur_kernel
  DBuf<double> part_tiles, part_coef;
  DBuf<rocblas_int> d_info;
  DBuf<int> d_band_info;
  int n_pairs = 0, nb_chi = 1, n_chi_partials = 1;
  long long schur_entries = 0;
  // the projection edges' payload (88 bytes per edge) goes straight to the device when the edges are set, in the caller's order;
  // the structure phase permutes it there (ba_gather_rows_kernel)
  DBuf<double> raw_uv, raw_info, raw_intr, raw_huber;
  // every projection edge with the same information matrix / intrinsics (decided by comparing the caller's records when they are set or
  // appended): the kernels then read these 4 + 4 doubles instead of the per-edge records (BaView::info_u / intr_u).  CS_BA_UNIFORM=0: never.
  bool info_uniform = false, intr_uniform = false;
  // the per-edge records are not stored while every edge carries the handle's reference record (uni8): 64 bytes per edge that no kernel would
  // read -- a third of a C4 problem's upload; they are written out from the reference record the moment an appended edge brings another one
  bool raw_info_virtual = false, raw_intr_virtual = false;
  double uni8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  DBuf<double> d_uni;
  bool have_huber = false;
  // robust kernels (cs_ba_set_robust_kernels; cs_robust.h): kinds per edge in the caller's order, empty = none of the class has one.
  // The projection edges' deltas live in raw_huber (Huber is the fast path: kinds all 0 / 1 -> no kind array on the device).
  std::vector<int> rk_proj;
  DBuf<int> d_pm_rk, d_cm_rk, d_ce_rk, d_oe_rk;
  DBuf<double> d_ce_rdelta, d_oe_rdelta;
  int rk_off = 0;                    // cs_ba_set_kernels_enabled: bit (1 << cs_edge_class) set = the class's kernels are switched off (BaView::rk_off)
  // Edge levels (OptimizableGraph::Edge::setLevel; cs_ba_set_edge_levels / cs_ba_classify_edges).  The master copy per class, in the caller's edge
  // order; empty = every edge of the class at level 0.  On the device a projection edge's level is the sign of its width record in both edge orders
  // (ba_kernels.hip: edge_off) plus d_lvl, one byte per edge in e_pt's order (mono edges, then stereo), which exists only once a level may be 1; a
  // cuboid / odometry edge's level is folded into d_ce_active / d_oe_active (h_ce_shard / h_oe_shard keep the sharding's own words).
  // lvl_host_stale: cs_ba_classify_edges wrote d_lvl on the device and the host vectors have not been refreshed from it yet.
  std::vector<unsigned char> lvl_mono, lvl_stereo;      // (the pose classes' levels: ec[].lvl)
  DBuf<unsigned char> d_lvl;
  bool lvl_on_device = false, lvl_host_stale = false;
  int lvl_nM = 0, lvl_nS = 0;        // d_lvl's layout: the class counts of the structure phase that filled it
  std::vector<int> h_ce_shard, h_oe_shard;
  DBuf<int> d_pm_cm, d_cls_counts;   // point-major -> camera-major slot (the inverse of cm_pm, built for the first classification of a structure); [mono, stereo] outlier counters
  bool pm_cm_valid = false;
  DBuf<double> d_cls_chi;            // the classification's per-edge plain chi2, when the caller asks for it
  // external (host-evaluated) edges: the coupling pattern of the binary ones (structure), the terms of the current linearisation
  int ext_n = 0;
  std::vector<int> ext_e4;                       // (class_i, idx_i, class_j, idx_j) per edge; idx_j < 0: unary
  DBuf<int> d_ext_e4, d_ext_order, d_ext_gptr;   // (+ the binary ones grouped by destination pair: ba_ext_offdiag_kernel)
  int ext_groups = 0;
  DBuf<double> ext_cam36, ext_cam6, ext_cub81, ext_cub9, ext_pt9, ext_pt3, ext_Hij;
  std::vector<double> h_ext_Hij;                 // host copy (cs_ba_get_system's dense H_pp)
  bool ext_has_cam = false, ext_has_cub = false, ext_has_pt = false, ext_terms_set = false;
  double ext_chi2 = 0;
  cs_external_fn ext_fn = nullptr; void* ext_ctx = nullptr;
  // last solution / rhs on the host (for LM's scale term and for inspection)
  std::vector<double> h_b, h_x;
  // The linear system in device memory is ONE linearisation of the current graph: set by build_system_device, cleared by the structure phase, by new
  // estimates or external terms, and by every optimize call that ran an iteration (what that leaves behind is blocks of up to three states: H_pl of
  // its first iteration, pose blocks of the speculated linearisation, landmark blocks of the trial before).
  bool have_system = false;
  // cams_bak / points_bak / cubes_bak hold what cs_ba_push saved (one level).  Dead after the structure phase, cs_ba_set_estimates, an optimize call
  // that ran an iteration (its update kernel saves every trial's estimates there) and after cs_ba_pop has restored it.
  bool backup_live = false;
  cs_ba_timing tm{};
  cs::BaView view{};
};

// ---- across the two files
// ba_host.cpp: the structure phase (a no-op on a clean handle); CS_BA_DEBUG_NAN's scan of estimates, errors and blocks after a step
int finalize_structure(cs_ba* B);
void debug_nan_scan(cs_ba* B, const char* where);
bool debug_nan_enabled();
// ba_lm.cpp: the guard of every call that reads the linear system (see cs_ba::have_system); lambda of a damped reduce into the pinned word and,
// queued on the stream, into device memory; cs_ba_optimize_sharded behind its exception guard (cs_ba_optimize_rounds runs it per round)
int need_system(cs_ba* B, const char* who);
int put_lambda(cs_ba* B, double lambda);
int cs_ba_optimize_sharded_impl(cs_ba* B, int iterations, cs_allreduce_fn fn, void* ctx, int* iterations_done, double* chi_hist, double* lambda_hist, int* trials_hist, int cap);

#pragma GCC visibility pop
