// detect_host.cpp -- host side of path A (detect_cuboid) behind the C ABI of include/cubeslam_hip.h.
//
// Stages of one cs_batch_run() (production path: pipe_launch / pipe_finish):
//   setup   (host, threaded)  per frame: camera cache (box_proposal_detail.cpp:45-56); per box and height sample: integer
//                             box/ROI geometry (:143-256), yaw / top-edge / roll-pitch sample lists (:180-184, :212-219,
//                             :344-355)  ->  JobDesc + pooled SoA arrays in pinned memory, one H2D copy;
//   sweep   (HIP)             line setup (ROI filter + merge_break_lines) and VP support, vanishing points + corner
//                             construction + ordered compaction, the crowded ROIs' line setup; the scorer joins them
//                             (detect_kernels.hip, line_setup_kernels.hip).  On three streams of the process's stream set with eight hardware
//                             queues or more, on one stream per detector with fewer (StreamSet below);
//   rank    (HIP)             fuse_normalize_scores_v2 (object_3d_util.cpp:726-837) and the final skew-weighted ranking
//                             (box_proposal_detail.cpp:766-838) on the compacted (dist, angle, skew) columns; only the
//                             winners come back;
//   finish  (host, threaded)  cs_cuboid records of the winners (:740-798, object_3d_util.cpp:941-1011); the few boxes whose
//                             ties could reach the output are fetched and ranked with the exact std::partial_sort.
// The same stages exist as a general round-based path (debug getters, host ranking / host line setup on request).
// What the paths share is stated once: the rules in front of the kernels in detect_jobs_host.h, those behind them in detect_rank_host.h
// (the exact ranking, the host's corner rebuild, the record writers over the caller's output: OutView, write_exact_winners,
// write_device_records), the camera cache in detect_cam_host.h, the device tables and the view over them in SweepBuffers, the tie boxes'
// pass in TiePass, the launch / collect protocol of a lean path's slot in PipeSlot (begin, mark_in_flight, wait).  The worker pool of the
// host stages is cs_worker_pool.h.
// With whether_sample_cam_roll_pitch the reference carries cam_pose.camera_yaw from one box to the next
// (:180 reads what :374/:734 left behind), so boxes of a frame are processed in rounds (round r = box r of
// every frame), each ranked on the device; without it all boxes of all frames go through the sweep in one launch.
//
// There is no CPU fallback for the sweep: without a HIP device cs_detector_create() fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "cs_hip_util.h"
#include "cs_worker_pool.h"
#include "detect_cam_host.h"      // (with detect_jobs_host.h and detect_rank_host.h)
#include "detect_hooks.h"
#include "detect_types.h"
#include "edge_types.h"

thread_local std::string g_cs_err;  // shared by every path (cs_hip_util.h: cs_set_error)
void cs_set_error(const std::string& s) { g_cs_err = s; }

using namespace cs_dh;   // detect_jobs_host.h: the job-table rules; detect_rank_host.h: FrameIn, the slot decode, the exact ranking, the record writers; detect_cam_host.h: the camera cache

namespace {

using cs::DevBuf;
using cs::PinBuf;
using cs::WorkerPool;
using cs::now_ms;

// merge_break_lines (object_3d_util.cpp:431-543) on a row-major n x 4 array.
void merge_lines(std::vector<double>& L, double dist_thre, double angle_thre_deg, double len_thre) {
  int total = (int)(L.size() / 4);
  const double athre = angle_thre_deg / 180.0 * CS_PI;
  // The reference recomputes every segment's angle at the top of each round (:451-456).  Only two rows change per
  // merge (row a is overwritten, row b receives the last row), so the cached angles below are the same doubles.
  std::vector<double> ang(total);
  for (int i = 0; i < total; i++) ang[i] = cs::cs_atan2(L[4 * i + 3] - L[4 * i + 1], L[4 * i + 2] - L[4 * i]);
  bool merged = true;
  int rounds = 0;
  while (merged && rounds < 500) {
    rounds++;
    merged = false;
    for (int a = 0; a < total - 1 && !merged; a++) {
      for (int b = a + 1; b < total; b++) {
        double diff = std::abs(ang[a] - ang[b]);
        if (std::min(diff, CS_PI - diff) >= athre) continue;
        double d_ab = cs::v2_dist(cs::v2(L[4 * a + 2], L[4 * a + 3]), cs::v2(L[4 * b], L[4 * b + 1]));
        double d_ba = cs::v2_dist(cs::v2(L[4 * b + 2], L[4 * b + 3]), cs::v2(L[4 * a], L[4 * a + 1]));
        if (!((d_ab < dist_thre) || (d_ba < dist_thre))) continue;
        const double* s = (L[4 * a] < L[4 * b]) ? &L[4 * a] : &L[4 * b];
        const double* e = (L[4 * a + 2] > L[4 * b + 2]) ? &L[4 * a + 2] : &L[4 * b + 2];
        double sx = s[0], sy = s[1], ex = e[0], ey = e[1];
        double ma = cs::cs_atan2(ey - sy, ex - sx);
        double t = std::abs(ang[a] - ma);
        if (std::min(t, CS_PI - t) < athre) {
          L[4 * a] = sx; L[4 * a + 1] = sy; L[4 * a + 2] = ex; L[4 * a + 3] = ey;
          for (int c = 0; c < 4; c++) L[4 * b + c] = L[4 * (total - 1) + c];  // swap-remove (matrix_utils.cpp:183)
          ang[a] = ma;               // atan2 of the merged row == merged_angle (:490)
          ang[b] = ang[total - 1];
          total--;
          merged = true;
          break;
        }
      }
    }
  }
  if (len_thre > 0) {
    int k = 0;
    for (int i = 0; i < total; i++) {
      double len = cs::v2_dist(cs::v2(L[4 * i + 2], L[4 * i + 3]), cs::v2(L[4 * i], L[4 * i + 1]));
      if (len > len_thre) {
        if (k != i) for (int c = 0; c < 4; c++) L[4 * k + c] = L[4 * i + c];
        k++;
      }
    }
    total = k;
  }
  L.resize(4 * (size_t)total);
}

// ---- the working streams of all detectors of a process on one device ---------------------------------------------------------
// The ROCm runtime multiplexes a process's normal-priority streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless the environment
// says otherwise) and a queue hands its packets out in order.  With six streams of their own per detector, WHICH roles of which detectors
// shared a queue followed from the order the streams were created in (profiles/stream_queue_map_per_detector_streams_4_queues.txt: one
// detector's chain had a queue to itself, the three others' chains shared one).  Now the library owns one set of streams per device,
// sized by the queue count, and a detector borrows the streams of a SLOT of the set (the lowest free one; more detectors than slots
// share slots):
//   fewer than 8 queues   a slot is ONE stream and there are as many slots as queues: a batch's whole sweep -- tables, corner construction,
//                         line setup, VP support, scorer, ranking, records, results -- runs on it in order, beside the other slots' sweeps.
//                         Measured against every split by role that four queues allow: the device is kept busy by
//                         the OTHER pipelines' kernels, and a role stream shared between pipelines makes a ready kernel wait behind one
//                         whose inputs are not there yet.  A detector whose sweep finds the device to ITSELF (the usual integration, a
//                         single-frame call: no other detector's kernels fill its batch's holes) runs the corner construction and the crowded
//                         line setup on two of the idle slots' streams, as a batch alone wants them: decided per enqueue block by whether
//                         another detector has a sweep in flight (sweep_side_streams).
//   8 queues or more      the set holds no streams: every detector has streams of its OWN for the chain, the corner construction and the crowded
//                         line setup, a fourth that runs nothing and a high-priority one, created in that order when the detector is -- with
//                         queues to spare a batch's own roles side by side pay, and this is the form that was measured fastest there.  WHICH
//                         streams then share a queue is the runtime's choice by creation order (the fourth stream is part of that order:
//                         profiles/stream_queue_map_per_detector_streams_8_queues.txt -- four chains on queues of their own, a detector's
//                         corner construction with its neighbour's crowded line setup).  Set-owned slots of three streams that land on the
//                         queues in the same way were 5-9 % slower, so nothing is shared here and no lock is taken.
// With fewer than 8 queues the tie boxes' fetches run on a high-priority stream per slot (the runtime keeps hardware queues per priority class: they take none
// from the sweep, and a host thread that synchronises its slot's stream waits for its own slot's fetches only); an image-input batch's upload
// stream has the lowest priority for the same reason and stays the batch's own.
// Several host threads may enqueue into one stream: HIP's stream calls are thread safe, every call in an enqueue block is asynchronous,
// and an event is waited for only after the call that recorded it has returned -- in the order the runtime saw the calls every operation
// depends on earlier ones only, so no interleaving can deadlock and no detector ever waits for another one's host thread.  ONE lock,
// `enqueue_mu`, is held around a batch's enqueue block (pipe_launch, rp_launch) all the same: the batch's launches then sit back to back
// in a shared stream (no other batch's big kernel between two of its small ones, and the per-stage events of timing() bracket this batch's
// kernels only).  Nothing that waits for the device or for another thread happens under it, no allocation, and no second lock is taken inside.
struct StreamSet {
  enum { MAX_SLOTS = 16 };
  int device = 0, refs = 0, n_queues = 4, n_slots = 0;
  std::atomic<int> busy{0};                        // sweeps queued and not yet collected, all detectors of the device (sweep_side_streams)
  bool own_streams = false;                        // 8 queues or more: the detectors create their streams themselves
  hipStream_t chain[MAX_SLOTS] = {};
  int users[MAX_SLOTS] = {};
  hipStream_t hi[MAX_SLOTS] = {};
  std::mutex enqueue_mu;
};
std::mutex g_sets_mu;
std::vector<StreamSet*> g_sets;      // one per device in use

// What the runtime will use: read, never set.  The runtime latches the variable when HIP initialises; the set reads it when a device's first
// detector is created and ASSUMES that nobody changed it in between (a host that sets it after its first HIP call gets a set sized for a
// queue count the runtime does not have -- more streams than queues, which share queues as the runtime pleases).
int hw_queue_count() {
  const char* e = getenv("GPU_MAX_HW_QUEUES");
  const int n = e ? atoi(e) : 4;
  return n < 1 ? 4 : std::min(n, 32);
}

void stream_set_destroy(StreamSet* s) {
  for (hipStream_t st : s->chain) if (st) (void)hipStreamDestroy(st);
  for (hipStream_t st : s->hi) if (st) (void)hipStreamDestroy(st);
  delete s;
}

// the device's set, created on first use (the caller has made `device` current); nullptr + *err on a HIP error
StreamSet* stream_set_acquire(int device, hipError_t* err) {
  std::lock_guard<std::mutex> lk(g_sets_mu);
  *err = hipSuccess;
  for (StreamSet* s : g_sets) if (s->device == device) { s->refs++; return s; }
  StreamSet* s = new StreamSet();
  s->device = device; s->n_queues = hw_queue_count();
  s->own_streams = s->n_queues >= 8;
  s->n_slots = s->own_streams ? 0 : s->n_queues;
  for (int i = 0; i < s->n_slots && *err == hipSuccess; i++) *err = hipStreamCreateWithFlags(&s->chain[i], hipStreamNonBlocking);
  if (*err == hipSuccess && s->n_slots > 0) {
    int prio_low = 0, prio_high = 0;   // (numerically lowest = greatest priority)
    *err = hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);
    for (int i = 0; i < s->n_slots && *err == hipSuccess; i++) *err = hipStreamCreateWithPriority(&s->hi[i], hipStreamNonBlocking, prio_high);
  }
  if (*err != hipSuccess) { stream_set_destroy(s); return nullptr; }
  s->refs = 1;
  g_sets.push_back(s);
  return s;
}

// a new detector's slot: the one the fewest live detectors hold (the lowest of them); out: chain, corner construction, crowded line setup, tie fetches
// (not with own_streams: -1, nothing borrowed)
int stream_set_borrow(StreamSet* s, hipStream_t out[4]) {
  std::lock_guard<std::mutex> lk(g_sets_mu);
  if (s->own_streams) return -1;
  int i = 0;
  for (int k = 1; k < s->n_slots; k++) if (s->users[k] < s->users[i]) i = k;
  s->users[i]++;
  out[0] = s->chain[i];
  out[1] = out[0];
  out[2] = out[0];
  out[3] = s->hi[i];
  return i;
}

// the detector's slot goes back; the last detector of a device takes the set with it (its streams are idle: a detector is destroyed after its batches)
void stream_set_release(StreamSet* s, int slot) {
  std::lock_guard<std::mutex> lk(g_sets_mu);
  if (slot >= 0 && slot < s->n_slots) s->users[slot]--;
  if (--s->refs > 0) return;
  g_sets.erase(std::find(g_sets.begin(), g_sets.end(), s));
  stream_set_destroy(s);
}

}  // namespace

// ================================================================== handles ======================
struct cs_detector {
  cs_detect_params prm;
  int device = 0;
  // borrowed from the device's StreamSet (above), shared with the other detectors of the process
  StreamSet* streams = nullptr;
  int stream_slot = -1;
  std::atomic<int> busy{0};        // this detector's sweeps queued and not yet COLLECTED by the host (not: still on the device -- a finished sweep counts until cs_batch_collect)
  hipStream_t stream_idle = nullptr;   // own_streams only: runs nothing, holds the fourth place in the order the runtime assigns queues by
  hipStream_t stream = nullptr;    // a batch's chain (and everything outside the sweep: front end, segment producers, the round path)
  hipStream_t stream2 = nullptr;   // vanishing points + corner construction: beside the line setup, or -- few queues -- the chain's stream
  hipStream_t stream3 = nullptr;   // line setup of the crowded ROIs: beside the line setup of all the others, or the chain's stream
  hipStream_t stream_hi = nullptr; // high priority: the small fetches of the tie boxes, which the host waits for while another batch's sweep owns the device
  cs::Event ev[12];
  int n_threads = 1;
  int cpu_grant = 1;          // CPUs this process may use at once (cgroup quota, else the hardware threads)
  std::unique_ptr<WorkerPool> pool;
  // cs_detect_cuboids / cs_detect_cuboids_gray: one resident single-frame batch whose device and pinned buffers are reused from
  // call to call (a batch built and torn down per frame spent most of the call in hipMalloc / hipFree)
  cs_batch* single = nullptr;
  std::mutex single_mu;
  // the resident scratch of the segment producers and the descriptor path, one slot each (cs::ScratchSlot; the holder owns the type, `free` gives it back)
  struct { void* p = nullptr; void (*free)(void*) = nullptr; } scratch[cs::N_SCRATCH_SLOTS];
  std::mutex lines_mu;
  // CS_DETECT_PROF (diagnostics): the host phase clock of this detector's lean-path runs, reported every eighth run (prof_report)
  const bool prof = getenv("CS_DETECT_PROF") != nullptr;
  double prof_mark[16] = {};
  int prof_runs = 0;
};

// The side streams of one enqueue block (call it under enqueue_mu): the detector's own; or, with one stream per slot and no OTHER detector's
// sweep in flight on the device, the streams of two other slots -- nobody else's kernels fill this batch's holes, so it runs corner
// construction, crowded line setup and chain side by side on three queues.  Batches own their buffers and events, so another detector's
// sweep that arrives while such a batch is in flight changes nothing for it.
static void sweep_side_streams(const cs_detector* d, hipStream_t* corners, hipStream_t* crowded) {
  const StreamSet* s = d->streams;
  *corners = d->stream2; *crowded = d->stream3;
  if (!s->own_streams && s->n_slots >= 3 && s->busy.load() == d->busy.load()) {
    *corners = s->chain[(d->stream_slot + 1) % s->n_slots];
    *crowded = s->chain[(d->stream_slot + 2) % s->n_slots];
  }
}

struct JobHost {          // host-side companion of a JobDesc of the current round
  int yaw_off_local;
  std::vector<double> mids_x, mids_y, angs;
  std::vector<int> tops;
  int line_cap = 0;          // entries reserved in the pooled line tables (device setup: the frame's segment count)
};

struct FrameRound {       // setup products of one frame in one round
  std::vector<cs::JobDesc> jobs;
  std::vector<JobHost> jh;
  std::vector<double> yaw, yaw_c, yaw_s;   // concatenated yaw lists of the boxes in this round
};

struct JobResult {        // rank-stage products retained for cs_batch_debug_*
  int n_valid;
  std::vector<double> rows9;     // V x 9
  std::vector<long long> slots;  // V
  std::vector<int> keep;
  std::vector<double> score;
  std::vector<double> corners;   // V x 16 when debug is on
};

// The device tables of one sweep with their pinned companions, for all three paths (a PipeSlot holds one, the round path's is the batch's).
// What only one path needs (flag, bound3, the fb_* pool of the lean roll/pitch path) that path grows itself.
struct cs_batch;
struct SweepBuffers {
  DevBuf<cs::JobDesc> jobs;
  DevBuf<long long> slot_prefix, job_cbase, c_slot, fb_slot;
  DevBuf<int> vp_prefix, top_x, flag, job_valid, c_flag, box_job0, box_njobs, win_count, fallback, fb_flag;
  DevBuf<double> mid_x, mid_y, ang, yaw, yaw_c, yaw_s, vp, bound, bound3, c_dist, c_angle, c_skew, fb_dist, fb_angle, fb_skew;
  DevBuf<cs::RankWinner> winners;
  PinBuf<long long> h_job_cbase, h_fb_src, h_fb_dst, h_fb_slot, h_win_slots;      // h_fb_*, h_win_*: what the tie boxes' gather kernels read and write
  PinBuf<int> h_job_valid, h_win_count, h_fallback, h_fb_cnt, h_fb_flag;
  PinBuf<double> h_fb_dist, h_fb_angle, h_fb_skew, h_win_corners;
  // nj jobs, n_prefix prefix entries (nj + 1; lean roll/pitch: one more per round), pooled line / yaw / top-sample entries, (rp, yaw) samples, nb boxes
  int ensure_tables(size_t nj, size_t n_prefix, size_t n_lines, size_t n_yaw, size_t n_top, size_t vp_total, size_t nb, int kmax) {
    CS_ENSURE(jobs, nj); CS_ENSURE(slot_prefix, n_prefix); CS_ENSURE(vp_prefix, n_prefix); CS_ENSURE(job_valid, nj); CS_ENSURE(job_cbase, n_prefix);
    CS_ENSURE(mid_x, n_lines + 1); CS_ENSURE(mid_y, n_lines + 1); CS_ENSURE(ang, n_lines + 1); CS_ENSURE(yaw, n_yaw + 1); CS_ENSURE(yaw_c, n_yaw + 1); CS_ENSURE(yaw_s, n_yaw + 1);
    CS_ENSURE(top_x, n_top + 1); CS_ENSURE(vp, 6 * vp_total + 6); CS_ENSURE(bound, 6 * vp_total + 6);
    CS_ENSURE(box_job0, nb + 1); CS_ENSURE(box_njobs, nb + 1); CS_ENSURE(win_count, nb + 1); CS_ENSURE(fallback, nb + 1); CS_ENSURE(winners, nb * (size_t)kmax + 1);
    CS_ENSURE(h_win_count, nb + 1); CS_ENSURE(h_fallback, nb + 1); CS_ENSURE(h_job_valid, nj); CS_ENSURE(h_job_cbase, n_prefix);
    return CS_OK;
  }
  int ensure_slots(long long rows) {      // the compacted columns
    return c_slot.ensure(rows + 1) || c_flag.ensure(rows + 1) || c_dist.ensure(rows + 1) || c_angle.ensure(rows + 1) || c_skew.ensure(rows + 1) ? CS_ERR_HIP : CS_OK;
  }
  // The view over n_jobs jobs from job j0, prefix entry p0 on (io: a small production call's tables lie in its I/O block, laid out as A).
  // Pointers of buffers a path never grew are null or stale; its kernels do not read them.
  void bind(cs::DetectDeviceView& v, const cs_batch& b, size_t n_jobs, size_t j0 = 0, size_t p0 = 0, unsigned char* io = nullptr, const SmallCallArena* A = nullptr) const;
  // one height sample's rows [p0, p0 + V) of the fetched tie columns
  HeightCols fb_cols(long long p0, int V) const { return HeightCols{h_fb_dist.p + p0, h_fb_angle.p + p0, h_fb_skew.p + p0, h_fb_flag.p + p0, h_fb_slot.p + p0, V}; }
};

// One of the two in-flight chunks of the pipelined production path (pipe_launch / pipe_finish).  Its buffers and events free themselves.
struct PipeSlot {
  SweepBuffers sb;
  DevBuf<unsigned char> tab_arena;       // a small call's tables in one block: one upload instead of ten (single-frame latency)
  PinBuf<unsigned char> h_tab_arena;
  bool merged_io = false;                // this slot's call went through the block: its results are unpacked from h_tab_arena in pipe_finish
  SmallCallArena arena;                  // ... laid out like this
  DevBuf<int> ls_order, blk_info, ls_crowded;
  PinBuf<int> h_ls_order;
  DevBuf<cs_cuboid> records;        // the winners' records of the device-ranked boxes (record_kernel)
  PinBuf<cs_cuboid> h_records;
  PinBuf<cs::JobDesc> h_jobs_in, h_jobs_out;
  PinBuf<long long> h_slot_prefix;
  PinBuf<int> h_vp_prefix, h_top_x, h_box_job0, h_box_njobs;
  PinBuf<double> h_yaw, h_yaw_c, h_yaw_s;
  cs::Event done, ev[13];                   // 0-6: phase marks on the main stream; 7: inputs resident; 8-11: second stream (corner construction); 12: line setup of the crowded ROIs done (third stream)
  cs::DetectDeviceView view{};
  int vp_total = 0;
  size_t nj = 0, nb = 0;
  long long slot_total = 0;
  bool in_flight = false;
  bool counted_busy = false;      // this sweep is in the detector's and the stream set's `busy` counts
  // ---- the slot protocol of both lean paths: begin (launch), ... enqueue ..., mark_in_flight (launch), wait (finish)
  int begin() { if (!done) { CS_TRY(done.create()); for (auto& e : ev) CS_TRY(e.create()); } return CS_OK; }      // the events, on first use
  // `done` closes the sweep queued on st; from here it counts as in flight for sweep_side_streams (a launch that queued kernels calls it still under enqueue_mu)
  int mark_in_flight(cs_detector* d, hipStream_t st) {
    CS_HIP_TRY(hipEventRecord(done, st));
    in_flight = counted_busy = true; d->busy.fetch_add(1); d->streams->busy.fetch_add(1);
    return CS_OK;
  }
  void uncount(cs_detector* d) { if (counted_busy) { counted_busy = false; d->busy.fetch_sub(1); d->streams->busy.fetch_sub(1); } }
  // the host collects the sweep.  The counts go down BEFORE the wait: an error return must not leave them up
  int wait(cs_detector* d, cs_detect_timing& tm) {
    const double tw = now_ms();
    uncount(d);
    CS_HIP_TRY(hipEventSynchronize(done));
    tm.d2h_ms += now_ms() - tw;   // time the host actually waited for the GPU
    in_flight = false;
    return CS_OK;
  }
};

// The lean roll/pitch path's own state (rp_launch / rp_finish: all rounds of the batch queued at once), once per batch beside pipe[0]
struct RpLean {
  struct Round { size_t j0 = 0, nj = 0, b0 = 0, nb = 0; long long slot_cap = 0; int vp_cap = 0; };
  std::vector<Round> rounds;
  std::vector<int> box_frame, box_index;      // per box (all rounds): frame, box of the frame
  DevBuf<int> trip_cnt, cur_idx, tab_count, maps;   // valid slots per (job of a round, compaction trip); per frame: list in force; (frame, list) -> samples; per round: box / first job / jobs of a frame
  DevBuf<long long> last_slot, box_base;
  DevBuf<unsigned long long> pool_used;
  DevBuf<double> raw_euler;
  PinBuf<int> h_tab_count, h_maps;
  PinBuf<double> h_raw_euler;
  PinBuf<long long> h_last_slot, h_box_base;
  PinBuf<unsigned long long> h_pool_used;
  long long pool_cap = 0;
  std::deque<cs::Event> ev;       // (a deque: it grows without moving an event)  5 per round: start, corners + compaction, VP support, scorer, ranking + records
};

struct BatchRunState;   // what a submitted (not yet collected) sweep keeps alive: camera caches, timing, the caller's output arrays
struct cs_batch {
  cs_detector* det = nullptr;
  BatchRunState* run_state = nullptr;
  cs::Stream copy_stream;                   // cs_batch_refill_gray's upload stream (first among the device resources: it dies after the image buffers it fills)
  PinBuf<cs::RpPose> h_rp;
  DevBuf<unsigned char> d_gray, d_cls;      // image input: gray images and Canny's class bytes (kept: a refilled batch reuses them)
  DevBuf<cs::EdgeRoi> d_edge_rois;
  // cs_batch_refill_gray: a second image buffer (the upload of the next images runs on copy_stream beside the sweep over the current maps),
  // what launch_edge_maps needs again, and the events that order copy -> front end -> the buffer's next upload
  DevBuf<unsigned char> d_gray2;
  cs::Event ev_copied[2], ev_edge_done[2];
  int gray_cur = 0, gray_w = 0, gray_h = 0, edge_n_rois = 0, edge_max_w = 1;
  long long edge_max_px = 1;
  bool gray_batch = false;
  int refill_q[2] = {-1, -1}, n_refill = 0;   // image buffers whose upload is on its way, oldest first; the next submit queues the oldest one's front end
  PinBuf<float> h_maps_stage;               // map upload staging
  PipeSlot pipe[2];
  std::unique_ptr<RpLean> rp;               // created by the first rp_launch
  // capacity layout of the lean path's staging pools (from the inputs alone): first job / first box of a frame, first
  // merged-segment row of a frame's jobs, first top-edge sample of a box
  std::vector<int> job_base, box_base, top_base;
  std::vector<long long> line_base;
  bool force_no_pipeline = false;
  int pipe_chunks = 1;   // chunks of the two-slot pipeline (cs_batch_set_pipeline_chunks)
  int n_frames = 0, max_boxes = 0;
  std::vector<FrameIn> frames;
  DevBuf<float> d_maps;
  const float* maps = nullptr;   // the map pool the sweep reads: d_maps.p (batch_fill), or -- the lean roll/pitch path's redo batch -- the parent batch's
  DevBuf<double> d_invK, d_frame_lines;
  DevBuf<int> d_frame_line_ptr;
  bool device_setup = false;   // every frame's segment count fits the line-setup kernel's LDS table
  bool force_host_setup = false;
  DevBuf<cs::RpPose> d_rp;      // the frames' roll/pitch sample poses, all paths
  // round path: the device tables of the round in flight, and what only this path brings back (every compacted column for the host
  // ranking, the device's winners with their corners, the carried proposal, the job table)
  SweepBuffers round;
  DevBuf<int> round_ls_lists;       // the line setup's two lists of crowded jobs: 2 (nj + 1) ints
  PinBuf<long long> h_c_slot;
  PinBuf<int> h_c_flag;
  PinBuf<double> h_c_dist, h_c_angle, h_c_skew;
  DevBuf<long long> d_last_slot;
  PinBuf<long long> h_last_slot;
  PinBuf<cs::RankWinner> h_winners;
  PinBuf<cs::JobDesc> h_jobs;
  PinBuf<unsigned char> h_tables;   // the job tables of one round, staged in pinned memory: their uploads are asynchronous and back to back
  bool force_host_rank = false;
  bool force_round_path = false;   // roll/pitch sampling through the round-by-round path (the lean path's redo of frames with tie boxes)
  // state
  bool debug = false, ran = false;
  std::vector<JobResult> results;             // all jobs of the last run (index via job_index)
  std::vector<int> job_index;                 // (frame*max_boxes + box)*3 + k -> results idx or -1
  cs_detect_timing timing{};
  // (the caller has made the device current.)  The upload stream first: nothing may still be writing the image buffers when the
  // members -- every device and pinned buffer above -- free themselves after this body
  ~cs_batch() { if (copy_stream) (void)hipStreamSynchronize(copy_stream); }
};

void SweepBuffers::bind(cs::DetectDeviceView& v, const cs_batch& b, size_t n_jobs, size_t j0, size_t p0, unsigned char* io, const SmallCallArena* A) const {
  v = cs::DetectDeviceView{};
  v.jobs = jobs.p + j0; v.n_jobs = (int)n_jobs; v.slot_prefix = slot_prefix.p + p0; v.vp_prefix = vp_prefix.p + p0; v.maps = b.maps;
  v.mid_x = mid_x.p; v.mid_y = mid_y.p; v.line_angle = ang.p; v.yaw = yaw.p; v.yaw_cos = yaw_c.p; v.yaw_sin = yaw_s.p; v.top_x = top_x.p;
  v.rp = b.d_rp.p; v.invK = b.d_invK.p; v.vp = vp.p; v.bound = bound.p; v.bound3 = bound3.p; v.flag = flag.p; v.job_valid = job_valid.p + j0;
  v.job_cbase = job_cbase.p + p0; v.c_slot = c_slot.p; v.c_flag = c_flag.p; v.c_dist = c_dist.p; v.c_angle = c_angle.p; v.c_skew = c_skew.p;
  if (!io) return;
  v.jobs = reinterpret_cast<cs::JobDesc*>(io + A->o_jobs); v.slot_prefix = reinterpret_cast<long long*>(io + A->o_sp); v.vp_prefix = reinterpret_cast<int*>(io + A->o_vp);
  v.yaw = reinterpret_cast<double*>(io + A->o_y); v.yaw_cos = reinterpret_cast<double*>(io + A->o_yc); v.yaw_sin = reinterpret_cast<double*>(io + A->o_ys);
  v.top_x = reinterpret_cast<int*>(io + A->o_tx); v.job_valid = reinterpret_cast<int*>(io + A->o_jv); v.job_cbase = reinterpret_cast<long long*>(io + A->o_cb);
}


// The C ABI is the trust boundary: a 2D box must lie inside the image (its far edges are pixel coordinates the sweep
// intersects rays with and samples the distance map at).  The reference indexes the map unchecked (object_3d_util.cpp:651), so a
// box outside the image is undefined behaviour there; here it is CS_ERR_INVALID_ARG.
static bool box_inside_image(const double* box5, int img_w, int img_h) {
  if (img_w <= 0 || img_h <= 0) return false;
  for (int q = 0; q < 4; q++) if (!(box5[q] > -1e9 && box5[q] < 1e9)) return false;   // NaN / inf / absurd
  const int left = (int)box5[0], top = (int)box5[1], w = (int)box5[2], h = (int)box5[3];
  const int right = (int)(left + box5[2]), bottom = top + h;
  return left >= 0 && top >= 0 && w > 0 && h > 0 && right <= img_w - 1 && bottom <= img_h - 1;
}

extern "C" {

const char* cs_last_error(void) { return g_cs_err.c_str(); }

int cs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int cs_diag_build(void) {
#ifdef CS_DIAG
  return 1;
#else
  return 0;
#endif
}

int cs_check_score_atan2(const double* y, const double* x, int n, double* out, int* accepted) {
  if (n < 0 || (n > 0 && (!y || !x || !out || !accepted))) { cs_set_error("cs_check_score_atan2: null array"); return CS_ERR_INVALID_ARG; }
  if (n > (1 << 30)) { cs_set_error("cs_check_score_atan2: more than 2^30 pairs"); return CS_ERR_CAPACITY; }
  if (int rc = cs::check_device(0)) return rc;
  if (n == 0) return CS_OK;
  CS_HIP_TRY(hipSetDevice(0));
  DevBuf<double> d;       // y, x, out
  DevBuf<int> a;
  int rc = d.ensure(3 * (size_t)n);
  if (rc == CS_OK) rc = a.ensure((size_t)n);
  auto run = [&]() -> int {
    CS_HIP_TRY(hipMemcpy(d.p, y, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    CS_HIP_TRY(hipMemcpy(d.p + n, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    cs::launch_score_atan2_check(d.p, d.p + n, n, d.p + 2 * (size_t)n, a.p, nullptr);
    CS_HIP_TRY(hipGetLastError());
    CS_HIP_TRY(hipMemcpy(out, d.p + 2 * (size_t)n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    CS_HIP_TRY(hipMemcpy(accepted, a.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return CS_OK;
  };
  if (rc == CS_OK) rc = run();
  return rc;
}

int cs_check_score_sample_index(const double* sy, const double* sx, const int* map_w, const double* a, const double* b, int n, int* index, double* probe) {
  if (n < 0 || (n > 0 && (!sy || !sx || !map_w || !a || !b || !index || !probe))) { cs_set_error("cs_check_score_sample_index: null array"); return CS_ERR_INVALID_ARG; }
  if (n > (1 << 28)) { cs_set_error("cs_check_score_sample_index: more than 2^28 samples"); return CS_ERR_CAPACITY; }
  if (int rc = cs::check_device(0)) return rc;
  if (n == 0) return CS_OK;
  CS_HIP_TRY(hipSetDevice(0));
  DevBuf<double> d;       // sy, sx, a, b, probe
  DevBuf<int> w;          // map_w, index
  const size_t N = (size_t)n;
  int rc = d.ensure(5 * N);
  if (rc == CS_OK) rc = w.ensure(2 * N);
  auto run = [&]() -> int {
    const double* in[4] = {sy, sx, a, b};
    for (int q = 0; q < 4; q++) CS_HIP_TRY(hipMemcpy(d.p + q * N, in[q], sizeof(double) * N, hipMemcpyHostToDevice));
    CS_HIP_TRY(hipMemcpy(w.p, map_w, sizeof(int) * N, hipMemcpyHostToDevice));
    cs::launch_score_sample_index_check(d.p, d.p + N, w.p, d.p + 2 * N, d.p + 3 * N, n, w.p + N, d.p + 4 * N, nullptr);
    CS_HIP_TRY(hipGetLastError());
    CS_HIP_TRY(hipMemcpy(index, w.p + N, sizeof(int) * N, hipMemcpyDeviceToHost));
    CS_HIP_TRY(hipMemcpy(probe, d.p + 4 * N, sizeof(double) * N, hipMemcpyDeviceToHost));
    return CS_OK;
  };
  if (rc == CS_OK) rc = run();
  return rc;
}

int cs_check_line_setup(const double* lines, int n, const int* rois, const int* yt, int r, double dist_thre, double angle_thre_deg, double len_thre,
                        int* dev_m, double* dev_tab, int* host_m, double* host_tab) {
  if (n < 0 || r < 0 || (n > 0 && !lines) || (r > 0 && (!rois || !yt || !dev_m || !dev_tab || !host_m || !host_tab))) { cs_set_error("cs_check_line_setup: null array"); return CS_ERR_INVALID_ARG; }
  if (n > cs::line_setup_capacity()) { cs_set_error("cs_check_line_setup: more segments than the line setup's rows"); return CS_ERR_CAPACITY; }
  if (r > (1 << 16)) { cs_set_error("cs_check_line_setup: more than 2^16 ROIs"); return CS_ERR_CAPACITY; }
  if (int rc = cs::check_device(0)) return rc;
  if (r == 0) return CS_OK;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(0));
  const size_t N = (size_t)n, R = (size_t)r, plane = R * N;
  std::vector<cs::JobDesc> jobs(R);
  std::memset(jobs.data(), 0, sizeof(cs::JobDesc) * R);
  std::fill(host_tab, host_tab + 3 * plane, 0.0);
  for (size_t k = 0; k < R; k++) {
    cs::JobDesc& jd = jobs[k];
    jd.g.el = rois[4 * k]; jd.g.et = rois[4 * k + 1]; jd.g.er = rois[4 * k + 2]; jd.g.eb = rois[4 * k + 3];
    jd.Y = yt[2 * k]; jd.T = yt[2 * k + 1]; jd.line_off = (int)(k * N);
    // the host's tables: what the sweep computes under force_host_setup (a skipped job has no segments)
    host_m[k] = 0;
    if (jd.Y == 0 || jd.T == 0) continue;
    std::vector<double> in;
    for (size_t e = 0; e < N; e++) {
      const double* l = lines + 4 * e;
      if (cs::inside_box(cs::v2(l[0], l[1]), jd.g.el, jd.g.et, jd.g.er, jd.g.eb) && cs::inside_box(cs::v2(l[2], l[3]), jd.g.el, jd.g.et, jd.g.er, jd.g.eb)) in.insert(in.end(), l, l + 4);
    }
    merge_lines(in, dist_thre, angle_thre_deg, len_thre);
    host_m[k] = (int)(in.size() / 4);
    for (size_t i = 0; i < in.size() / 4; i++) {
      host_tab[k * N + i] = cs::cs_atan2(in[4 * i + 3] - in[4 * i + 1], in[4 * i + 2] - in[4 * i]);
      host_tab[plane + k * N + i] = (in[4 * i] + in[4 * i + 2]) / 2;
      host_tab[2 * plane + k * N + i] = (in[4 * i + 1] + in[4 * i + 3]) / 2;
    }
  }
  // the device's: the production launcher, everything on the null stream
  DevBuf<cs::JobDesc> d_jobs;
  DevBuf<double> d_lines, d_tab;      // d_tab: angle, mid x, mid y planes of r x n
  DevBuf<int> d_ptr, d_lists;
  cs::Event fork, join;
  CS_ENSURE(d_jobs, R); CS_ENSURE(d_lines, 4 * N + 4); CS_ENSURE(d_tab, 3 * plane + 1); CS_ENSURE(d_ptr, 2); CS_ENSURE(d_lists, 2 * (R + 1));
  CS_TRY(fork.create()); CS_TRY(join.create());
  const int ptr[2] = {0, n};
  CS_HIP_TRY(hipMemcpy(d_jobs.p, jobs.data(), sizeof(cs::JobDesc) * R, hipMemcpyHostToDevice));
  if (n) CS_HIP_TRY(hipMemcpy(d_lines.p, lines, sizeof(double) * 4 * N, hipMemcpyHostToDevice));
  CS_HIP_TRY(hipMemcpy(d_ptr.p, ptr, sizeof(ptr), hipMemcpyHostToDevice));
  CS_HIP_TRY(hipMemset(d_tab.p, 0, sizeof(double) * (3 * plane + 1)));
  cs::launch_line_setup_listed(d_jobs.p, r, d_lines.p, d_ptr.p, d_tab.p + plane, d_tab.p + 2 * plane, d_tab.p, dist_thre, angle_thre_deg, len_thre, nullptr, nullptr, nullptr, fork, join, d_lists.p);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipMemcpy(jobs.data(), d_jobs.p, sizeof(cs::JobDesc) * R, hipMemcpyDeviceToHost));
  if (plane) CS_HIP_TRY(hipMemcpy(dev_tab, d_tab.p, sizeof(double) * 3 * plane, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < R; k++) dev_m[k] = jobs[k].m;
  return CS_OK;
  CS_GUARD_END("cs_check_line_setup")
}

// VP_support_edge_infos (object_3d_util.cpp:548-619) for one point, written plainly: the angle of every segment, the inlier test, the
// unwrap against the first inlier, strict first-occurrence extremes.  What cs_check_vp_support sets the device's decisions against.
static void vp_support_reference(const double* mx, const double* my, const double* la, int m, double vpx, double vpy, double thre, bool swapped, double* out2) {
  bool have = false;
  double base = 0, hi = 0, lo = 0;
  int i_hi = -1, i_lo = -1;
  for (int i = 0; i < m; i++) {
    const double raw = cs::cs_atan2(my[i] - vpy, mx[i] - vpx);
    const double nrm = cs::normalize_to_pi(raw);
    double d = cs::dabs(la[i] - nrm);
    d = cs::dmin(d, CS_PI - d);
    if (!(d < thre)) continue;
    if (!have) { have = true; base = hi = lo = raw; i_hi = i_lo = i; continue; }
    double sh = raw;
    if ((raw - base) < -CS_PI) sh = raw + 2 * CS_PI;
    else if ((raw - base) > CS_PI) sh = raw - 2 * CS_PI;
    if (sh > hi) { hi = sh; i_hi = i; }
    if (sh < lo) { lo = sh; i_lo = i; }
  }
  const double NaN = __builtin_nan("");
  const double a_hi = have ? la[i_hi] : NaN, a_lo = have ? la[i_lo] : NaN;
  out2[0] = swapped ? a_lo : a_hi;
  out2[1] = swapped ? a_hi : a_lo;
}

int cs_check_vp_support(const double* mid_x, const double* mid_y, const double* angle, int m, const double* vp_x, const double* vp_y, int n, double thre, int swapped, int form,
                        double* dev, double* host) {
  if (m < 0 || n < 0 || (m > 0 && (!mid_x || !mid_y || !angle)) || (n > 0 && (!vp_x || !vp_y || !dev || !host))) { cs_set_error("cs_check_vp_support: null array"); return CS_ERR_INVALID_ARG; }
  if (form < 0 || form > 2) { cs_set_error("cs_check_vp_support: form must be 0, 1 or 2"); return CS_ERR_INVALID_ARG; }
  if (m > (1 << 20) || n > (1 << 20)) { cs_set_error("cs_check_vp_support: more than 2^20 segments or points"); return CS_ERR_CAPACITY; }
  if (int rc = cs::check_device(0)) return rc;
  if (n == 0) return CS_OK;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(0));
  for (int p = 0; p < n; p++) vp_support_reference(mid_x, mid_y, angle, m, vp_x[p], vp_y[p], thre, swapped != 0, host + 2 * (size_t)p);
  const size_t M = (size_t)m, N = (size_t)n;
  DevBuf<double> d;       // mid x, mid y, angle | vp x, vp y | out
  CS_ENSURE(d, 3 * M + 4 * N + 1);
  double* seg = d.p;
  double* pts = d.p + 3 * M;
  double* out = pts + 2 * N;
  if (m) {
    CS_HIP_TRY(hipMemcpy(seg, mid_x, sizeof(double) * M, hipMemcpyHostToDevice));
    CS_HIP_TRY(hipMemcpy(seg + M, mid_y, sizeof(double) * M, hipMemcpyHostToDevice));
    CS_HIP_TRY(hipMemcpy(seg + 2 * M, angle, sizeof(double) * M, hipMemcpyHostToDevice));
  }
  CS_HIP_TRY(hipMemcpy(pts, vp_x, sizeof(double) * N, hipMemcpyHostToDevice));
  CS_HIP_TRY(hipMemcpy(pts + N, vp_y, sizeof(double) * N, hipMemcpyHostToDevice));
  CS_HIP_TRY(hipMemset(out, 0, sizeof(double) * 2 * N));
  cs::launch_vp_support_check(seg, seg + M, seg + 2 * M, m, pts, pts + N, n, thre, swapped != 0, form, out, nullptr);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipMemcpy(dev, out, sizeof(double) * 2 * N, hipMemcpyDeviceToHost));
  return CS_OK;
  CS_GUARD_END("cs_check_vp_support")
}

void cs_detect_default_params(cs_detect_params* p) {
  if (!p) return;
  p->consider_config_1 = 1; p->consider_config_2 = 1;
  p->whether_sample_cam_roll_pitch = 1; p->whether_sample_bbox_height = 0;
  p->max_cuboid_num = 1; p->nominal_skew_ratio = 1; p->max_cut_skew = 3;
  p->yaw_range_deg = 45; p->yaw_step_deg = 6;
  p->vp12_edge_angle_thre = 15; p->vp3_edge_angle_thre = 10; p->shorted_edge_thre = 20;
  p->weight_vp_angle = 0.8; p->weight_skew_error = 1.5;
  p->pre_merge_dist_thre = 20; p->pre_merge_angle_thre = 5; p->edge_length_threshold = 30;
  p->host_threads = 0;
}

int cs_box_rois(const double box5[5], int img_w, int img_h, int sample_height, cs_roi out[3]) {
  if (!box5 || !out) return CS_ERR_INVALID_ARG;
  int left = box5[0], top = box5[1], w = box5[2], h = box5[3];
  int right = left + box5[2];
  int downs[3], nd = 0;
  downs[nd++] = 0;
  if (sample_height) {
    int r = std::max(std::min(20, h - 90), 20);
    r = std::min(r, img_h - top - h - 1);
    if (r > 10) downs[nd++] = (int)std::round(r / 2);
    downs[nd++] = r;
  }
  for (int k = 0; k < nd; k++) {
    int he = h + downs[k];
    int dy = top + he;
    int e = std::min(std::max(std::min(20, w - 100), 10), std::max(std::min(20, he - 100), 10));
    int l = std::max(0, left - e), r = std::min(img_w - 1, right + e);
    int t = std::max(0, top - e), b = std::min(img_h - 1, dy + e);
    out[k].left = l; out[k].top = t; out[k].width = r - l; out[k].height = b - t; out[k].down_expand = downs[k];
  }
  return nd;
}

int cs_cam_euler_zyx(const double T_wc[16], double euler3[3]) {
  if (!T_wc || !euler3) return CS_ERR_INVALID_ARG;
  double R[9];
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = T_wc[4 * i + j];
  rot_to_euler(R, euler3);
  return CS_OK;
}

// internal (not in the public header): the line-segment producer (lines_host.cpp) runs on the detector's stream
void* cs_internal_detector_stream(cs_detector* d) { return (void*)d->stream; }
// the scratch slots (detect_hooks.h), their holders' lock, and the detector's worker pool
void** cs_internal_detector_scratch_slot(cs_detector* d, int which, void (*deleter)(void*)) { d->scratch[which].free = deleter; return &d->scratch[which].p; }
void* cs_internal_detector_lines_mutex(cs_detector* d) { return (void*)&d->lines_mu; }
void cs_internal_detector_parallel(cs_detector* d, int n, void (*fn)(int, void*), void* ctx) { d->pool->run(n, [&](int i) { fn(i, ctx); }); }
// (for the segment producers' image-long items: two threads per granted CPU at most, see cs_detector_create)
void cs_internal_detector_parallel_long(cs_detector* d, int n, void (*fn)(int, void*), void* ctx) { d->pool->run(n, [&](int i) { fn(i, ctx); }, 2 * d->cpu_grant + 1); }
int cs_internal_detector_device(cs_detector* d) { return d->device; }

int cs_detector_create(const cs_detect_params* params, int device, cs_detector** out) {
  if (!out) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  { const int rc = cs::check_device(device); if (rc) return rc; }
  CS_GUARD_BEGIN
  cs::Guard<cs_detector> g(new cs_detector(), cs_detector_destroy);   // freed on every early return
  cs_detector* d = g.h;
  if (params) d->prm = *params; else cs_detect_default_params(&d->prm);
  if (d->prm.max_cuboid_num < 1 || !(d->prm.yaw_step_deg > 0) || !(d->prm.yaw_range_deg >= 0)) { cs_set_error("bad params"); return CS_ERR_INVALID_ARG; }
  d->device = device;
  CS_HIP_TRY(hipSetDevice(device));
  {
    hipError_t se = hipSuccess;
    d->streams = stream_set_acquire(device, &se);
    CS_HIP_TRY(se);
    if (d->streams->own_streams) {
      CS_HIP_TRY(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
      CS_HIP_TRY(hipStreamCreateWithFlags(&d->stream2, hipStreamNonBlocking));
      CS_HIP_TRY(hipStreamCreateWithFlags(&d->stream3, hipStreamNonBlocking));
      CS_HIP_TRY(hipStreamCreateWithFlags(&d->stream_idle, hipStreamNonBlocking));
      int prio_low = 0, prio_high = 0;   // (numerically lowest = greatest priority)
      CS_HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high));
      CS_HIP_TRY(hipStreamCreateWithPriority(&d->stream_hi, hipStreamNonBlocking, prio_high));
    } else {
      hipStream_t st4[4];
      d->stream_slot = stream_set_borrow(d->streams, st4);
      d->stream = st4[0]; d->stream2 = st4[1]; d->stream3 = st4[2]; d->stream_hi = st4[3];
    }
  }
  for (auto& e : d->ev) CS_TRY(e.create());
  int hc = (int)std::thread::hardware_concurrency();
  // default worker count: 64 on an unrestricted 256-thread EPYC (beats 32 and 128); under a cgroup CPU quota three threads
  // per granted CPU (measured under a 16-CPU quota: 48 threads 187 k frames/s, 32: 184 k, 64: 171-181 k, 16: 166-172 k --
  // the stages are short bursts, more runnable threads than the quota tolerates get the process throttled)
  int dflt = std::max(1, std::min(hc, 64));
  d->cpu_grant = std::max(1, hc);
  if (FILE* fq = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    long long quota = 0, period = 0;
    if (std::fscanf(fq, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) {
      dflt = std::max(1, std::min(dflt, std::max(8, (int)(3 * quota / period))));
      d->cpu_grant = std::max(1, std::min(d->cpu_grant, (int)(quota / period)));
    }
    std::fclose(fq);
  }
  d->n_threads = d->prm.host_threads > 0 ? d->prm.host_threads : dflt;
  d->pool.reset(new WorkerPool(d->n_threads - 1));
  *out = g.disarm();
  return CS_OK;
  CS_GUARD_END("cs_detector_create")
}

void cs_detector_destroy(cs_detector* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  // (the streams are shared: what this detector queued outside a batch -- a front end, a segment producer's tail -- is waited for here,
  // before the resident batch and the producers' scratch go)
  if (d->stream) (void)hipStreamSynchronize(d->stream);
  if (d->single) { cs_batch_destroy(d->single); d->single = nullptr; }
  for (auto& s : d->scratch) if (s.p && s.free) { s.free(s.p); s.p = nullptr; }      // (EDLines, LSD, descriptors)
  if (d->streams) {
    // the five working streams are this detector's own or the shared set's, so they stay raw and go here
    if (d->streams->own_streams)
      for (hipStream_t st : {d->stream, d->stream2, d->stream3, d->stream_idle, d->stream_hi}) if (st) (void)hipStreamDestroy(st);
    stream_set_release(d->streams, d->stream_slot);
  }
  delete d;
}

static int batch_fill(cs_detector* d, cs_batch* b, const cs_frame_desc* fr, const unsigned char* const* grays, int n_frames);
// Launch order of the distance-map front end's workgroups (one per ROI, its time grows with the ROI's area): largest first, so that the
// kernels do not end on a late-started large ROI.  The entries carry their own offsets: their order in the table means nothing else.
static void edge_rois_largest_first(std::vector<cs::EdgeRoi>& er) {
  if (er.size() <= 1024) return;
  std::stable_sort(er.begin(), er.end(), [](const cs::EdgeRoi& a, const cs::EdgeRoi& c) { return (long long)a.w * a.h > (long long)c.w * c.h; });
}
static int batch_layout(cs_detector* d, cs_batch* b);
static int batch_run_impl(cs_detector* d, cs_batch* b, cs_cuboid* out, int* out_counts, bool defer);
static int batch_flush_refill(cs_detector* d, cs_batch* b);
static int batch_create_impl(cs_detector* d, const cs_frame_desc* fr, const unsigned char* const* grays, int n_frames, cs_batch** out) {
  if (!d || !out || (!fr && n_frames) || n_frames < 0) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(d->device));
  cs::Guard<cs_batch> g(new cs_batch(), cs_batch_destroy);   // freed on every early return
  g.h->det = d;
  int rc = batch_fill(d, g.h, fr, grays, n_frames);
  if (rc) return rc;
  *out = g.disarm();
  return CS_OK;
  CS_GUARD_END("cs_batch_create")
}
// (Re)describe the frames of a batch: host copies, ROIs, the map pool (uploaded, or produced in place from gray images), the
// segment pool, the capacity layout.  Device and pinned buffers only ever grow, so refilling a batch with frames of a similar size --
// the resident single-frame batch of cs_detect_cuboids -- allocates nothing.
static int batch_fill(cs_detector* d, cs_batch* b, const cs_frame_desc* fr, const unsigned char* const* grays, int n_frames) {
  b->n_frames = n_frames;
  b->max_boxes = 0;
  b->ran = false;
  b->frames.resize(n_frames);
  size_t map_floats = 0;
  for (int f = 0; f < n_frames; f++) {
    const cs_frame_desc& s = fr[f];
    FrameIn& F = b->frames[f];
    if (!s.K || !s.T_wc || s.n_boxes < 0 || s.n_lines < 0 || (s.n_boxes && (!s.boxes || (!grays && !s.dist_maps))) || (s.n_lines && !s.lines) || (grays && !grays[f])) {
      cs_set_error("bad frame descriptor"); return CS_ERR_INVALID_ARG;
    }
    for (int i = 0; i < s.n_boxes; i++)
      if (!box_inside_image(s.boxes + 5 * (size_t)i, s.img_w, s.img_h)) { cs_set_error("2D box outside the image (need 0 <= x, 0 <= y, x + w <= img_w - 1, y + h <= img_h - 1)"); return CS_ERR_INVALID_ARG; }
    if (s.T_wc[12] != 0 || s.T_wc[13] != 0 || s.T_wc[14] != 0 || s.T_wc[15] != 1) {
      cs_set_error("T_wc must have last row 0 0 0 1"); return CS_ERR_INVALID_ARG;
    }
    std::memcpy(F.K, s.K, sizeof(F.K));
    inv3(F.K, F.invK);  // set_calibration (box_proposal_detail.cpp:38-42)
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) F.R[3 * i + j] = s.T_wc[4 * i + j];
      F.t[i] = s.T_wc[4 * i + 3];
    }
    F.img_w = s.img_w; F.img_h = s.img_h; F.n_boxes = s.n_boxes; F.n_lines = s.n_lines;
    F.boxes.assign(s.boxes, s.boxes + 5 * (size_t)s.n_boxes);
    F.lines.assign(s.lines, s.lines + 4 * (size_t)s.n_lines);
    for (int i = 0; i < s.n_lines; i++)  // align_left_right_edges
      if (F.lines[4 * i + 2] < F.lines[4 * i]) {
        std::swap(F.lines[4 * i], F.lines[4 * i + 2]);
        std::swap(F.lines[4 * i + 1], F.lines[4 * i + 3]);
      }
    F.rois.resize(3 * (size_t)s.n_boxes);
    F.n_heights.resize(s.n_boxes);
    F.map_offs.assign(3 * (size_t)s.n_boxes, -1);
    for (int i = 0; i < s.n_boxes; i++) {
      int nh = cs_box_rois(&F.boxes[5 * i], F.img_w, F.img_h, d->prm.whether_sample_bbox_height, &F.rois[3 * i]);
      F.n_heights[i] = nh;
      for (int k = 0; k < nh; k++) {
        const cs_roi& r = F.rois[3 * i + k];
        if (r.width <= 0 || r.height <= 0 || (!grays && !s.dist_maps[3 * i + k])) { cs_set_error("missing distance map / empty ROI"); return CS_ERR_INVALID_ARG; }
        F.map_offs[3 * i + k] = (long long)map_floats;
        map_floats += (size_t)r.width * r.height + r.width + 1;  // + one row + one float of zero padding
      }
    }
    b->max_boxes = std::max(b->max_boxes, s.n_boxes);
  }
  // upload the distance maps (zero padded) and the per-frame invK
  int rc = b->d_maps.ensure(map_floats + 1);
  if (rc) { return rc; }
  b->maps = b->d_maps.p;
  {
    if (!grays) {
      // small pools (a frame, a few frames) go through pinned staging kept by the batch and a queued copy; a large batch's pool is
      // staged once in pageable memory and copied synchronously -- pinning gigabytes for a one-off upload costs more than it saves
      const bool pinned = map_floats + 1 <= ((size_t)16 << 20);
      std::vector<float> big;
      float* stage = nullptr;
      if (pinned) { rc = b->h_maps_stage.ensure(map_floats + 1); if (rc) return rc; stage = b->h_maps_stage.p; std::memset(stage, 0, sizeof(float) * (map_floats + 1)); }
      else { big.assign(map_floats + 1, 0.0f); stage = big.data(); }
      for (int f = 0; f < n_frames; f++) {
        FrameIn& F = b->frames[f];
        for (int i = 0; i < F.n_boxes; i++)
          for (int k = 0; k < F.n_heights[i]; k++) {
            const cs_roi& r = F.rois[3 * i + k];
            std::memcpy(&stage[F.map_offs[3 * i + k]], fr[f].dist_maps[3 * i + k], sizeof(float) * (size_t)r.width * r.height);
          }
      }
      if (pinned) CS_HIP_TRY(hipMemcpyAsync(b->d_maps.p, stage, sizeof(float) * (map_floats + 1), hipMemcpyHostToDevice, d->stream));   // the sweep follows on the same stream
      else CS_HIP_TRY(hipMemcpy(b->d_maps.p, stage, sizeof(float) * (map_floats + 1), hipMemcpyHostToDevice));
    } else {
      // image in: upload the gray images, produce every job's map in place in the pool (Canny + distance transform on the
      // device, box_proposal_detail.cpp:320-327); the padding between the maps stays zero.  All frames share one size.
      const int W = n_frames ? fr[0].img_w : 0, H = n_frames ? fr[0].img_h : 0;
      std::vector<cs::EdgeRoi> er;
      long long cls_tot = 0, max_px = 1;
      int max_w = 1;
      for (int f = 0; f < n_frames; f++) {
        FrameIn& F = b->frames[f];
        if (F.img_w != W || F.img_h != H) { cs_set_error("cs_batch_create_gray: all frames must have the same image size"); return CS_ERR_INVALID_ARG; }
        for (int i = 0; i < F.n_boxes; i++)
          for (int k = 0; k < F.n_heights[i]; k++) {
            const cs_roi& r = F.rois[3 * i + k];
            if (r.left < 0 || r.top < 0 || r.left + r.width > W || r.top + r.height > H) { cs_set_error("ROI outside the image"); return CS_ERR_INVALID_ARG; }
            er.push_back(cs::EdgeRoi{r.left, r.top, r.width, r.height, (long long)f * W * H, cls_tot, F.map_offs[3 * i + k]});
            cls_tot += (long long)r.width * r.height;
            max_w = std::max(max_w, r.width); max_px = std::max(max_px, 4LL * ((r.width + 5) / 4) * (r.height + 2));
          }
      }
      DevBuf<unsigned char>& d_gray = b->d_gray; DevBuf<unsigned char>& d_cls = b->d_cls;
      DevBuf<cs::EdgeRoi>& d_rois = b->d_edge_rois;
      if ((rc = d_gray.ensure((size_t)W * H * std::max(1, n_frames))) || (rc = d_cls.ensure((size_t)cls_tot + 8)) || (rc = d_rois.ensure(er.size() + 1))) { return rc; }
      hipStream_t st = d->stream;
      b->gray_batch = true; b->gray_w = W; b->gray_h = H; b->edge_n_rois = (int)er.size(); b->edge_max_w = max_w; b->edge_max_px = max_px; b->gray_cur = 0;
      CS_HIP_TRY(hipMemsetAsync(b->d_maps.p, 0, sizeof(float) * (map_floats + 1), st));
      for (int f = 0; f < n_frames; f++) CS_HIP_TRY(hipMemcpyAsync(d_gray.p + (size_t)f * W * H, grays[f], (size_t)W * H, hipMemcpyHostToDevice, st));
      if (!er.empty()) {
        edge_rois_largest_first(er);
        CS_HIP_TRY(hipMemcpyAsync(d_rois.p, er.data(), sizeof(cs::EdgeRoi) * er.size(), hipMemcpyHostToDevice, st));
        cs::launch_edge_maps(d_gray.p, W, H, d_rois.p, (int)er.size(), d_cls.p, b->d_maps.p, max_w, max_px, 80, 200, st);
        CS_HIP_TRY(hipGetLastError());
      }
      CS_HIP_TRY(hipStreamSynchronize(st));      // (the host arrays `grays` and `er` are read by the copies above)
    }
  }
  return batch_layout(d, b);
}
// Second half of describing a batch: per-frame invK, the pooled line segments, the capacity layout of the staging pools.
static int batch_layout(cs_detector* d, cs_batch* b) {
  const int n_frames = b->n_frames;
  {
    std::vector<double> ik(9 * (size_t)std::max(1, n_frames));
    for (int f = 0; f < n_frames; f++) std::memcpy(&ik[9 * f], b->frames[f].invK, 9 * sizeof(double));
    CS_ENSURE(b->d_invK, ik.size());
    CS_HIP_TRY(hipMemcpy(b->d_invK.p, ik.data(), sizeof(double) * ik.size(), hipMemcpyHostToDevice));
    // line segments (already left-to-right aligned), pooled, for the device-side line setup
    std::vector<int> lp(n_frames + 1, 0);
    b->device_setup = true;
    for (int f = 0; f < n_frames; f++) { lp[f + 1] = lp[f] + b->frames[f].n_lines; if (b->frames[f].n_lines > cs::line_setup_capacity()) b->device_setup = false; }
    std::vector<double> fl(4 * (size_t)std::max(1, lp[n_frames]));
    for (int f = 0; f < n_frames; f++) if (b->frames[f].n_lines) std::memcpy(&fl[4 * (size_t)lp[f]], b->frames[f].lines.data(), 32 * (size_t)b->frames[f].n_lines);
    CS_ENSURE(b->d_frame_lines, fl.size()); CS_ENSURE(b->d_frame_line_ptr, lp.size());
    CS_HIP_TRY(hipMemcpy(b->d_frame_lines.p, fl.data(), 8 * fl.size(), hipMemcpyHostToDevice));
    CS_HIP_TRY(hipMemcpy(b->d_frame_line_ptr.p, lp.data(), 4 * lp.size(), hipMemcpyHostToDevice));
  }
  {
    b->job_base.assign(n_frames + 1, 0); b->box_base.assign(n_frames + 1, 0); b->line_base.assign(n_frames + 1, 0);
    b->top_base.assign(1, 0);
    for (int f = 0; f < n_frames; f++) {
      const FrameIn& F = b->frames[f];
      int nj = 0;
      for (int bi = 0; bi < F.n_boxes; bi++) {
        nj += F.n_heights[bi];
        b->top_base.push_back(b->top_base.back() + top_samples(&F.boxes[5 * bi], nullptr));   // :215-219: the count depends on the box alone
      }
      b->job_base[f + 1] = b->job_base[f] + nj;
      b->box_base[f + 1] = b->box_base[f] + F.n_boxes;
      b->line_base[f + 1] = b->line_base[f] + (long long)nj * F.n_lines;
    }
  }
  return CS_OK;
}

int cs_batch_create(cs_detector* d, const cs_frame_desc* fr, int n_frames, cs_batch** out) { return batch_create_impl(d, fr, nullptr, n_frames, out); }

int cs_batch_create_gray(cs_detector* d, const cs_frame_desc* fr, const unsigned char* const* grays, int n_frames, cs_batch** out) {
  if (n_frames > 0 && !grays) return CS_ERR_INVALID_ARG;
  return batch_create_impl(d, fr, grays, n_frames, out);
}

// New images for the frames of an image-input batch (same frame descriptions: boxes, segments, cameras): the upload goes to the batch's OTHER
// image buffer on a copy stream of its own -- beside whatever sweep is running --, the front end (Canny + distance transform of every ROI)
// is queued by the next cs_batch_submit in front of its sweep.  Up to two uploads may be queued (one per image buffer): a caller that
// queues the upload AFTER next before each submit keeps the copy engine busy without a gap, and the whole device side of a step (front end
// + sweep) runs beside an upload.  Returns at once.
int cs_batch_refill_gray(cs_detector* d, cs_batch* b, const unsigned char* const* grays) {
  if (!d || !b || !grays || b->det != d) return CS_ERR_INVALID_ARG;
  if (!b->gray_batch) { cs_set_error("cs_batch_refill_gray: the batch was not created by cs_batch_create_gray"); return CS_ERR_INVALID_ARG; }
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(d->device));
  const size_t px = (size_t)b->gray_w * b->gray_h;
  const int n = b->n_frames;
  if (n <= 0 || px == 0) return CS_OK;
  int rc;
  if ((rc = b->d_gray2.ensure(px * (size_t)n))) return rc;
  if (b->n_refill == 2) { cs_set_error("cs_batch_refill_gray: two uploads are queued already (one per image buffer); cs_batch_submit / cs_batch_run takes the older one"); return CS_ERR_INVALID_ARG; }
  if (!b->copy_stream) {
    // (lowest priority: bulk traffic, and a hardware queue of its own)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    CS_TRY(b->copy_stream.create(hipStreamNonBlocking, prio_least));
    for (auto& e : b->ev_copied) CS_TRY(e.create(hipEventDisableTiming));
    for (auto& e : b->ev_edge_done) CS_TRY(e.create(hipEventDisableTiming));
    CS_HIP_TRY(hipEventRecord(b->ev_edge_done[0], d->stream));      // buffer 0's reader so far: the front end of cs_batch_create_gray (finished)
    CS_HIP_TRY(hipEventRecord(b->ev_edge_done[1], d->stream));
  }
  // Which buffer: the one that is neither being read (gray_cur, or -- with an upload already queued -- that upload's target, which the next
  // submit's front end reads) ...  With one upload queued the new one goes BEHIND it on the copy stream into the buffer of the current maps:
  // the stream never idles between two batches of images, whatever the host does in between.
  const int nxt = b->n_refill == 1 ? 1 - b->refill_q[0] : 1 - b->gray_cur;
  unsigned char* dst = nxt ? b->d_gray2.p : b->d_gray.p;
  // the buffer's last reader -- the front end queued when it became current -- must be through before it is overwritten
  CS_HIP_TRY(hipStreamWaitEvent(b->copy_stream, b->ev_edge_done[nxt], 0));
  // images that follow each other in host memory go up as one copy (a batch decoded into one pinned block: a single DMA)
  for (int f = 0; f < n;) {
    int g = f + 1;
    while (g < n && grays[g] == grays[g - 1] + px) g++;
    // The copy engine, not the shader cores: a kernel that reads pinned host memory keeps hundreds of PCIe reads in flight through the same
    // request queues the other kernels' HBM traffic takes -- with it beside them the distance transform ran 0.8 -> 7.7 ms and Canny
    // 2.4 -> 7.5 ms (profiles/r6_image_in_timeline.txt); the engine's 8.3 ms for 467 MB is the same and costs the kernels nothing.
    CS_HIP_TRY(hipMemcpyAsync(dst + (size_t)f * px, grays[f], px * (size_t)(g - f), hipMemcpyHostToDevice, b->copy_stream));
    f = g;
  }
  CS_HIP_TRY(hipEventRecord(b->ev_copied[nxt], b->copy_stream));
  b->refill_q[b->n_refill++] = nxt;
  return CS_OK;
  CS_GUARD_END("cs_batch_refill_gray")
}
// The front end over freshly uploaded images, queued by the next cs_batch_submit / cs_batch_run: the HOST waits for the upload and then queues
// the kernels.  (First form: the detector's stream waited for the copy's event on the device.  A wait that sits in a hardware queue for the
// 8 ms of a 467 MB upload blocks every stream the runtime maps to that queue -- the tie boxes' gather on the detector's second stream
// waited behind it and a step took 16.7 ms instead of 8.3.)
static int batch_flush_refill(cs_detector* d, cs_batch* b) {
  if (b->n_refill == 0) return CS_OK;
  const int nxt = b->refill_q[0];
  CS_HIP_TRY(hipEventSynchronize(b->ev_copied[nxt]));
  hipStream_t st = d->stream;
  if (b->edge_n_rois > 0) {
    cs::launch_edge_maps(nxt ? b->d_gray2.p : b->d_gray.p, b->gray_w, b->gray_h, b->d_edge_rois.p, b->edge_n_rois, b->d_cls.p, b->d_maps.p, b->edge_max_w, b->edge_max_px, 80, 200, st);
    CS_HIP_TRY(hipGetLastError());
  }
  CS_HIP_TRY(hipEventRecord(b->ev_edge_done[nxt], st));
  b->gray_cur = nxt;
  b->refill_q[0] = b->refill_q[1]; b->refill_q[1] = -1; b->n_refill--;
  return CS_OK;
}
// ... and wait for the upload only (the host images may be reused / freed from here; the front end may still be queued)
int cs_batch_refill_wait(cs_batch* b) {
  if (!b) return CS_ERR_INVALID_ARG;
  if (!b->copy_stream) return CS_OK;
  CS_HIP_TRY(hipSetDevice(b->det->device));
  CS_HIP_TRY(hipStreamSynchronize(b->copy_stream));
  return CS_OK;
}

int cs_batch_max_boxes(const cs_batch* b) { return b ? b->max_boxes : CS_ERR_INVALID_ARG; }

static void batch_drop_run_state(cs_batch* b);
void cs_batch_destroy(cs_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->det->device);
  if (b->run_state) { (void)hipDeviceSynchronize(); batch_drop_run_state(b); }   // a submitted sweep that was never collected
  for (PipeSlot& S : b->pipe) S.uncount(b->det);
  delete b;
}

int cs_batch_set_debug(cs_batch* b, int enable) {
  if (!b) return CS_ERR_INVALID_ARG;
  b->debug = (enable & 1) != 0;
  b->force_host_rank = (enable & 2) != 0;
  b->force_host_setup = (enable & 4) != 0;
  b->force_no_pipeline = (enable & 8) != 0;
  return CS_OK;
}

}  // extern "C"


// ================================================================== pipelined production path =====
// No roll/pitch sampling, no debug retention: boxes are independent, line setup and ranking run on the device, and
// nothing but the winners comes back.  The batch is cut into chunks that flow through a two-slot software pipeline:
// while the GPU sweeps chunk k, the host packs chunk k+1 and writes the records of chunk k-1.
namespace {

struct PipeCtx {
  cs_detector* d; cs_batch* b; OutView O;
  const std::vector<CamCache>* cam_raw; const std::vector<int>* rp_off;
  cs::SweepParams sp; cs_detect_timing* tm;
  const std::vector<std::vector<CamCache>>* cam_rp_all = nullptr;
};

}  // namespace
struct BatchRunState {
  std::vector<CamCache> cam_raw;
  std::vector<std::vector<CamCache>> cam_rp;
  std::vector<int> rp_off;
  cs_detect_timing tm{};
  double t_begin = 0;
  PipeCtx C{};
  bool rp_lean = false;     // ... of the lean roll/pitch path (rp_launch / rp_finish)
};
namespace {

// CS_DETECT_PROF: phase k of detector d's host clock (cs_detector::prof_mark)
// the device time between two events of a finished sweep, onto a timing field
int add_elapsed(double& field, hipEvent_t a, hipEvent_t b) { float ms = 0; CS_HIP_TRY(hipEventElapsedTime(&ms, a, b)); field += ms; return CS_OK; }
#define MARK(k, t_ref) do { if (d->prof) { double t_now = now_ms(); d->prof_mark[k] += t_now - (t_ref); (t_ref) = t_now; } } while (0)

// The tie boxes of a finished sweep (B.h_fallback; B.h_job_cbase / h_job_valid say where their columns lie) get the exact ranking on the
// host: enqueue_columns, wait, rank(q) per box on any thread, enqueue_corners, wait, corners(q, r) -- enqueue and wait apart, so that a
// caller can work while something travels.  The gather kernels read the lists from, and write the rows to, B's pinned host pools themselves
// (coalesced rows; no copy engine between the device and a host that is waiting for a few kilobytes).
struct TiePass {
  SweepBuffers& B; const cs::DetectDeviceView& v; hipStream_t st;
  const int *box_job0, *box_njobs;                   // the sweep's box table, on the host
  std::vector<int> boxes;                            // the flagged boxes
  std::vector<long long> col0_of_job;                // first fetched row of a flagged box's job
  std::vector<std::vector<ExactWinner>> winners;     // per box of the sweep (filled for the flagged ones)
  std::vector<size_t> corner0;                       // per box: first of its winners in h_win_corners
  TiePass(SweepBuffers& B_, const cs::DetectDeviceView& v_, hipStream_t st_, const int* job0, const int* njobs, size_t nj, size_t nb)
      : B(B_), v(v_), st(st_), box_job0(job0), box_njobs(njobs), col0_of_job(nj, -1), winners(nb), corner0(nb, 0) {
    for (size_t q = 0; q < nb; q++) if (B.h_fallback.p[q]) boxes.push_back((int)q);
  }
  int enqueue_columns() {
    size_t nr = 0, z = 0;
    long long tot = 0;
    for (int q : boxes) nr += (size_t)box_njobs[q];
    if (boxes.empty()) return CS_OK;
    CS_ENSURE(B.h_fb_src, nr); CS_ENSURE(B.h_fb_dst, nr); CS_ENSURE(B.h_fb_cnt, nr);
    for (int q : boxes)
      for (int j = box_job0[q]; j < box_job0[q] + box_njobs[q]; j++, z++) {
        B.h_fb_src.p[z] = B.h_job_cbase.p[j]; B.h_fb_cnt.p[z] = B.h_job_valid.p[j]; B.h_fb_dst.p[z] = col0_of_job[j] = tot;
        tot += B.h_job_valid.p[j];
      }
    CS_ENSURE(B.h_fb_dist, tot + 1); CS_ENSURE(B.h_fb_angle, tot + 1); CS_ENSURE(B.h_fb_skew, tot + 1); CS_ENSURE(B.h_fb_flag, tot + 1); CS_ENSURE(B.h_fb_slot, tot + 1);
    cs::launch_gather_ranges(v, B.h_fb_src.p, B.h_fb_cnt.p, B.h_fb_dst.p, (int)nr, B.h_fb_dist.p, B.h_fb_angle.p, B.h_fb_skew.p, B.h_fb_flag.p, B.h_fb_slot.p, st);
    return CS_OK;
  }
  int wait() { if (!boxes.empty()) { CS_HIP_TRY(hipGetLastError()); CS_HIP_TRY(hipStreamSynchronize(st)); } return CS_OK; }      // (no tie box: no call into the runtime)
  // the exact winners of flagged box q into winners[q]; returns the last kept slot of its last height sample (exact_rank_box)
  long long rank(size_t q, const RankWeights& RW, int kmax) {
    HeightCols cols[3];
    for (int h = 0; h < box_njobs[q]; h++) cols[h] = B.fb_cols(col0_of_job[box_job0[q] + h], B.h_job_valid.p[box_job0[q] + h]);
    return exact_rank_box(cols, box_njobs[q], RW, kmax, winners[q]);
  }
  int enqueue_corners(const cs::SweepParams& sp) {
    size_t nw = 0;
    for (int q : boxes) { corner0[q] = nw; nw += winners[q].size(); }
    if (nw == 0) return CS_OK;
    CS_ENSURE(B.h_win_slots, nw); CS_ENSURE(B.h_win_corners, 16 * nw);
    for (int q : boxes) for (size_t r = 0; r < winners[q].size(); r++) B.h_win_slots.p[corner0[q] + r] = winners[q][r].slot;
    cs::launch_gather_corners(v, sp, B.h_win_slots.p, (int)nw, B.h_win_corners.p, st);
    return CS_OK;
  }
  const double* corners(size_t q, size_t r) const { return B.h_win_corners.p + 16 * (corner0[q] + r); }
};

int pipe_launch(PipeCtx& C, PipeSlot& S, int f0, int f1) {
  cs_detector* d = C.d; cs_batch* b = C.b;
  const cs_detect_params& P = d->prm;
  hipStream_t st = d->stream;
  const int KMAX = P.max_cuboid_num;
  double t0 = now_ms(), tq = t0;
  CS_TRY(S.begin());
  const int nf = f1 - f0;
  // ---- per frame, in parallel and straight into the pinned staging pools: job descriptors + sample lists (everything
  // else of the setup happens in the line setup kernels).  The pools use a capacity layout fixed by the inputs (a frame's
  // jobs, yaw samples and top-edge samples have known upper bounds), so no frame waits for another one's counts; a
  // box the reference skips (:215) leaves null jobs (Y = T = 0) that own no slots.
  const int jb0 = b->job_base[f0], bx0 = b->box_base[f0], tp0 = b->top_base[bx0];
  const long long ln0 = b->line_base[f0];
  const size_t nj = (size_t)(b->job_base[f1] - jb0), n_lines = (size_t)(b->line_base[f1] - ln0);
  const int YCAP = yaw_list_capacity(P.yaw_range_deg, P.yaw_step_deg);
  const size_t n_yaw = (size_t)nf * YCAP, n_top = (size_t)(b->top_base[b->box_base[f1]] - tp0);
  if ((long long)nj * 1 > 0x7fffffffLL || (long long)n_lines > 0x7fffffffLL) { cs_set_error("chunk too large"); return CS_ERR_CAPACITY; }
  S.nj = nj;
  if (nj == 0) { S.nb = 0; S.slot_total = 0; S.vp_total = 0; C.tm->setup_host_ms += now_ms() - t0; return S.mark_in_flight(d, st); }
  CS_ENSURE(S.h_jobs_in, nj); CS_ENSURE(S.h_slot_prefix, nj + 1); CS_ENSURE(S.h_vp_prefix, nj + 1); CS_ENSURE(S.h_yaw, n_yaw + 1); CS_ENSURE(S.h_yaw_c, n_yaw + 1); CS_ENSURE(S.h_yaw_s, n_yaw + 1);
  CS_ENSURE(S.h_top_x, n_top + 1); CS_ENSURE(S.h_box_job0, nj); CS_ENSURE(S.h_box_njobs, nj); CS_ENSURE(S.h_ls_order, nj);
  std::atomic<int> overflow{0};
  d->pool->run(nf, [&](int q) {
    const int f = f0 + q;
    const FrameIn& F = b->frames[f];
    cs::JobDesc* jout = S.h_jobs_in.p + (b->job_base[f] - jb0);
    double* yw = S.h_yaw.p + (size_t)q * YCAP; double* yc = S.h_yaw_c.p + (size_t)q * YCAP; double* ys = S.h_yaw_s.p + (size_t)q * YCAP;
    int nY = -1, ji = 0;
    for (int bi = 0; bi < F.n_boxes; bi++) {
      const double* bb = &F.boxes[5 * bi];
      const bool swept = top_sample_step(bb) >= 1;
      const int tb = b->top_base[b->box_base[f] + bi] - tp0;
      if (swept && nY < 0) {  // cam_pose never changes without roll/pitch sampling: one yaw list per frame (:180-184)
        nY = fill_yaw_list((*C.cam_raw)[f].cam_yaw, P.yaw_range_deg, P.yaw_step_deg, YCAP, yw, yc, ys);
        if (nY < 0) { overflow = 1; nY = 0; }
      }
      const int nT = top_samples(bb, S.h_top_x.p + tb);      // (as many as batch_layout reserved: top_base counts them by the same rule)
      for (int k = 0; k < F.n_heights[bi]; k++) {
        cs::JobDesc jd;
        fill_job_geometry(jd, F, bi, k, (*C.rp_off)[f]);
        jd.frame = f; jd.Y = swept ? nY : 0; jd.T = nT; jd.RP = 1;
        jd.yaw_off = q * YCAP; jd.top_off = tb;
        jd.line_off = (int)(b->line_base[f] - ln0) + ji * F.n_lines;
        jout[ji++] = jd;
      }
    }
  });
  if (overflow) { cs_set_error("yaw sample list exceeds its capacity"); return CS_ERR_CAPACITY; }
  MARK(0, tq);   // per-frame jobs + sample lists
  // ---- slot / vanishing-point prefixes and the box table: one serial pass over the jobs
  size_t nb = 0;
  long long real_slots = 0;      // proposals (the slot space itself is padded per job)
  {
    JobSpan at{0, 0};
    for (size_t j = 0; j < nj; j++) {
      cs::JobDesc& jd = S.h_jobs_in.p[j];
      const JobSpan own = span_padded(jd);
      jd.slot_off = S.h_slot_prefix.p[j] = at.slots; jd.vp_off = S.h_vp_prefix.p[j] = (int)at.vps;
      real_slots += span_exact(jd).slots; at.slots += own.slots; at.vps += own.vps;
      // (the null jobs of a box the reference skips open no box)
      if (jd.hid == 0 && jd.Y > 0 && jd.T > 0) { S.h_box_job0.p[nb] = (int)j; S.h_box_njobs.p[nb++] = b->frames[jd.frame].n_heights[jd.box]; }
    }
    S.h_slot_prefix.p[nj] = S.slot_total = at.slots; S.h_vp_prefix.p[nj] = S.vp_total = (int)at.vps;
    line_setup_order(S.h_jobs_in.p, nj, b->frames, S.h_ls_order.p);
    if (at.vps > 0x7fffffffLL) { cs_set_error("too many yaw samples in one chunk"); return CS_ERR_CAPACITY; }
  }
  S.nb = nb;
  MARK(1, tq);   // prefixes + box table
  C.tm->setup_host_ms += now_ms() - t0;
  C.tm->n_jobs += (long long)nj; C.tm->n_slots += real_slots;
  // ---- device buffers, H2D, kernels, D2H: all asynchronous on the detector's stream
  const long long slot_total = S.slot_total;
  SweepBuffers& B = S.sb;
  CS_TRY(B.ensure_tables(nj, nj + 1, n_lines, n_yaw, n_top, (size_t)S.vp_total, nb, KMAX)); CS_TRY(B.ensure_slots(slot_total));
  CS_ENSURE(B.bound3, nj * (size_t)cs::vp3_table_doubles_per_job());
  CS_ENSURE(S.ls_order, nj); CS_ENSURE(S.blk_info, 2 * (size_t)(slot_total >> 8) + 4); CS_ENSURE(S.ls_crowded, 2 * (nj + 1) + 2);
  CS_ENSURE(S.records, nb * KMAX + 1); CS_ENSURE(S.h_records, nb * KMAX + 1); CS_ENSURE(S.h_jobs_out, nj);
  // the tables' device addresses: the slot's own buffers, or -- a call of a frame or two, where ten copies of a few hundred bytes cost ten
  // launch latencies (~150 us of a 0.46 ms call) -- pieces of ONE block that goes up in one copy
  cs::DetectDeviceView& v = S.view;
  cs::RankView rv{};
  rv.box_job0 = B.box_job0.p; rv.box_njobs = B.box_njobs.p; rv.n_boxes = (int)nb; rv.winners = B.winners.p; rv.win_count = B.win_count.p; rv.fallback = B.fallback.p;
  int* p_ls_order = S.ls_order.p; cs_cuboid* p_records = S.records.p;
  // from the first launch to the `done` record: this batch's launches, back to back in the shared streams (StreamSet::enqueue_mu; asynchronous
  // calls only)
  std::unique_lock<std::mutex> enqueue(d->streams->enqueue_mu, std::defer_lock);
  S.merged_io = nj <= SMALL_CALL_JOBS;
  if (S.merged_io) {
    const SmallCallArena& A = S.arena = SmallCallArena(nj, n_yaw, n_top, nb, KMAX);
    CS_ENSURE(S.tab_arena, A.o_end + 256); CS_ENSURE(S.h_tab_arena, A.o_end + 256);
    unsigned char *hb = S.h_tab_arena.p, *db = S.tab_arena.p;
    memcpy(hb + A.o_ls, S.h_ls_order.p, sizeof(int) * nj); memcpy(hb + A.o_jobs, S.h_jobs_in.p, sizeof(cs::JobDesc) * nj);
    memcpy(hb + A.o_sp, S.h_slot_prefix.p, sizeof(long long) * (nj + 1)); memcpy(hb + A.o_vp, S.h_vp_prefix.p, sizeof(int) * (nj + 1));
    if (n_yaw) { memcpy(hb + A.o_y, S.h_yaw.p, 8 * n_yaw); memcpy(hb + A.o_yc, S.h_yaw_c.p, 8 * n_yaw); memcpy(hb + A.o_ys, S.h_yaw_s.p, 8 * n_yaw); }
    if (n_top) memcpy(hb + A.o_tx, S.h_top_x.p, sizeof(int) * n_top);
    if (nb) { memcpy(hb + A.o_b0, S.h_box_job0.p, sizeof(int) * nb); memcpy(hb + A.o_bn, S.h_box_njobs.p, sizeof(int) * nb); }
    if (!d->streams->own_streams) enqueue.lock();
    CS_HIP_TRY(hipMemcpyAsync(db, hb, A.in_end, hipMemcpyHostToDevice, st));
    B.bind(v, *b, nj, 0, 0, db, &A);
    p_ls_order = reinterpret_cast<int*>(db + A.o_ls); p_records = reinterpret_cast<cs_cuboid*>(db + A.o_rec);
    rv.box_job0 = reinterpret_cast<int*>(db + A.o_b0); rv.box_njobs = reinterpret_cast<int*>(db + A.o_bn);
    rv.win_count = reinterpret_cast<int*>(db + A.o_wc); rv.fallback = reinterpret_cast<int*>(db + A.o_fb);
  } else {
    // a batch's tables: one kernel reads all ten out of the pinned staging pools (no copy-engine ring in the sweep: see multi_copy_kernel)
    cs::CopySegs cp{};
    cs::add_copy(cp, S.ls_order, S.h_ls_order, nj); cs::add_copy(cp, B.jobs, S.h_jobs_in, nj); cs::add_copy(cp, B.slot_prefix, S.h_slot_prefix, nj + 1);
    cs::add_copy(cp, B.vp_prefix, S.h_vp_prefix, nj + 1); cs::add_copy(cp, B.yaw, S.h_yaw, n_yaw); cs::add_copy(cp, B.yaw_c, S.h_yaw_c, n_yaw);
    cs::add_copy(cp, B.yaw_s, S.h_yaw_s, n_yaw); cs::add_copy(cp, B.top_x, S.h_top_x, n_top); cs::add_copy(cp, B.box_job0, S.h_box_job0, nb);
    cs::add_copy(cp, B.box_njobs, S.h_box_njobs, nb);
    if (!d->streams->own_streams) enqueue.lock();
    cs::launch_multi_copy(cp, st);
    B.bind(v, *b, nj);
  }
  // The corner construction needs the vanishing points but not the segments: it runs on the second stream (where this block has one:
  // otherwise stB == st and the cross-stream waits are not enqueued) beside line
  // setup + VP support (a latency-bound and an ALU-bound kernel), and the scorer waits for both.
  hipStream_t stB = nullptr, stC = nullptr;
  sweep_side_streams(d, &stB, &stC);
  if (stB != st) {
    CS_HIP_TRY(hipEventRecord(S.ev[7], st));                      // inputs resident
    CS_HIP_TRY(hipStreamWaitEvent(stB, S.ev[7], 0));
  }
  CS_HIP_TRY(hipEventRecord(S.ev[8], stB));
  // vanishing points, corner construction and ordered compaction of a job in one workgroup (candidate_compact_kernel); the compacted rows
  // of job j start at slot_prefix[j]: no scan over all jobs between this kernel and the scorer
  v.blk_info = S.blk_info.p;
  CS_HIP_TRY(hipMemsetAsync(S.blk_info.p, 0, sizeof(int), stB));
  cs::launch_candidate_compact(v, C.sp, stB);
  CS_HIP_TRY(hipEventRecord(S.ev[9], stB));
  CS_HIP_TRY(hipEventRecord(S.ev[10], stB));
  CS_HIP_TRY(hipEventRecord(S.ev[0], st));
  cs::launch_line_setup_listed(const_cast<cs::JobDesc*>(v.jobs), (int)nj, b->d_frame_lines.p, b->d_frame_line_ptr.p, B.mid_x.p, B.mid_y.p, B.ang.p, P.pre_merge_dist_thre, P.pre_merge_angle_thre, P.edge_length_threshold, st, p_ls_order,
                               stC, S.ev[0], S.ev[12], S.ls_crowded.p);
  CS_HIP_TRY(hipEventRecord(S.ev[1], st));
  cs::launch_vp_support_only(v, C.sp, S.vp_total, st, 1);      // (this path's jobs have one roll/pitch sample: jd.RP = 1 above)
  CS_HIP_TRY(hipEventRecord(S.ev[2], st));
  if (stB != st) CS_HIP_TRY(hipStreamWaitEvent(st, S.ev[10], 0));
  CS_HIP_TRY(hipEventRecord(S.ev[4], st));
  cs::launch_score(v, C.sp, slot_total, slot_total, st);
  CS_HIP_TRY(hipEventRecord(S.ev[5], st));
  const cs::RankParams rkp = rank_params(P, C.sp);
  cs::launch_rank(v, rv, rkp, st, 0, false);          // (the host reads no winner of the device: record_kernel rebuilds their corners)
  cs::launch_records(v, rv, KMAX, p_records, st, nullptr, rkp.short_sq_bound);     // the records of the boxes the device ranked: only they come back
  CS_HIP_TRY(hipEventRecord(S.ev[6], st));
  CS_HIP_TRY(hipGetLastError());
  if (S.merged_io) {
    CS_HIP_TRY(hipMemcpyAsync(S.h_tab_arena.p + S.arena.o_jobs, S.tab_arena.p + S.arena.o_jobs, S.arena.o_end - S.arena.o_jobs, hipMemcpyDeviceToHost, st));   // unpacked in pipe_finish
  } else {   // the results: written to the pinned host pools by one kernel
    cs::CopySegs cp{};
    cs::add_copy(cp, S.h_records, S.records, nb * KMAX); cs::add_copy(cp, B.h_win_count, B.win_count, nb); cs::add_copy(cp, B.h_fallback, B.fallback, nb);
    cs::add_copy(cp, B.h_job_valid, B.job_valid, nj); cs::add_copy(cp, B.h_job_cbase, B.job_cbase, nj + 1);      // (the job table itself is not read back: pipe_finish works from the host's own copy)
    cs::launch_multi_copy(cp, st);
  }
  CS_TRY(S.mark_in_flight(d, st));
  MARK(3, tq);   // allocations + enqueue of copies and kernels
  return CS_OK;
}

int pipe_finish(PipeCtx& C, PipeSlot& S, const std::vector<std::vector<CamCache>>& cam_rp) {
  cs_detector* d = C.d; cs_batch* b = C.b;
  const cs_detect_params& P = d->prm;
  const int KMAX = P.max_cuboid_num;
  cs_detect_timing& tm = *C.tm;
  double tq = now_ms();
  CS_TRY(S.wait(d, tm));
  const size_t nj = S.nj, nb = S.nb;
  if (nj == 0) return CS_OK;
  SweepBuffers& B = S.sb;
  if (S.merged_io) {     // a small call's results came back in one block (pipe_launch): to the places the rest of this function reads
    const unsigned char* hb = S.h_tab_arena.p;
    const SmallCallArena& A = S.arena;
    memcpy(S.h_jobs_out.p, hb + A.o_jobs, sizeof(cs::JobDesc) * nj);
    if (nb) { memcpy(S.h_records.p, hb + A.o_rec, sizeof(cs_cuboid) * nb * KMAX); memcpy(B.h_win_count.p, hb + A.o_wc, sizeof(int) * nb); memcpy(B.h_fallback.p, hb + A.o_fb, sizeof(int) * nb); }
    memcpy(B.h_job_valid.p, hb + A.o_jv, sizeof(int) * nj); memcpy(B.h_job_cbase.p, hb + A.o_cb, sizeof(long long) * (nj + 1));
  }
  double t0 = now_ms();
  {
    CS_TRY(add_elapsed(tm.line_setup_ms, S.ev[0], S.ev[1]));
    CS_TRY(add_elapsed(tm.vp_kernel_ms, S.ev[1], S.ev[2]));
    CS_TRY(add_elapsed(tm.cand_kernel_ms, S.ev[8], S.ev[9]));    // second stream: vanishing points + corners
    CS_TRY(add_elapsed(tm.compact_ms, S.ev[9], S.ev[10]));
    CS_TRY(add_elapsed(tm.score_kernel_ms, S.ev[4], S.ev[5]));
    CS_TRY(add_elapsed(tm.rank_kernel_ms, S.ev[5], S.ev[6]));
    tm.cand_kernel_launches += 1;
    long long n_valid = 0;      // (the capacity layout has no running total: job_cbase[j] = slot_prefix[j])
    for (size_t j = 0; j < nj; j++) n_valid += B.h_job_valid.p[j];
    tm.n_valid += n_valid;
    // algorithmic bytes of the corner construction: the vanishing points it writes (48 B each) + 12 bytes (slot id, flag) per VALID proposal
    tm.cand_kernel_bytes += 48LL * S.vp_total + 12LL * n_valid;
    long long sbytes = 96LL * S.vp_total + (28LL + 8LL + 4LL) * n_valid;
    for (size_t j = 0; j < nj; j++) if (S.h_jobs_in.p[j].Y > 0 && S.h_jobs_in.p[j].T > 0) sbytes += 4LL * S.h_jobs_in.p[j].map_w * (S.h_jobs_in.p[j].g.eb - S.h_jobs_in.p[j].g.et);
    tm.score_kernel_bytes += sbytes;
  }
  const cs::JobDesc* jobs = S.h_jobs_in.p;
  MARK(4, tq);   // wait for the GPU + timing bookkeeping
  // ---- boxes the kernel flagged (a tie at a cut or at the top): exact std::partial_sort ranking on the host.  Their
  // columns are fetched on the high-priority stream: the host waits for them while other sweeps (the next chunk's, or another
  // batch's of the same process) fill the device, and these few small kernels should not queue behind those.
  TiePass tie(B, S.view, d->stream_hi, S.h_box_job0.p, S.h_box_njobs.p, nj, nb);
  CS_TRY(tie.enqueue_columns());
  MARK(5, tq);   // tie lists + gather enqueue
  // ---- records of the winners.  The boxes the device ranked are written while the tie boxes' columns travel.
  const std::vector<int>& fbq = tie.boxes;
  auto write_box = [&](size_t q) {
    const cs::JobDesc* bj = jobs + S.h_box_job0.p[q];
    const int f = bj[0].frame;
    write_exact_winners(C.O, b->frames[f], bj, tie.winners[q], S.h_yaw.p, cam_rp[f], (*C.cam_raw)[f].euler, false, corners_at(tie.corners(q, 0)));
  };
  const RankWeights RW = rank_weights(P);
  tm.n_fallback_boxes += (int)fbq.size();
  auto records = [&](int qi) {      // a device-ranked box: its records are complete but for the caller's rectangle
    const size_t q = (size_t)qi;
    if (B.h_fallback.p[q]) return;
    const cs::JobDesc& j0 = jobs[S.h_box_job0.p[q]];
    write_device_records(C.O, b->frames[j0.frame], j0.frame, j0.box, S.h_records.p + q * KMAX, B.h_win_count.p[q]);
  };
  if (fbq.size() <= 64) {
    // a handful of tie boxes (the usual case): their columns are a few kilobytes and already here; their exact ranking
    // (tens of microseconds each) rides in the same parallel pass as the records of the other boxes, first in the queue
    CS_TRY(tie.wait());
    MARK(7, tq);   // wait for the tie columns
    const int nfb = (int)fbq.size();
    constexpr int RCH = 256;           // records are a 400-byte copy each: hand them out in chunks
    const int nch = ((int)nb + RCH - 1) / RCH;
    d->pool->run(nfb + nch, [&](int z) {
      if (z < nfb) { (void)tie.rank((size_t)fbq[z], RW, KMAX); return; }
      for (int q = (z - nfb) * RCH, q1 = std::min((int)nb, q + RCH); q < q1; q++) records(q);
    });
    MARK(6, tq);   // records of the device-ranked boxes (+ exact ranking of the tie boxes)
  } else {
    d->pool->run((int)nb, records);
    MARK(6, tq);   // records of the device-ranked boxes, written while the tie boxes' columns travel
    CS_TRY(tie.wait());
    MARK(7, tq);   // wait for the tie columns
    d->pool->run((int)fbq.size(), [&](int z) { (void)tie.rank((size_t)fbq[z], RW, KMAX); });
  }
  MARK(8, tq);   // exact ranking of the tie boxes
  CS_TRY(tie.enqueue_corners(C.sp)); CS_TRY(tie.wait());
  MARK(9, tq);   // corners of the tie winners
  if (fbq.size() <= 24) { for (int q : fbq) write_box((size_t)q); }
  else d->pool->run((int)fbq.size(), [&](int z) { write_box((size_t)fbq[z]); });
  MARK(10, tq);  // records of the tie boxes
  tm.finalize_ms += now_ms() - t0;
  return CS_OK;
}

// ================================================================== lean roll/pitch path =========
// whether_sample_cam_roll_pitch = 1 (the reference class's default; main_obj.cpp:623 uses it from the second frame on).  The boxes of a
// frame depend on each other through cam_pose.camera_yaw (box_proposal_detail.cpp:180 reads what :374 / :734 left), so box r of
// every frame forms round r.  The carried value is the camera yaw of one of the frame's RP roll/pitch samples (or the raw pose's before
// the first box): the host lays down all 1 + RP yaw lists of every frame up front -- glibc's cos / sin, as everywhere -- and
// rp_carry_kernel picks the list of the next round on the device.  All rounds are queued back to back; nothing comes back before the
// last one.  Per round the kernels are those of the production path on the round's jobs (slot / vanishing-point numbering relative to
// the round; slots laid out for the longest list a box can get).  A box whose ranking needs the exact host order (a tie that can
// reach the output or the carried proposal) invalidates what the device assumed for the rest of its frame: those frames -- under one
// in a hundred boxes -- are redone through the round-by-round path below, as a small batch that shares this one's distance maps.
int rp_launch(PipeCtx& C, PipeSlot& S, const std::vector<std::vector<CamCache>>& cam_rp) {
  cs_detector* d = C.d; cs_batch* b = C.b;
  const cs_detect_params& P = d->prm;
  hipStream_t st = d->stream;
  const int KMAX = P.max_cuboid_num, NF = b->n_frames, MB = b->max_boxes;
  double t0 = now_ms();
  CS_TRY(S.begin());
  if (!b->rp) b->rp.reset(new RpLean());
  RpLean& R = *b->rp;
  // ---- yaw lists: NT = 1 + max RP per frame, YCAP samples each
  int max_rp = 1;
  for (int f = 0; f < NF; f++) max_rp = std::max(max_rp, (int)cam_rp[f].size());
  const int NT = 1 + max_rp;
  const int YCAP = yaw_list_capacity(P.yaw_range_deg, P.yaw_step_deg);
  const size_t n_yaw = (size_t)NF * NT * YCAP;
  if (n_yaw > 0x7fffffffULL) { cs_set_error("too many yaw samples"); return CS_ERR_CAPACITY; }
  CS_ENSURE(S.h_yaw, n_yaw + 1); CS_ENSURE(S.h_yaw_c, n_yaw + 1); CS_ENSURE(S.h_yaw_s, n_yaw + 1); CS_ENSURE(R.h_tab_count, (size_t)NF * NT + 1); CS_ENSURE(R.h_raw_euler, 3 * (size_t)NF + 1);
  std::atomic<int> overflow{0};
  std::vector<int> ycap_f(NF, 0);     // longest list of the frame: its boxes' slots are laid out for it
  d->pool->run(NF * NT, [&](int z) {
    const int f = z / NT, i = z % NT;
    const int nrp = (int)cam_rp[f].size();
    int* cnt = R.h_tab_count.p + (size_t)f * NT + i;
    *cnt = 0;
    if (i > nrp) return;
    const double cam_yaw = i == 0 ? (*C.cam_raw)[f].cam_yaw : cam_rp[f][i - 1].cam_yaw;
    const size_t at = ((size_t)f * NT + i) * YCAP;
    const int n = fill_yaw_list(cam_yaw, P.yaw_range_deg, P.yaw_step_deg, YCAP, S.h_yaw.p + at, S.h_yaw_c.p + at, S.h_yaw_s.p + at);
    if (n < 0) { overflow = 1; return; }
    *cnt = n;
  });
  if (overflow) { cs_set_error("yaw sample list exceeds its capacity"); return CS_ERR_CAPACITY; }
  for (int f = 0; f < NF; f++) {
    for (int i = 0; i < NT; i++) ycap_f[f] = std::max(ycap_f[f], R.h_tab_count.p[(size_t)f * NT + i]);
    for (int e = 0; e < 3; e++) R.h_raw_euler.p[3 * f + e] = (*C.cam_raw)[f].euler[e];
  }
  // ---- jobs of all rounds: (round, frame, height sample); per round its own slot / vanishing-point numbering
  size_t nj_tot = 0, nb_tot = 0;
  for (int f = 0; f < NF; f++) for (int bi = 0; bi < b->frames[f].n_boxes; bi++) nj_tot += b->frames[f].n_heights[bi];
  const size_t n_top = (size_t)b->top_base[b->box_base[NF]];
  CS_ENSURE(S.h_jobs_in, nj_tot + 1); CS_ENSURE(S.h_slot_prefix, nj_tot + MB + 1); CS_ENSURE(S.h_vp_prefix, nj_tot + MB + 1); CS_ENSURE(S.h_top_x, n_top + 1);
  CS_ENSURE(S.h_box_job0, nj_tot + 1); CS_ENSURE(S.h_box_njobs, nj_tot + 1); CS_ENSURE(S.h_ls_order, nj_tot + 1); CS_ENSURE(R.h_maps, 3 * (size_t)MB * NF + 1);
  R.rounds.assign(MB, RpLean::Round{});
  R.box_frame.clear(); R.box_index.clear();
  size_t ji = 0;
  long long n_lines = 0, slot_cap_max = 0, slots_all = 0, max_job_slots = 0;
  int vp_cap_max = 0;
  size_t nj_round_max = 0;
  for (int r = 0; r < MB; r++) {
    RpLean::Round& Rr = R.rounds[r];
    Rr.j0 = ji; Rr.b0 = nb_tot;
    JobSpan at{0, 0};
    int* box_of = R.h_maps.p + (size_t)(3 * r) * NF; int* job0_of = box_of + NF; int* njobs_of = job0_of + NF;
    for (int f = 0; f < NF; f++) {
      box_of[f] = -1; job0_of[f] = -1; njobs_of[f] = 0;
      const FrameIn& F = b->frames[f];
      if (r >= F.n_boxes) continue;
      const int bi = r;
      const double* bb = &F.boxes[5 * bi];
      if (top_sample_step(bb) < 1) continue;              // :215: the box is skipped and leaves the carried yaw alone
      const int tb = b->top_base[b->box_base[f] + bi];
      const int nT = top_samples(bb, S.h_top_x.p + tb);     // (as many as batch_layout reserved: top_base counts them by the same rule)
      const int nrp = (int)cam_rp[f].size();
      box_of[f] = (int)(nb_tot - Rr.b0); job0_of[f] = (int)(ji - Rr.j0); njobs_of[f] = F.n_heights[bi];
      S.h_box_job0.p[nb_tot] = (int)(ji - Rr.j0); S.h_box_njobs.p[nb_tot++] = F.n_heights[bi];
      R.box_frame.push_back(f); R.box_index.push_back(bi);
      for (int k = 0; k < F.n_heights[bi]; k++) {
        cs::JobDesc jd;
        fill_job_geometry(jd, F, bi, k, (*C.rp_off)[f]);
        jd.frame = f; jd.T = nT; jd.RP = nrp;
        jd.Y = R.h_tab_count.p[(size_t)f * NT];            // list 0 (the raw pose) until rp_carry_kernel says otherwise
        jd.yaw_off = (int)(((size_t)f * NT) * YCAP);
        jd.top_off = tb;
        jd.line_off = (int)n_lines; n_lines += F.n_lines;
        const JobSpan own = span_longest_list(jd, ycap_f[f]);
        jd.slot_off = S.h_slot_prefix.p[ji + r] = at.slots; jd.vp_off = S.h_vp_prefix.p[ji + r] = (int)at.vps;
        max_job_slots = std::max(max_job_slots, own.slots); at.slots += own.slots; at.vps += own.vps;
        S.h_jobs_in.p[ji++] = jd;
      }
    }
    const long long so = at.slots, vo = at.vps;
    Rr.nj = ji - Rr.j0; Rr.nb = nb_tot - Rr.b0; Rr.slot_cap = so; Rr.vp_cap = (int)vo;
    S.h_slot_prefix.p[ji + r] = so; S.h_vp_prefix.p[ji + r] = (int)vo;
    if (vo > 0x7fffffffLL || so > 0x7fffffff00LL) { cs_set_error("too many samples in one round"); return CS_ERR_CAPACITY; }
    slot_cap_max = std::max(slot_cap_max, so); vp_cap_max = std::max(vp_cap_max, (int)vo); nj_round_max = std::max(nj_round_max, Rr.nj);
    slots_all += so;
  }
  const size_t nj = ji, nb = nb_tot;
  S.nj = nj; S.nb = nb; S.slot_total = slots_all; S.vp_total = vp_cap_max;
  if (n_lines > 0x7fffffffLL) { cs_set_error("chunk too large"); return CS_ERR_CAPACITY; }
  for (size_t j = 0; j < nj; j++) S.h_ls_order.p[j] = (int)j;
  C.tm->setup_host_ms += now_ms() - t0;
  C.tm->n_jobs += (long long)nj;
  if (nj == 0) return S.mark_in_flight(d, st);
  // ---- device buffers; the per-round arrays are sized for the largest round and reused from round to round (one stream: in order)
  SweepBuffers& B = S.sb;
  CS_TRY(B.ensure_tables(nj, nj + MB + 1, (size_t)n_lines, n_yaw, n_top, (size_t)vp_cap_max, nb, KMAX)); CS_TRY(B.ensure_slots(slot_cap_max));
  CS_ENSURE(B.flag, slot_cap_max + 1); CS_ENSURE(B.bound3, nj_round_max * (size_t)cs::vp3_table_doubles_per_job() + 1);
  const int max_trips = (int)std::min<long long>((max_job_slots + 4095) / 4096, 1 << 20);      // compaction trips of the largest job (4096 slots each)
  CS_ENSURE(R.trip_cnt, (size_t)nj_round_max * (size_t)std::max(1, max_trips) + 1);
  CS_ENSURE(S.ls_order, nj); CS_ENSURE(S.ls_crowded, 2 * (nj + 1) + 2); CS_ENSURE(R.last_slot, nb + 1);
  CS_ENSURE(S.records, nb * KMAX + 1); CS_ENSURE(S.h_records, nb * KMAX + 1);
  R.pool_cap = std::max<long long>(1 << 18, slots_all / 64);        // columns of the flagged boxes (about one box in a hundred)
  CS_ENSURE(B.fb_dist, (size_t)R.pool_cap + 1); CS_ENSURE(B.fb_angle, (size_t)R.pool_cap + 1); CS_ENSURE(B.fb_skew, (size_t)R.pool_cap + 1); CS_ENSURE(B.fb_flag, (size_t)R.pool_cap + 1); CS_ENSURE(B.fb_slot, (size_t)R.pool_cap + 1);
  CS_ENSURE(R.box_base, nb + 1); CS_ENSURE(R.pool_used, 1); CS_ENSURE(R.h_box_base, nb + 1); CS_ENSURE(R.h_pool_used, 1); CS_ENSURE(R.h_last_slot, nb + 1); CS_ENSURE(S.h_jobs_out, nj + 1);
  CS_ENSURE(R.cur_idx, (size_t)NF + 1); CS_ENSURE(R.tab_count, (size_t)NF * NT + 1); CS_ENSURE(R.maps, 3 * (size_t)MB * NF + 1); CS_ENSURE(R.raw_euler, 3 * (size_t)NF + 1);
  while (R.ev.size() < 5 * (size_t)MB) { R.ev.emplace_back(); if (int rc = R.ev.back().create()) { R.ev.pop_back(); return rc; } }
  std::unique_lock<std::mutex> enqueue(d->streams->enqueue_mu, std::defer_lock);      // all rounds of this batch back to back in the shared streams (see pipe_launch)
  if (!d->streams->own_streams) enqueue.lock();
  hipStream_t stB = nullptr, stC = nullptr;      // (corner construction stays on the chain here: stB is not used)
  sweep_side_streams(d, &stB, &stC);
  CS_HIP_TRY(hipMemsetAsync(R.pool_used.p, 0, sizeof(unsigned long long), st));
  {     // (one kernel reads all thirteen tables out of the pinned pools: multi_copy_kernel)
    cs::CopySegs cp{};
    cs::add_copy(cp, S.ls_order, S.h_ls_order, nj); cs::add_copy(cp, B.jobs, S.h_jobs_in, nj); cs::add_copy(cp, B.slot_prefix, S.h_slot_prefix, nj + MB);
    cs::add_copy(cp, B.vp_prefix, S.h_vp_prefix, nj + MB); cs::add_copy(cp, B.yaw, S.h_yaw, n_yaw); cs::add_copy(cp, B.yaw_c, S.h_yaw_c, n_yaw);
    cs::add_copy(cp, B.yaw_s, S.h_yaw_s, n_yaw); cs::add_copy(cp, B.top_x, S.h_top_x, n_top); cs::add_copy(cp, B.box_job0, S.h_box_job0, nb);
    cs::add_copy(cp, B.box_njobs, S.h_box_njobs, nb); cs::add_copy(cp, R.tab_count, R.h_tab_count, (long long)NF * NT);
    cs::add_copy(cp, R.maps, R.h_maps, 3LL * MB * NF); cs::add_copy(cp, R.raw_euler, R.h_raw_euler, 3LL * NF);
    cs::launch_multi_copy(cp, st);
  }
  CS_HIP_TRY(hipMemsetAsync(B.job_valid.p, 0, sizeof(int) * nj, st));
  CS_HIP_TRY(hipMemsetAsync(R.cur_idx.p, 0, sizeof(int) * NF, st));
  CS_HIP_TRY(hipEventRecord(S.ev[0], st));
  // ---- line setup of every job of the batch at once (it depends on the box and the frame's segments only)
  cs::launch_line_setup_listed(B.jobs.p, (int)nj, b->d_frame_lines.p, b->d_frame_line_ptr.p, B.mid_x.p, B.mid_y.p, B.ang.p, P.pre_merge_dist_thre, P.pre_merge_angle_thre, P.edge_length_threshold, st, S.ls_order.p,
                               stC, S.ev[0], S.ev[12], S.ls_crowded.p);
  CS_HIP_TRY(hipEventRecord(S.ev[1], st));
  const cs::RankParams rkp = rank_params(P, C.sp);
  for (int r = 0; r < MB; r++) {
    const RpLean::Round& Rr = R.rounds[r];
    if (Rr.nj == 0) continue;
    const auto re = R.ev.begin() + 5 * (size_t)r;
    cs::DetectDeviceView v;
    B.bind(v, *b, Rr.nj, Rr.j0, Rr.j0 + r);      // (the prefixes carry one closing entry per earlier round)
    if (r > 0) {      // the carried yaw: this round's jobs get the list the previous round's result selects
      // (the previous round WITH jobs decides for the frames it held a box of; a frame without a box there keeps its list)
      int rq = r - 1;
      while (rq > 0 && R.rounds[rq].nj == 0) rq--;
      const RpLean::Round& Rq = R.rounds[rq];
      cs::RpCarryView c{};
      c.n_frames = NF; c.NT = NT; c.YCAP = YCAP;
      c.prev_box_of_frame = Rq.nj ? R.maps.p + (size_t)(3 * rq) * NF : nullptr;
      c.prev_last_slot = R.last_slot.p + Rq.b0; c.prev_jobs = B.jobs.p + Rq.j0; c.prev_box_job0 = B.box_job0.p + Rq.b0; c.prev_box_njobs = B.box_njobs.p + Rq.b0;
      c.job0_of_frame = R.maps.p + (size_t)(3 * r + 1) * NF; c.njobs_of_frame = R.maps.p + (size_t)(3 * r + 2) * NF;
      c.tab_count = R.tab_count.p; c.cur_idx = R.cur_idx.p;
      cs::launch_rp_carry(c, B.jobs.p + Rr.j0, st);
    }
    CS_HIP_TRY(hipEventRecord(re[0], st));
    cs::launch_vp_points(v, Rr.vp_cap, st);
    cs::launch_candidates(v, C.sp, Rr.slot_cap, st);
    cs::launch_scan_compact_trips(v, R.trip_cnt.p, max_trips, st);
    CS_HIP_TRY(hipEventRecord(re[1], st));
    cs::launch_vp_support_only(v, C.sp, Rr.vp_cap, st);
    CS_HIP_TRY(hipEventRecord(re[2], st));
    cs::launch_score(v, C.sp, Rr.slot_cap, Rr.slot_cap, st);
    CS_HIP_TRY(hipEventRecord(re[3], st));
    cs::RankView rv{};
    rv.box_job0 = B.box_job0.p + Rr.b0; rv.box_njobs = B.box_njobs.p + Rr.b0; rv.n_boxes = (int)Rr.nb; rv.winners = B.winners.p + Rr.b0 * KMAX;
    rv.win_count = B.win_count.p + Rr.b0; rv.fallback = B.fallback.p + Rr.b0; rv.last_slot = R.last_slot.p + Rr.b0;
    cs::launch_rank(v, rv, rkp, st, Rr.nb ? (long long)(Rr.slot_cap / (long long)Rr.nb) : 0, false);      // (average slots per box of the round: which instance ranks)
    cs::launch_records(v, rv, KMAX, S.records.p + Rr.b0 * KMAX, st, R.raw_euler.p, rkp.short_sq_bound);
    {   // the flagged boxes' columns, before the next round reuses the arrays
      cs::RpSaveView sv{};
      sv.fallback = rv.fallback; sv.box_job0 = rv.box_job0; sv.box_njobs = rv.box_njobs; sv.n_boxes = rv.n_boxes; sv.pool_used = R.pool_used.p; sv.pool_cap = R.pool_cap;
      sv.box_base = R.box_base.p + Rr.b0; sv.p_dist = B.fb_dist.p; sv.p_angle = B.fb_angle.p; sv.p_skew = B.fb_skew.p; sv.p_flag = B.fb_flag.p; sv.p_slot = B.fb_slot.p;
      cs::launch_rp_save_fallback(v, sv, st);
    }
    CS_HIP_TRY(hipEventRecord(re[4], st));
    CS_HIP_TRY(hipGetLastError());
  }
  CS_HIP_TRY(hipEventRecord(S.ev[6], st));
  {
    cs::CopySegs cp{};
    cs::add_copy(cp, S.h_records, S.records, nb * KMAX); cs::add_copy(cp, B.h_win_count, B.win_count, nb); cs::add_copy(cp, B.h_fallback, B.fallback, nb);
    cs::add_copy(cp, B.h_job_cbase, B.job_cbase, nj + MB); cs::add_copy(cp, B.h_job_valid, B.job_valid, nj); cs::add_copy(cp, S.h_jobs_out, B.jobs, nj);
    cs::add_copy(cp, R.h_last_slot, R.last_slot, nb); cs::add_copy(cp, R.h_box_base, R.box_base, nb); cs::add_copy(cp, R.h_pool_used, R.pool_used, 1);
    cs::launch_multi_copy(cp, st);
  }
  return S.mark_in_flight(d, st);
}

// The lean roll/pitch path's redo: frames `ids` of C's batch again, as a small batch through the round-by-round path (force_round_path) that
// reads the parent's map pool at the same offsets; its records and counts go to the parent's output.
int rp_redo_frames(PipeCtx& C, const std::vector<int>& ids) {
  cs_detector* d = C.d; const cs_batch* b = C.b;
  cs_batch sub;
  sub.det = d; sub.force_round_path = true; sub.maps = b->maps; sub.n_frames = (int)ids.size();
  for (int f : ids) { sub.frames.push_back(b->frames[f]); sub.max_boxes = std::max(sub.max_boxes, b->frames[f].n_boxes); }
  CS_TRY(batch_layout(d, &sub));
  std::vector<cs_cuboid> o2(ids.size() * std::max(1, sub.max_boxes) * C.O.kmax);
  std::vector<int> c2(ids.size() * std::max(1, sub.max_boxes), 0);
  const OutView O2{o2.data(), c2.data(), sub.max_boxes, C.O.kmax};
  CS_TRY(batch_run_impl(d, &sub, O2.out, O2.out_counts, false));
  for (size_t z = 0; z < ids.size(); z++) {
    const int f = ids[z];
    for (int bi = 0; bi < b->frames[f].n_boxes; bi++) {
      const int nw = O2.count((int)z, bi);
      C.O.count(f, bi) = nw;
      for (int r = 0; r < nw; r++) C.O.rec(f, bi, r) = O2.rec((int)z, bi, r);
    }
  }
  return CS_OK;
}

int rp_finish(PipeCtx& C, PipeSlot& S) {
  cs_detector* d = C.d; cs_batch* b = C.b;
  const cs_detect_params& P = d->prm;
  const int KMAX = P.max_cuboid_num, MB = b->max_boxes, NF = b->n_frames;
  cs_detect_timing& tm = *C.tm;
  CS_TRY(S.wait(d, tm));
  if (S.nj == 0) return CS_OK;
  RpLean& R = *b->rp;
  double t0 = now_ms();
  {
    CS_TRY(add_elapsed(tm.line_setup_ms, S.ev[0], S.ev[1]));
    for (int r = 0; r < MB; r++) {
      if (R.rounds[r].nj == 0) continue;
      const auto re = R.ev.begin() + 5 * (size_t)r;
      CS_TRY(add_elapsed(tm.cand_kernel_ms, re[0], re[1]));      // vanishing points, corners, compaction
      CS_TRY(add_elapsed(tm.vp_kernel_ms, re[1], re[2]));
      CS_TRY(add_elapsed(tm.score_kernel_ms, re[2], re[3]));
      CS_TRY(add_elapsed(tm.rank_kernel_ms, re[3], re[4]));      // ranking, records, the flagged boxes' columns
      tm.cand_kernel_launches += 1;
    }
    tm.n_slots += S.slot_total;
    for (int r = 0; r < MB; r++) if (R.rounds[r].nj) tm.n_valid += S.sb.h_job_cbase.p[R.rounds[r].j0 + r + R.rounds[r].nj];
  }
  // ---- the flagged boxes: exact ranking on the host from their saved columns.  A frame is only redone when the exact ranking
  // carries a different camera yaw to the frame's next box than the device assumed (or the columns did not fit the pool).
  std::vector<char> redo(NF, 0);
  std::vector<char> host_done(S.nb, 0);     // box written from the host ranking
  int n_redo = 0;
  size_t n_fb = 0;
  for (size_t q = 0; q < S.nb; q++) n_fb += S.sb.h_fallback.p[q] ? 1 : 0;
  tm.n_fallback_boxes += (int)n_fb;
  if (n_fb) {
    hipStream_t st2 = d->stream_hi;
    const size_t used = (size_t)std::min<unsigned long long>(*R.h_pool_used.p, (unsigned long long)R.pool_cap);
    CS_ENSURE(S.sb.h_fb_dist, used + 1); CS_ENSURE(S.sb.h_fb_angle, used + 1); CS_ENSURE(S.sb.h_fb_skew, used + 1); CS_ENSURE(S.sb.h_fb_flag, used + 1); CS_ENSURE(S.sb.h_fb_slot, used + 1);
    if (used) {
      cs::CopySegs cp{};
      cs::add_copy(cp, S.sb.h_fb_dist, S.sb.fb_dist, used); cs::add_copy(cp, S.sb.h_fb_angle, S.sb.fb_angle, used); cs::add_copy(cp, S.sb.h_fb_skew, S.sb.fb_skew, used);
      cs::add_copy(cp, S.sb.h_fb_flag, S.sb.fb_flag, used); cs::add_copy(cp, S.sb.h_fb_slot, S.sb.fb_slot, used);
      cs::launch_multi_copy(cp, st2);
      CS_HIP_TRY(hipStreamSynchronize(st2));
    }
    const std::vector<std::vector<CamCache>>& cam_rp = *C.cam_rp_all;
    // boxes of a frame in round order
    std::vector<std::vector<size_t>> boxes_of(NF);
    for (size_t q = 0; q < S.nb; q++) boxes_of[R.box_frame[q]].push_back(q);
    auto carry_idx = [](const cs::JobDesc& jl, long long last) { return last < 0 ? jl.RP : 1 + decode_slot(jl, last).rp; };
    const RankWeights RW = rank_weights(P);
    std::vector<int> fb_frames;
    for (int f = 0; f < NF; f++) { bool any = false; for (size_t q : boxes_of[f]) any = any || S.sb.h_fallback.p[q]; if (any) fb_frames.push_back(f); }
    d->pool->run((int)fb_frames.size(), [&](int z) {
      const int f = fb_frames[z];
      const FrameIn& F = b->frames[f];
      for (size_t bq = 0; bq < boxes_of[f].size(); bq++) {
        const size_t q = boxes_of[f][bq];
        if (!S.sb.h_fallback.p[q]) continue;
        const long long base = R.h_box_base.p[q];
        if (base < 0) { redo[f] = 1; return; }
        // which round the box belongs to: its jobs are relative to that round's first job
        size_t r = 0;
        while (r + 1 < R.rounds.size() && q >= R.rounds[r + 1].b0) r++;
        const cs::JobDesc* jobs = S.h_jobs_out.p + R.rounds[r].j0;
        const int* jvalid = S.sb.h_job_valid.p + R.rounds[r].j0;
        const int j0 = S.h_box_job0.p[q], nh = S.h_box_njobs.p[q];
        HeightCols cols[3];
        long long run = base;
        for (int h = 0; h < nh; h++) {
          cols[h] = S.sb.fb_cols(run, jvalid[j0 + h]);
          run += jvalid[j0 + h];
        }
        std::vector<ExactWinner> wl;
        const long long exact_last = exact_rank_box(cols, nh, RW, KMAX, wl);
        double c16[16];      // the winner's corners, rebuilt on the host
        write_exact_winners(C.O, F, jobs + j0, wl, S.h_yaw.p, cam_rp[f], (*C.cam_raw)[f].euler, true, [&](size_t, const cs::JobDesc& jd, const SlotRef& s) {
          host_corners16(cam_rp[f][s.rp].pose.KinvR, S.h_yaw_c.p[jd.yaw_off + s.y], S.h_yaw_s.p[jd.yaw_off + s.y], jd, s, (double)S.h_top_x.p[jd.top_off + s.t], C.sp.short_sq_bound, c16);
          return (const double*)c16;
        });
        host_done[q] = 1;
        // does the frame's next box start from the yaw the device assumed?
        const cs::JobDesc& jl = jobs[j0 + nh - 1];
        if (bq + 1 < boxes_of[f].size() && carry_idx(jl, exact_last) != carry_idx(jl, R.h_last_slot.p[q])) { redo[f] = 1; return; }
      }
    });
    for (int f = 0; f < NF; f++) n_redo += redo[f] ? 1 : 0;
  }
  constexpr int RCH = 256;
  const int nch = ((int)S.nb + RCH - 1) / RCH;
  d->pool->run(nch, [&](int z) {
    for (size_t q = (size_t)z * RCH, q1 = std::min(S.nb, q + RCH); q < q1; q++) {
      const int f = R.box_frame[q], bi = R.box_index[q];
      if (redo[f] || host_done[q]) continue;
      write_device_records(C.O, b->frames[f], f, bi, S.h_records.p + q * KMAX, S.sb.h_win_count.p[q]);
    }
  });
  if (n_redo) {
    std::vector<int> ids;
    for (int f = 0; f < NF; f++) if (redo[f]) ids.push_back(f);
    CS_TRY(rp_redo_frames(C, ids));
    tm.n_redo_frames += n_redo;
  }
  tm.finalize_ms += now_ms() - t0;
  return CS_OK;
}

}  // namespace

extern "C" int cs_batch_set_pipeline_chunks(cs_batch* b, int n_chunks) {
  if (!b || n_chunks < 1) return CS_ERR_INVALID_ARG;
  b->pipe_chunks = n_chunks;
  return CS_OK;
}

static int batch_collect_impl(cs_detector* d, cs_batch* b);
extern "C" int cs_batch_run(cs_detector* d, cs_batch* b, cs_cuboid* out, int* out_counts) {
  CS_GUARD_BEGIN
  return batch_run_impl(d, b, out, out_counts, false);
  CS_GUARD_END("cs_batch_run")
}
// cs_batch_run in two halves: submit packs the batch on the host and queues the whole sweep on the detector's streams, collect waits
// for it and writes the records.  A caller that owns several batches keeps the next one queued while the current one is on the
// device (one submit outstanding per batch; batches of one detector are submitted and collected from one thread, in order).
extern "C" int cs_batch_submit(cs_detector* d, cs_batch* b, cs_cuboid* out, int* out_counts) {
  CS_GUARD_BEGIN
  return batch_run_impl(d, b, out, out_counts, true);
  CS_GUARD_END("cs_batch_submit")
}
extern "C" int cs_batch_collect(cs_detector* d, cs_batch* b) {
  CS_GUARD_BEGIN
  if (!d || !b || b->det != d) return CS_ERR_INVALID_ARG;
  return batch_collect_impl(d, b);
  CS_GUARD_END("cs_batch_collect")
}
static void batch_drop_run_state(cs_batch* b) { delete b->run_state; b->run_state = nullptr; }
// CS_DETECT_PROF: the host phase clock of the lean path, every eighth run
static void prof_report(cs_detector* d, double total_ms) {
  if (!d->prof || (++d->prof_runs % 8) != 0) return;
  const char* nm[11] = {"jobs+samples", "prefix+pack", nullptr, "alloc+enqueue", "gpu wait", "tie lists", "records", "tie wait", "tie rank", "tie corners", "tie records"};
  fprintf(stderr, "[detect] host ms/run:");
  for (int k = 0; k < 11; k++) { if (nm[k]) fprintf(stderr, " %s %.3f", nm[k], d->prof_mark[k] / 8); d->prof_mark[k] = 0; }
  fprintf(stderr, " | pre %.3f total %.3f\n", d->prof_mark[11] / 8, total_ms); d->prof_mark[11] = 0;
}
static int batch_collect_impl(cs_detector* d, cs_batch* b) {
  if (!b->run_state) return CS_OK;                        // nothing outstanding (or the sweep ran to completion inside submit)
  std::unique_ptr<BatchRunState> rs(b->run_state);
  b->run_state = nullptr;
  CS_HIP_TRY(hipSetDevice(d->device));
  CS_TRY(rs->rp_lean ? rp_finish(rs->C, b->pipe[0]) : pipe_finish(rs->C, b->pipe[0], rs->cam_rp));
  rs->tm.total_ms = now_ms() - rs->t_begin;
  b->timing = rs->tm;
  b->ran = true;
  prof_report(d, rs->tm.total_ms);
  return CS_OK;
}

// Per-frame camera caches: raw pose and the roll/pitch sample poses (:78-79, :344-355, :368-377).  The pose pool is the same for every
// round: uploaded once.
static int build_camera_caches(cs_detector* d, cs_batch* b, BatchRunState* rs, bool sample_rp) {
  const int NF = b->n_frames;
  const double t0 = now_ms();
  std::vector<CamCache>& cam_raw = rs->cam_raw; cam_raw.resize(NF);
  std::vector<std::vector<CamCache>>& cam_rp = rs->cam_rp; cam_rp.resize(NF);
  d->pool->run(NF, [&](int f) {
    const FrameIn& F = b->frames[f];
    make_cam(F.K, F.R, F.t, cam_raw[f]);
    if (sample_rp) sample_rp_poses(F.K, F.t, cam_raw[f], cam_rp[f]);
    else cam_rp[f].push_back(cam_raw[f]);
  });
  std::vector<int>& rp_off = rs->rp_off; rp_off.assign(NF + 1, 0);
  for (int f = 0; f < NF; f++) rp_off[f + 1] = rp_off[f] + (int)cam_rp[f].size();
  // (pinned staging owned by the batch: the copy is queued behind whatever the detector's stream still runs -- another batch's sweep --
  // and nobody waits for it here)
  const size_t np_ = (size_t)std::max(1, rp_off[NF]);
  CS_ENSURE(b->h_rp, np_);
  for (int f = 0; f < NF; f++)
    for (size_t k = 0; k < cam_rp[f].size(); k++) b->h_rp.p[rp_off[f] + k] = cam_rp[f][k].pose;
  CS_ENSURE(b->d_rp, np_);
  CS_HIP_TRY(hipMemcpyAsync(b->d_rp.p, b->h_rp.p, sizeof(cs::RpPose) * np_, hipMemcpyHostToDevice, d->stream));
  rs->tm.setup_host_ms += now_ms() - t0;
  return CS_OK;
}

// what both lean paths (pipe_launch / pipe_finish, rp_launch / rp_finish) need of a batch: nothing retained for the debug getters, nothing
// forced to the host, line setup and ranking within the kernels' capacities
static bool lean_path_allowed(const cs_batch* b, int kmax) {
  return !b->debug && !b->force_host_rank && !b->force_host_setup && !b->force_no_pipeline && b->device_setup && kmax <= cs::RANK_KMAX && b->max_boxes > 0;
}

// ================================================================== round-by-round path ==========
// The general path (debug getters, host ranking / host line setup on request, the lean roll/pitch path's redo of frames with tie
// boxes): per round setup -> upload -> sweep -> ranking on the device or on the host -> records, the host deciding after every round.
namespace {

struct RoundTables {      // the job tables of one round and the device view of its sweep
  std::vector<cs::JobDesc> jobs;
  std::vector<long long> slot_prefix;
  std::vector<int> vp_prefix, top_x, box_job0, box_njobs;      // (the round's boxes: first job, height samples -- consecutive jobs)
  std::vector<double> mid_x, mid_y, ang, yaw, yaw_c, yaw_s;
  size_t nj = 0, n_lines = 0;      // n_lines: entries of the pooled line tables (mid_x / mid_y / ang hold them only with the host line setup)
  long long slot_total = 0;
  int vp_total = 0;
  cs::DetectDeviceView v{};
};

struct RoundRun {         // one cs_batch_run through the round path
  PipeCtx& C;
  bool sample_rp, dev_setup;
  std::vector<double> cur_yaw;      // cam_pose.camera_yaw as the next box of a frame will see it (:180)
};

// cam_pose.camera_yaw as the next box of this frame reads it (:180): the reference's last set_cam_pose() of this box is
// the one for the last kept proposal of the last height sample (:727-737), or, when nothing was kept, the sweep's last
// (roll, pitch) sample (:368-377).  jl: the box's last job.  (One box per frame and round: no two workers write the same entry.)
void carry_yaw(RoundRun& X, const cs::JobDesc& jl, long long last_slot) {
  const std::vector<CamCache>& rp = (*X.C.cam_rp_all)[jl.frame];
  X.cur_yaw[jl.frame] = last_slot < 0 ? rp.back().cam_yaw : rp[(size_t)decode_slot(jl, last_slot).rp].cam_yaw;
}

// the exact winners wl of the box whose jobs start at `jobs`, their corners one after the other from corners16
void round_write_exact(const RoundRun& X, const RoundTables& T, const cs::JobDesc* jobs, const std::vector<ExactWinner>& wl, const double* corners16) {
  const PipeCtx& C = X.C;
  const int f = jobs[0].frame;
  write_exact_winners(C.O, C.b->frames[f], jobs, wl, T.yaw.data(), (*C.cam_rp_all)[f], (*C.cam_raw)[f].euler, X.sample_rp, corners_at(corners16));
}

// ---- setup (host): the round's jobs per frame, then packed into pooled tables
int round_setup(RoundRun& X, int round, RoundTables& T) {
  cs_detector* d = X.C.d; cs_batch* b = X.C.b;
  const cs_detect_params& P = d->prm;
  const int NF = b->n_frames;
  const bool sample_rp = X.sample_rp, dev_setup = X.dev_setup;
  const std::vector<std::vector<CamCache>>& cam_rp = *X.C.cam_rp_all;
  const std::vector<int>& rp_off = *X.C.rp_off;
  cs_detect_timing& tm = *X.C.tm;
  const double t0 = now_ms();
  std::vector<FrameRound> fr(NF);
  d->pool->run(NF, [&](int f) {
    const FrameIn& F = b->frames[f];
    FrameRound& R = fr[f];
    int b0 = sample_rp ? round : 0, b1 = sample_rp ? std::min(round + 1, F.n_boxes) : F.n_boxes;
    int shared_yoff = -1, shared_Y = 0;  // without roll/pitch sampling cam_pose never changes: every box of the frame sweeps the same yaw list (:180-184)
    for (int bi = b0; bi < b1; bi++) {
      const double* bb = &F.boxes[5 * bi];
      if (top_sample_step(bb) < 1) continue;  // :215 break (same for every height sample)
      // yaw samples (:180-184)
      int yoff, nY;
      if (shared_yoff >= 0) { yoff = shared_yoff; nY = shared_Y; }
      else {
        double yl[LINESPACE_MAX], yc[LINESPACE_MAX], ys[LINESPACE_MAX];      // (no list is longer: this path's tables have no other capacity)
        yoff = (int)R.yaw.size(); nY = std::max(0, fill_yaw_list(X.cur_yaw[f], P.yaw_range_deg, P.yaw_step_deg, LINESPACE_MAX, yl, yc, ys));
        R.yaw.insert(R.yaw.end(), yl, yl + nY); R.yaw_c.insert(R.yaw_c.end(), yc, yc + nY); R.yaw_s.insert(R.yaw_s.end(), ys, ys + nY);
        if (!sample_rp) { shared_yoff = yoff; shared_Y = nY; }
      }
      std::vector<int> tops(LINESPACE_MAX);
      tops.resize((size_t)top_samples(bb, tops.data()));
      for (int k = 0; k < F.n_heights[bi]; k++) {
        cs::JobDesc jd;
        fill_job_geometry(jd, F, bi, k, rp_off[f]);
        jd.frame = f; jd.Y = nY; jd.T = (int)tops.size(); jd.RP = (int)cam_rp[f].size();
        JobHost jh;
        jh.yaw_off_local = yoff; jh.tops = tops;
        // ROI line filter (:271-283) + merge (:288-296) + angles/midpoints (:309-315): the line setup kernels, or here
        if (dev_setup) { jd.m = 0; jh.line_cap = F.n_lines; R.jobs.push_back(jd); R.jh.push_back(std::move(jh)); continue; }
        std::vector<double> in;
        for (int e = 0; e < F.n_lines; e++) {
          const double* l = &F.lines[4 * e];
          if (cs::inside_box(cs::v2(l[0], l[1]), jd.g.el, jd.g.et, jd.g.er, jd.g.eb) &&
              cs::inside_box(cs::v2(l[2], l[3]), jd.g.el, jd.g.et, jd.g.er, jd.g.eb))
            in.insert(in.end(), l, l + 4);
        }
        merge_lines(in, P.pre_merge_dist_thre, P.pre_merge_angle_thre, P.edge_length_threshold);
        jd.m = (int)(in.size() / 4);
        for (int i = 0; i < jd.m; i++) {
          jh.angs.push_back(cs::cs_atan2(in[4 * i + 3] - in[4 * i + 1], in[4 * i + 2] - in[4 * i]));
          jh.mids_x.push_back((in[4 * i] + in[4 * i + 2]) / 2);
          jh.mids_y.push_back((in[4 * i + 1] + in[4 * i + 3]) / 2);
        }
        jh.line_cap = jd.m;
        R.jobs.push_back(jd);
        R.jh.push_back(std::move(jh));
      }
    }
  });
  // pack: per-frame sizes -> offsets (serial prefix over frames) -> parallel copy into the pooled arrays
  std::vector<size_t> f_job(NF + 1, 0), f_line(NF + 1, 0), f_yaw(NF + 1, 0), f_top(NF + 1, 0);
  std::vector<long long> f_slot(NF + 1, 0), f_vp(NF + 1, 0);
  for (int f = 0; f < NF; f++) {
    size_t nl = 0, nt = 0;
    JobSpan fs{0, 0};
    for (size_t q = 0; q < fr[f].jobs.size(); q++) {
      const JobSpan s = span_exact(fr[f].jobs[q]);
      nl += fr[f].jh[q].line_cap; nt += fr[f].jh[q].tops.size();
      fs.slots += s.slots; fs.vps += s.vps;
    }
    f_job[f + 1] = f_job[f] + fr[f].jobs.size(); f_line[f + 1] = f_line[f] + nl; f_yaw[f + 1] = f_yaw[f] + fr[f].yaw.size();
    f_top[f + 1] = f_top[f] + nt; f_slot[f + 1] = f_slot[f] + fs.slots; f_vp[f + 1] = f_vp[f] + fs.vps;
  }
  const size_t nj = f_job[NF];
  T.nj = nj; T.n_lines = f_line[NF];
  if (nj == 0) { tm.setup_host_ms += now_ms() - t0; return CS_OK; }
  if (f_vp[NF] > 0x7fffffffLL) { cs_set_error("too many (roll,pitch,yaw) samples in one round"); return CS_ERR_CAPACITY; }
  T.jobs.resize(nj); T.slot_prefix.resize(nj + 1); T.vp_prefix.resize(nj + 1);
  const size_t n_lines_host = dev_setup ? 0 : T.n_lines;  // with the device line setup these tables are only ever written by the kernel
  T.mid_x.resize(n_lines_host); T.mid_y.resize(n_lines_host); T.ang.resize(n_lines_host);
  T.yaw.resize(f_yaw[NF]); T.yaw_c.resize(f_yaw[NF]); T.yaw_s.resize(f_yaw[NF]); T.top_x.resize(f_top[NF]);
  d->pool->run(NF, [&](int f) {
    FrameRound& R = fr[f];
    size_t ji = f_job[f], lo = f_line[f], yo = f_yaw[f], to = f_top[f];
    JobSpan at{f_slot[f], f_vp[f]};
    std::copy(R.yaw.begin(), R.yaw.end(), T.yaw.begin() + yo);
    std::copy(R.yaw_c.begin(), R.yaw_c.end(), T.yaw_c.begin() + yo);
    std::copy(R.yaw_s.begin(), R.yaw_s.end(), T.yaw_s.begin() + yo);
    for (size_t q = 0; q < R.jobs.size(); q++, ji++) {
      cs::JobDesc& jd = R.jobs[q];
      const JobHost& jh = R.jh[q];
      jd.line_off = (int)lo; jd.yaw_off = (int)(yo + jh.yaw_off_local); jd.top_off = (int)to;
      if (!dev_setup) {
        std::copy(jh.mids_x.begin(), jh.mids_x.end(), T.mid_x.begin() + lo);
        std::copy(jh.mids_y.begin(), jh.mids_y.end(), T.mid_y.begin() + lo);
        std::copy(jh.angs.begin(), jh.angs.end(), T.ang.begin() + lo);
      }
      std::copy(jh.tops.begin(), jh.tops.end(), T.top_x.begin() + to);
      lo += jh.line_cap; to += jh.tops.size();
      jd.slot_off = T.slot_prefix[ji] = at.slots; jd.vp_off = T.vp_prefix[ji] = (int)at.vps;
      at.slots += span_exact(jd).slots; at.vps += span_exact(jd).vps;
      T.jobs[ji] = jd;
    }
  });
  T.slot_prefix[nj] = f_slot[NF]; T.vp_prefix[nj] = (int)f_vp[NF];
  T.slot_total = T.slot_prefix[nj]; T.vp_total = T.vp_prefix[nj];
  for (size_t j = 0; j < nj; j++)      // (every job here belongs to a swept box; a box whose yaw list came out empty is still listed)
    if (T.jobs[j].hid == 0) { T.box_job0.push_back((int)j); T.box_njobs.push_back(b->frames[T.jobs[j].frame].n_heights[T.jobs[j].box]); }
  tm.setup_host_ms += now_ms() - t0;
  tm.n_jobs += (long long)nj; tm.n_slots += T.slot_total;
  return CS_OK;
}

// ---- H2D: the round's tables.  They are small (a frame: ~10 of them, a few KB each).  From the std::vectors every hipMemcpyAsync is a
// staged, effectively synchronous copy (10-25 us apiece, ~150 us per call); copied first into ONE pinned block they go out back to back
// and the host does not wait (the round's results are awaited before the block is written again).
int round_upload(RoundRun& X, RoundTables& T) {
  cs_batch* b = X.C.b;
  SweepBuffers& B = b->round;
  hipStream_t st = X.C.d->stream;
  const double t0 = now_ms();
  const size_t nj = T.nj;
  CS_TRY(B.ensure_tables(nj, nj + 1, T.n_lines, T.yaw.size(), T.top_x.size(), (size_t)T.vp_total, T.box_job0.size(), X.C.d->prm.max_cuboid_num));
  CS_ENSURE(B.flag, T.slot_total + 1);
  struct Tab { void* dst; const void* src; size_t bytes; };
  auto tab = [](auto& dst, const auto& vec) { return Tab{dst.p, vec.data(), sizeof(vec[0]) * vec.size()}; };
  const Tab tabs[] = {tab(B.jobs, T.jobs), tab(B.slot_prefix, T.slot_prefix), tab(B.vp_prefix, T.vp_prefix), tab(B.mid_x, T.mid_x), tab(B.mid_y, T.mid_y), tab(B.ang, T.ang),
                      tab(B.yaw, T.yaw), tab(B.yaw_c, T.yaw_c), tab(B.yaw_s, T.yaw_s), tab(B.top_x, T.top_x), tab(B.box_job0, T.box_job0), tab(B.box_njobs, T.box_njobs)};
  size_t need = 0;      // every table on a 64-byte boundary of the block
  for (const Tab& t : tabs) need += (size_t)whole_waves((long long)t.bytes);
  CS_ENSURE(b->h_tables, need + 64);
  unsigned char* hb = b->h_tables.p;
  for (const Tab& t : tabs) {
    if (t.bytes) { memcpy(hb, t.src, t.bytes); CS_HIP_TRY(hipMemcpyAsync(t.dst, hb, t.bytes, hipMemcpyHostToDevice, st)); }
    hb += whole_waves((long long)t.bytes);
  }
  CS_HIP_TRY(hipMemsetAsync(B.job_valid.p, 0, sizeof(int) * nj, st));
  X.C.tm->h2d_ms += now_ms() - t0;
  return CS_OK;
}

// ---- sweep (HIP): line setup, VP support, corner construction
int round_sweep(RoundRun& X, RoundTables& T) {
  cs_detector* d = X.C.d; cs_batch* b = X.C.b;
  SweepBuffers& B = b->round;
  const cs_detect_params& P = d->prm;
  hipStream_t st = d->stream;
  const size_t nj = T.nj;
  cs::DetectDeviceView& v = T.v;
  B.bind(v, *b, nj);      // (the c_* columns: bound again once they are sized, round_compact_score)
  CS_HIP_TRY(hipEventRecord(d->ev[6], st));
  if (X.dev_setup) {      // (one stream in both roles: the crowded ROIs' instances in stream order, between the classification and the others)
    CS_ENSURE(b->round_ls_lists, 2 * (nj + 1));
    cs::launch_line_setup_listed(B.jobs.p, (int)nj, b->d_frame_lines.p, b->d_frame_line_ptr.p, B.mid_x.p, B.mid_y.p, B.ang.p,
                                 P.pre_merge_dist_thre, P.pre_merge_angle_thre, P.edge_length_threshold, st, nullptr, st, d->ev[9], d->ev[10], b->round_ls_lists.p);
  }
  CS_HIP_TRY(hipEventRecord(d->ev[7], st));
  if (X.dev_setup) {
    // the merged segment counts come back with the results (byte accounting, debug getters)
    CS_ENSURE(b->h_jobs, nj);
    CS_HIP_TRY(hipMemcpyAsync(b->h_jobs.p, B.jobs.p, sizeof(cs::JobDesc) * nj, hipMemcpyDeviceToHost, st));
  }
  CS_HIP_TRY(hipEventRecord(d->ev[0], st));
  cs::launch_vp_support(v, X.C.sp, T.vp_total, st);
  CS_HIP_TRY(hipEventRecord(d->ev[1], st));
  cs::launch_candidates(v, X.C.sp, T.slot_total, st);
  CS_HIP_TRY(hipEventRecord(d->ev[2], st));
  CS_HIP_TRY(hipGetLastError());
  return CS_OK;
}

// compaction into the c_* columns (`rows` of them) and the scorer
int round_compact_score(RoundRun& X, RoundTables& T, long long rows) {
  cs_detector* d = X.C.d; cs_batch* b = X.C.b;
  SweepBuffers& B = b->round;
  hipStream_t st = d->stream;
  cs::DetectDeviceView& v = T.v;
  if (int rc = B.ensure_slots(rows)) return rc;
  B.bind(v, *b, T.nj);
  CS_HIP_TRY(hipEventRecord(d->ev[3], st));
  cs::launch_scan_compact(v, st);
  CS_HIP_TRY(hipEventRecord(d->ev[8], st));
  cs::launch_score(v, X.C.sp, rows, T.slot_total, st);
  CS_HIP_TRY(hipEventRecord(d->ev[4], st));
  return CS_OK;
}

// Kernel times and algorithmic bytes of a finished round: geometry kernel = vanishing points read once per
// (job, rp, yaw) + one flag per slot (the corners stay in registers); scoring kernel = each distance map once + the vanishing points and
// the VP support table once per (job, rp, yaw) + per valid proposal 12 B read (slot id, flag) and 28 B of scores written.
// ranked: the round was ranked on the device (events 4 -> 5).
int account_sweep(cs_detector* d, cs_detect_timing& tm, const RoundTables& T, long long n_valid, bool ranked) {
  CS_TRY(add_elapsed(tm.vp_kernel_ms, d->ev[0], d->ev[1]));
  CS_TRY(add_elapsed(tm.cand_kernel_ms, d->ev[1], d->ev[2]));
  CS_TRY(add_elapsed(tm.compact_ms, d->ev[3], d->ev[8]));
  CS_TRY(add_elapsed(tm.score_kernel_ms, d->ev[8], d->ev[4]));
  if (ranked) { CS_TRY(add_elapsed(tm.rank_kernel_ms, d->ev[4], d->ev[5])); }
  CS_TRY(add_elapsed(tm.line_setup_ms, d->ev[6], d->ev[7]));
  tm.cand_kernel_launches += 1;
  tm.cand_kernel_bytes += 48LL * T.vp_total + 4LL * T.slot_total;
  long long sbytes = 96LL * T.vp_total + (28LL + 8LL + 4LL) * n_valid;
  for (const cs::JobDesc& jd : T.jobs) sbytes += 4LL * jd.map_w * (jd.g.eb - jd.g.et);
  tm.score_kernel_bytes += sbytes;
  return CS_OK;
}

// ---- rank on the device (nothing has to come back to the host before the ranking), records on the host; boxes flagged by the kernel
// are re-ranked exactly
int round_rank_device(RoundRun& X, RoundTables& T) {
  PipeCtx& C = X.C;
  cs_detector* d = C.d; cs_batch* b = C.b;
  SweepBuffers& B = b->round;
  const cs_detect_params& P = d->prm;
  const int KMAX = P.max_cuboid_num;
  hipStream_t st = d->stream;
  cs_detect_timing& tm = *C.tm;
  const cs::DetectDeviceView& v = T.v;
  const size_t nj = T.nj, nb = T.box_job0.size();
  CS_TRY(round_compact_score(X, T, T.slot_total));   // the exact number of valid proposals stays on the device
  CS_ENSURE(b->h_winners, nb * KMAX);
  cs::RankView rv{};
  rv.box_job0 = B.box_job0.p; rv.box_njobs = B.box_njobs.p; rv.n_boxes = (int)nb; rv.winners = B.winners.p; rv.win_count = B.win_count.p; rv.fallback = B.fallback.p;
  if (X.sample_rp) { CS_ENSURE(b->d_last_slot, nb); CS_ENSURE(b->h_last_slot, nb); rv.last_slot = b->d_last_slot.p; }
  cs::launch_rank(v, rv, rank_params(P, C.sp), st);
  CS_HIP_TRY(hipEventRecord(d->ev[5], st));
  CS_HIP_TRY(hipGetLastError());
  double t0 = now_ms();
  CS_HIP_TRY(hipMemcpyAsync(b->h_winners.p, B.winners.p, sizeof(cs::RankWinner) * nb * KMAX, hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipMemcpyAsync(B.h_win_count.p, B.win_count.p, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipMemcpyAsync(B.h_fallback.p, B.fallback.p, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
  if (X.sample_rp) CS_HIP_TRY(hipMemcpyAsync(b->h_last_slot.p, b->d_last_slot.p, sizeof(long long) * nb, hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipMemcpyAsync(B.h_job_valid.p, B.job_valid.p, sizeof(int) * nj, hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipMemcpyAsync(B.h_job_cbase.p, B.job_cbase.p, sizeof(long long) * (nj + 1), hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipStreamSynchronize(st));
  tm.d2h_ms += now_ms() - t0;
  if (X.dev_setup) for (size_t j = 0; j < nj; j++) T.jobs[j].m = b->h_jobs.p[j].m;
  const long long n_valid = B.h_job_cbase.p[nj];
  tm.n_valid += n_valid;
  CS_TRY(account_sweep(d, tm, T, n_valid, true));
  t0 = now_ms();
  // the flagged boxes' columns come in one gather (this path has nothing to do meanwhile: it waits at once)
  TiePass tie(B, v, st, T.box_job0.data(), T.box_njobs.data(), nj, nb);
  CS_TRY(tie.enqueue_columns()); CS_TRY(tie.wait());
  tm.n_fallback_boxes += (int)tie.boxes.size();
  // the boxes the device ranked: their records; the flagged ones: the exact ranking only (their corners are fetched below, in one gather)
  const RankWeights RW = rank_weights(P);
  d->pool->run((int)nb, [&](int q) {
    const int j0 = T.box_job0[q], nh = T.box_njobs[q];
    const cs::JobDesc* jobs = &T.jobs[j0];
    const int f = jobs[0].frame, bi = jobs[0].box;
    if (B.h_fallback.p[q]) {
      const long long last = tie.rank((size_t)q, RW, KMAX);
      if (X.sample_rp) carry_yaw(X, jobs[nh - 1], last);
      return;
    }
    if (X.sample_rp) carry_yaw(X, jobs[nh - 1], b->h_last_slot.p[q]);
    const int nw = B.h_win_count.p[q];
    const cs::RankWinner* wq = b->h_winners.p + (size_t)q * KMAX;      // the box's winners as the device ranked them
    for (int r = 0; r < nw; r++) {
      const cs::RankWinner& w = wq[r];
      int h = 0;
      while (h + 1 < nh && w.slot >= jobs[h + 1].slot_off) h++;
      const cs::JobDesc& jd = jobs[h];
      const SlotRef s = decode_slot(jd, w.slot);
      write_winner_record(b->frames[f], jd, s, w.flag, w.dist_err, w.angle_err, T.yaw[jd.yaw_off + s.y], (*C.cam_rp_all)[f][s.rp].pose, w.corners, (*C.cam_raw)[f].euler, X.sample_rp,
                          w.normalized_error, C.O.rec(f, bi, r));
    }
    C.O.count(f, bi) = nw;
  });
  CS_TRY(tie.enqueue_corners(C.sp)); CS_TRY(tie.wait());
  d->pool->run((int)tie.boxes.size(), [&](int z) {
    const size_t q = (size_t)tie.boxes[z];
    round_write_exact(X, T, &T.jobs[T.box_job0[q]], tie.winners[q], tie.corners(q, 0));
  });
  tm.finalize_ms += now_ms() - t0;
  return CS_OK;
}

// ---- rank on the host: every column comes back, every box gets the exact ranking; the candidates are retained for cs_batch_debug_*
int round_rank_host(RoundRun& X, RoundTables& T) {
  PipeCtx& C = X.C;
  cs_detector* d = C.d; cs_batch* b = C.b;
  SweepBuffers& B = b->round;
  const cs_detect_params& P = d->prm;
  const int KMAX = P.max_cuboid_num, MB = b->max_boxes;
  hipStream_t st = d->stream;
  cs_detect_timing& tm = *C.tm;
  const std::vector<std::vector<CamCache>>& cam_rp = *C.cam_rp_all;
  const size_t nj = T.nj, nb = T.box_job0.size();
  // valid counts -> host -> size the compact arrays
  CS_HIP_TRY(hipMemcpyAsync(B.h_job_valid.p, B.job_valid.p, sizeof(int) * nj, hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipStreamSynchronize(st));
  if (X.dev_setup) for (size_t j = 0; j < nj; j++) T.jobs[j].m = b->h_jobs.p[j].m;
  long long n_valid = 0;
  for (size_t j = 0; j < nj; j++) { B.h_job_cbase.p[j] = n_valid; n_valid += B.h_job_valid.p[j]; }
  B.h_job_cbase.p[nj] = n_valid;
  tm.n_valid += n_valid;
  CS_TRY(round_compact_score(X, T, n_valid));
  CS_HIP_TRY(hipGetLastError());
  CS_ENSURE(b->h_c_slot, n_valid + 1); CS_ENSURE(b->h_c_flag, n_valid + 1); CS_ENSURE(b->h_c_dist, n_valid + 1); CS_ENSURE(b->h_c_angle, n_valid + 1); CS_ENSURE(b->h_c_skew, n_valid + 1);
  double t0 = now_ms();
  if (n_valid) {
    CS_HIP_TRY(hipMemcpyAsync(b->h_c_slot.p, B.c_slot.p, sizeof(long long) * n_valid, hipMemcpyDeviceToHost, st));
    CS_HIP_TRY(hipMemcpyAsync(b->h_c_flag.p, B.c_flag.p, sizeof(int) * n_valid, hipMemcpyDeviceToHost, st));
    CS_HIP_TRY(hipMemcpyAsync(b->h_c_dist.p, B.c_dist.p, sizeof(double) * n_valid, hipMemcpyDeviceToHost, st));
    CS_HIP_TRY(hipMemcpyAsync(b->h_c_angle.p, B.c_angle.p, sizeof(double) * n_valid, hipMemcpyDeviceToHost, st));
    CS_HIP_TRY(hipMemcpyAsync(b->h_c_skew.p, B.c_skew.p, sizeof(double) * n_valid, hipMemcpyDeviceToHost, st));
  }
  CS_HIP_TRY(hipStreamSynchronize(st));
  tm.d2h_ms += now_ms() - t0;
  CS_TRY(account_sweep(d, tm, T, n_valid, false));

  // per job: the candidate rows and fuse_normalize_scores_v2, retained
  t0 = now_ms();
  const size_t res_base = b->results.size();
  b->results.resize(res_base + nj);
  d->pool->run((int)nj, [&](int j) {
    const cs::JobDesc& jd = T.jobs[j];
    JobResult& R = b->results[res_base + j];
    const long long c0 = B.h_job_cbase.p[j];
    const int V = B.h_job_valid.p[j];
    R.n_valid = V;
    R.rows9.resize(9 * (size_t)V);
    R.slots.assign(b->h_c_slot.p + c0, b->h_c_slot.p + c0 + V);
    for (int i = 0; i < V; i++) {
      const SlotRef s = decode_slot(jd, R.slots[i]);
      const cs::RpPose& pose = cam_rp[jd.frame][s.rp].pose;
      candidate_row9(s, b->h_c_flag.p[c0 + i], b->h_c_dist.p[c0 + i], b->h_c_angle.p[c0 + i], T.yaw[jd.yaw_off + s.y], jd.down_expand, pose.roll, pose.pitch, &R.rows9[9 * (size_t)i]);
    }
    fuse_scores(b->h_c_dist.p + c0, b->h_c_angle.p + c0, V, P.weight_vp_angle, R.keep, R.score);
  });
  for (size_t j = 0; j < nj; j++) b->job_index[((size_t)T.jobs[j].frame * MB + T.jobs[j].box) * 3 + T.jobs[j].hid] = (int)(res_base + j);
  // per box: proposals over its height samples (in order), final ranking (:804-838)
  const RankWeights RW = rank_weights(P);
  std::vector<std::vector<ExactWinner>> win_per_box(nb);
  d->pool->run((int)nb, [&](int q) {
    const int j0 = T.box_job0[q], nh = T.box_njobs[q];
    HeightCols cols[3];
    for (int h = 0; h < nh; h++) {
      const long long c0 = B.h_job_cbase.p[j0 + h];
      const JobResult& R = b->results[res_base + j0 + h];
      cols[h] = HeightCols{b->h_c_dist.p + c0, b->h_c_angle.p + c0, b->h_c_skew.p + c0, b->h_c_flag.p + c0, b->h_c_slot.p + c0, R.n_valid, &R.keep, &R.score};
    }
    const long long last = exact_rank_box(cols, nh, RW, KMAX, win_per_box[q]);
    if (X.sample_rp) carry_yaw(X, T.jobs[j0 + nh - 1], last);
  });
  tm.rank_host_ms += now_ms() - t0;

  // ---- finish: the winners' corners (debug: those of every valid candidate of the round) and the records
  t0 = now_ms();
  std::vector<long long> wslots;
  for (const auto& wl : win_per_box) for (const ExactWinner& w : wl) wslots.push_back(w.slot);
  const size_t nw = wslots.size();
  if (b->debug) wslots.insert(wslots.end(), b->h_c_slot.p, b->h_c_slot.p + n_valid);
  const size_t n_gather = wslots.size();
  if (n_gather) {
    CS_ENSURE(B.h_win_slots, n_gather); CS_ENSURE(B.h_win_corners, 16 * n_gather);
    std::copy(wslots.begin(), wslots.end(), B.h_win_slots.p);
    cs::launch_gather_corners(T.v, C.sp, B.h_win_slots.p, (int)n_gather, B.h_win_corners.p, st);     // (pinned host memory on both sides, as in TiePass)
    CS_HIP_TRY(hipGetLastError());
    CS_HIP_TRY(hipStreamSynchronize(st));
  }
  size_t i = 0;
  for (size_t q = 0; q < nb; q++) {
    round_write_exact(X, T, &T.jobs[T.box_job0[q]], win_per_box[q], B.h_win_corners.p + 16 * i);
    i += win_per_box[q].size();
  }
  if (b->debug) {
    for (size_t j = 0; j < nj; j++) {
      JobResult& R = b->results[res_base + j];
      const long long c0 = B.h_job_cbase.p[j];
      R.corners.assign(B.h_win_corners.p + 16 * (nw + c0), B.h_win_corners.p + 16 * (nw + c0 + R.n_valid));
    }
  }
  tm.finalize_ms += now_ms() - t0;
  return CS_OK;
}

}  // namespace

static int batch_run_impl(cs_detector* d, cs_batch* b, cs_cuboid* out, int* out_counts, bool defer) {
  if (!d || !b || b->det != d || !out || !out_counts) return CS_ERR_INVALID_ARG;
  if (b->run_state) { cs_set_error("cs_batch_submit: the previous submit of this batch has not been collected"); return CS_ERR_INVALID_ARG; }
  CS_HIP_TRY(hipSetDevice(d->device));
  { const int rcf = batch_flush_refill(d, b); if (rcf) return rcf; }      // (cs_batch_refill_gray: the new images' maps, in front of this sweep)
  std::unique_ptr<BatchRunState> rs_owner(new BatchRunState());
  BatchRunState* rs = rs_owner.get();
  const cs_detect_params& P = d->prm;
  const bool sample_rp = P.whether_sample_cam_roll_pitch != 0;
  const int NF = b->n_frames, MB = b->max_boxes, KMAX = P.max_cuboid_num;
  cs_detect_timing& tm = rs->tm;
  const double t_begin = now_ms();
  rs->t_begin = t_begin;

  std::fill(out_counts, out_counts + (size_t)NF * std::max(MB, 0), 0);
  b->results.clear();
  b->job_index.assign((size_t)NF * std::max(MB, 1) * 3, -1);

  cs::SweepParams sp;
  sp.vp12_thre_rad = P.vp12_edge_angle_thre / 180.0 * CS_PI;
  sp.vp3_thre_rad = P.vp3_edge_angle_thre / 180.0 * CS_PI;
  sp.short_thre = P.shorted_edge_thre;
  sp.short_sq_bound = cs::sqrt_lt_bound(P.shorted_edge_thre);
  sp.consider_config_1 = P.consider_config_1; sp.consider_config_2 = P.consider_config_2;

  CS_TRY(build_camera_caches(d, b, rs, sample_rp));
  rs->C = PipeCtx{d, b, OutView{out, out_counts, MB, KMAX}, &rs->cam_raw, &rs->rp_off, sp, &rs->tm, &rs->cam_rp};
  PipeCtx& C = rs->C;
  if (d->prof) d->prof_mark[11] += now_ms() - t_begin;   // camera caches + pose pool upload

  // ---- production path: chunked two-slot pipeline (host packs chunk k+1 / finishes chunk k-1 while the GPU sweeps k)
  if (!sample_rp && lean_path_allowed(b, KMAX)) {
    const int n_chunks = std::max(1, std::min(NF, b->pipe_chunks));
    if (n_chunks == 1) {    // the usual shape: one launch, one finish -- the finish may be left to cs_batch_collect
      CS_TRY(pipe_launch(C, b->pipe[0], 0, NF));
      b->run_state = rs_owner.release();
      return defer ? CS_OK : batch_collect_impl(d, b);
    }
    for (int k = 0; k <= n_chunks; k++) {
      if (k < n_chunks) {
        int f0 = (int)((long long)NF * k / n_chunks), f1 = (int)((long long)NF * (k + 1) / n_chunks);
        CS_TRY(pipe_launch(C, b->pipe[k & 1], f0, f1));
      }
      if (k >= 1) CS_TRY(pipe_finish(C, b->pipe[(k - 1) & 1], rs->cam_rp));
    }
    tm.total_ms = now_ms() - t_begin;
    b->timing = tm;
    b->ran = true;
    prof_report(d, tm.total_ms);
    return CS_OK;
  }

  // ---- roll/pitch sampling, lean path: every round queued at once, the carried yaw picked on the device
  int max_rp = 0;
  for (int f = 0; f < NF; f++) max_rp = std::max(max_rp, (int)rs->cam_rp[f].size());
  if (sample_rp && lean_path_allowed(b, KMAX) && !b->force_round_path && max_rp <= cs::vp3_table_doubles_per_job() / 2) {
    CS_TRY(rp_launch(C, b->pipe[0], rs->cam_rp));
    rs->rp_lean = true;
    b->run_state = rs_owner.release();
    return defer ? CS_OK : batch_collect_impl(d, b);
  }

  // ---- the round path: with roll/pitch sampling round r = box r of every frame, else one round of all boxes
  RoundRun X{C, sample_rp, b->device_setup && !b->force_host_setup, std::vector<double>(NF)};
  for (int f = 0; f < NF; f++) X.cur_yaw[f] = rs->cam_raw[f].cam_yaw;
  const bool device_rank = !b->debug && !b->force_host_rank && KMAX <= cs::RANK_KMAX;
  const int n_rounds = sample_rp ? MB : (MB > 0 ? 1 : 0);
  for (int round = 0; round < n_rounds; round++) {
    RoundTables T;
    CS_TRY(round_setup(X, round, T));
    if (T.nj == 0) continue;
    CS_TRY(round_upload(X, T)); CS_TRY(round_sweep(X, T)); CS_TRY(device_rank ? round_rank_device(X, T) : round_rank_host(X, T));
  }
  tm.total_ms = now_ms() - t_begin;
  b->timing = tm;
  b->ran = true;
  return CS_OK;
}

extern "C" {

int cs_batch_last_timing(const cs_batch* b, cs_detect_timing* t) {
  if (!b || !t) return CS_ERR_INVALID_ARG;
  if (!b->ran) return CS_ERR_NOT_RUN;
  *t = b->timing;
  return CS_OK;
}

int cs_batch_debug_candidates(cs_batch* b, int frame, int box, int k, int cap, double* rows9, double* corners16) {
  if (!b || frame < 0 || frame >= b->n_frames || box < 0 || box >= b->max_boxes || k < 0 || k > 2) return CS_ERR_INVALID_ARG;
  if (!b->ran) return CS_ERR_NOT_RUN;
  int ri = b->job_index[((size_t)frame * b->max_boxes + box) * 3 + k];
  if (ri < 0) return 0;
  const JobResult& R = b->results[ri];
  int n = std::min(cap, R.n_valid);
  if (rows9) std::memcpy(rows9, R.rows9.data(), sizeof(double) * 9 * (size_t)n);
  if (corners16) {
    if (R.corners.size() < 16 * (size_t)R.n_valid) { cs_set_error("corners not retained: call cs_batch_set_debug(b,1) before cs_batch_run"); return CS_ERR_NOT_RUN; }
    std::memcpy(corners16, R.corners.data(), sizeof(double) * 16 * (size_t)n);
  }
  return R.n_valid;
}

int cs_batch_debug_kept(cs_batch* b, int frame, int box, int k, int cap, int* keep_ids, double* scores) {
  if (!b || frame < 0 || frame >= b->n_frames || box < 0 || box >= b->max_boxes || k < 0 || k > 2) return CS_ERR_INVALID_ARG;
  if (!b->ran) return CS_ERR_NOT_RUN;
  int ri = b->job_index[((size_t)frame * b->max_boxes + box) * 3 + k];
  if (ri < 0) return 0;
  const JobResult& R = b->results[ri];
  int n = std::min(cap, (int)R.keep.size());
  if (keep_ids) std::memcpy(keep_ids, R.keep.data(), sizeof(int) * (size_t)n);
  if (scores) std::memcpy(scores, R.score.data(), sizeof(double) * (size_t)n);
  return (int)R.keep.size();
}

// ------------------------------------------------------------------ distance-map front end -----
int cs_bgr_to_gray(const unsigned char* bgr, int n_pixels, unsigned char* gray) {   // cvtColor(BGR2GRAY), box_proposal_detail.cpp:84
  if (n_pixels < 0 || (n_pixels && (!bgr || !gray))) return CS_ERR_INVALID_ARG;
  for (int i = 0; i < n_pixels; i++) gray[i] = (unsigned char)((bgr[3 * i] * 1868 + bgr[3 * i + 1] * 9617 + bgr[3 * i + 2] * 4899 + (1 << 13)) >> 14);
  return CS_OK;
}

int cs_edge_distance_maps_multi(cs_detector* d, const unsigned char* const* grays, int n_images, int img_w, int img_h, const cs_roi* rois, const int* roi_image,
                                int n_rois, float* const* out_maps, double* kernel_ms) {
  if (!d || n_images <= 0 || !grays || img_w <= 0 || img_h <= 0 || n_rois < 0 || (n_rois && (!rois || !roi_image))) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(d->device));
  if (kernel_ms) *kernel_ms = 0;
  if (n_rois == 0) return CS_OK;
  const size_t img_px = (size_t)img_w * img_h;
  std::vector<cs::EdgeRoi> er(n_rois);
  long long tot = 0, max_px = 1;
  int max_w = 1;
  for (int k = 0; k < n_rois; k++) {
    const cs_roi& r = rois[k];
    if (r.width <= 0 || r.height <= 0 || r.left < 0 || r.top < 0 || r.left + r.width > img_w || r.top + r.height > img_h || roi_image[k] < 0 || roi_image[k] >= n_images ||
        (out_maps && !out_maps[k])) {
      cs_set_error("cs_edge_distance_maps: ROI outside the image");
      return CS_ERR_INVALID_ARG;
    }
    er[k] = cs::EdgeRoi{r.left, r.top, r.width, r.height, (long long)(roi_image[k] * img_px), tot, tot};
    tot += (long long)r.width * r.height;
    max_w = std::max(max_w, r.width); max_px = std::max(max_px, 4LL * ((r.width + 5) / 4) * (r.height + 2));
  }
  DevBuf<unsigned char> d_gray, d_cls;
  DevBuf<cs::EdgeRoi> d_rois;
  DevBuf<float> d_map;
  int rc;
  if ((rc = d_gray.ensure(img_px * n_images)) || (rc = d_cls.ensure((size_t)tot + 8)) || (rc = d_rois.ensure((size_t)n_rois)) || (rc = d_map.ensure((size_t)tot))) return rc;
  hipStream_t st = d->stream;
  for (int i = 0; i < n_images; i++) {
    if (!grays[i]) { cs_set_error("cs_edge_distance_maps: null image"); return CS_ERR_INVALID_ARG; }
    CS_HIP_TRY(hipMemcpyAsync(d_gray.p + img_px * i, grays[i], img_px, hipMemcpyHostToDevice, st));
  }
  std::vector<cs::EdgeRoi> er_launch(er.begin(), er.end());      // (er keeps the caller's order for the copies back)
  edge_rois_largest_first(er_launch);
  CS_HIP_TRY(hipMemcpyAsync(d_rois.p, er_launch.data(), sizeof(cs::EdgeRoi) * n_rois, hipMemcpyHostToDevice, st));
  CS_HIP_TRY(hipEventRecord(d->ev[0], st));
  // cv::Canny(gray_img(object_bbox), im_canny, 80, 200): the thresholds are literals of the reference (:324)
  cs::launch_edge_maps(d_gray.p, img_w, img_h, d_rois.p, n_rois, d_cls.p, d_map.p, max_w, max_px, 80, 200, st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipEventRecord(d->ev[1], st));
  if (out_maps)
    for (int k = 0; k < n_rois; k++)
      CS_HIP_TRY(hipMemcpyAsync(out_maps[k], d_map.p + er[k].map_off, sizeof(float) * (size_t)er[k].w * er[k].h, hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipStreamSynchronize(st));
  if (kernel_ms) { float ms = 0; CS_HIP_TRY(hipEventElapsedTime(&ms, d->ev[0], d->ev[1])); *kernel_ms = ms; }
  return CS_OK;
  CS_GUARD_END("cs_edge_distance_maps")
}

int cs_edge_distance_maps(cs_detector* d, const unsigned char* gray, int img_w, int img_h, const cs_roi* rois, int n_rois, float* const* out_maps) {
  if (!gray || (n_rois > 0 && !out_maps)) return CS_ERR_INVALID_ARG;
  std::vector<int> zero(std::max(n_rois, 1), 0);
  return cs_edge_distance_maps_multi(d, &gray, 1, img_w, img_h, rois, zero.data(), n_rois, out_maps, nullptr);
}

// One frame through the detector's resident single-frame batch (gray == nullptr: the frame's dist_maps are uploaded; else they are
// produced on the device from the gray image, in place in the map pool).
static int detect_single(cs_detector* d, const cs_frame_desc* frame, const unsigned char* gray, cs_cuboid* out, int* out_counts) {
  if (!d || !frame || !out || !out_counts) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  std::lock_guard<std::mutex> lk(d->single_mu);
  CS_HIP_TRY(hipSetDevice(d->device));
  if (!d->single) { d->single = new cs_batch(); d->single->det = d; }
  int rc = batch_fill(d, d->single, frame, gray ? &gray : nullptr, 1);
  if (rc) return rc;
  return cs_batch_run(d, d->single, out, out_counts);
  CS_GUARD_END("cs_detect_cuboids")
}
// image in, cuboids out: the frame's dist_maps are ignored and computed from the gray image on the device
int cs_detect_cuboids_gray(cs_detector* d, const cs_frame_desc* frame, const unsigned char* gray, cs_cuboid* out, int* out_counts) {
  if (!gray) return CS_ERR_INVALID_ARG;
  return detect_single(d, frame, gray, out, out_counts);
}

int cs_detect_cuboids(cs_detector* d, const cs_frame_desc* frame, cs_cuboid* out, int* out_counts) {
  return detect_single(d, frame, nullptr, out, out_counts);
}

}  // extern "C"
