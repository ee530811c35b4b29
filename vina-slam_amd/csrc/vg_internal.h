// vg_internal.h — device context of the MI355X LIO hot path (not part of the
// C-ABI). One vg_ctx owns every device buffer of one LiDAR-inertial sequence:
// the scan staging area, the downsample workspace, the device-resident voxel
// map (root hash + octree node pool + per-slot window point arrays + point_fix
// arena) and the sliding-window state.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <functional>
#include <mutex>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include "../../include/vina_gpu.h"
#include "vg_la.h"
#include "vg_lm_loop.h"  // BaLoop: an LM run's host loop state (vg_ctx::ba_loop)
#include "vg_scratch.h"

#define VG_HIP(call)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
      return VG_E_HIP;                                                                  \
    }                                                                                   \
  } while (0)

#define VG_TRY(expr)            \
  do {                          \
    int r_ = (expr);            \
    if (r_ != VG_OK) return r_; \
  } while (0)

namespace vg {

constexpr int kBlock = 256;
constexpr int64_t kKeyOff = 1 << 20;  // packed voxel key: 21 bits per axis
constexpr uint64_t kKeyEmpty = ~0ull;

inline int grid_for(long n, int block = kBlock, int cap = 8192) {
  long g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// Bump allocator over one hipMalloc'd slab (16-byte aligned carve-outs).
// In measure mode (base == nullptr) take() only accumulates the size and hands
// out placeholder addresses, so vg_create can size the slab exactly.
struct Arena {
  char* base = nullptr;
  size_t size = 0, used = 0;
  bool measure = false;
  template <class T>
  T* take(size_t n) {
    size_t b = (n * sizeof(T) + 255) & ~size_t(255);
    if (measure) {
      T* p = (T*)(uintptr_t)(4096 + used);
      used += b;
      return p;
    }
    if (used + b > size) return nullptr;
    T* p = (T*)(base + used);
    used += b;
    return p;
  }
};

// Initialisation map of lio_state_estimation_kdtree (odometry.cpp:267-439,
// SURVEY A14): float points (0.5 m downsampled), bucketed by 1 m cells for an
// exact k = 5 nearest-neighbour search (kdlio.hip)
struct KdMap {
  float *x = nullptr, *y = nullptr, *z = nullptr;     // map points (key order of the last downsample)
  float *sx = nullptr, *sy = nullptr, *sz = nullptr;  // the same, grouped by cell
  int* sidx = nullptr;                                // map index of each grouped point
  uint64_t *keys = nullptr, *keys_s = nullptr;
  uint32_t *idx = nullptr, *idx_s = nullptr;
  uint64_t* hkey = nullptr;                           // cell hash: key -> [start, end) in s*
  int *hstart = nullptr, *hend = nullptr;
  int hmask = 0, cap = 0, n = 0;
  double *ds = nullptr, *dir = nullptr, *part = nullptr;  // per scan point: plane offset, normal; block partials
  double* h_part = nullptr;                           // pinned copy of the partials
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
};

struct HdsIn {  // the per-scan downsample's input (k_hds_args -> device, read by every k_hds_* kernel)
  const float *x, *y, *z, *in;
  int n, pad;
};
struct DownsampleBufs {
  HdsIn* arg = nullptr;       // the current scan's input cloud (device copy, see k_hds_args)
  uint64_t *keys = nullptr, *keys_sorted = nullptr;
  uint32_t *idx = nullptr, *idx_sorted = nullptr;
  uint32_t *head = nullptr, *pos = nullptr, *seg = nullptr;
  float *ox = nullptr, *oy = nullptr, *oz = nullptr, *oi = nullptr, *oc = nullptr;
  int* flags = nullptr;  // [0] range error, [1] n_out
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  // the per-scan pipeline's downsample (ds_enqueue): hashed grouping, every
  // count on the device. Voxel table (open addressing, cleared by its users):
  uint64_t* hkey = nullptr;
  int *hfirst = nullptr, *hcnt = nullptr, *hfill = nullptr, *hrank = nullptr, *hoff = nullptr;
  int hmask = 0;
  int cap = 0;                // max points per scan (bigv's length: dense voxels from the front, mid-size from the back)
  uint32_t* pslot = nullptr;  // per point: its voxel's table slot
  uint32_t* pseg = nullptr;   // point indices grouped by voxel
  int* vfirst = nullptr;      // per voxel (output rank): its first point
  int* bigv = nullptr;        // dense voxels (output ranks) deferred to k_hds_big
  uint32_t* pseg2 = nullptr;  // dense voxels' segments back in input order
  int* tsum = nullptr;        // per 1024-point tile: first points, their points
  int* hflags = nullptr;      // [0] range error (until the insert takes it), [1] n_out, [2] fallback needed, [3] dense voxels, [4] mid-size voxels
};

// ---- device-resident voxel map (replaces unordered_map<VOXEL_LOC, OctoTree*>
// surf_map, octree.hpp:21-97, slide_window.hpp:6-20) ----
struct NodeHdr {            // 96 B: everything the correspondence descent reads
  double center[3];         // voxel_center
  int child[8];             // leaves[8] (-1 = none)
  float qlen;               // quater_length
  int8_t layer, octo, isexist, is_plane;
  int8_t has_sw, mk, pad1, pad2;  // mk: marker publication flags (kMkUpdated | kMkPublished, markers.hip)
  int opt_state, last_num;
  int fix_off, fix_cnt, fix_cap;
  int parent;
};
struct PlaneRec {           // 224 B: Plane (plane.hpp:5-24) as read by OctoTree::match
  double center[3], normal[3];
  double var[21];           // plane_var, packed upper 6x6
  float radius;
  int pad;
};
constexpr int kCovN = 45;   // cov_add packed upper 9x9
// Plane's publication flags (plane.hpp:18-21) in NodeHdr::mk: is_update /
// is_normal_update and is_published / is_normal_published move in lock-step
// (the two collectors run back to back), so one pair of bits serves both
constexpr int kMkUpdated = 1, kMkPublished = 2;

struct DevMap {
  int cap_nodes = 0, cap_fix = 0, hash_mask = 0, W = 0, cap_wp = 0;
  int shard_rank = 0, shard_world = 1;  // spatial-tile sharding (shard.cpp)
  NodeHdr* hdr = nullptr;
  PlaneRec* pl = nullptr;
  Clu* pcr_add = nullptr;
  Clu* pcr_fix = nullptr;
  double* cov_add = nullptr;   // cap_nodes * 45
  double* eig = nullptr;       // cap_nodes * 12 (eig_value 3, eig_vector 9 row-major)
  double* jour = nullptr;
  double* dbox = nullptr;      // cap_nodes * 6: the descent's region per node (lo[3] exclusive, hi[3] inclusive; vg_dev.h dbox_*)
  Clu* pcrs = nullptr;         // cap_nodes * W (SlideWindow::pcrs_local, physical slot)
  int* nscr = nullptr;         // per-node scratch (cap_nodes * 4)
  unsigned long long* pend = nullptr;  // margi: per internal node, children still to report (high 32) | existing ones (low 32)
  int* cfirst = nullptr;       // per-node per-octant first-event scratch (cap_nodes * 8)
  uint64_t* hkey = nullptr;    // root hash
  int* hval = nullptr;
  int* hfirst = nullptr;
  int* slide = nullptr;        // surf_map_slide (root ids)
  uint8_t* in_slide = nullptr;
  int* leaf_cnt = nullptr;     // insert bucketing: points of this scan per leaf (0 between inserts)
  int* leaf_seg = nullptr;     // insert bucketing: the leaf's segment
  int* creq_cnt = nullptr;     // insert bucketing: points of this scan per child request (parent * 8 + octant; 0 between inserts)
  double* fix_pnt = nullptr;   // point_fix arena: pnt (world) 3, var 6
  double* fix_var = nullptr;
  double* wp_pnt = nullptr;    // window points per physical slot: body pnt
  double* wp_var = nullptr;    // world var (after pvec_update), packed 6
  int* wp_leaf = nullptr;      // leaf holding the point in its list, -1 = not listed
  float* wp_int = nullptr;     // intensity of the window point (pointVar::intensity; /map_cmap only)
  // SlideWindow::points per leaf (octree.cpp:151-177): per physical slot, the
  // slot's listed point indices grouped by leaf, each leaf's run in index order
  // — [0, cap_wp) written by the insert, then an arena the recut's children
  // take their runs from (a point moves one layer down per subdivision, so
  // max_layer arenas of cap_wp suffice); lseg locates a leaf's run per slot
  int* wp_ord = nullptr;       // W * ord_stride
  uint64_t* lseg = nullptr;    // cap_nodes * W: start 24 | count 21 | slot epoch 19 bits (lseg_pack)
  int* slot_epoch = nullptr;   // per physical slot: inserts into it so far (a run of an older epoch is stale)
  int* arena = nullptr;        // per physical slot: next free wp_ord entry of the children's arena
  int ord_stride = 0;
  int* counters = nullptr;     // device counters (see kCnt*)
  int* stamp = nullptr;        // per-node tag of the last IEKF iteration that read its plane (P_k, profiling pass)
  int* wpn = nullptr;          // window points per physical slot (written by the insert, read by k_make_win)
};
enum {
  kCntNodes = 0, kCntFix = 1, kCntSlide = 2, kCntNew = 3, kCntTouched = 4, kCntSegCur = 5, kCntNext = 6,
  kCntSub = 7, kCntEvents = 8, kCntFactors = 9, kCntCreate = 10, kCntErr = 11, kCntLeaves = 12, kCntMisc = 13, kCntSeg = 14, kCntRoots = 15,
  kCntGTouched = 16, kCntGSlide = 17,  // all-reduced copies (sharded mode) for the thread_num quirks
  kCntPlaneUpd = 18, kCntFixFull = 19,  // margi: plane_update calls, leaves with pcr_fix.N >= max_points
  kCntSlideBase = 20,                   // insert: surf_map_slide size before the scan's roots
  kCntNds = 21,                         // insert: the downsampled points it took (N_ds of the scan)
  kCntN = 22
  // kCntSegCur: the insert's segment cursor (the next free entry of the bucketed point order)
};

// per-scan work buffers
struct Work {
  int cap = 0;                 // entries
  uint64_t *k0 = nullptr, *k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr;
  uint32_t *u0 = nullptr, *u1 = nullptr;
  uint32_t *ac_cnt = nullptr, *ac_off = nullptr;  // child allocation scratch
  int *list0 = nullptr, *list1 = nullptr, *list2 = nullptr, *cand = nullptr;
  int* leaf = nullptr;         // per ds point leaf / per event target
  double* pw = nullptr;        // per ds point world coords
  void* tmp = nullptr;
  void* tmp2 = nullptr;        // sort workspace of the second stream
  size_t tmp_bytes = 0;
  double* partials = nullptr;  // reduction partials
  int* iekf_cache = nullptr;   // per raw point cached leaf
  int* pk_leaf = nullptr;      // per raw point leaf read by the profiled IEKF iteration (P_k count)
  int* rc = nullptr;           // device-side level counts (recut / margi, vg_dev.h kRc*)
  uint32_t* cand_bits = nullptr;  // factor candidates of an asynchronous recut, one bit per node id
  int* plan = nullptr;         // per-leaf point_fix copy plan (margi)
  // the recut's odd levels: subdividing leaves, rcinfo, events (even levels: list2, v1, k0)
  unsigned long long* gran = nullptr;  // per 1024-point tile: the root registration's look-back granules
  int ngran = 0;
  int* sub_odd = nullptr;
  int* info_odd = nullptr;
  uint64_t* ev_odd = nullptr;
  int nparts = 0;
};

// BA device buffers
struct BaBufs {
  int cap_f = 0;
  int* fac_node = nullptr;
  double* fac_eig = nullptr;   // trial eig values/vectors (12) per factor
  Clu* fac_pcr = nullptr;      // trial merged cluster per factor
  double* hpart = nullptr;     // chunk partials
  double* hout = nullptr;      // reduced LiDAR system: 6W x 6W packed lower rows + 6W gradient + the residual
  double* hout_part = nullptr; // this shard's part of it (sharded mode)
  double* rpart = nullptr;
  double* xs = nullptr;        // 1024 doubles of WinD / counts staging (map stages), then the LM's carved block (vg_ba.h carve)
};

// ---- device-resident estimator state (state.hip) ----
// The per-scan state lives in HBM for the whole scan: the IEKF update, the
// window push, the BA and the slide all read and write it on the device, so
// the host never waits for an intermediate result. The host mirror (host_mirror.cpp)
// is refreshed from the host-mapped publication block below.
constexpr int kXS = 24;             // per-frame state: R 9, p 3, v 3, bg 3, ba 3, g 3
constexpr int kXC = kXS + 225;      // x_curr: frame state + cov 15x15 (row-major)
constexpr int kMaxWin = 32;
constexpr int kBaImuRec = 64 + 225;  // IMU_PRE record (doubles): deltas, bias Jacobians, dtime, cov_inv
// In-kernel clocks of the roofline kernels (vg_profile bit 2): the device's
// constant-rate wall clock (wall_clock64), kernel-only spans, no atomics on
// the timed kernels' paths (a hot atomic from every workgroup cost k_iekf
// ~3 us per launch). A k_iekf launch runs from workgroup 0's start to the
// last workgroup's end: workgroup 0 stores the start, every workgroup its end,
// into a ring slot per (scan, iteration); the host takes the maximum when it
// reads the clock (vg_profile_read). k_ba_solve is one workgroup, timed by its
// thread 0.
constexpr int kClkRing = 256;    // k_iekf launch slots: the last 64 scans x 4 iterations
constexpr int kClkBlocks = 512;  // >= the IEKF grid (iekf_blocks)
// The recut's level kernels (k_rc_level0 + max_layer x k_rc_level), one span
// per scan: k_rc_level0's workgroup 0 stamps the start, every workgroup of the
// last level kernel its end. k_ba_hess: executed launches like k_iekf, slot
// (scan, LM iteration).
constexpr int kClkRcScans = 64;   // recut spans of the last 64 scans
constexpr int kClkRcBlocks = 256; // the level kernels' grid
constexpr int kClkHRing = 512;    // k_ba_hess slots: 64 scans x 8 LM iterations
constexpr int kClkHBlocks = 272;  // >= k_ba_hess's grid (chunk workgroups + IMU workgroups)
struct KClock {
  unsigned long long solve_ticks, solve_n;  // executed k_ba_solve launches
  int on, scan;                             // scans opened since vg_profile (k_scan_begin / k_scan_prop)
  int exec[kClkRing];                       // the slot's k_iekf ran (not a no-op after convergence)
  unsigned long long t0[kClkRing];
  unsigned long long tend[kClkRing][kClkBlocks];
  int rc_exec[kClkRcScans];
  unsigned long long rc_t0[kClkRcScans];
  unsigned long long rc_tend[kClkRcScans][kClkRcBlocks];
  int h_exec[kClkHRing];
  unsigned long long h_t0[kClkHRing];
  unsigned long long h_tend[kClkHRing][kClkHBlocks];
};

struct DState {
  double xc[256];                   // x_curr (IMUST, types.hpp:43-113)
  double xp[256];                   // x_prop (odometry.cpp:67)
  double G6[96];                    // G(:, 0:6) of the last IEKF iteration (odometry.cpp:198)
  double nnt[8];                    // sum n n^T of the last iteration (odometry.cpp:145)
  double traj[16];                  // R, p right after the IEKF (pub_localtraj, local_mapping.cpp:427)
  double xs[kMaxWin * kXS];         // window states x_buf by ord (local_mapping.cpp:434)
  double bias[kMaxWin * 12];        // IMU_PRE bias state per window factor: dbg, dba, dbg_buf, dba_buf
  int it, rematch, done, iters, degenerate, matches[4], ticket, planes[4], rc_ctr, pad1;  // planes: P_k (profiling pass)
  // rc_ctr: asynchronous recuts so far (k_fac_sort publishes it; vg_ctx::rc_pub mirrors it)
  // the scan this IEKF reads (set by k_scan_begin's caller, so the IEKF
  // launches are the same every scan and replay as one hipGraph)
  const float *sx, *sy, *sz;
  int sn, seq2;
  // IMU_PRE records of the window factors (preintegrated deltas, bias
  // Jacobians, cov_inv; constant once pushed): a ring, factor k at slot
  // (imu_head + k) % kMaxWin, so the slide is one index step
  int imu_head, margi_seq;  // margi_seq: the last margi head's publication number (k_margi_copy signals it)
  // the scan graph's per-scan numbers (HostIn::ph, copied by k_ins_prep's block 0):
  // [0] the LM's first flag number, [1] / [2] the margi tail's publication
  // numbers, [3] the recut-done flag value, [4] the margi prefix's flag value,
  // [5] the tail's jour_check (WinArg::jour_check)
  int ph[6];
  // jour (local_mapping.cpp:510-518) on the device, so the margi prefix's
  // stamps (k_set_jour) never wait for the host: jour_check is set by the margi
  // head, the update runs in k_slide_compact (x_buf.back().p before the slide)
  int jour_check, pad_j;
  double jour, last_pos[3];
  double imurec[kMaxWin * kBaImuRec];
  KClock clk;
  // sharded mode (world > 1): the scan's points this rank can match, made
  // once per scan at the opening pose (iekf.hip k_keep_*): raw indices,
  // ascending; null: every point. The IEKF uses the list while the pose
  // stays within kmargin of kpose for every point (|dR|_F krmax + |dp|).
  const int* skeep;
  int snk, iekf_pts;  // kept points; points the point loop processed this scan (vg_stats::iekf_points)
  double kpose[12], krmax, kmargin;
};
// x_buf.push_back(x_curr) + a new IMU_PRE record, as kernel arguments (k_push_state,
// or folded into the insert's first launch, map_insert)
struct PushArg {
  int ord, new_imu;
  double rec[kBaImuRec];
};
// IMUEKF::process's propagation (imu_ekf.cpp:13-86) on the device: the scan's
// IMU samples and times as kernel arguments; the state it starts from is the
// device's x_curr (the previous scan's, after its BA), so the host never waits
// for that state before opening the next scan (state.hip k_scan_prop)
constexpr int kPropMax = 48;  // IMU samples per scan in the arguments (more: the host path)
struct PropArg {
  int n, pad;
  double last_end, beg, end, sg;                 // last_pcl_end_time, pcl_beg/end, imupre_scale_gravity
  double cov_gyr, cov_acc, rdw_gyr, rdw_acc;     // Odometry.* (node.cpp:211-214)
  double imu[kPropMax * 7];                      // t, gyr[3], acc[3] per sample
};
// per-scan inputs of the replayed graphs, in host-mapped memory: the host
// writes them before the launch, the kernels read them in place. One per ring
// position (the steady state's graphs are per ring position, so a slot is
// rewritten W scans after the graph that read it)
struct HostIn {
  PushArg push;
  int ph[6];  // DState::ph
};
// Spatial-tile sharding of one sequence over `world` contexts (one per GPU):
// every context keeps the root voxels of the tiles it owns (tile_owner) and
// sums only its own points / factors; the normal equations are all-reduced
// (RCCL on the context stream, or a host callback for CPU-mediated tests).
constexpr int kShardBuf = 4096;  // doubles of exchange scratch / staging
constexpr int kShardSmall = 64;   // doubles of a small exchange frame (payload + guard pair)
// a frame its producer kernel packed and its consumer kernel checks (the IEKF
// sums, the LM's Hessian and residual): the all-reduce alone, no pack / unpack
// launches (shard.hip)
int shard_exchange(vg_ctx* ctx, int n, hipStream_t s = nullptr);  // s: the producer's stream (default ctx->stream)
struct Shard {
  int rank = 0, world = 1;
  int mode = 0;              // 0 none, 1 RCCL, 2 host callback
  void* comm = nullptr;      // ncclComm_t
  vg_host_allreduce_fn host_fn = nullptr;
  void* user = nullptr;
  double* h_buf = nullptr;   // pinned staging (host mode)
  double* d_buf = nullptr;   // device scratch for the exchanged sums (4096 doubles)
  int frame_n = 0;           // doubles per exchange (shard.hip: payload + guard pair)
  double* d_frame = nullptr; // the exchange frame (+ this rank's guard value)
  unsigned* d_seq = nullptr; // the device's count of exchanges (the guard's sequence number)
  // the scan's kept points (world > 1, iekf.hip k_keep_*): per raw point its
  // flag and exclusive prefix, the kept list, max |pnt| (float bits), scan scratch
  int *keep_flag = nullptr, *keep_pos = nullptr, *keep_list = nullptr;
  unsigned* keep_rmax = nullptr;
  void* keep_tmp = nullptr;
  size_t keep_tmp_bytes = 0;
};

// Host-mapped publication block (written by the device with system-scope
// stores, each part closed by a sequence flag the host spins on).
struct Pub {
  int seq_ds, n_ds, ds_err, pad0;          // downsample (after k_ds_*)
  int seq_ba, ba_word, pad1, pad1b;  // LM iteration flags (k_ba_control): iterations * 2 + done, one word (no torn pair)
  int seq_rc, rc_status, rc_nf, pad5;      // asynchronous recut status (k_fac_sort)
  int seq1, iekf_iters, degenerate, matches[4], ba_iters1, ba_hess1, planes[4], iekf_pts, pad2[2];  // P1: state after IEKF/BA
  int seq2, pad3[3];
  int counters[kCntN];                      // P2: map counters at the end of the scan
  double xc[256];
  double traj[16];
  double nnt[8];
  double xs[kMaxWin * kXS];
};
// The query-side scratch below is made of DevBuf / KernelTimer members
// (vg_scratch.h): each buffer is reserved where it is first needed and freed by
// its owner's destructor (delete ctx, or the change layer's / place index's delete)
//
// vg_score_poses / vg_relocalize scratch (score.hip): allocated on first use,
// grown geometrically (reserve_pow2)
struct ScoreBufs {
  DevBuf<float> xyz;           // the scored cloud, n x 3 as the caller gave it
  DevBuf<double> poses;        // K x 12
  DevBuf<double> partials;     // [chunk][pose of the slab][kScoreVals], or [chunk][34] + the 34 reduced sums (the normal equations)
  DevBuf<vg_pose_score> out;   // K records
  DevBuf<vg_point_match> pp;   // n records
  int n = 0;                   // points of the cloud in xyz
  KernelTimer t;               // around the last vg_score_poses call's kernels (vgx_score_ms)
};
// vg_raycast / vg_scan_diff staging (raycast.hip): one slab of
// max_points_per_scan rays (out.cap), allocated on first use
struct RayBufs {
  DevBuf<double> org;      // cap x 3 origins (vg_scan_diff: the points' |m.range - r| terms)
  DevBuf<double> dir;      // cap x 3 directions (vg_scan_diff: the cloud, n x 3 floats)
  DevBuf<vg_ray_hit> out;  // cap records (vg_scan_diff: vg_diff_point records, half the size)
  DevBuf<vg_diff_summary> sum;  // one
  KernelTimer t;           // around the last call's kernels (vgx_ray_ms)
};
// vg_localizability / vg_scan_info staging (localizability.hip), allocated on first use
constexpr int kInfoSlab = 4096;     // places per launch of k_info_places
constexpr int kInfoMaxDirs = 4096;  // D's limit
struct InfoPart;                    // localizability.hip
struct InfoBufs {
  DevBuf<double> pos;        // slab x 3 origins
  DevBuf<double> dirs;       // kInfoMaxDirs x 3 directions
  DevBuf<vg_info_rec> out;   // slab records (vg_scan_info: the first)
  DevBuf<InfoPart> part;     // vg_scan_info: one per workgroup of max_points_per_scan points
  int slab_want = 0;         // vgx_info_slab (0: kInfoSlab)
  KernelTimer t;             // around a launch's kernels; ms: the last call's, summed over its slabs (vgx_info_ms)
};
// vg_occupancy staging (occupancy.hip), allocated on first use and grown to the
// largest grid asked for
struct OccBufs {
  DevBuf<double> pos;      // kInfoSlab x 3 origins
  DevBuf<double> dirs;     // kInfoMaxDirs x 3 directions
  DevBuf<int> planes;      // 2 x cells: n_free, then n_occ
  DevBuf<int8_t> grid;     // cells
  DevBuf<vg_occ_summary> sum;  // one
  int nx = 0, ny = 0;      // the grid the last call left in `grid` (0: none yet); vg_clearance's grid == NULL reads it
  KernelTimer t;           // around a launch's kernels; ms: the last call's, summed over its slabs (vgx_occ_ms)
};
// vg_terrain planes (terrain.hip), allocated on first use and grown to the largest
// grid asked for. The origins, the directions, the two count planes and the grid
// are OccBufs': the call leaves its grid where vg_occupancy leaves its own
struct TerBufs {
  DevBuf<int> gn, gmin, gmax;      // cells each: the ground planes g_n, g_min, g_max
  DevBuf<unsigned long long> gsum; // cells: g_sum (a signed sum in two's complement)
  DevBuf<int> elev, step;          // cells each
  DevBuf<unsigned long long> sum;  // kTerSlots: the summary's counts as the kernels index them
  int nx = 0, ny = 0;              // the grid whose ground planes the last call left (0: none); vgx_ter_ground reads them
  KernelTimer t[4];                // around k_ter_ground, k_ter_cells, k_ter_marks, k_ter_classify; ms: the last call's (vgx_ter_ms)
};
// vg_clearance staging (clearance.hip), allocated on first use and grown to the
// largest grid asked for (grid.cap cells: when it grows, the other planes go). dist2 /
// nearest / cost exist only once a call asked for that output
struct ClrBufs {
  DevBuf<int8_t> grid;       // cells: a host grid's upload (grid == NULL reads OccBufs::grid instead)
  DevBuf<int16_t> dy;        // cells: k_clr_cols' plane, oy - iy of the column's nearest obstacle (kClrNone: none)
  DevBuf<int> dist2;         // cells
  DevBuf<int> nearest;       // cells
  DevBuf<uint8_t> cost;      // cells
  int nx = 0, ny = 0;        // the plane the last call that asked for `cost` left there (0: none); vg_navfn's cost == NULL reads it
  DevBuf<uint8_t> table;     // the cost by dist2, table_n entries
  DevBuf<vg_clr_summary> sum;  // one
  int table_n = 0;           // entries in use; 0: none built yet
  double table_key[4] = {0, 0, 0, 0};  // res, inscribed_radius, inflation_radius, cost_scaling the table was built from
  KernelTimer t;             // around the call's kernels; ms: the last call's (vgx_clr_ms)
};
// vg_navfn / vg_nav_paths planes and staging (navfn.hip), allocated on first use
// and grown to the largest plane asked for
struct NavBufs {
  DevBuf<uint8_t> cost;       // cells: a host plane's upload (cost == NULL reads ClrBufs::cost instead)
  DevBuf<uint16_t> trav;      // cells: the price of standing on the cell, 0 impassable (k_nav_init)
  DevBuf<uint32_t> pot;       // cells: the field
  DevBuf<int> act;            // two activity planes of act.cap / 2 tiles each: this round's and the next's
  DevBuf<uint16_t> table;     // 256 entries: trav by cost byte
  DevBuf<int> goals;          // 2 kNavMaxPoints: goals (vg_navfn) or starts (vg_nav_paths)
  DevBuf<unsigned> marks;     // kNavBatchMax counters, one per round of a batch: tiles that woke a neighbour
  DevBuf<vg_nav_summary> sum; // one
  DevBuf<int> cells_out;      // vg_nav_paths: n_starts max_len path cells
  DevBuf<int> len;            // kNavMaxPoints each: len, status; path_cost
  DevBuf<int> status;
  DevBuf<long long> path_cost;
  int nx = 0, ny = 0;         // the field the last vg_navfn call left in `pot` (0: none)
  KernelTimer t;              // around the call's kernels; ms: the last call's (vgx_nav_ms)
};
// vg_frontiers planes and staging (frontier.hip), allocated on first use and grown
// to the largest grid asked for
struct FrontierBufs {
  DevBuf<int8_t> grid;        // cells: a host grid's upload (grid == NULL reads OccBufs::grid instead)
  DevBuf<uint8_t> cost;       // cells: a host plane's upload (cost == NULL reads ClrBufs::cost instead)
  DevBuf<int> parent;         // cells: the union-find forest, -1 off the frontier; after the flatten a root's dense id
  DevBuf<int> label;          // cells: the output plane
  DevBuf<int> counts;         // kFrMaxCounts + 1: per-workgroup counts, scanned in place (roots, then kept records)
  DevBuf<vg_frontier_rec> rec;  // one per component, in ascending label; grown to the count a call finds
  DevBuf<vg_frontier_rec> out;  // VG_FRONTIER_MAX_RECORDS: the records that leave
  DevBuf<unsigned long long> sum;  // vg_frontier_summary's 16 slots, then the capacity flag
  int combine = 1;            // k_fr_stats: lanes of a wave on one component add once (vgx_frontier_combine)
  KernelTimer t;              // around the call's kernels; ms: the last call's (vgx_frontier_ms)
};
// vg_view_gain planes and staging (view.hip), allocated on first use and grown
struct ViewBufs {
  DevBuf<int8_t> grid;        // cells: a host grid's upload (grid == NULL reads OccBufs::grid instead)
  DevBuf<int> views;          // 2 VG_NAV_MAX_POINTS: the viewpoints
  DevBuf<vg_view_rec> rec;    // one per viewpoint, grown to the count a call brings
  DevBuf<int> seen;           // cells: the viewpoints per cell (kept whether or not the caller asks for it: the
                              // summary's cells_seen and unknown_seen are counted from it)
  DevBuf<unsigned long long> sum;  // vg_view_summary's 16 slots, then the packed key behind best_view
  int stage = 0;              // k_view_rays: the window's classes staged in LDS where they fit (vgx_view_stage)
  KernelTimer t;              // around the call's kernels; ms: the last call's (vgx_view_ms)
};
// The change layer (vina_gpu.h "Change layer"; change.hip, change_host.cpp): a
// side structure of the context that owns a frozen map, never part of DevMap.
// Only integer atomics write it, one accumulate call at a time (vg_ctx::change_mu of the owner).
struct ChangeNode {  // 20 B per node of the owner's pool
  int n_consistent, n_vanished, n_occluded, n_scans, last_epoch;
};
struct ChangeCell {  // 40 B per slot of the cell table (the slot's key: ChangeDev::ckey)
  long long sum_q[3];
  int n_appeared, n_scans, last_epoch, pad;
};
enum { kChgDropped = 0, kChgOutOfRange = 1, kChgTot = 2 };
struct ChangeDev {   // what the kernels take: views of the layer's buffers
  ChangeNode* node = nullptr;          // cap_nodes
  unsigned long long* ckey = nullptr;  // mask + 1 packed cell keys, kKeyEmpty: free
  ChangeCell* cell = nullptr;          // mask + 1
  long long* tot = nullptr;            // kChgTot device totals
  int cap_nodes = 0, mask = 0;
  double cell_size = 0.0;
};
struct ChangeLayer {
  ChangeDev d;
  vg_diff_params diff;   // as vg_change_begin was given them
  int epoch = 0;         // accumulate calls that succeeded so far
  long long calls = 0, points = 0, cls[4] = {0, 0, 0, 0};
  DevBuf<ChangeNode> node;  // the layer's device memory (d's pointers), freed with the layer
  DevBuf<unsigned long long> ckey;
  DevBuf<ChangeCell> cell;
  DevBuf<long long> tot;
  DevBuf<int> blk;       // the report's per-workgroup counts / offsets
  DevBuf<char> out;      // the report's record staging (bytes), grown on demand
};
// The live obstacle layer (vina_gpu.h "Live obstacle layer"; live.hip, live_host.cpp): the two stamp planes beside a
// private base grid, owned by the context it was begun on. Only integer atomic maxima write the planes.
struct LivePrm {  // vg_live_params with the defaults applied (the diff parameters: LiveLayer::diff)
  double x0, y0, res;
  double z_lo, z_hi, r_min, mark_max, clear_max;
  int nx, ny;
  int persist, unknown_marks;
};
struct LiveLayer {
  LivePrm q;
  vg_diff_params diff;        // as vg_live_begin was given them
  int stamp = 0;              // the largest stamp so far
  vg_live_summary tot = {};   // the marks' summaries summed (host side)
  DevBuf<int8_t> base;        // cells
  DevBuf<int> hit, clear;     // cells each
  DevBuf<vg_live_point> rec;  // the last mark's records, grown to the count a call brings
  DevBuf<unsigned long long> sum;  // vg_live_summary's 16 slots as the kernels index them
  DevBuf<int> cls;            // diff_wave_counts' six ints
  KernelTimer t_mark, t_walk, t_comp;  // around the last mark's kernels, its k_live_walk, the last compose (vgx_live_ms)
};
// The place index (vina_gpu.h "Place index"; places.hip, places_host.cpp): a side
// structure of the context that owns a frozen map, like the change layer. One
// query at a time (vg_ctx::places_mu of the owner): the scan's histogram, its
// descriptor and the match's results are the index's own scratch.
struct PlaceIndex {
  vg_places_params prm;       // as vg_places_build was given them (zeros: the defaults)
  int M = 0, A = 0, E = 0, n_valid = 0;
  double frame[9];            // rows ex, ey, up
  double spacing = 0.0;       // median nearest-neighbour distance of the places in the ex-ey plane (0: M == 1)
  std::vector<double> pos;    // M x 3, as given
  std::vector<int> hit;       // per place: its hit bins
  DevBuf<double> d_pos;       // M x 3
  DevBuf<double> d_dirs;      // A E x 3, world
  DevBuf<uint16_t> d_desc;    // M x E x A
  DevBuf<int> d_hit;          // M
  DevBuf<unsigned long long> d_sum;  // A E: the scan's sums of q
  DevBuf<unsigned> d_cnt;     // A E: its points per bin
  DevBuf<uint16_t> d_scan;    // A E: its descriptor
  DevBuf<int> d_scan_valid;   // its non-empty bins
  DevBuf<int> d_best;         // M x 4: best shift, its score, second shift, its score
  DevBuf<int> d_scores;       // M x A, allocated on the first request
  KernelTimer t_build;        // around the build's kernel
  KernelTimer t_query;        // around the last query's kernels, scan pass to match pass (armed: a query has run)
};
// window view for the map kernels, built on the device from DState::xs
struct WinArg {
  int mp[kMaxWin];      // mp[] ring (octree.cpp:75)
  int nper[kMaxWin];    // window points per ord
  int win_count;
  int set_xc;           // x_curr.R/p <- x_buf.back() first (local_mapping.cpp:501-502)
  int seq2;             // end-of-scan publication number (stored in DState::seq2)
  int jour_check;       // (win_base + win_count) % 10 == 0: the jour update follows the margi (local_mapping.cpp:510)
};

}  // namespace vg

struct vg_ctx {
  vg_config cfg;
  vg_capacity cap;
  int device = 0;
  hipStream_t stream = nullptr;
  // the downsample runs on its own stream: it reads only the raw scan, so it
  // overlaps the previous scan's recut/BA/margi and this scan's IEKF
  hipStream_t stream_ds = nullptr;
  // the downsample / margi prefix get a stream of their own, created on the
  // first scan; the multi-sequence mode turns it off before any scan, so its
  // contexts never hold a second hardware queue (vg_multi_create)
  bool want_ds_stream = true;
  hipEvent_t ev_ds_done = nullptr, ev_ds_free = nullptr;
  hipEvent_t ds_free_ev = nullptr;  // what the next downsample waits for: ev_ds_free, or ev_recut_done when one record marks both
  hipEvent_t ev_recut_done = nullptr, ev_prefix_done = nullptr;  // margi prefix on the second stream
  // The next scan's IEKF overlaps the margi's map-only remainder: it runs on
  // stream_iekf behind ev_tail_a (recorded after k_margi_leaf's plane updates,
  // the last margi work the IEKF reads), and the main stream waits for it
  // (ev_iekf_done) before anything else (map_margi, pipeline.cpp lio_state_estimation)
  hipStream_t stream_iekf = nullptr;
  hipEvent_t ev_tail_a = nullptr, ev_iekf_done = nullptr;
  bool tail_a_valid = false;  // ev_tail_a marks the latest main-stream work the next IEKF depends on
  hipEvent_t ev_scan_ready = nullptr;  // deskew done (row f1)
  // the IEKF's 8 launches captured once and replayed (iekf.hip iekf_run)
  hipGraphExec_t g_iekf[4] = {nullptr, nullptr, nullptr, nullptr};  // [0] the four iterations, [3] the same, signalling the insert ([1], [2] unused)
  hipGraphExec_t g_margi[4] = {};  // margi after the window view (margi.hip map_margi): [gated + 2 * signalling]
  hipGraphExec_t g_ba = nullptr;     // one LM iteration (ba.hip ba_run)
  hipGraphExec_t g_ba2 = nullptr;    // the first two LM iterations
  hipGraphExec_t g_ds = nullptr;     // the per-scan downsample chain (downsample.hip ds_enqueue_hashed)
  // steady state: the insert + recut of one scan, per ring position mp[0] (pipeline.cpp stage_insert_recut)
  hipGraphExec_t g_mid[vg::kMaxWin] = {};
  bool capturing = false;  // a stream capture is open (host-side steps that cannot be captured are deferred)
  int rc_pub = 0;          // asynchronous recuts enqueued (mirrors DState::rc_ctr, k_fac_sort)
  int ba_last_iters = 2;   // LM iterations of the previous run (ba_run's enqueue-ahead policy)
  vg::BaLoop ba_loop;      // a deferred LM run (ba_run / ba_resolve)
  bool lm_defer = true;    // the fused step returns before the LM outcome (vgx_debug 26: 0 = waits for it)
  // kernels do not run concurrently (AMD_SERIALIZE_KERNEL, or VG_SERIAL_KERNELS=1 as rocprofv3 --pmc
  // runs set): no device-flag hand-offs (a polling kernel would wait for a producer queued behind it)
  bool serial_kernels = false;
  bool counted = false;          // in the per-device live-context count (dev_ctx_count)
  bool shard_force = false;       // vg_shard_rccl at world 1 still sets up the sharded path (vgx_debug 30)
  bool flag_force = false;       // flag hand-offs even beside other contexts (vgx_debug 14 = 2: the caller drains between them)
  vg::HostIn* h_in = nullptr;  // host-mapped per-scan inputs of replayed graphs, kMaxWin slots (host address)
  vg::HostIn* d_in = nullptr;  // its device address
  int in_sel = 0;              // the slot map_insert uses (the ring position of a scan graph)
  bool in_ph = false;          // map_insert copies the slot's per-scan numbers into DState::ph (scan graph capture)
  // the scan graph (pipeline.cpp stage_insert_recut): insert + recut + k_ba_init
  // + two LM iterations + the gated margi tail, one per ring position
  hipGraphExec_t g_scan[vg::kMaxWin] = {};
  bool scan_graph = true;   // vgx_debug 27: 0 = separate insert+recut graph, LM graph, margi tail
  int ba_seq0_pre = 0;      // the LM flag numbers a scan graph's k_ba_init uses (ba_run pre > 0)
  bool ba_no_defer = false; // set by stage_ba's prefix step when the recut needs the host (no deferral)
  unsigned rc_flag_ctr = 0, pre_flag_ctr = 0;  // d_sync[3] / d_sync[4] values (scan graph hand-offs)
  bool pool_zeroed = false;  // map_reset has cleared the node records once (then only the used ids)
  bool ins_ev_pending = false;  // ev_ds_free / ev_recut_done of the last insert+recut graph not recorded yet
  bool use_graphs = true;  // margi prefix on the second stream
  bool overlap_iekf = true;  // the next IEKF under the margi remainder (lio_state_estimation)
  int pub_flags = 0;         // vg_set_publish: bit 0 = /map_cmap after each window BA (k_local_map),
                             // bit 1 = the /voxel_plane + /voxel_normal events after each recut (markers.hip)
  vg::DevBuf<vg_plane_marker> d_mk;  // the last collection's event records (allocated while bit 1 is set)
  vg::DevBuf<int> d_mk_cnt;          // [0] events reserved by the last collection (past mk_cap: deferred)
  int mk_cap = 1 << 16;             // vg_marker_capacity
  bool mk_fresh = false;            // the last opened scan ran a collection
  bool mk_keep = false;             // a checkpoint load brought the nodes' publication flags: the next enable keeps them
  float4* d_cmap = nullptr;  // the last /map_cmap cloud (x, y, z, intensity) and its size
  int* d_cmap_n = nullptr;
  bool ds_early = true;      // a fused step's downsample enqueued before the host waits for the previous state (host_step)
  bool ds_after_iekf = true; // vgx_debug 37: ... behind the device propagation's launch (0: ahead of it)
  bool spec_tail = true;     // the margi tail behind the predicted LM iterations (stage_ba)
  std::string err;
  vg::Arena arena;
  // raw scan staging (SoA)
  float *d_x = nullptr, *d_y = nullptr, *d_z = nullptr, *d_i = nullptr, *d_t = nullptr;
  // the scan the stage-level API works on (own staging or caller's HBM)
  const float *cur_x = nullptr, *cur_y = nullptr, *cur_z = nullptr, *cur_i = nullptr;
  int cur_n = -1;
  vg::DownsampleBufs ds;
  vg::KdMap kd;
  vg::DevMap map;
  vg::Work wk;
  vg::BaBufs ba;
  vg::DState* st = nullptr;     // device-resident estimator state
  vg::Shard shard;              // spatial-tile sharding across contexts (shard.cpp)
  vg::Pub* h_pub = nullptr;     // host-mapped publication block (host address)
  vg::Pub* d_pub = nullptr;     // its device address
  double* h_stage = nullptr;    // pinned staging for asynchronous H2D copies (kStageBytes)
  double* d_deskew = nullptr;   // deskew parameters (x_curr pose, extrinsic, IMU poses)
  int pub_seq = 0;
  int wait_spin_us = 0, wait_sleep_us = 0;  // vg_set_wait_policy (0 sleep: spin)
  int plane_tag = 0;        // IEKF iteration tag of the P_k count (vg_profile stages)
  int* h_pinned = nullptr;  // small pinned host scratch for counters
  // host-input scans (vg_step / vg_step_deskew): two slots in flight, each the
  // caller's arrays copied once into pinned memory, one DMA to HBM and an
  // AoS -> SoA unpack on stream_ds ahead of the scan's kernels, no host wait
  // on the device (vina_gpu.cpp upload_scan)
  struct InSlot {
    char* h = nullptr;          // pinned: xyz AoS (12 B/pt) | intensity | time, packed by n
    float* d = nullptr;         // HBM: the DMA image (5 cap floats), then the SoA planes x y z i t
    hipEvent_t up = nullptr;    // unpack done (stream_ds): the DMA has read h
    hipEvent_t done = nullptr;  // main stream past the scan that read the planes
    bool live = false;
  } in_slot[2];
  size_t in_cap = 0;  // points per slot
  void* copy_pool = nullptr;  // helper threads of the pinned copy (vina_gpu.cpp CopyPool)
  int in_next = 0;
  hipEvent_t in_ev = nullptr;  // the current scan's unpack (the split IEKF stream waits for it)

  bool mapping = true;       // vg_set_mapping: false = the map is read-only (pipeline.cpp frozen_step)
  // map views (vg_map_attach, localize.cpp): a tracker's `map` holds the owner's
  // pointers, read-only; its own records wait in own_map until the detach
  vg_ctx* view_of = nullptr;  // attached: the owner
  int views = 0;              // an owner: the trackers attached to its map
  vg::DevMap own_map;         // an attached tracker's own map
  void* fleet = nullptr;      // a fleet's tracker (vg_fleet_create): stepped only through the fleet
  vg::ScoreBufs score;       // vg_score_poses / vg_relocalize scratch (score.hip), allocated on first use
  vg::RayBufs ray;           // vg_raycast / vg_scan_diff staging (raycast.hip), allocated on first use
  vg::InfoBufs info;         // vg_localizability / vg_scan_info staging (localizability.hip), allocated on first use
  vg::OccBufs occ;           // vg_occupancy staging and count planes (occupancy.hip), allocated on first use
  vg::TerBufs ter;           // vg_terrain planes (terrain.hip), allocated on first use
  vg::ClrBufs clr;           // vg_clearance staging and planes (clearance.hip), allocated on first use
  vg::NavBufs nav;           // vg_navfn / vg_nav_paths planes (navfn.hip), allocated on first use
  vg::FrontierBufs fr;       // vg_frontiers planes (frontier.hip), allocated on first use
  vg::ViewBufs view;         // vg_view_gain planes (view.hip), allocated on first use
  vg::ChangeLayer* change = nullptr;  // the change layer of this context's map (vg_change_begin .. vg_change_end)
  std::mutex change_mu;      // serialises every call into this context's layer, vg_change_end included: a caller
                             // (the owner or an attached tracker) reads `change` only while holding it
  vg::LiveLayer* live = nullptr;     // the live obstacle layer of this context (vg_live_begin .. vg_live_end)
  vg::PlaceIndex* places = nullptr;  // the place index of this context's map (vg_places_build .. vg_places_end)
  std::mutex places_mu;      // the same discipline for `places`
  vg_stats stats;
  void* host = nullptr;     // host-side pipeline state (HostPipe, vg_host.h)
  // stage timing with HIP events on the context stream (vg_profile)
  bool prof_on = false;      // k_iekf launch events (vg_profile bit 0)
  int prof_every = 0;        // sample k_ba_solve events on every n-th BA run (vg_profile bits 8-15)
  long prof_runs = 0;
  int rc_total = 0, rc_thread_num = 0;  // the last recut's window point total / thread_num (its resume)
  bool prof_stages = false;  // per-stage events (vg_profile bit 1)
  bool ins_count = true;     // vgx_debug 38: the insert counts its buckets in the descent (0: k_ins_resolve + k_seg_offsets)
  bool push_pipe = false;    // vgx_debug 39: 1 = k_push_window loads a block's records ahead of the previous block's sums and ranks
                             // mid-size segments from LDS (bit-identical; measured 29.0 -> 30.6 us, so off: DESIGN.md section 6)
  bool roots_lb = true;      // root registration in one look-back launch (vgx_debug 16: 0 = two launches)
  bool ba_graph2 = true;     // the first two LM iterations as one graph (vgx_debug 17: 0 = one graph each)
  bool margi_batch = true;    // vgx_debug 24: k_margi_leaf reads a leaf's frame clusters four at a time (r04k +0.4 %)
  bool margi_fused = true;    // margi isexist bottom-up in k_margi_copy, erase in one launch (vgx_debug 21: 0 = per-level launches)
  bool iekf_prefetch = true;  // vgx_debug 23: k_iekf touches a cached match's plane record beside its header (r04i A/B +0.9 %)
  bool ba_structural = true;      // vgx_debug 31: k_ba_prep's structural elimination order (0: Eigen's |diag| order)
  bool ba_resid_hess = true;      // vgx_debug 34: k_ba_resid_hess in the two-iteration LM graphs (0: k_ba_resid + k_ba_hess)
  bool ba_init_hess = true;       // vgx_debug 35: k_ba_init inside the scan graph's first Hessian pass (0: its own launch)
  bool rc_init_finish = true;     // vgx_debug 32: the asynchronous recut's factor bookkeeping inside k_ba_init (0: k_factor_finish_dev)
  bool rc_finish_in_init = false; // set by map_recut for the next k_ba_init
  bool rc_begin_fold = true;      // vgx_debug 33: the recut's head in the insert's k_push_window (insert + recut graph)
  const vg::WinArg* rc_begin_wa = nullptr;  // set for one map_insert: its k_push_window runs the recut's head
  bool rc_begun = false;          // ... and the map_recut after it skips k_make_win_recut_begin
  bool ba_fuse_ctl = true;    // vgx_debug 19: the LM bookkeeping in k_ba_resid's IMU workgroup (A/Bs r04e 0, r04g/h +0.8-0.9 %)
  bool ba_graph = true;      // LM iterations replay one captured graph each (vgx_debug 15: 0 = direct launches)
  bool flag_sync = true;     // counter hand-offs instead of event waits on the critical path (vgx_debug 14)
  unsigned* d_sync = nullptr;  // hand-off flags: [0] margi leaf -> next IEKF, [1] IEKF -> insert, [2] margi head -> propagation,
                               // [3] recut done -> margi prefix, [4] margi prefix -> tail (scan graph)
  bool sync_tail_armed = false;  // the last margi's leaf pass stores sync_tail_value into d_sync[0]
  unsigned sync_tail_value = 0, sync_iekf_value = 0;
  bool dev_prop = false;     // host_step propagates on the device (k_scan_prop; vgx_debug 13: 1 = on the device)
  bool rc_fused = true;      // the fused recut levels (vgx_debug 11: 0 = the four-launch level loop)
  bool prof_clock = false;   // in-kernel clocks instead of k_ba_solve events (vg_profile bit 2, KClock)
  hipEvent_t prof_ev[8][2] = {};
  hipEvent_t sync_ev = nullptr;  // host-spin synchronisation (vg::stream_wait)
  hipEvent_t iekf_ev[16][2] = {};  // k_iekf launches of the last two scans (vg_profile), 8 per scan
  int iekf_ring_n = 0, iekf_ring_base = 0;
  hipEvent_t solve_ev[10][2] = {};  // k_ba_solve launches of the current BA run (vg_profile)
  int dbg_apply_cap = -1;        // test knob (vgx_debug): recut apply event capacity
  int dbg_ins_cap = -1;   // vgx_debug 3: k_ins_alloc capacity override (forces the insert replay)
  int dbg_fac_max = -1;   // vgx_debug 4: device factor-sort limit override (forces the host factor path)
  int dbg_capture = 0;    // vgx_debug 5: capture the next LM run's first Hessian pass (vgx_ba_capture)
  double* dbg_cap_buf = nullptr;  // device copy: LiDAR hl (lower) + IMU factor blocks
  int dbg_cap_n = 0;
  bool prof_pending[16] = {};
  double prof_ms[16] = {};  // [0, 8): device time (events); [8, 16): host time of the stage calls
  int prof_n[16] = {};
};

namespace vg {
constexpr int kTrajRow = 13;  // vg_trajectory: t, R 9, p 3
constexpr int kPathRow = 14;  // vg_path: t, R 9, p 3, jour (the path point's curvature)
constexpr size_t kStageBytes = 1 << 17;
constexpr size_t kStageDeskewOff = 8192;  // doubles: the deskew block's part of the staging area
constexpr int kDeskewBuf = 4096;          // doubles (up to 180 IMU segments per scan)
// Spin until a Pub sequence flag reaches seq (the device publishes with a
// system-scope release); checks the stream for errors while spinning.
// Wait policy (vg_set_wait_policy): spin for spin_us, then sleep sleep_us per
// poll. Pure spinning (the default) has the lowest latency for one context;
// several contexts driven from their own threads under a CPU quota need the
// sleeping polls, or the spinning threads starve each other's launches.
inline void wait_pause(const vg_ctx* c, long spin, std::chrono::steady_clock::time_point t0);
inline int pub_wait(vg_ctx* c, const int* flag, int seq, const char* what, hipStream_t producer = nullptr) {
  hipStream_t st = producer ? producer : c->stream;  // the stream the publishing kernel runs on
  const auto t0 = std::chrono::steady_clock::now();
  for (long spin = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) < seq; spin++) {
    wait_pause(c, spin, t0);
    if ((spin & 4095) == 4095) {
      const hipError_t e = hipStreamQuery(st);
      if (e != hipSuccess && e != hipErrorNotReady) {
        c->err = std::string(what) + ": " + hipGetErrorString(e);
        return VG_E_HIP;
      }
      if (e == hipSuccess && __atomic_load_n(flag, __ATOMIC_ACQUIRE) < seq) {
        c->err = std::string(what) + ": stream drained without publishing";
        return VG_E_HIP;
      }
    }
  }
  return VG_OK;
}
enum { kProfDownsample = 0, kProfIekfKernel = 1, kProfInsert = 2, kProfRecut = 3, kProfBA = 4, kProfMargi = 5,
       kProfIekf = 6, kProfBaSolve = 7, kProfN = 8,
       // host (CPU) time spent in the stage calls: enqueue work plus any wait
       kHostPropagate = 8, kHostDownsample = 9, kHostIekf = 10, kHostPush = 11, kHostInsert = 12, kHostRecut = 13,
       kHostBA = 14, kHostMargi = 15, kProfAll = 16 };
// host-time scope for a stage call (vg_profile bit 0)
struct HostTimer {
  vg_ctx* c;
  int id;
  std::chrono::steady_clock::time_point t0;
  HostTimer(vg_ctx* ctx, int i) : c(ctx), id(i), t0(std::chrono::steady_clock::now()) {}
  ~HostTimer() {
    if (!c->prof_on) return;
    c->prof_ms[id] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->prof_n[id] += 1;
  }
};
inline void prof_begin(vg_ctx* c, int id, hipStream_t s = nullptr) {
  if (c->prof_stages) (void)hipEventRecord(c->prof_ev[id][0], s ? s : c->stream);
}
inline void prof_end(vg_ctx* c, int id, hipStream_t s = nullptr) {
  if (c->prof_stages) {
    (void)hipEventRecord(c->prof_ev[id][1], s ? s : c->stream);
    c->prof_pending[id] = true;
  }
}
// Wait for the context stream by spinning on an event: a blocking
// hipStreamSynchronize may sleep and costs up to ~100+ us of wake-up latency
// per round trip, and the map stages make several per scan.
inline hipError_t stream_wait(vg_ctx* c, hipStream_t s = nullptr) {
  hipError_t e = hipEventRecord(c->sync_ev, s ? s : c->stream);
  if (e != hipSuccess) return e;
  const auto t0 = std::chrono::steady_clock::now();
  for (long spin = 0; (e = hipEventQuery(c->sync_ev)) == hipErrorNotReady; spin++) wait_pause(c, spin, t0);
  return e;
}
inline void wait_pause(const vg_ctx* c, long spin, std::chrono::steady_clock::time_point t0) {
#if defined(__x86_64__)
  __builtin_ia32_pause();
#endif
  if (c->wait_sleep_us <= 0 || (spin & 63) != 63) return;
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  if (us >= c->wait_spin_us) std::this_thread::sleep_for(std::chrono::microseconds(c->wait_sleep_us));
}
}  // namespace vg

namespace vg {
// Hot-path parameters in kernel-argument form (node.cpp:52-291 values).
struct MP {
  double vs;          // Odometry.voxel_size
  double min_eig;     // Odometry.min_eigen_value
  double thre[4];     // 1 / LocalBA.plane_eigen_value_thre (node.cpp:256-259)
  double minpt[4];    // min_point (node.cpp:219)
  double extR[9], extt[3];
  float dept, beam;   // dept_err / beam_err as the float params of calcBodyVar
  int max_layer, max_points, W, pad;
  double beam_dv;     // sin^2(beam * pi / 180) of calcBodyVar (point_utils.cpp:13-14), with beam in float
};

struct WinD {           // window poses x_buf (by ord) and the ring mp[] (octree.cpp:75)
  double R[32][9];
  double p[32][3];
  int mp[32];
  int win_count;
  int pad;
};


// downsample.hip
int ds_alloc(vg_ctx* ctx);
// kdlio.hip
int kd_alloc(vg_ctx* ctx);
int kd_reset(vg_ctx* ctx);
// one pass of the kd-tree IEKF over the scan in ctx->d_x/y/z (n points, raw
// LiDAR frame) at pose (R row-major 9, p 3): refind -> kNN + plane fits, then
// the 28 sums (HTH upper 21, HTz 6, valid count) -> out28 (synchronous)
int kd_pass(vg_ctx* ctx, int n, const double* R, const double* p, int refind, double* out28);
// append the scan at pose (R, p) to the map, re-downsample at 0.5 m, rebuild
// the cell index (synchronous); or only append + index when the map is seeding
int kd_update(vg_ctx* ctx, int n, const double* R, const double* p, bool downsample);
// Voxel-grid downsample of a device-resident SoA cloud; results land in
// ctx->ds.o* (n_out voxels, ascending packed-key order). Host-synchronous
// (returns n_out).
int ds_run(vg_ctx* ctx, const float* x, const float* y, const float* z, const float* in, int n, double voxel,
           int* n_out);
// down_sampling_close of a device cloud (the initialisation's raw-cloud
// reduction): out = the chosen points (x, y, z, t) sorted by time, stable over
// ascending voxel keys; t == nullptr gives every point the time tconst.
// Host-synchronous.
int ds_close(vg_ctx* ctx, const float* x, const float* y, const float* z, const float* t, float tconst, int n,
             double voxel, float4* out, int* n_out);
// The per-scan pipeline's downsample (hashed, no sort, no host count; output
// in first-occurrence order), asynchronous on s, with the /2 fallback on the
// device when `fallback`; the voxel count stays in ds.hflags[1].
int ds_enqueue_hashed(vg_ctx* ctx, hipStream_t s, const float* x, const float* y, const float* z, const float* in,
                      int n, double voxel, bool fallback, int pub_seq);
int ds_reset(vg_ctx* ctx);
// Same, asynchronous: n_out and the range flag are published to Pub (seq_ds).
int ds_enqueue(vg_ctx* ctx, hipStream_t s, const float* x, const float* y, const float* z, const float* in, int n,
               double voxel, int pub_seq);
// map.hip
int map_alloc(vg_ctx* ctx);
// The insert+recut graph's completion events are recorded lazily: right
// behind the LM's k_ba_init when the LM follows (a marker packet straight
// after the graph delays the next dispatch), else before their first waiter.
// Recording later only makes the waiters wait longer.
inline hipError_t flush_insert_events(vg_ctx* ctx) {
  if (!ctx->ins_ev_pending) return hipSuccess;
  ctx->ins_ev_pending = false;
  ctx->ds_free_ev = ctx->ev_recut_done;  // one record marks both (each record is a gap in the stream)
  return hipEventRecord(ctx->ev_recut_done, ctx->stream);
}
int map_reset(vg_ctx* ctx);
// iekf.hip
int iekf_iteration(vg_ctx* ctx, const MP& mp, const float* x, const float* y, const float* z, int n, int it,
                   hipEvent_t ev0, hipEvent_t ev1, int tag = 0, hipStream_t s = nullptr,
                   unsigned* done_flag = nullptr);
// all four iterations; replays the captured graph when possible
// begin_xc != nullptr: open the scan on the device first (x_curr after
// propagation, one launch with the scan binding)
// *signalled: the run itself advanced the IEKF -> insert hand-off flag
// (d_sync[1], by one; k_iekf_all's update workgroup after a release), so the
// caller need not enqueue k_sync_set (signal: the caller wants it)
int iekf_run(vg_ctx* ctx, const MP& mp, const float* x, const float* y, const float* z, int n, int bank,
             const double* begin_xc = nullptr, hipStream_t s = nullptr, const PropArg* begin_prop = nullptr,
             bool signal = false, bool* signalled = nullptr, bool opened = false);  // opened: scan already bound
int iekf_grid(vg_ctx* ctx);  // k_iekf's workgroups (iekf.hip iekf_blocks)
int map_memo_probe(vg_ctx* ctx, const MP& mp, int* out);  // test-only (vgx_memo_probe)
// insert.hip
// the initialisation's insert source (cut_voxel, initialization.cpp:229-246):
// n fp64 body points, the kXC pose/covariance block of x_buf[i], both device
struct InsPre {
  const double* pnt;
  const double* pose;
  int var_identity;  // 1: identity body covariance, no pvec_update (before convergence)
};
// push: the window push to fold into the insert's first launch (or nullptr);
// pre: insert precomputed body points instead of the downsampled scan
// nd: the point count on the device (n is then an upper bound, for grid sizes)
int map_insert(vg_ctx* ctx, const MP& mp, int slot, int n, int epoch, int thread_num, const PushArg* push = nullptr,
               const InsPre* pre = nullptr, const int* nd = nullptr);
int map_insert_replay(vg_ctx* ctx, const MP& mp, int slot, int n, int thread_num);
int map_insert_segments(vg_ctx* ctx, int* key, int* len, int cap, int* info);  // test hook (vgx_insert_segments)
// recut.hip
constexpr int kNeedInsertReplay = 1;  // map_recut: the insert overflowed k_ins_alloc, replay it first
int map_recut(vg_ctx* ctx, const MP& mp, const WinArg& wa, int thread_num, int* n_factors, bool replay = false,
              int pub_seq = 0);
int map_recut_resume(vg_ctx* ctx, const MP& mp, int* n_factors);
const int* map_rc_status(vg_ctx* ctx);  // the asynchronous recut's status word (k_fac_sort)
int map_factor_finish(vg_ctx* ctx);  // k_factor_finish_dev when no k_ba_init took it
// margi.hip
// multi_margi + the device-state slide; publishes the state (pub_seq, before
// the margi kernels) and the end-of-scan counters (pub_seq2)
// flags (the scan graph): {recut-done value of d_sync[3] to wait for, value to
// store into d_sync[4] at the end}; nullptr: event waits
int map_margi_prefix(vg_ctx* ctx, const MP& mp, int slot0, int n_oldest, int thread_num,
                     const unsigned* flags = nullptr);
int map_margi(vg_ctx* ctx, const MP& mp, const WinArg& wa, int n_oldest, int thread_num, int pub_seq, int pub_seq2,
              const int* gate);
int map_margi_tail_capture(vg_ctx* ctx, const MP& mp, const WinArg& wa);  // the scan graph's gated margi tail
// state.hip
int sync_set(vg_ctx* ctx, hipStream_t s, int k, unsigned value, const int* gate = nullptr);  // cross-stream flags
int sync_wait(vg_ctx* ctx, hipStream_t s, int k, unsigned target);
int sync_wait_dev(vg_ctx* ctx, hipStream_t s, int k, const int* target, const int* gate);  // target / gate on the device
int state_alloc(vg_ctx* ctx);
// x_curr / x_prop / IEKF flags; with x != nullptr also the scan the IEKF reads
// prop: propagate on the device (k_scan_prop), optionally waiting inside for
// the margi head's flag (before the rotation chain) and the leaves' flag (at
// its end); see state.hip
int state_scan_begin(vg_ctx* ctx, const double* xc249, const float* x = nullptr, const float* y = nullptr,
                     const float* z = nullptr, int n = 0, hipStream_t s = nullptr, const PropArg* prop = nullptr,
                     const unsigned* head_flag = nullptr, unsigned head_target = 0,
                     const unsigned* leaf_flag = nullptr, unsigned leaf_target = 0);
int state_set_scan(vg_ctx* ctx, const float* x, const float* y, const float* z, int n, hipStream_t s = nullptr);
int state_push(vg_ctx* ctx, int ord, int new_imu, const double* imurec);  // imurec: kBaImuRec doubles (new_imu >= 0)
int state_publish(vg_ctx* ctx, int win_count, const int* ba_iters_dev, int seq, const int* gate = nullptr);
int state_publish_counters(vg_ctx* ctx, int seq);
int state_publish_ds(vg_ctx* ctx, hipStream_t s, int seq, int* flags, bool reset);
int state_deskew(vg_ctx* ctx, const double* par, int npose, const float* x, const float* y, const float* z,
                 const float* in, const float* t, int n);
int state_unpack_scan(vg_ctx* ctx, hipStream_t s, int n, const float* img, bool has_i, bool has_t, float* x, float* y, float* z,
                      float* in, float* t);
// initialisation: motion_blur's per-point part on a close-downsampled
// cloud (pts, ascending time) -> nout fp64 body points; par (host): frame pose,
// extrinsic, npose IMU pose records (descending start); synchronous
int state_blur_init(vg_ctx* ctx, const double* par, int npose, const float4* pts, int n, int j0, int q0, int nout,
                    double* d_par, double* pnt);
// window states / x_curr / IMU records (+ zero bias, ring head 0) -> DState; synchronous
int state_load(vg_ctx* ctx, const double* xs, int nw, const double* xc, const double* recs, int nrec);
// ba.hip (the driver), ba_factor.hip (ba_lidar_pass, ba_factor_normals,
// ba_control_test, ba_factors_test), ba_solve.hip (ba_solve_test, ba_step_test)
constexpr int kBaX = 24;       // per-frame state: R 9, p 3, v 3, bg 3, ba 3, g 3
int ba_alloc(vg_ctx* ctx);
// LM on the device state (window states, IMU_PRE records and bias records in
// DState; the factor count in the map counters). Returns once the LM has
// converged on the device (the flags are read without draining the stream).
// before_first_wait: enqueued once the first iterations are; spec_tail (may
// decline through its flag): the margi tail, enqueued right behind the
// iteration count the previous run converged at and gated on the device by
// ba_gate_dev; *tail_ok tells whether that copy is the one that runs
// pending != nullptr: the run may return once the speculative tail is queued
// (*pending = true, *iters = -1); ba_resolve then continues it
// pre > 0: the scan graph already holds k_ba_init, the first `pre`
// iterations and the gated margi tail (flag numbers from ctx->ba_seq0_pre)
int ba_run(vg_ctx* ctx, int nf, const int* mp_ring, int* iters,
           const std::function<int()>& before_first_wait = nullptr,
           const std::function<int(bool*)>& spec_tail = nullptr, bool* tail_ok = nullptr, bool* pending = nullptr,
           int pre = 0);
// the scan graph's LM part, captured on the context stream (k_ba_init with its
// numbers from DState::ph, iterations 0 and 1)
int ba_capture_scan_lm(vg_ctx* ctx, const int* mp_ring);
// the rest of a deferred run (ctx->ba_loop): waits for the iteration flags and
// enqueues further iterations as ba_run would have. block = false: returns
// with *finished = false as soon as a flag it needs is not published yet.
// *tail_ok: the speculative tail is the copy that runs (else the caller
// enqueues the real one)
int ba_resolve(vg_ctx* ctx, bool block, bool* finished, int* iters, bool* tail_ok);
const int* ba_iters_dev(vg_ctx* ctx);
const int* ba_gate_dev(vg_ctx* ctx);  // 1 once the LM run has finished (converged or 10 iterations)
const int* ba_hess_dev(vg_ctx* ctx);  // Hessian passes of the last LM run (I_H of SURVEY 8(d))
// LiDAR factor passes for a host-driven LM (initialisation): Hessian pass at
// `poses` (lower 6W x 6W, gradient, residual into out) or residual pass at
// `poses` (*out); synchronous
int ba_lidar_pass(vg_ctx* ctx, bool hessian, const double* poses, const int* mp_ring, double* out);
int ba_factor_normals(vg_ctx* ctx, std::vector<double>& normals);
int ba_solve_test(vg_ctx* ctx, const double* A, const double* b, double* x);  // vgx_ba_solve  // column 0 of each factor's eigenvectors
int ba_step_test(vg_ctx* ctx, const double* hl, const double* imuout, const double* xs, const double* bias, double u,
                 double v, int calc_hess, double* dxi, double* xt, double* bias_out, double* q1_res1, int* ipg,
                 double* Hcalc, double* Jcalc);  // vgx_ba_step
int ba_control_test(vg_ctx* ctx, double* sd, int* si, const double* imures, const double* rpart, int nrb, double* xs,
                    const double* xt, double* bias);  // vgx_ba_control
int ba_factors_test(vg_ctx* ctx, int nf, const int* fac_node, int nn, const int* nodes, const double* clus,
                    const double* fix, const double* poses, const int* mp_ring, int G, int nrb, double* hl,
                    double* resid, double* eig, double* pcr);  // vgx_ba_factors
int ba_imu_test(vg_ctx* ctx, int head, const double* rec, const double* bias, const double* xs, const double* xt,
                double poison, double* imuout_hess, double* imures_resid, double* imuout_rh,
                double* imures_rh);  // vgx_ba_imu
// host_mirror.cpp: the host mirror's lifetime, absorption and accessors
// (host_sync, host_stats_log below as well)
void host_init(vg_ctx* ctx);
void host_free(vg_ctx* ctx);
void host_reset(vg_ctx* ctx);
void host_seed(vg_ctx* ctx, const double* s);
int host_state(vg_ctx* ctx, double* s);
int host_window(vg_ctx* ctx, double* out);
int host_traj(vg_ctx* ctx, double* out, int cap, int from = 0);  // rows [from, from + cap), returns the row count
int host_path(vg_ctx* ctx, double* out, int cap);
int host_poll(vg_ctx* ctx);
int host_win_count(vg_ctx* ctx);
// pipeline.cpp: the per-scan loop (host_step_deskew, the stage_* entry points,
// host_quiesce and host_release_* below as well)
int host_step(vg_ctx* ctx, const float* dx, const float* dy, const float* dz, const float* di, int n, double beg,
              double end, const double* imu, int m);
int host_memo_probe(vg_ctx* ctx, int* out);  // map_memo_probe with the context's map parameters
int iekf_update_test(vg_ctx* ctx, int nb, const double* partials, int n_points, const double* x_curr,
                     const double* x_prop, int it, int rematch, double* x_out, double* G6_out,
                     int* flags_out);  // vgx_iekf_update
// imu_prop.cpp
int scan_prop_test(vg_ctx* ctx, const double* x_in, int n, const double* imu, double last_end, double beg, double end,
                   double* xc_out, double* xp_out, double* host_out);  // vgx_scan_prop
int imu_record_test(const double* bg, const double* ba, const double* imu, int n, double sg, const double* noise_meas,
                    const double* noise_walk, double* rec);  // vgx_imu_record
// shard.cpp
int shard_alloc(vg_ctx* ctx);
void shard_free(vg_ctx* ctx);
int shard_allreduce(vg_ctx* ctx, const void* send, void* recv, int count, int dtype, int site);
int host_sync(vg_ctx* ctx);
// the sharded path (collectives at the exchange points, direct launches): a
// shard transport is set (vg_shard_rccl / vg_shard_host with world > 1, or
// world 1 with vgx_debug 30: the sharded path's own cost on one GPU)
inline bool sharded(const vg_ctx* c) { return c->shard.mode != 0; }
// live contexts on a HIP device in this process (vina_gpu.cpp): with more than
// one, each context's three streams share the device's hardware queues
// (GPU_MAX_HW_QUEUES, 4 by default) with another's, and a polling hand-off
// kernel could wait on a producer queued behind it: the flag hand-offs are off
int dev_ctx_count(int device);
// Graph capture and instantiation are serialised across the process's
// contexts (one-time work per context): the multi-sequence mode's worker
// threads otherwise capture concurrently (B = 16: sixteen threads at once).
std::recursive_mutex& capture_mutex();
// Capture `body` (int(): VG_OK or an error) on `s` once and keep the
// instantiated graph in *ge (a no-op once *ge is set). Holds capture_mutex();
// the capture is thread-local and always ended; the body's error comes before
// the capture's.
template <class Body>
int capture_once(vg_ctx* ctx, hipStream_t s, hipGraphExec_t* ge, Body&& body) {
  if (*ge) return VG_OK;
  std::lock_guard<std::recursive_mutex> cap_lk_(capture_mutex());
  VG_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  const int r = body();
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(s, &g);
  if (r != VG_OK) {
    if (e == hipSuccess && g) (void)hipGraphDestroy(g);
    return r;
  }
  VG_HIP(e);
  VG_HIP(hipGraphInstantiate(ge, g, nullptr, nullptr, 0));
  VG_HIP(hipGraphDestroy(g));
  return VG_OK;
}
void graphs_drop(vg_ctx* ctx);  // destroy every captured graph (vina_gpu.cpp): ctx->map is about to name other memory
int host_release_far(vg_ctx* ctx, int flags, long long* out);
bool host_release_pending(vg_ctx* ctx);  // jour advanced in an absorbed scan since the last release
// lifetime.hip: the journey release + the node pool / point_fix arena compaction
int map_release(vg_ctx* ctx, bool release, int thr, double jour, int compact, long long* out);
int map_roots(vg_ctx* ctx, long long* key, double* jour, int* flags, int* nodes, int* nfix, int cap, int* count);
// map_dump.cpp (test hook vgx_map_nodes): the map node for
// node in the oracle's record (oracle/vina_oracle.h ORC_NODE_REC / ORC_NODE_SLOT),
// assembled on the host from copies of the pool arrays; no device state changes
constexpr int kNodeRec = 131, kNodeSlot = 11;
int host_map_nodes(vg_ctx* ctx, double* rec, int cap, double* fixp, long long* fix_off, double* winp,
                   long long* win_off, long long* info);
// the root hash rebuilt from (key, id) pairs filed by id, by the bidding rounds (lifetime.hip)
int map_hash_place(vg_ctx* ctx, int nl, long nroots, const uint64_t* rkey, int* pos, int* rcnt, const char* who);
// checkpoint.hip / ckpt_host.cpp: the host mirror's part of a checkpoint (a byte
// blob, one section of the file). host_ckpt_parse only reads: it fills an
// opaque snapshot that host_ckpt_install puts in place after the reset
// (host_ckpt_drop frees one that was not installed)
int host_ckpt_allowed(vg_ctx* ctx, const char* who, bool save);  // VG_E_STATE: open scan, sharded, (save) cold start initialising
void host_ckpt_blob(vg_ctx* ctx, std::vector<unsigned char>& out);
int host_ckpt_parse(vg_ctx* ctx, const unsigned char* p, size_t n, void** snap);
void host_ckpt_install(vg_ctx* ctx, void* snap);
void host_ckpt_drop(void* snap);
int checkpoint_save(vg_ctx* ctx, const char* path, long long* bytes, double* t_ms);  // t_ms: 4 phase times or null
int checkpoint_load(vg_ctx* ctx, const char* path, double* t_ms);
// markers.hip: the /voxel_plane + /voxel_normal events (local_mapping.cpp:455-470)
int markers_enable(vg_ctx* ctx, bool on);  // blank slate either way; the event buffer lives while on
int markers_collect(vg_ctx* ctx);          // one collection over surf_map_slide, on the context stream
int markers_read(vg_ctx* ctx, vg_plane_marker* out, int cap, int* n, int* deferred);
int map_planes(vg_ctx* ctx, int flags, vg_plane_marker* out, int cap, int* n);
// score.hip: OctoTree::match for one cloud under K poses (host arrays in, host
// records out; synchronous on the context stream, which the caller drained).
// xyz == nullptr: the cloud the last call uploaded
int score_poses_dev(vg_ctx* ctx, const MP& mp, const float* xyz, int n, const double* poses, int K,
                    const double* pose_var, vg_pose_score* out, void* per_point);
// the IEKF's 34 sums (HTH, HTz, nnt, matches) of the uploaded cloud at one pose
int score_normal_dev(vg_ctx* ctx, const MP& mp, const double* pose12, const double* pose_var, double* out34);
// raycast.hip: rays through the map to the first plane (host arrays in, host
// records out; synchronous on the context stream, which the caller drained)
int raycast_dev(vg_ctx* ctx, const MP& mp, const double* origins, int n_origins, const double* dirs, int n,
                const vg_ray_params* prm, vg_ray_hit* out);
// a scan's points against the map's expected range along their beams, at pose12
int scan_diff_dev(vg_ctx* ctx, const MP& mp, const float* xyz, int n, const double* pose12,
                  const vg_diff_params* prm, vg_diff_point* per_point, vg_diff_summary* out);
int ray_bufs(vg_ctx* ctx);  // the staging, allocated on first use
void diff_sum_launch(hipStream_t s, const double* absv, int n, vg_diff_summary* d_sum);  // k_diff_sum
// localizability.hip: the information matrix per place / of a scan at pose12 (host arrays in, host records out;
// synchronous on the context stream, which the caller drained)
int localizability_dev(vg_ctx* ctx, const MP& mp, const double* positions, int M, const double* dirs, int D,
                       const vg_info_params* prm, vg_info_rec* out);
int scan_info_dev(vg_ctx* ctx, const MP& mp, const float* xyz, int n, const double* pose12,
                  const vg_diff_params* diff, const vg_info_params* prm, vg_info_rec* out);
// occupancy.hip: the occupancy grid of M origins x D directions (host arrays in; grid, counts (or null) and
// summary out; synchronous on the context stream, which the caller drained). prm: checked by the caller
int occupancy_dev(vg_ctx* ctx, const MP& mp, const double* positions, int M, const double* dirs, int D,
                  const vg_occ_params* prm, int8_t* grid, int32_t* counts, vg_occ_summary* out);
// terrain.hip: the terrain layer of M origins x D directions (host arrays in; grid, elev, step, counts (each or
// null) and summary out; synchronous on the context stream, which the caller drained). prm: checked by the caller
int terrain_dev(vg_ctx* ctx, const MP& mp, const double* positions, int M, const double* dirs, int D,
                const vg_terrain_params* prm, int8_t* grid, int32_t* elev, int32_t* step, int32_t* counts,
                vg_terrain_summary* out);
// clearance.hip: the clearance field and costmap of an nx x ny grid (host grid in, or null: the grid the last
// vg_occupancy left on the device; dist2, nearest, cost (each or null) and summary out; synchronous on the
// context stream, which the caller drained). prm: checked by the caller; table: the cost by dist2, table_n
// entries (dist2 >= table_n costs 0), or null where clr_table_current says the device's is that table
bool clr_table_current(const vg_ctx* ctx, const vg_clr_params* prm, int table_n);
int clearance_dev(vg_ctx* ctx, const int8_t* grid, const vg_clr_params* prm, const uint8_t* table, int table_n,
                  int32_t* dist2, int32_t* nearest, uint8_t* cost, vg_clr_summary* out);
// navfn.hip: the navigation function of an nx x ny cost plane (host plane in, or null: the plane the last
// vg_clearance left on the device; pot (or null) and summary out) and the paths down the field it left; synchronous
// on the context stream, which the caller drained. Arguments: checked by the caller; table: trav by cost byte
int navfn_dev(vg_ctx* ctx, const uint8_t* cost, const vg_nav_params* prm, const uint16_t* table, const int32_t* goals,
              int n_goals, uint32_t* pot, vg_nav_summary* out);
int nav_paths_dev(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells, int32_t* len,
                  int32_t* status, int64_t* path_cost);
// frontier.hip: the frontiers of an nx x ny grid (host grid and cost in, or null: the planes the last vg_occupancy /
// vg_clearance left on the device; with flags bit 1 NavBufs::pot is read; labels (or null), the first max_records
// records and the summary out); synchronous on the context stream, which the caller drained. Arguments: checked
// by the caller
int frontiers_dev(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm, int32_t* labels,
                  vg_frontier_rec* recs, int max_records, vg_frontier_summary* out);
// view.hip: the view gain of n_views cells of an nx x ny grid (host grid in, or null: the plane the last vg_occupancy
// left on the device; the records, seen (or null) and the summary out); synchronous on the context stream, which the
// caller drained. Arguments: checked by the caller
int view_gain_dev(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views, int n_views,
                  vg_view_rec* recs, int32_t* seen, vg_view_summary* out);
// change.hip: the change layer's device side. The caller holds the owner's change_mu and has drained ctx's stream
int change_alloc(vg_ctx* owner, ChangeLayer* L, int hash_log2);
int change_clear_dev(vg_ctx* ctx, ChangeLayer* L);
// one scan into L at `epoch`, through ctx's map, staging and stream; x, y, z: host AoS (stride 3, dev false) or
// device arrays (stride 1)
int change_accum_dev(vg_ctx* ctx, ChangeLayer* L, const MP& mp, const float* x, const float* y, const float* z,
                     int stride, bool dev, int n, const double* pose12, int epoch, vg_diff_point* per_point,
                     vg_diff_summary* out);
// every selected record, in report order; tot4: points dropped, out of range, nodes touched, cells used
int change_report_dev(vg_ctx* ctx, ChangeLayer* L, const vg_change_query& q, std::vector<vg_change_leaf>& leaves,
                      std::vector<vg_change_cell>& cells, long long* tot4);
// live.hip: the live obstacle layer's device side; synchronous on the context stream, which the caller drained.
// Arguments: checked by the caller
int live_alloc(vg_ctx* ctx, LiveLayer* L, const int8_t* base_grid);  // the planes zeroed, the base from the host or the held grid
int live_clear_dev(vg_ctx* ctx, LiveLayer* L);
// one scan into L at `stamp`; x, y, z: host AoS (stride 3, dev false) or device arrays (stride 1)
int live_mark_dev(vg_ctx* ctx, LiveLayer* L, const MP& mp, const float* x, const float* y, const float* z, int stride,
                  bool dev, int n, const double* pose12, int stamp, vg_live_point* per_point, vg_live_summary* out);
int live_walk_dev(vg_ctx* ctx, LiveLayer* L, const vg_live_point* recs, int n, int stamp);  // k_live_walk on host records
int live_compose_dev(vg_ctx* ctx, LiveLayer* L, int now, int flags, int8_t* grid, vg_live_summary* out);
// places.hip: the place index's device side. The caller holds the owner's places_mu and has drained ctx's stream
int places_prm_ok(const vg_places_params* prm, int* A, int* E);  // VG_E_ARG: a limit exceeded, a bad span
int places_dirs(const vg_places_params* prm, double* out, int cap, int* count);
int places_build_dev(vg_ctx* ctx, PlaceIndex* I, const MP& mp);  // I->prm, pos, frame, M set: allocates, casts, reads hit
// the scan's descriptor into I->d_scan through ctx's staging and stream; desc / n_per_bin: host copies or null
int places_scan_dev(vg_ctx* ctx, PlaceIndex* I, const MP& mp, const float* xyz, int n, const double* R_level9,
                    uint16_t* desc, int32_t* n_per_bin, int* n_valid);
// I->d_scan against every place: best (M x 4 ints, host), scores_all (M x A, host) or null
int places_match_dev(vg_ctx* ctx, PlaceIndex* I, int* best, int32_t* scores_all);
// raycast_host.cpp: the two calls behind the C-ABI
int host_raycast(vg_ctx* ctx, const double* origins, int n_origins, const double* dirs, int n,
                 const vg_ray_params* prm, vg_ray_hit* out);
int host_scan_diff(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* prm,
                   vg_diff_point* per_point, vg_diff_summary* out);
// localizability_host.cpp: the two calls behind the C-ABI
int host_localizability(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                        const vg_info_params* prm, vg_info_rec* out);
int host_scan_info(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* diff,
                   const vg_info_params* prm, vg_info_rec* out);
// occupancy_host.cpp: the call behind the C-ABI
int host_occupancy(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D, const vg_occ_params* prm,
                   int8_t* grid, int32_t* counts, vg_occ_summary* out);
// terrain_host.cpp: the call behind the C-ABI
int host_terrain(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D, const vg_terrain_params* prm,
                 int8_t* grid, int32_t* elev, int32_t* step, int32_t* counts, vg_terrain_summary* out);
// clearance_host.cpp: the call behind the C-ABI
int host_clearance(vg_ctx* ctx, const int8_t* grid, const vg_clr_params* prm, int32_t* dist2, int32_t* nearest,
                   uint8_t* cost, vg_clr_summary* out);
// navfn_host.cpp: the calls behind the C-ABI
int host_navfn(vg_ctx* ctx, const uint8_t* cost, const vg_nav_params* prm, const uint16_t* trav, const int32_t* goals,
               int n_goals, uint32_t* pot, vg_nav_summary* out);
int host_nav_paths(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells, int32_t* len,
                   int32_t* status, int64_t* path_cost);
// frontier_host.cpp: the call behind the C-ABI
int host_frontiers(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm, int32_t* labels,
                   vg_frontier_rec* recs, int max_records, vg_frontier_summary* out);
// view_host.cpp: the call behind the C-ABI
int host_view_gain(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views, int n_views,
                   vg_view_rec* recs, int32_t* seen, vg_view_summary* out);
// live_host.cpp: the calls behind the C-ABI
int host_live_begin(vg_ctx* ctx, const vg_live_params* prm, const int8_t* base_grid);
int host_live_mark(vg_ctx* ctx, const float* xyz, const float* d_x, const float* d_y, const float* d_z, int n,
                   const double* pose12, int stamp, vg_live_point* per_point, vg_live_summary* out);
int host_live_compose(vg_ctx* ctx, int now, int flags, int8_t* grid, vg_live_summary* out);
int host_live_info(vg_ctx* ctx, int32_t* hit, int32_t* clear, vg_live_summary* totals);
int host_live_clear(vg_ctx* ctx);
int host_live_end(vg_ctx* ctx);
// localize.cpp: the frozen-map switch, scoring and relocalisation behind the C-ABI
int host_set_mapping(vg_ctx* ctx, int on);
int host_map_attach(vg_ctx* tracker, vg_ctx* owner);
int host_map_detach(vg_ctx* tracker);
// what a map view rules out (vina_gpu.h "Map views"): VG_E_STATE with the reason in ctx->err
inline int refuse_attached(vg_ctx* ctx, const char* who) {
  if (!ctx->view_of) return VG_OK;
  ctx->err = std::string(who) + ": the context is attached to another context's map (vg_map_detach first)";
  return VG_E_STATE;
}
inline int refuse_owner(vg_ctx* ctx, const char* who) {
  if (ctx->views == 0) return VG_OK;
  ctx->err = std::string(who) + ": " + std::to_string(ctx->views) +
             " context(s) are attached to this context's map (vg_map_detach them first)";
  return VG_E_STATE;
}
// what a change layer rules out on its owner (vina_gpu.h "Change layer"): node ids must not move, the map not change
// ... and a place index, whose rows are the map's ranges (places = false: the caller ends the index itself)
inline int refuse_layer(vg_ctx* ctx, const char* who, bool places = true) {
  if (ctx->change) {
    ctx->err = std::string(who) + ": the context's map has a change layer (vg_change_end first)";
    return VG_E_STATE;
  }
  if (places && ctx->places) {
    ctx->err = std::string(who) + ": the context's map has a place index (vg_places_end first)";
    return VG_E_STATE;
  }
  return VG_OK;
}
inline int refuse_fleet(vg_ctx* ctx, const char* who) {
  if (!ctx->fleet) return VG_OK;
  ctx->err = std::string(who) + ": the context is a fleet's tracker (vg_fleet_step_dev steps it; vg_fleet_destroy first)";
  return VG_E_STATE;
}
// fleet.hip: the batched launches of one fleet step (fleet_host.cpp)
struct FleetIn {  // one tracker's opening, host-mapped: written by the host before the step's launches
  double xc[kXC];            // x_curr after the propagation
  const float *x, *y, *z;    // the scan
  int n, active;             // active 0: the tracker sits this step out
  int win_count, seq1, seq2, pad;  // the publication (k_publish_state / k_publish_counters)
};
struct FleetTab {  // one tracker's device memory (constant while the fleet lives)
  DState* st;
  int* cache;        // Work::iekf_cache
  double* partials;  // Work::partials
  Pub* pub;          // the tracker's own publication block (device address)
  int* act;          // this step's active flag on the device (k_fleet_open)
};
int fleet_launch(hipStream_t s, const MP& mp, const DevMap& m, const FleetIn* in, const FleetTab* tab, int B, int nb,
                 bool prefetch, std::string* err);
int host_score_poses(vg_ctx* ctx, const float* xyz, int n, const double* poses, int K, const double* pose_var,
                     vg_pose_score* out, void* per_point);
int host_relocalize(vg_ctx* ctx, const float* xyz, int n, const double* guess, const vg_reloc_params* prm,
                    int install, double* out_pose, vg_pose_score* out_score, int* ok);
bool reloc_better(const vg_pose_score& a, const vg_pose_score& b);  // vg_relocalize's ranking
int reloc_install(vg_ctx* ctx, const double* pose12);               // ... and what its install does
int host_quiesce(vg_ctx* ctx);  // host_sync between scans; inside an open scan the context stream's drain
int host_lio_kdtree(vg_ctx* ctx, const float* xyz, int n, double* state, int* valid, int* iters);  // kdlio_host.cpp
int decode_scan(vg_ctx* ctx, const void* records, int n, const vg_lidar_format* fmt, float* xyz, float* inten,
                float* time, int* n_out);  // decode.hip
int host_stats_log(vg_ctx* ctx, vg_stats* out, int cap);
int stage_propagate(vg_ctx* ctx, const double* imu, int m, double beg, double end, bool dev = false);  // dev: k_scan_prop
int stage_deskew(vg_ctx* ctx, const float* x, const float* y, const float* z, const float* in, const float* t,
                 int n);
int host_step_deskew(vg_ctx* ctx, const float* dx, const float* dy, const float* dz, const float* di,
                     const float* dt, int n, double beg, double end, const double* imu, int m);
int stage_downsample(vg_ctx* ctx, const float* dx, const float* dy, const float* dz, const float* di, int n,
                     int* n_ds_out);
int stage_iekf(vg_ctx* ctx, const float* dx, const float* dy, const float* dz, int n, int* degenerate_out);
int stage_window_push(vg_ctx* ctx, const double* imu, int m);
int stage_insert(vg_ctx* ctx);
int stage_recut(vg_ctx* ctx, int* nf_out);
int stage_ba(vg_ctx* ctx, int* iters_out, bool margi_follows = false);  // margi_follows: the fused step
int stage_margi_slide(vg_ctx* ctx);
int stage_finish(vg_ctx* ctx);
}  // namespace vg

// ---- phase probes (instrumented build only, make probe) -------------------
#ifdef VG_PROBE
// one probe array per translation unit (no relocatable device code); each
// .hip exports its reader with VG_PROBE_READER(name)
namespace vg {
static __device__ unsigned long long g_probe[64];
}
#define VG_PROBE_READER(fn)                                                                        \
  extern "C" int fn(unsigned long long* out, int n) {                                              \
    if (n > 64) n = 64;                                                                            \
    if (hipDeviceSynchronize() != hipSuccess) return -2;                                           \
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vg::g_probe), n * sizeof(unsigned long long)) != hipSuccess) \
      return -2;                                                                                   \
    unsigned long long z[64] = {0};                                                                \
    if (hipMemcpyToSymbol(HIP_SYMBOL(vg::g_probe), z, sizeof(z)) != hipSuccess) return -2;         \
    return 0;                                                                                      \
  }
#define VG_PROBE_BEGIN() unsigned long long vg_probe_t = wall_clock64()
#define VG_PROBE_MARK(k)                                  \
  do {                                                    \
    if (threadIdx.x == 0) {                               \
      const unsigned long long now_ = wall_clock64();     \
      atomicAdd(&vg::g_probe[(k)], now_ - vg_probe_t);    \
      vg_probe_t = now_;                                  \
    }                                                     \
  } while (0)
#define VG_PROBE_MARK_T(k, t)                             \
  do {                                                    \
    if (threadIdx.x == (t)) {                             \
      const unsigned long long now_ = wall_clock64();     \
      atomicAdd(&vg::g_probe[(k)], now_ - vg_probe_t);    \
      vg_probe_t = now_;                                  \
    }                                                     \
  } while (0)
#else
#define VG_PROBE_BEGIN() (void)0
#define VG_PROBE_MARK(k) (void)0
#define VG_PROBE_MARK_T(k, t) (void)0
#endif
