/* vina_gpu.h — C-ABI of the MI355X-native VINA-SLAM per-scan LIO hot path.
 *
 * The reference (SheepYang666/VINA-SLAM) has no plugin/FFI layer: its hot path
 * is a plain C++ API called from the odometry thread. Each entry point below
 * replaces one of those calls (reference file:line cited); a C++ caller shaped
 * like src/pipeline/local_mapping.cpp binds them directly.
 *
 * Conventions
 *  - Every function returns int: 0 = ok, < 0 = error (VG_E_*); vg_last_error()
 *    gives text. Nothing calls exit() (the reference does: octree.cpp:407,
 *    optimizers.cpp:70).
 *  - Pointers without a _dev suffix are caller-owned HOST buffers; *_dev entry
 *    points take device pointers already resident in HBM.
 *  - Calls are synchronous with respect to the host unless stated; work inside
 *    is ordered on the context's HIP stream.
 *  - State vector (250 doubles), the reference's IMUST (types.hpp:43-113):
 *      [0] t, [1..9] R row-major, [10..12] p, [13..15] v, [16..18] bg,
 *      [19..21] ba, [22..24] g, [25..249] cov 15x15 row-major.
 *  - IMU samples: m rows of 7 doubles [t, gx, gy, gz, ax, ay, az]
 *    (sensor_msgs::Imu subset, m/s^2 and rad/s).
 *  - A context runs on three HIP streams and hands work between them through
 *    device flags that kernels poll, which needs kernels of different streams
 *    to run concurrently. Where they may not, the context uses event waits
 *    instead: serialised-kernel runs (AMD_SERIALIZE_KERNEL, VG_SERIAL_KERNELS=1,
 *    or rocprofv3 --pmc, detected at vg_create), and several live contexts on
 *    one device in one process (their streams would share the device's
 *    hardware queues; use vg_multi_* for several sequences). A hand-off that
 *    still times out (~1 s) fails the scan with VG_E_STATE; device errors are
 *    sticky: every later call returns them until vg_reset.
 */
#ifndef VINA_GPU_H
#define VINA_GPU_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VG_OK 0
#define VG_E_ARG (-1)
#define VG_E_HIP (-2)
#define VG_E_CAPACITY (-3)
#define VG_E_RANGE (-4)
#define VG_E_STATE (-5)

#define VG_STATE_LEN 250

/* Hot-path parameters: the reference's ROS 2 keys (node.cpp:52-291). */
typedef struct vg_config {
  double voxel_size;                /* Odometry.voxel_size (node.cpp:192) */
  double down_size;                 /* Odometry.down_size (node.cpp:183) */
  double min_eigen_value;           /* Odometry.min_eigen_value (node.cpp:198) */
  double plane_eigen_value_thre[4]; /* LocalBA.plane_eigen_value_thre as written in YAML; inverted internally (node.cpp:256-259) */
  double min_point[4];              /* {20,20,15,10} (node.cpp:219) */
  double dept_err, beam_err;        /* Odometry.dept_err / beam_err (node.cpp:186-190) */
  double imu_coef;                  /* LocalBA.imu_coef (node.cpp:247) */
  double ba_cov_gyr, ba_cov_acc, ba_rdw_gyr, ba_rdw_acc;     /* LocalBA.* -> noiseMeas/noiseWalk (node.cpp:262-265) */
  double odo_cov_gyr, odo_cov_acc, odo_rdw_gyr, odo_rdw_acc; /* Odometry.* -> IMUEKF (node.cpp:211-214) */
  double ext_R[9], ext_t[3];        /* General.extrinsic_rota / extrinsic_tran (node.cpp:78-82, 217-218) */
  int max_layer;                    /* LocalBA.max_layer */
  int max_points;                   /* octree.cpp:70 (100) */
  int win_size;                     /* LocalBA.win_size */
  int thread_num;                   /* LocalBA.thread_num: only its semantic quirks (voxel_map.cpp:96-97, local_mapping.cpp:27,93) */
  int if_BA;                        /* General.if_BA (default 0, node.cpp:96) */
  int reserved0, reserved1;
  /* 1: cold start — the reference's initialisation (node.cpp:293-366, SURVEY
   * row f2) runs on the first scans: IMU_init (+ gravity scale), then per scan
   * the kd-tree LIO (A14) until the window is full, then motion_init (map
   * rounds with the gravity-optimising BA, align_gravity, gravity-norm and
   * degeneracy checks; failure -> system_reset); the steady state follows.
   * Scans given with per-point times (vg_step_deskew*) are deskewed as the
   * reference's; without, every point is at pcl_end_time. Only the whole-scan
   * entry points (vg_step*) may be used until vg_stats::init_phase reports 3.
   * 0: start from vg_seed's state on an empty map. */
  int cold_start;
  /* IMUEKF::scale_gravity / imupre_scale_gravity (ekf_imu.hpp:27,
   * imu_preintegration.cpp:3): every accelerometer sample is multiplied by it
   * in the propagation (imu_ekf.cpp:51) and the preintegration
   * (imu_preintegration.cpp:51). 1 for IMUs reporting m/s^2; the reference
   * sets G_m_s2 = 9.8 when the static mean |acc| < 2 (IMU in g, e.g. Livox
   * Mid-360; imu_ekf.cpp:182-185, node.cpp:309). vg_imu_init derives it the
   * same way. 0 is read as 1. */
  double scale_gravity;
  /* Journey release distance in metres (local_mapping.cpp:324: roots whose
   * jour stamp is >= 700 behind are erased, vg_release_far); 0 is read as 700. */
  int release_dis;
  int pad_r;
} vg_config;

/* Capacities of the device-resident map (HBM). Zero fields take defaults. */
typedef struct vg_capacity {
  int max_points_per_scan;   /* raw points per scan (default 2,000,000) */
  int max_nodes;             /* octree nodes (default 4,000,000) */
  int max_fix_points;        /* point_fix arena, points (default 16,000,000) */
  int hash_log2;             /* root voxel hash slots = 2^hash_log2 (default 23) */
} vg_capacity;

/* Per-scan counters (SURVEY §8(d) byte model inputs). */
typedef struct vg_stats {
  int n_raw, n_ds, iekf_iters, iekf_matches[4];
  int roots_new, n_slide, n_factors, ba_iters, degenerate;
  int nodes_used, fix_used;
  int plane_updates; /* margi: OctoTree::plane_update calls this scan (octree.cpp:441-446) */
  int fix_full;      /* margi: leaves past max_points, pcr_fix.N >= max_points (octree.cpp:461-469) */
  /* SURVEY 8(d) byte-model inputs: distinct plane records read per IEKF
   * iteration (P_k; counted in vg_profile's per-stage pass only, else 0),
   * leaves the insert touched (V_ins), LM Hessian passes (I_H) */
  int iekf_planes[4];
  int v_ins;
  int ba_hess;
  /* cold start (vg_config::cold_start): 0 steady state, 1 IMU_init consumed
   * the scan, 2 initialisation-window scan (kd-tree LIO), 3 motion_init
   * succeeded on this scan (which then ran the window tail too), 4 motion_init
   * failed (system_reset); motion_init rounds run on this scan; the kd-tree
   * LIO's valid correspondences (-1: the scan seeded the map) */
  int init_phase, init_rounds, init_valid;
  /* points the IEKF point loop processed, summed over the executed iterations
   * (sharded mode, world > 1: this rank's kept points, iekf.hip k_keep_*) */
  int iekf_points;
} vg_stats;

typedef struct vg_ctx vg_ctx;
typedef int (*vg_host_allreduce_fn)(void* buf, int count, int dtype, void* user);

/* Context lifecycle. Replaces the VINA_SLAM members surf_map, surf_map_slide,
 * sws, x_buf, pvec_buf, imu_pre_buf (node.hpp:34-70). device = HIP ordinal. */
int vg_create(const vg_config* cfg, const vg_capacity* cap, int device, vg_ctx** out);
int vg_destroy(vg_ctx* ctx);
const char* vg_last_error(const vg_ctx* ctx);
/* Drop the map and window; replaces VINA_SLAM::system_reset (node.cpp:368-408). */
int vg_reset(vg_ctx* ctx);

/* A1 — down_sampling_voxel (include/vina_slam/core/point_utils.hpp:7-44).
 * xyz: n x 3 floats (AoS), intensity: n floats (may be NULL).
 * out_xyzic: n x 5 floats [x, y, z, intensity(first point), count] in
 * ascending voxel-key order (the reference emits unordered_map order; the SET
 * is identical, bit-for-bit). Returns the voxel count in *n_out. */
int vg_downsample(vg_ctx* ctx, const float* xyz, const float* intensity, int n, double voxel_size,
                  float* out_xyzic, int* n_out);
/* f2 — down_sampling_close (include/vina_slam/core/point_utils.hpp:46-113) +
 * the time sort of VINA_SLAM::initialization (node.cpp:337-345): per voxel the
 * input point nearest the float mean of the voxel's points. time: n floats
 * (may be NULL: every point at time 0). out_xyzt: n x 4 floats [x, y, z, time]
 * sorted by time; equal times in ascending voxel-key order (the reference
 * std::sorts its unordered_map order, leaving their order unspecified).
 * Synchronous; drains the pipeline first (diagnostic / test entry point). */
int vg_downsample_close(vg_ctx* ctx, const float* xyz, const float* time, int n, double voxel_size, float* out_xyzt,
                        int* n_out);

/* Per-scan pipeline — the steady-state branch of
 * VINA_SLAM::thd_odometry_localmapping (local_mapping.cpp:389-547):
 * IMU propagation (imu_ekf.cpp:28-94) -> downsample (+ /2 fallback) ->
 * var_init -> IEKF (odometry.cpp:64-255) -> pvec_update -> cut_voxel_multi ->
 * multi_recut + tras_opt -> [win full] LI_BA damping_iter -> multi_margi -> slide.
 * vg_seed sets x_curr (the output of initialisation). */
int vg_seed(vg_ctx* ctx, const double* state);
int vg_step(vg_ctx* ctx, const float* xyz, const float* intensity, int n, double pcl_beg_time,
            double pcl_end_time, const double* imu, int m);
/* Same, with the scan already in HBM as SoA x/y/z/intensity device arrays. */
int vg_step_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, const float* d_intensity, int n,
                double pcl_beg_time, double pcl_end_time, const double* imu, int m);
/* vg_step / vg_step_dev return once the scan is ENQUEUED: the device runs it
 * asynchronously (the host waits only for device-side counts it needs, without
 * draining the stream). Every query below completes the outstanding work first.
 * vg_step / vg_step_deskew copy the caller's host arrays into one of two pinned
 * in-flight slots before returning (the caller may reuse them at once); the
 * H2D copy and the SoA unpack run on the device ahead of the scan's kernels.
 * vg_step_dev / vg_step_deskew_dev read the caller's device arrays while the
 * scan runs: keep them unchanged until a later query (vg_get_state, vg_get_stats, ...) returns. */
/* SURVEY row f1 — the same scan step with IMUEKF::motion_blur's per-point
 * deskew (imu_ekf.cpp:114-144) on the device first: `time` holds each point's
 * offset from pcl_beg_time in seconds (the reference's `curvature` field),
 * ascending (the reference's time-sorted cloud). The propagation records the
 * IMU poses; one lane per point moves it into the LiDAR frame at
 * pcl_end_time. Inputs as vg_step / vg_step_dev. */
int vg_step_deskew(vg_ctx* ctx, const float* xyz, const float* intensity, const float* time, int n,
                   double pcl_beg_time, double pcl_end_time, const double* imu, int m);
int vg_step_deskew_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, const float* d_intensity,
                       const float* d_time, int n, double pcl_beg_time, double pcl_end_time, const double* imu,
                       int m);
/* SURVEY row A14 — VINA_SLAM::lio_state_estimation_kdtree (odometry.cpp:267-439),
 * the initialisation-phase LIO (node.cpp:317). xyz: the scan downsampled at
 * max(down_size, 0.5), raw LiDAR frame, n x 3 floats (var_init applies the
 * extrinsic). state: 250 doubles (vg_get_state layout), updated in place.
 * While the context's init map holds fewer than 100 points the scan only seeds
 * it (*valid = -1, *iters = 0); otherwise up to 4 IEKF iterations against the
 * exact 5 nearest map points (device hashed grid in place of the kd-tree,
 * plane fit by column-pivoting Householder QR as colPivHouseholderQr), then the
 * registered scan is appended and the map re-downsampled at 0.5 m.
 * *valid: correspondences of the last iteration. vg_reset clears the map.
 * Synchronous; completes outstanding work first. */
int vg_lio_kdtree(vg_ctx* ctx, const float* xyz, int n, double* state, int* valid, int* iters);
/* the init map (float xyz, n x 3, key order of its last downsample): *n = its
 * size; up to cap points copied when xyz != NULL */
int vg_kdmap_get(vg_ctx* ctx, float* xyz, int cap, int* n);
/* SURVEY row f3 — sensor decode (LidarPointCloudDecoder, lidar_pointcloud_decoder.cpp:21-240)
 * and pcl_handler's scan preparation (lidar_decoder.cpp:7-43): per record the
 * xyz / intensity / per-point time of the sensor format, the point_filter_num
 * stride and blind test, then ascending time order and the tail beyond 0.11 s
 * dropped (an empty result becomes the reference's two dummy points).
 * records: n little-endian records of `stride` bytes; offsets are byte offsets
 * of the fields, -1 when absent. Field types per kind (the reference's point
 * structs): LIVOX x,y,z f32, reflectivity u8, offset_time u32 ns; VELODYNE
 * x,y,z,time f32 (a sweep without usable times takes the yaw-derived time,
 * omega_l deg/s, sequentially on the host as the reference does); OUSTER
 * x,y,z,intensity f32, t u32 ns; HESAI x,y,z,intensity f32, timestamp f64
 * (minus the first record's); ROBOSENSE x,y,z,intensity f32, timestamp f64
 * (minus time_base, the header stamp; blind on x,y only); TARTANAIR x,y,z f32
 * (no filter, time 0). blind in metres (squared as node.cpp:210 does).
 * Outputs (host, capacity n + 2): xyz n_out x 3, intensity, time (s). The
 * time sort is stable (std::sort's order among equal times is unspecified). */
enum { VG_LIVOX = 0, VG_VELODYNE = 1, VG_OUSTER = 2, VG_HESAI = 3, VG_ROBOSENSE = 4, VG_TARTANAIR = 5 };
typedef struct vg_lidar_format {
  int kind;
  int stride;
  int off_x, off_y, off_z, off_intensity, off_time;
  int point_filter_num;
  double blind;
  double omega_l;
  double time_base;
} vg_lidar_format;
int vg_decode_scan(vg_ctx* ctx, const void* records, int n, const vg_lidar_format* fmt, float* xyz, float* intensity,
                   float* time, int* n_out);
/* SURVEY row f3 (replay side) — sync_packages (src/sensor/sync.cpp:18-96) as a
 * host packager, no context: push scans (header time, the last point's time
 * offset after vg_decode_scan, an id) and IMU samples (t, gyr 3, acc 3) in
 * arrival order; vg_sync_pop sets *ready = 1 with one scan's window [beg, end]
 * and its IMU samples (stamped <= end; up to cap copied, *m = count) once an
 * IMU sample newer than end has arrived; *ready = 0: wait for more data;
 * *ready = -1: a scan was consumed and dropped (<= 4 samples, as the
 * reference), pop again. point_notime (Odometry.point_notime) windows scans by
 * consecutive header times. VG_E_STATE: the IMU queue ran dry (the reference
 * exits). */
typedef struct vg_sync vg_sync;
vg_sync* vg_sync_create(int point_notime);
void vg_sync_destroy(vg_sync* s);
int vg_sync_push_scan(vg_sync* s, double header_time, double last_point_time, int scan_id);
int vg_sync_push_imu(vg_sync* s, const double* imu7);
int vg_sync_pop(vg_sync* s, int* scan_id, double* beg, double* end, double* imu7, int cap, int* m, int* ready);
int vg_get_state(vg_ctx* ctx, double* state);
/* The last completed scan's downsampled cloud (body frame, after the deskew;
 * the map path's pl_down, local_mapping.cpp:396-406) as n x 3 floats, up to
 * cap copied, *n = its size: what pub_localtraj moves to the world and
 * publishes on /map_scan (publishers.cpp:65-97). Completes outstanding work. */
int vg_scan_points(vg_ctx* ctx, float* xyz, int cap, int* n);
int vg_get_stats(vg_ctx* ctx, vg_stats* out);
/* Per-scan counters of every completed scan since vg_create / vg_reset, in
 * order: copies min(n, cap) records, *n = total (out may be NULL to query). */
int vg_stats_log(vg_ctx* ctx, vg_stats* out, int cap, int* n);
/* The map's lifetime — the idle branch of thd_odometry_localmapping
 * (local_mapping.cpp:317-344), which the caller runs when it has no package
 * (sync_packages false): once jour has advanced (release_flag, :510-518),
 * every root voxel whose jour stamp is >= vg_config::release_dis (700 m)
 * behind is erased with its subtree (OctoTree::tras_ptr, octree.cpp:597-608).
 * The device then reclaims: erased nodes, point_fix blocks abandoned by
 * growth and the blocks of leaves past max_points (octree.cpp:467-468) are
 * compacted out of the node pool and the point_fix arena (order-preserving;
 * results are unchanged). flags bit 0: compact even without a release; bit
 * 1: report the census (out[2..5]) even without one. The pool is also
 * compacted when over half the arena is abandoned blocks. With flags 0 and no
 * release pending among the scans already published it returns at once (no
 * wait; out[] = -1), so a caller may call it whenever sync_packages comes back
 * empty; otherwise it completes outstanding work first. Between scans only.
 * out (6): [0] roots erased (-1: no release was pending), [1] nodes erased,
 * [2] roots, [3] nodes in the map after it, [4] point_fix points held,
 * [5] point_fix arena used.
 * A root still in surf_map_slide is never erased (the reference would keep a
 * dangling pointer in it; unreachable at 700 m). */
int vg_release_far(vg_ctx* ctx, int flags, long long* out);
/* Checkpoint and resume: everything of a context that outlives a scan — the
 * voxel map (node records, point_fix arena, window points, slide list, the
 * root keys), the estimator state and the host mirror with the trajectory and
 * path rows — to one file and back. A context that loads a file and goes on
 * stepping produces the same bits as the one that wrote it would have.
 * vg_checkpoint_save completes the outstanding work, then compacts the node
 * pool and the point_fix arena (as vg_release_far with flags bit 0 does:
 * results are unchanged), so the file is proportional to the live map and
 * independent of max_nodes / max_fix_points / hash_log2; *bytes (may be NULL)
 * = the file's size. Between scans and in the steady state only: VG_E_STATE
 * while a cold start is still initialising (before init_phase 3), on a sharded
 * context (world > 1) and while a stage-level scan is open. Saving changes no
 * later result of the saving context.
 * vg_checkpoint_load installs a file into an existing context, fresh or used
 * (vg_reset semantics first). The context's vg_config must equal the saved
 * one byte for byte and max_points_per_scan must be the saver's (the window
 * arrays' stride), else VG_E_ARG; the other capacities may differ, and a
 * context too small returns VG_E_CAPACITY. Every check — magic and version,
 * configuration, section table and file length, every section's checksum
 * (recomputed on the device), capacity — runs before anything is touched: a
 * rejected load leaves the context exactly as it was, and vg_last_error names
 * the failed check. Not part of a checkpoint, kept as the loading context has
 * them: vg_set_publish flags and marker state (a blank slate), the wait
 * policy, vg_profile; vg_stats_log restarts at the load. */
int vg_checkpoint_save(vg_ctx* ctx, const char* path, long long* bytes);
int vg_checkpoint_load(vg_ctx* ctx, const char* path);

/* ---- Localising in a saved map --------------------------------------------
 * Frozen-map (localisation) mode. on = 1 (the default): vg_step* maps as
 * before. on = 0: the map is read-only. A scan with mapping off runs the
 * propagation (and the deskew where per-point times are given), the
 * downsample with its /2 fallback and the IEKF; x_curr becomes the IEKF
 * result and the scan ends: one TUM row, one path row (carrying the last value
 * of jour), the per-scan stats (n_raw, n_ds, iekf_*, degenerate as usual;
 * roots_new, n_slide, n_factors, ba_iters, plane_updates, fix_full and v_ins
 * 0; nodes_used and fix_used unchanged). No window push, insert, recut, LM,
 * margi or slide: the node pool, the point_fix arena, the root hash, the slide
 * list, the window arrays and win_count stay bit for bit what they were.
 * The switch completes the outstanding work first. Between scans only:
 * VG_E_STATE inside an open stage-level scan, before a cold start has reached
 * init_phase 3, and on a sharded context with world > 1.
 * With mapping off the stage-level API allows vg_scan_load / vg_scan_bind_dev,
 * vg_propagate, vg_downsample_scan, vg_lio_state_estimation and vg_step_end;
 * vg_window_push, vg_cut_voxel_multi, vg_multi_recut, vg_damping_iter and
 * vg_multi_margi return VG_E_STATE (the open scan stays usable).
 * vg_release_far erases nothing and returns out[0] = -1 (the census of flags
 * bit 1 still works); vg_checkpoint_save works; the mode is not part of a
 * checkpoint, and a load keeps the loading context's mode; vg_set_publish
 * bit 1 emits no markers. Turning mapping back on continues the saved session
 * from the frozen window. */
int vg_set_mapping(vg_ctx* ctx, int on);

/* Pose-hypothesis scoring: OctoTree::match (octree.cpp:551-595,
 * voxel_map.cpp:241-266) for one scan under K candidate poses in one
 * dispatch. Reads the map only. */
typedef struct vg_pose_score {   /* 80 bytes, no implicit padding */
  int32_t matches;               /* points for which match() returned 1 */
  int32_t in_map;                /* points whose root voxel exists and whose descent reached a leaf */
  double  cost;                  /* sum r^2 / (0.0005 + sigma_d) over the matches */
  double  sum_abs;               /* sum |r| over the matches */
  double  nn[6];                 /* sum n n^T, upper triangle (xx xy xz yy yz zz): the IEKF's degeneracy input */
  double  reserved;
} vg_pose_score;
/* per_point record of vg_score_poses (24 bytes) */
typedef struct vg_point_match {
  int32_t leaf;                  /* node id of the leaf the descent reached, -1: none */
  int32_t flag;                  /* match() returned 1 */
  double  r;                     /* n . (w - c), signed; 0 where flag = 0 */
  double  sigma_d;               /* the gate's variance; 0 where flag = 0 */
} vg_point_match;
#define VG_SCORE_MAX_POSES 65536
/* xyz: n x 3 floats, LiDAR frame (what the IEKF reads; vg_scan_points' or
 *   vg_downsample's output for a downsampled cloud); var_init as the IEKF
 *   applies it (extrinsic, calcBodyVar).
 * poses: K x 12 doubles [R row-major 9, p 3], IMU in world (state[1..12]).
 * pose_var: 18 doubles [rot_var 3x3, tsl_var 3x3] shared by all K, or NULL for
 *   zero: the two blocks the IEKF takes from the state covariance.
 * per_point (may be NULL; K must be 1): n vg_point_match records.
 * The sums are deterministic and independent of K: a pose's record has the
 * same bits scored alone or at any position of any batch. n == 0 or an empty
 * map gives all-zero records; a point whose voxel key is out of the packed
 * range (|key| >= 2^20) counts as not in the map. K <= 0, K >
 * VG_SCORE_MAX_POSES, n < 0, n > max_points_per_scan or a NULL pointer:
 * VG_E_ARG. Completes outstanding work first; between scans or inside an open
 * stage-level scan; works in either mode. Unsharded contexts only. */
int vg_score_poses(vg_ctx* ctx, const float* xyz, int n, const double* poses, int K,
                   const double* pose_var, vg_pose_score* out, void* per_point);

/* Relocalise: recover the pose of a scan in the map from a rough guess. A
 * grid of hypotheses around the guess is scored in one vg_score_poses
 * dispatch and ranked by matches, then by lower cost / matches; the best
 * refine_top are refined by LiDAR-only Gauss-Newton on the 6 pose unknowns
 * against the frozen map (the IEKF's own 6 x 6 normal equations, no prior,
 * solved on the host in double, one launch per iteration); the winner is the
 * best refined score. */
typedef struct vg_reloc_params {
  double half_xy, step_xy;       /* search window and step in x and y around the guess, metres */
  double half_z,  step_z;        /* 0 / 0: keep the guess's z */
  double half_yaw, step_yaw;     /* about the gravity direction of the context's state, radians */
  int    refine_top;             /* best coarse hypotheses refined (<= 0: 8) */
  int    refine_iters;           /* Gauss-Newton iterations each (<= 0: 8) */
  double min_match_ratio;        /* success: matches / n of the refined winner (<= 0: 0.5) */
  double reserved[4];
} vg_reloc_params;
/* The hypothesis grid of vg_relocalize, without a device: per axis the offsets
 * i * step for |i| <= floor(half / step) (one value, 0, where half or step is
 * 0). Order: z outermost, then yaw, then the x-y plane in 4 x 4 patches (patch
 * rows along y, patches and the cells inside each in row-major order, x
 * fastest), so that 16 consecutive hypotheses, one workgroup's pose tile in
 * vg_score_poses, are neighbours in the plane and touch the same root voxels.
 * out (may be NULL): cap x 4 doubles [dx, dy, dz, dyaw]; *count = the grid's
 * size. More than VG_SCORE_MAX_POSES hypotheses, a negative half or step:
 * VG_E_ARG. */
int vg_reloc_grid(const vg_reloc_params* prm, double* out, int cap, int* count);
/* guess_pose, out_pose: 12 doubles [R 9, p 3]. out_score: the refined winner's
 * record; *ok = 1 on success. install != 0 and success: x_curr takes the pose;
 * v, bg, ba and g keep the context's values (v = 0 when the context has never
 * stepped) and the covariance is reset to the initial covariance
 * (imu_ekf.cpp: 1e-4 on rotation, position and velocity, 1e-5 on the biases).
 * A failure (*ok = 0) returns VG_OK and leaves the context's state untouched.
 * Completes outstanding work; between scans only (VG_E_STATE inside one). */
int vg_relocalize(vg_ctx* ctx, const float* xyz, int n, const double* guess_pose,
                  const vg_reloc_params* prm, int install, double* out_pose, vg_pose_score* out_score, int* ok);

/* ---- Ray-casting the map ------------------------------------------------------
 * Rays through the hashed root voxels and their octrees to the first plane they
 * meet: the expected range of the map from a pose, and a scan checked against
 * it. Reads the map only (the DevMap the IEKF reads) and writes nothing.
 *
 * A ray is an origin o, a direction d (world frame; normalised on the device)
 * and an interval (t_min, t_max] (t_min < 0 counts as 0). A leaf the descent
 * can reach is a candidate when it holds a plane (n, c), |n.d| >= min_cos, and
 * h = o + t d with t = n.(c - o) / (n.d) has t in the interval and lies in the
 * leaf's cube (voxel centre +- 2 quater_length per axis, faces included). The
 * hit is the candidate of smallest t; equal t goes to the lower node id. */
typedef struct vg_ray_params {
  double t_min, t_max;   /* t_max <= 0: 100 m */
  double min_cos;        /* planes with |n.d| below it are passed through; <= 0: 0.05 */
  int    max_steps;      /* root cells + octree nodes a ray may visit; <= 0: 4096 */
  int    pad;
  double reserved[4];
} vg_ray_params;
typedef struct vg_ray_hit {   /* 64 bytes, no implicit padding */
  double  range;              /* t of the hit; 0 where there is none */
  double  var;                /* variance of range from the plane's covariance: J S J^T / (n.d)^2 with
                                 J = [h - c, -n] and S the plane's 6 x 6 (the first term of match()'s gate) */
  double  normal[3];          /* the plane's normal as stored */
  double  ndotd;              /* signed */
  int32_t leaf;               /* node id, -1: none */
  int32_t flags;              /* bit 0 hit, 1 truncated, 2 crossed an occupied leaf without a plane,
                                 3 left the key range, 4 invalid ray (zero or non-finite direction / origin) */
  double  reserved;
} vg_ray_hit;
#define VG_RAY_HIT 1
#define VG_RAY_TRUNCATED 2
#define VG_RAY_OCCUPIED 4
#define VG_RAY_LEFT_RANGE 8
#define VG_RAY_INVALID 16
/* origins: n_origins x 3 doubles, n_origins = 1 (shared by all rays) or n.
 * dirs: n x 3 doubles. prm: NULL for the defaults. out: n records.
 * A ray that visits max_steps cells and nodes ends as a miss with bit 1; one
 * that walks out of the packed key range (|cell index| >= 2^20) ends with bit
 * 3. Bit 2: before it ended the ray crossed a leaf that holds points but no
 * plane (occupied, surface unknown). A ray's record depends on the ray and the
 * map alone: the same bits alone or at any position of any batch. n is walked
 * in slabs of max_points_per_scan rays; the staging is allocated on the first
 * call. n == 0 is fine; an empty map gives all-miss records. A NULL pointer,
 * n < 0 or n_origins not in {1, n}: VG_E_ARG. Completes outstanding work first;
 * between scans or inside an open stage-level scan; with mapping on or off; on
 * an attached tracker (the owner's map) and on a fleet's tracker. Unsharded
 * contexts only (VG_E_STATE with world > 1). */
int vg_raycast(vg_ctx* ctx, const double* origins, int n_origins, const double* dirs, int n,
               const vg_ray_params* prm, vg_ray_hit* out);

/* Scan-vs-map change detection: every point of a scan against the range the map
 * expects along its beam. Per point x (LiDAR frame, as vg_score_poses), at the
 * pose (R, p): the sensor origin o = p + R ext_t, w = R (ext_R x + ext_t) + p,
 * r = |w - o|, and one ray from o along w - o cast to min(r + gate_max,
 * ray.t_max), gate_max = the gate below at |n.d| = min_cos with var = 0, plus
 * 1 m. With m the ray's hit and c = |m.ndotd|:
 *   gate^2 = gate_sigma^2 (m.var + dept_err^2 + (r sin(beam_err deg))^2 (1 - c^2) / c^2),
 *   floored at gate_floor^2 (dept_err, beam_err: the configuration's, as calcBodyVar uses them);
 *   no hit: UNKNOWN; |m.range - r| <= gate: CONSISTENT; m.range > r + gate:
 *   APPEARED (something stands in front of the mapped surface); m.range <
 *   r - gate: VANISHED (the beam passed through a mapped plane). */
enum { VG_DIFF_UNKNOWN = 0, VG_DIFF_CONSISTENT = 1, VG_DIFF_APPEARED = 2, VG_DIFF_VANISHED = 3 };
typedef struct vg_diff_params {
  vg_ray_params ray;
  double gate_sigma;     /* <= 0: 3 */
  double gate_floor;     /* metres, default 0 */
  double reserved[4];
} vg_diff_params;
typedef struct vg_diff_point {   /* 32 bytes */
  int32_t cls, leaf;             /* VG_DIFF_*; the hit's node id, -1: none */
  double  r_meas, r_map, gate;   /* r; the hit's range and the gate, 0 where there is no hit */
} vg_diff_point;
typedef struct vg_diff_summary {
  int32_t n[4];                  /* points per class, indexed by VG_DIFF_* */
  int32_t n_truncated, n_occupied_unknown;  /* rays with bit 1; rays with bit 2 */
  double  sum_abs_consistent;    /* sum |m.range - r| over the CONSISTENT points, one fixed-order reduction */
  double  reserved[3];
} vg_diff_summary;
/* xyz: n x 3 floats, n <= max_points_per_scan. pose12: [R row-major 9, p 3], or
 * NULL for the context's current state. prm: NULL for the defaults. per_point
 * (may be NULL): n records. A point's record and the counts do not depend on
 * its position in the batch. NULL xyz (n > 0) or out, n < 0, n too large:
 * VG_E_ARG. Legal where vg_raycast is. */
int vg_scan_diff(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* prm,
                 vg_diff_point* per_point, vg_diff_summary* out);

/* ---- Localisability: expected pose information ---------------------------------
 * How well the map constrains a pose: the 6 x 6 point-to-plane information
 * matrix, summed per place over the range image the map shows from there
 * (vg_localizability), and summed over a measured scan's consistent points at a
 * pose (vg_scan_info). Both read the map only and keep no state.
 *
 * The per-ray term. A ray from origin o along the unit direction d with the hit m
 * at range r, n = m.normal as stored, c = |m.ndotd|:
 *   J  = [n ; (r d) x n]   (6 entries): the derivative of the residual n.(h -
 *        centre), h = o + r d, under o -> o + dp, d -> Exp(dtheta) d. The
 *        unknowns are ordered [dp, dtheta], in the world frame, rotation about o;
 *   s2 = c^2 (m.var + dept_err^2 + (r sin(beam_err deg))^2 (1 - c^2) / c^2) +
 *        floor_var   (the bracket is gate^2 / gate_sigma^2 of vg_scan_diff);
 *   w  = 1 / s2.
 * The ray contributes w J J^T and counts as a hit only if m is a hit and s2 is
 * finite and > 0. The 21 unique entries of H and sum_w are accumulated in f64.
 *
 * The record. H: row-major, symmetric, both triangles filled with the same bits.
 * With H = [H_pp H_pt; H_tp H_tt] (p translation, t rotation), S_t = H_pp - H_pt
 * H_tt^-1 H_tp is the translation information with the rotation marginalised and
 * S_r = H_tt - H_tp H_pp^-1 H_pt its mirror image. eig_t / eig_r: their
 * eigenvalues in ascending order; dir_t / dir_r: the unit eigenvector of the
 * smallest one, its sign chosen so that its largest-magnitude component (the
 * first of equals) is positive. flags:
 *   bit 0 valid: n_hits >= min_hits. An invalid record carries its H, sum_w and
 *     counts; its eig and dir are zero and bits 1 and 2 are clear;
 *   bit 1 the rotation block is degenerate: the eigenvalues of H_tt have
 *     lambda_min <= 1e-12 lambda_max. Then S_t = H_pp is reported unmarginalised
 *     and eig_r / dir_r are zero;
 *   bit 2 the same for the translation block (H_pp; S_r = H_tt, eig_t / dir_t
 *     zero). Where both blocks are degenerate both bits are set and bit 1's rule
 *     holds: eig_t / dir_t are H_pp's, eig_r / dir_r zero;
 *   bit 3 some ray ended truncated or left the key range (VG_RAY_TRUNCATED,
 *     VG_RAY_LEFT_RANGE). */
typedef struct vg_info_params {
  vg_ray_params ray;     /* vg_localizability's rays; vg_scan_info casts with diff->ray */
  double floor_var;      /* m^2 added to every s2; default 0 */
  int    min_hits;       /* <= 0: 16 */
  int    pad;
  double reserved[4];
} vg_info_params;
typedef struct vg_info_rec {   /* 416 bytes, no implicit padding */
  double  H[36];
  double  eig_t[3], eig_r[3];
  double  dir_t[3], dir_r[3];
  double  sum_w, reserved;     /* sum of w over the hits */
  int32_t n_rays, n_hits;      /* rays cast (D; a scan's n); contributing rays */
  int32_t flags, pad;
} vg_info_rec;
#define VG_INFO_VALID 1
#define VG_INFO_ROT_DEGENERATE 2
#define VG_INFO_TRANS_DEGENERATE 4
#define VG_INFO_RAY_ENDED 8
/* One record per place. positions: M x 3 doubles, LiDAR origins in the world.
 * dirs: D x 3 doubles, world-frame directions shared by all places, 1 <= D <=
 * 4096 (vg_places_dirs gives a suitable set; normalised on the device). prm: NULL
 * for the defaults. out: M records. A zero or non-finite direction or origin is
 * an invalid ray (VG_RAY_INVALID) and contributes nothing. The sums are reduced
 * in an order that is a function of D alone, so a place's record has the same
 * bytes at any M, at any position in `positions` and in any call; M is walked
 * in slabs, the staging allocated on the first call. Only the records leave the
 * device. M == 0 is fine. NULL ctx, dirs, or (M > 0) positions / out, M < 0, D
 * outside [1, 4096]: VG_E_ARG. Legal where vg_raycast is: completes outstanding
 * work first; mapping on or off; on an owner, an attached tracker and a fleet's
 * tracker; unsharded contexts only (VG_E_STATE with world > 1). */
int vg_localizability(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                      const vg_info_params* prm, vg_info_rec* out);
/* One record for a measured scan at a pose: xyz, n, pose12 and diff as
 * vg_scan_diff takes them (pose12 NULL: the context's current state; diff NULL:
 * the defaults), and every point classified exactly as vg_scan_diff does. Only the
 * CONSISTENT points contribute, with o the sensor origin, r d = w - o (the
 * measured point) and the hit's n, c and var. n_rays = n, n_hits the contributing
 * points. Every workgroup reduces its 256 points in a fixed tree and one workgroup
 * adds the partial sums in block order: the record depends on the input and its
 * order alone. n == 0 gives a zero record. Arguments in error and where it is
 * legal: as vg_scan_diff. */
int vg_scan_info(vg_ctx* ctx, const float* xyz, int n, const double* pose12, const vg_diff_params* diff,
                 const vg_info_params* prm, vg_info_rec* out);

/* ---- Occupancy grid: a 2-D navigation map ray-cast from the voxel map ----------
 * M sensor origins x D shared directions are traced exactly as vg_raycast traces
 * them and rasterised on the device into a grid of nx x ny square cells of edge
 * res: cell (ix, iy) spans [x0 + ix res, x0 + (ix + 1) res] x [y0 + iy res, y0 +
 * (iy + 1) res] in the world's x, y. Two int32 count planes are summed over all
 * rays with integer atomics, n_free (the ray crossed the cell before its end)
 * and n_occ (the ray's hit lies in the cell), and classified per cell. Reads the
 * map only and keeps no state: every call starts from zero counts.
 *
 * Per ray (o, d), d the unit direction, with its vg_raycast record m. A ray with
 * VG_RAY_TRUNCATED, VG_RAY_LEFT_RANGE or VG_RAY_INVALID marks nothing. Its end
 * r_end is m.range where it hit, else free_on_miss where that is > 0, else the
 * ray marks nothing.
 *   Occupied mark. The hit is in band when z_lo <= m.range d_z <= z_hi (heights
 *     relative to the ray's own origin, so that floor and ceiling stay out of
 *     the grid). An in-band hit adds 1 to n_occ of the cell (floor((h_x - x0) /
 *     res), floor((h_y - y0) / res)), h = o + m.range d.
 *   Free marks. The free segment is the open interval of t between max(t_min,
 *     0) and r_end on which z_lo <= t d_z <= z_hi. Every cell whose interior the
 *     segment's (x, y) projection passes through gets n_free += 1, except the
 *     in-band hit's own cell; a ray with d_x = d_y = 0 marks only the cell it
 *     stands in. A ray marks a cell at most once. Marks outside the grid are
 *     dropped.
 *   flags bit 0: a ray whose record carries VG_RAY_OCCUPIED still marks its hit
 *     but no free cell. It crossed a leaf that holds points but no plane.
 * The limit of this grid: only planes are surfaces here. Clutter in a leaf
 * without a plane is not an obstacle in the grid (the traversal does not report
 * where along the ray that leaf was crossed); flags bit 0 at least keeps such a
 * ray from declaring the space behind the clutter free.
 *
 * Per cell, in this order: occupied (VG_OCC_OCCUPIED) when n_occ >= min_occ and
 * n_occ >= occ_ratio (n_occ + n_free), the product taken in double; else free
 * (VG_OCC_FREE) when n_free >= min_free; else unknown (VG_OCC_UNKNOWN) — the
 * values of nav_msgs/OccupancyGrid. */
#define VG_OCC_UNKNOWN (-1)
#define VG_OCC_FREE 0
#define VG_OCC_OCCUPIED 100
#define VG_OCC_MAX_CELLS (1 << 24)
typedef struct vg_occ_params {
  vg_ray_params ray;        /* as vg_raycast; zero fields: its defaults */
  double x0, y0;            /* world x, y of the lower corner of cell (0, 0) */
  double res;               /* cell edge, metres; > 0 */
  int    nx, ny;            /* cells; 1 <= nx, ny and nx * ny <= 2^24 */
  double z_lo, z_hi;        /* height band relative to each ray's origin: a point at o + t d is in the
                               band when z_lo <= t d_z <= z_hi; z_lo < z_hi */
  double free_on_miss;      /* a ray without a hit marks free up to this range; <= 0: marks nothing */
  int    min_occ;           /* <= 0: 1 */
  int    min_free;          /* <= 0: 1 */
  double occ_ratio;         /* <= 0: off */
  int    flags;             /* bit 0: a ray with VG_RAY_OCCUPIED marks no free cell */
  int    pad;
  double reserved[4];
} vg_occ_params;
typedef struct vg_occ_summary {   /* 128 bytes, no implicit padding */
  int64_t n_rays, n_hits, n_hits_in_band, n_truncated, n_occupied_unknown, n_invalid;
                                          /* M D; rays with VG_RAY_HIT; in-band hits of rays that mark; rays
                                             with bit 1, bit 2, bit 4 */
  int64_t free_marks, occ_marks;          /* sums of the two count planes */
  int64_t cells_free, cells_occupied, cells_unknown;
  int64_t reserved[5];
} vg_occ_summary;
/* positions: M x 3 doubles, sensor origins in the world (the positions the sensor
 * really stood at: vg_path's rows moved by ext_t; free space is known from
 * nowhere else). dirs: D x 3 doubles shared by all origins, 1 <= D <= 4096,
 * normalised on the device. grid: nx ny int8, row-major, cell (ix, iy) at iy nx +
 * ix. counts (may be NULL): 2 nx ny int32, the n_free plane, then the n_occ
 * plane. All sums are integer atomics: grid, counts and summary do not depend on
 * the order of the origins, on how M is walked in slabs or on the calling
 * context, and the counts of two calls over a split of the origins add up to the
 * counts of one. A plane's count is an int32: M D stays below 2^31. The planes
 * and the grid are device buffers allocated on the first call and re-used; only
 * grid, counts and summary leave the device. M == 0 gives an all-unknown grid.
 * NULL ctx, prm, grid, out, dirs or (M > 0) positions; M < 0; D outside [1,
 * 4096]; res not finite or <= 0; x0 or y0 not finite; nx or ny < 1 or nx ny >
 * 2^24; z_lo < z_hi not true; flags with a bit above 0: VG_E_ARG. Legal where
 * vg_raycast is: completes outstanding work first; mapping on or off; on an
 * owner, an attached tracker and a fleet's tracker; unsharded contexts only
 * (VG_E_STATE with world > 1). */
int vg_occupancy(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
                 const vg_occ_params* prm, int8_t* grid, int32_t* counts, vg_occ_summary* out);

/* ---- Terrain layer: ground elevation, steps and a ground-relative 2-D grid -------
 * vg_occupancy's band is relative to each ray's own origin, which is right only
 * while the sensor keeps one height above one flat floor. vg_terrain casts the
 * same M origins x D directions twice: first to collect the hits on ground planes
 * into a per-cell elevation, then to mark obstacle and free relative to the
 * ground under the ray. It leaves an int8 grid of VG_OCC_* values in the device
 * slot where vg_occupancy leaves its own (vg_clearance, vg_frontiers and
 * vg_view_gain with grid == NULL read it). Cells, r_end and which rays mark are
 * vg_occupancy's: a ray with VG_RAY_TRUNCATED, VG_RAY_LEFT_RANGE or
 * VG_RAY_INVALID marks nothing in either pass.
 *
 * Heights are integers: q(z) = (int64) floor(z / z_res), the division and the
 * floor in double. |q| >= 2^30 is out of range: such a hit is no ground hit and
 * adds no n_occ, such a piece is no free piece, and an origin's q(o_z -
 * sensor_height) is held to +-2^30. clo = q(clear_lo), chi = q(clear_hi) and
 * smax = q(step_max) are taken once on the host.
 *
 * Pass 1, ground. A marking ray with record m, unit direction d and h = o +
 * m.range d has a ground hit when it hit, d_z < 0, |m.normal[2]| >= up_min, g_lo
 * <= m.range d_z <= g_hi, q(h_z) is in range and the cell (floor((h_x - x0) /
 * res), floor((h_y - y0) / res)) lies inside the grid. Each ground hit adds to
 * four planes with integer atomics: g_n += 1 (int32), g_sum += q(h_z) (int64),
 * g_min = min(g_min, q(h_z)), g_max = max(g_max, q(h_z)) (int32; INT32_MAX and
 * INT32_MIN where g_n is 0). A hit of a marking ray whose q(h_z) is out of range
 * is counted in n_out_of_range, whatever its plane.
 *
 * Per cell. elev = floor(g_sum / g_n), the mathematical floor (sums can be
 * negative), when g_n >= min_ground; else VG_TER_NONE. spread = g_max - g_min, 0
 * when g_n is 0 (the summary's max_spread only). step[i] = max |elev[i] -
 * elev[j]| over the 8-neighbours j inside the grid with elev[j] != VG_TER_NONE; 0
 * when elev[i] is VG_TER_NONE or no neighbour has an elevation. The range of q
 * keeps spread and step inside int32.
 *
 * Pass 2, marks. Every marking ray is traced again and walks the lattice as in
 * vg_occupancy (the same pieces of positive length, a cell at most once) over
 * the whole open interval (max(t_min, 0), r_end), with no origin band. It
 * carries a ground reference ref, first q(o_z - sensor_height). On every piece
 * (t_in, t_out) in a cell inside the grid, in the order of the walk: where the
 * cell's elev != VG_TER_NONE, ref becomes that elevation; then the piece is a
 * free piece when clo <= q(o_z + 0.5 (t_in + t_out) d_z) - ref <= chi. After the
 * walk the hit is judged against elev of its own cell where that exists, else
 * against the ref the walk ended with (the last ground the ray passed over: what
 * stands under a wall's base cell that no ray sees into): it is in band when clo
 * <= q(h_z) - that reference <= chi. An in-band hit inside the grid adds 1 to
 * n_occ of its cell. Every free piece adds 1 to n_free of its cell, except in
 * the in-band hit's own cell (that cell's free mark waits until the hit is
 * judged). A ray with d_x = d_y = 0 marks only the cell it stands in. flags bit
 * 0: a ray with VG_RAY_OCCUPIED makes no free mark; it still carries ref and
 * marks its hit.
 *
 * Per cell, vg_occupancy's rule on n_free and n_occ first; then with flags bit 1
 * a cell with elev != VG_TER_NONE and step > smax becomes VG_OCC_OCCUPIED.
 *
 * One elevation per cell: a bridge over a road keeps the level inside the ground
 * band. Each ray is traced twice, the price of needing the whole elevation
 * before any mark. */
#define VG_TER_NONE INT32_MIN   /* elev where the cell has fewer than min_ground ground hits */
typedef struct vg_terrain_params {   /* 224 bytes, no implicit padding */
  vg_ray_params ray;        /* as vg_raycast; zero fields: its defaults */
  double x0, y0;            /* as vg_occ_params */
  double res;               /* as vg_occ_params */
  int    nx, ny;            /* as vg_occ_params */
  double free_on_miss;      /* as vg_occ_params */
  int    min_occ;           /* <= 0: 1 */
  int    min_free;          /* <= 0: 1 */
  double occ_ratio;         /* <= 0: off */
  int    flags;             /* bit 0: a ray with VG_RAY_OCCUPIED marks no free cell; bit 1: the step rule */
  int    min_ground;        /* ground hits a cell needs for an elevation; <= 0: 1 */
  double z_res;             /* the height quantum, metres; <= 0: 0.001; finite */
  double up_min;            /* a plane is ground when |normal[2]| >= up_min; <= 0: 0.8191520442889918 (cos 35 deg) */
  double g_lo, g_hi;        /* a ground hit's height relative to its ray's origin, g_lo <= range d_z <= g_hi;
                               both 0: -3.0 and -0.1; else g_lo < g_hi */
  double clear_lo, clear_hi;/* the band above the ground in which a hit is an obstacle and a crossed cell is
                               known free; both 0: 0.15 and 1.5; else clear_lo < clear_hi */
  double sensor_height;     /* ref before any elevation is met is q(o_z - sensor_height); finite, >= 0 */
  double step_max;          /* flags bit 1: the largest step that stays passable, metres; finite, >= 0 */
  double reserved[4];
} vg_terrain_params;
typedef struct vg_terrain_summary {   /* 128 bytes, no implicit padding */
  int64_t n_rays, n_hits, n_hits_in_band, n_truncated, n_occupied_unknown, n_invalid;
                                          /* as vg_occ_summary; in band: pass 2's, of rays that mark */
  int64_t n_ground_hits, n_out_of_range;  /* the sum of g_n; hits of marking rays with q(h_z) out of range */
  int64_t cells_ground;                   /* cells with elev != VG_TER_NONE */
  int32_t max_step, max_spread;           /* over all cells */
  int64_t cells_step_lethal;              /* flags bit 1: cells with an elevation and step > smax; else 0 */
  int64_t free_marks, occ_marks;          /* sums of the two count planes */
  int64_t cells_free, cells_occupied, cells_unknown;   /* of the grid as returned */
} vg_terrain_summary;
/* positions, M, dirs, D, grid: as vg_occupancy. elev, step (nx ny int32 each) and
 * counts (2 nx ny int32, n_free then n_occ) may each be NULL: that output is not
 * copied out. Every sum is an integer atomic and min and max commute: no output
 * depends on the order of the origins, on how M is walked in slabs or on the
 * calling context. The four ground planes of two calls over a split of the
 * origins combine to those of one (add, add, min, max). The counts, elev, step
 * and the grid of two such calls do not: pass 2 of a call reads the elevation of
 * that call's own ground hits, so every origin whose rays should share a ground
 * goes into one call. Only the outputs asked
 * for and the summary leave the device. M == 0 gives an all-unknown grid and
 * elev all VG_TER_NONE. vg_occupancy's argument errors; z_res, up_min,
 * sensor_height or (flags bit 1) step_max not finite; sensor_height or step_max
 * negative; g_lo, g_hi not both 0 and g_lo < g_hi not true; the same of
 * clear_lo, clear_hi; flags with a bit above 1: VG_E_ARG. Legal where vg_raycast
 * is; unsharded contexts only (VG_E_STATE with world > 1).
 *
 * The four ground planes are not an output of this call. Tests and tools reach
 * them through two hooks the library exports beside it (not part of the stable
 * interface, as every vgx_ symbol): vgx_ter_ground copies the last call's planes
 * out (given that call's nx, ny), vgx_ter_cells runs the per-cell stage alone on planes it is given. */
int vg_terrain(vg_ctx* ctx, const double* positions, int M, const double* dirs, int D,
               const vg_terrain_params* prm, int8_t* grid, int32_t* elev, int32_t* step, int32_t* counts,
               vg_terrain_summary* out);

/* ---- Clearance field and costmap: what a planner needs of the 2-D grid ---------
 * The exact Euclidean distance transform of an nx x ny grid of VG_OCC_* cells,
 * its feature transform, and nav2's inflation-layer cost of the distance, all on
 * the device. Cells are indexed i = iy nx + ix as in vg_occupancy. Reads no map
 * and keeps no state; everything is integer arithmetic or a table look-up, so the
 * same inputs give the same bytes from any context.
 *
 * The obstacle set O: the cells with value VG_OCC_OCCUPIED, and with flags bit 0
 * those with value VG_OCC_UNKNOWN too. Any other byte value is free.
 *   dist2[i]   = min over o in O of (ix - ox)^2 + (iy - oy)^2, an exact int32 in
 *                cells squared: 0 on an obstacle, VG_CLR_NONE when O is empty.
 *   nearest[i] = the linear index of the obstacle attaining that minimum, among
 *                equals the smallest linear index; -1 when O is empty.
 *   cost[i], with d = res sqrt((double)dist2[i]):
 *                VG_COST_LETHAL (254) if dist2 == 0;
 *                else VG_COST_INSCRIBED (253) if d <= inscribed_radius;
 *                else (uint8_t)(252.0 exp(-cost_scaling (d - inscribed_radius)))
 *                  if d <= inflation_radius;
 *                else VG_COST_FREE (0) — also where O is empty.
 *              An unknown cell that is not an obstacle (bit 0 clear) gets
 *              VG_COST_NO_INFO (255) unless the value above is at least 253; then
 *              it keeps that value (nav2's rule with inflate_unknown off).
 * The cost formula is evaluated on the host in double, into a table indexed by
 * dist2 with entries 0 .. floor((inflation_radius / res)^2) that the device looks
 * up; the device's exp never enters, and the cost is a pure function of dist2.
 *
 * Two passes. Per column, a down and an up sweep leave every cell the signed row
 * offset to the nearest obstacle of its own column (equal distances: the smaller
 * iy). Per row, every cell searches outward over the columns ix -+ k for the
 * lexicographic minimum of (k^2 + g^2, index), g the column's offset, and stops
 * once k^2 exceeds the best so far, which is exact. */
#define VG_CLR_NONE      INT32_MAX   /* dist2 where the grid holds no obstacle at all */
#define VG_CLR_MAX_SIDE  32768       /* nx, ny <= this: 2 * 32767^2 < 2^31 */
#define VG_COST_FREE 0
#define VG_COST_INSCRIBED 253
#define VG_COST_LETHAL 254
#define VG_COST_NO_INFO 255
typedef struct vg_clr_params {
  int    nx, ny;             /* as vg_occ_params; nx ny <= VG_OCC_MAX_CELLS, each <= VG_CLR_MAX_SIDE */
  double res;                /* cell edge, metres; finite, > 0 */
  int    flags;              /* bit 0: an unknown cell (-1) is an obstacle too */
  int    pad;
  double inscribed_radius;   /* metres, >= 0 */
  double inflation_radius;   /* metres, >= inscribed_radius */
  double cost_scaling;       /* 1/m, >= 0 (nav2's cost_scaling_factor) */
  double reserved[4];
} vg_clr_params;
typedef struct vg_clr_summary {   /* 128 bytes, no implicit padding */
  int64_t n_obstacles, n_unknown;         /* cells in O; cells with value VG_OCC_UNKNOWN (in O or not) */
  int64_t cells_lethal, cells_inscribed, cells_inflated, cells_free, cells_no_info;
                                          /* cells by cost: 254, 253, 1 .. 252, 0, 255; they sum to nx ny */
  int64_t max_dist2;                      /* the largest dist2 of any cell; 0 when O is empty */
  int64_t reserved[8];
} vg_clr_summary;
/* grid: nx ny int8 on the host, or NULL: the grid that the last vg_occupancy or
 * vg_terrain call on this context left on the device (both write the same slot),
 * of which nothing is uploaded (VG_E_STATE when there was no such call or its nx,
 * ny differ from prm's). dist2, nearest
 * (nx ny int32 each) and cost (nx ny uint8) may each be NULL: that output is not
 * copied out. The planes are device buffers allocated on first use and re-used;
 * only the outputs asked for and the summary leave the device. NULL ctx, prm or
 * out; nx or ny < 1 or > VG_CLR_MAX_SIDE, or nx ny > VG_OCC_MAX_CELLS; res not
 * finite or <= 0; a radius or cost_scaling negative or not finite;
 * inflation_radius < inscribed_radius; flags with a bit above 0; a cost table of
 * more than 2^24 entries: VG_E_ARG, and nothing is written. Legal where
 * vg_occupancy is: completes outstanding work first; mapping on or off; on an
 * owner, an attached tracker and a fleet's tracker; unsharded contexts only
 * (VG_E_STATE with world > 1). */
int vg_clearance(vg_ctx* ctx, const int8_t* grid, const vg_clr_params* prm,
                 int32_t* dist2, int32_t* nearest, uint8_t* cost, vg_clr_summary* out);

/* ---- Navigation function: cost-to-go over the costmap, and the paths down it ----
 * nav2's NavFn on the device: the minimum cost-to-go from every cell of an nx x ny
 * cost plane (uint8, the VG_COST_* values of vg_clearance, i = iy nx + ix) to the
 * nearest of a set of goal cells, and the paths that descend it. One field serves
 * every robot heading for the same goals. Everything is integer arithmetic, so the
 * outputs are a pure function of the inputs and equal a host Dijkstra bit for bit.
 *
 * A 256-entry uint16 table trav turns a cost byte into the price of standing on a
 * cell; trav[c] == 0 means impassable. The default table, filled on the host:
 *   trav[c]   = neutral + (int)floor(factor c)   for c < lethal_from,
 *   trav[c]   = 0                                for lethal_from <= c <= 254,
 *   trav[255] = 0, or with flags bit 0 trav[unknown_as].
 * The graph: the 8-connected grid over the passable cells. An edge a-b exists only
 * if both cells are passable and, for a diagonal step, both cells it squeezes
 * between, (ay, bx) and (by, ax), are passable too (no corner cutting). Its weight
 *   w(a, b) = K (trav[cost[a]] + trav[cost[b]]),  K = VG_NAV_K_ORTHO (12) for an
 * orthogonal and VG_NAV_K_DIAG (17) for a diagonal step (17 / 12 ~ sqrt 2), is
 * symmetric, so the field from the goals is also the cost to them.
 *
 * The goals: n_goals cells (ix, iy). One outside the grid or on an impassable cell
 * is ignored and counted. With D(i) the shortest-path weight from cell i to the
 * nearest used goal, as a mathematical integer,
 *   pot[i] = min(D(i), VG_NAV_SAT), and VG_NAV_UNREACHED where no path exists or
 *            the cell is impassable.
 * Every relaxation adds with saturation at VG_NAV_SAT; saturation is monotone, so
 * the fixed point of saturating relaxations is exactly min(D, VG_NAV_SAT).
 *
 * A path starts at a start cell c with pot[c] < VG_NAV_UNREACHED and repeats: among
 * the neighbours n joined to c by an edge with pot[n] < pot[c], step to the one
 * minimising pot[n] + w(c, n) (64-bit), among equals the smallest linear index;
 * stop when pot[c] == 0. pot strictly falls, so a walk ends within nx ny steps. */
#define VG_NAV_SAT        0xFFFFFFFEu   /* pot: the cost-to-go is this or more */
#define VG_NAV_UNREACHED  0xFFFFFFFFu   /* pot: impassable, or no path to any used goal */
#define VG_NAV_K_ORTHO 12
#define VG_NAV_K_DIAG  17
#define VG_NAV_MAX_POINTS 65536         /* n_goals, n_starts <= this */
#define VG_NAV_MAX_PATH_CELLS (1 << 27) /* n_starts max_len <= this */
#define VG_NAV_REACHED   0   /* the path's last cell is a goal */
#define VG_NAV_NO_PATH   1   /* the start is outside the grid, impassable or unreached; len 0 */
#define VG_NAV_TRUNCATED 2   /* max_len cells were written before a goal */
#define VG_NAV_STUCK     3   /* no strictly lower neighbour: only inside a saturated plateau */
typedef struct vg_nav_params {   /* 64 bytes, no implicit padding */
  int    nx, ny;        /* as vg_clr_params; nx ny <= VG_OCC_MAX_CELLS, each <= VG_CLR_MAX_SIDE */
  int    flags;         /* bit 0: an unknown cell (255) is passable at trav[unknown_as] */
  int    neutral;       /* 0: 50 (nav2's neutral_cost); else >= 1 */
  int    lethal_from;   /* 0: 253; else 1 .. 255: cost bytes from here to 254 are impassable */
  int    unknown_as;    /* 0 .. 254: the cost byte an unknown cell is priced as (flags bit 0) */
  double factor;        /* 0: 0.8 (nav2's cost_factor); else finite, > 0 */
  double reserved[4];
} vg_nav_params;
typedef struct vg_nav_summary {   /* 128 bytes, no implicit padding */
  int64_t n_goals_used, n_goals_ignored;  /* they sum to n_goals (a cell named twice counts twice) */
  int64_t cells_passable;                 /* cells with trav[cost] > 0 */
  int64_t cells_reached;                  /* cells with pot < VG_NAV_UNREACHED (the saturated ones among them) */
  int64_t cells_saturated;                /* cells with pot == VG_NAV_SAT */
  int64_t max_pot;                        /* the largest pot of a reached cell; 0 when none is reached */
  int64_t rounds, tile_runs;              /* relaxation rounds launched and tiles relaxed in them: these two
                                             depend on scheduling and are not reproducible; every other
                                             field is a pure function of the input */
  int64_t reserved[8];
} vg_nav_summary;
/* cost: nx ny uint8 on the host, or NULL: the cost plane that the last vg_clearance
 * call on this context left on the device, of which nothing is uploaded
 * (VG_E_STATE when no call produced one or its nx, ny differ from prm's). trav: 256
 * uint16, or NULL: the default table of prm (an explicit table makes neutral,
 * lethal_from, unknown_as, factor and flags bit 0 irrelevant; their ranges are
 * still checked, the default table's overflow is not, no such table being
 * built). goals: n_goals pairs (ix, iy). pot: nx ny uint32, or NULL: the field is
 * not copied out. It stays on the device for vg_nav_paths until the next vg_navfn
 * call or vg_destroy. NULL ctx, prm, goals or out; nx or ny < 1 or >
 * VG_CLR_MAX_SIDE, or nx ny > VG_OCC_MAX_CELLS; n_goals < 1 or > VG_NAV_MAX_POINTS;
 * flags with a bit above 0; neutral < 0; lethal_from < 0 or > 255; unknown_as < 0
 * or > 254; factor negative or not finite; a default-table entry above 65535:
 * VG_E_ARG, and nothing is written. The relaxation is iterated from the host to
 * its fixed point, at most nx ny + 2 rounds; were that cap ever hit the call
 * returns VG_E_CAPACITY and leaves no field. Legal where vg_clearance is. */
int vg_navfn(vg_ctx* ctx, const uint8_t* cost, const vg_nav_params* prm, const uint16_t* trav,
             const int32_t* goals, int n_goals, uint32_t* pot, vg_nav_summary* out);
/* Paths down the field of the last vg_navfn call on this context (VG_E_STATE
 * without one). starts: n_starts pairs (ix, iy). cells: n_starts rows of max_len
 * int32, row s holding the linear indices of path s from its start on, len[s] of
 * them, the rest -1. status: VG_NAV_* per start. path_cost (or NULL): pot[start]
 * per start, -1 with VG_NAV_NO_PATH. NULL ctx, starts, cells, len or status;
 * n_starts < 1 or > VG_NAV_MAX_POINTS; max_len < 1; n_starts max_len >
 * VG_NAV_MAX_PATH_CELLS: VG_E_ARG, and nothing is written. */
int vg_nav_paths(vg_ctx* ctx, const int32_t* starts, int n_starts, int max_len, int32_t* cells,
                 int32_t* len, int32_t* status, int64_t* path_cost);

/* ---- Exploration frontiers: the free / unknown boundary, labelled and ranked -----
 * What a robot that is still mapping heads for: the free cells of an nx x ny grid
 * of VG_OCC_* values (i = iy nx + ix as in vg_occupancy) that touch unknown space,
 * grouped into connected components on the device, one record per component.
 * Everything is integer arithmetic, so every output byte is a pure function of the
 * inputs.
 *
 * Cell i is a frontier cell when all of these hold:
 *   grid[i] == VG_OCC_FREE (exactly 0; any other byte value is not free here);
 *   at least one of its 4-neighbours inside the grid equals VG_OCC_UNKNOWN (what
 *     lies outside the grid is not unknown);
 *   with flags bit 0: cost[i] < cost_max, cost the VG_COST_* plane of vg_clearance;
 *   with flags bit 1: pot[i] != VG_NAV_UNREACHED, pot the field that the last
 *     vg_navfn call left on this context. w(a, b) is symmetric, so a field computed
 *     with the robot's own cell as the only goal is the cost from the robot to
 *     every cell: this test keeps what the robot can reach, and best_cell below is
 *     the cheapest cell of a frontier to drive to.
 * The cost test comes before the reach test: a free cell beside an unknown one
 * that fails the cost test is counted in n_rejected_cost and not looked at again;
 * one that passes it and fails the reach test is counted in n_rejected_unreached.
 *
 * A frontier is an 8-connected component of frontier cells. label[i] is the
 * smallest linear index among the cells of i's component, -1 where i is no
 * frontier cell. The components are found by a union-find that takes a fixed
 * number of launches whatever their shape. */
#define VG_FRONTIER_MAX_RECORDS 65536
typedef struct vg_frontier_params {   /* 56 bytes, no implicit padding */
  int    nx, ny;        /* as vg_clr_params; nx ny <= VG_OCC_MAX_CELLS, each <= VG_CLR_MAX_SIDE */
  int    flags;         /* bit 0: the cost test; bit 1: the reach test, and best_cell */
  int    cost_max;      /* 0: 253 (VG_COST_INSCRIBED); else 1 .. 255 (flags bit 0) */
  int    min_size;      /* a component of fewer cells gets no record; <= 0: 1 */
  int    pad;
  double reserved[4];
} vg_frontier_params;
typedef struct vg_frontier_rec {      /* 64 bytes, no implicit padding */
  int32_t  label, size;               /* the component's smallest linear index; its cells */
  int32_t  x_min, y_min, x_max, y_max;
  int64_t  sum_x, sum_y;              /* sums of ix and of iy over the component: the centroid is sum / size */
  int32_t  best_cell;                 /* flags bit 1: the component's cell with the smallest pot, among equals the
                                         smallest linear index; else -1 */
  uint32_t best_pot;                  /* its pot; 0 without bit 1 */
  int64_t  reserved[2];
} vg_frontier_rec;
typedef struct vg_frontier_summary {  /* 128 bytes, no implicit padding; every field is reproducible */
  int64_t n_frontier_cells, n_components; /* frontier cells; their components */
  int64_t n_kept, n_written;              /* components with size >= min_size; records written: min(n_kept, max_records) */
  int64_t max_size;                       /* the largest component's cells; 0 without any */
  int64_t cells_free, cells_unknown;      /* cells with value VG_OCC_FREE; VG_OCC_UNKNOWN */
  int64_t n_rejected_cost, n_rejected_unreached;
  int64_t reserved[7];
} vg_frontier_summary;
#ifdef __cplusplus
static_assert(sizeof(vg_frontier_params) == 56 && sizeof(vg_frontier_rec) == 64 && sizeof(vg_frontier_summary) == 128,
              "the frontier records have no implicit padding");
#else
_Static_assert(sizeof(vg_frontier_params) == 56 && sizeof(vg_frontier_rec) == 64 && sizeof(vg_frontier_summary) == 128,
               "the frontier records have no implicit padding");
#endif
/* grid: nx ny int8 on the host, or NULL: the grid that the last vg_occupancy or
 * vg_terrain call on this context left on the device (VG_E_STATE when there was no such call or its nx,
 * ny differ from prm's). cost: consulted only with flags bit 0; nx ny uint8 on the
 * host, or NULL: the plane that the last vg_clearance call on this context left on
 * the device (VG_E_STATE when no call produced one or its nx, ny differ). With
 * flags bit 1 the field of the last vg_navfn call on this context is read where it
 * lies (VG_E_STATE without one, or when its nx, ny differ). labels: nx ny int32, or
 * NULL: not copied out. recs: the components with size >= min_size in ascending
 * label, the first max_records of them. All planes are device buffers allocated on
 * first use and re-used; only labels (when asked for), the records written and
 * the summary leave the device. NULL ctx, prm or out; nx or ny < 1 or >
 * VG_CLR_MAX_SIDE, or nx ny > VG_OCC_MAX_CELLS; flags with a bit above 1; cost !=
 * NULL with flags bit 0 clear; cost_max < 0 or > 255; max_records < 0 or >
 * VG_FRONTIER_MAX_RECORDS; recs == NULL with max_records > 0: VG_E_ARG, and nothing
 * is written. Every device loop that follows parent links is bounded by nx ny
 * steps; were that bound ever hit the call returns VG_E_CAPACITY with nothing
 * written. Legal where vg_clearance is. */
int vg_frontiers(vg_ctx* ctx, const int8_t* grid, const uint8_t* cost, const vg_frontier_params* prm,
                 int32_t* labels, vg_frontier_rec* recs, int max_records, vg_frontier_summary* out);

/* ---- View gain: the unknown space a 2-D sensor would see from candidate cells -----
 * What a robot would learn by driving to a cell: from cell (ox, oy) of an nx x ny
 * grid of VG_OCC_* values (i = iy nx + ix as in vg_occupancy), which cells does a
 * 2-D sensor of range R cells see, and how many of them are unknown? All
 * arithmetic is integer, so every output byte is a pure function of the inputs. A
 * byte value that is neither VG_OCC_OCCUPIED nor VG_OCC_UNKNOWN is free, as in
 * vg_clearance.
 *
 * Targets: 8R per viewpoint, every offset (dx, dy) with max(|dx|, |dy|) = R. For a
 * target let n = R, ax = |dx|, ay = |dy| and sx, sy the signs of dx, dy.
 * Ray cells: cell k of the ray, k = 1 .. n, is
 *   c_k = (ox + sx ((2 k ax + n) div (2 n)), oy + sy ((2 k ay + n) div (2 n))),
 * div the division of non-negative integers: rounding half away from zero, so the
 * set is symmetric under the grid's eight reflections, and consecutive cells
 * differ by at most 1 in each coordinate. (The remainder may be kept
 * incrementally; that is exact.)
 * The walk: c_0 is the origin. A ray walks k = 1, 2, ... with u = 0 and at each k
 * tests in this order:
 *   1. c_k outside the grid: the ray ends (open).
 *   2. (cx - ox)^2 + (cy - oy)^2 > R^2: the ray ends (open).
 *   3. the step from c_{k-1} to c_k is diagonal and both cells it squeezes
 *      between, (c_{k-1}.x, c_k.y) and (c_k.x, c_{k-1}.y), are VG_OCC_OCCUPIED: the
 *      ray ends (blocked). (Both lie inside the grid.) This is vg_navfn's
 *      no-corner-cutting rule: a one-cell-thick diagonal wall does not leak.
 *   4. c_k becomes visible.
 *   5. grid[c_k] == VG_OCC_OCCUPIED: the ray ends (blocked).
 *   6. grid[c_k] == VG_OCC_UNKNOWN: u += 1; with max_unknown > 0 and u >=
 *      max_unknown the ray ends (open).
 *   7. after k = n the ray ends (open).
 * The visible set of a viewpoint is the union over its 8R rays, plus the origin's
 * own cell. Each cell counts once, however many rays cross it.
 * Status: an origin outside the grid gives VG_VIEW_OUTSIDE, one on an occupied
 * cell VG_VIEW_BLOCKED; both give zero counts and contribute to nothing. Anything
 * else is VG_VIEW_OK. */
#define VG_VIEW_MAX_RADIUS 255
#define VG_VIEW_OK       0
#define VG_VIEW_OUTSIDE  1   /* the origin is outside the grid */
#define VG_VIEW_BLOCKED  2   /* the origin is an occupied cell */
typedef struct vg_view_params {    /* 56 bytes, no implicit padding */
  int    nx, ny;        /* as vg_frontier_params; nx ny <= VG_OCC_MAX_CELLS, each <= VG_CLR_MAX_SIDE */
  int    radius;        /* R, cells: 1 .. VG_VIEW_MAX_RADIUS */
  int    max_unknown;   /* >= 0; > 0: a ray ends at its max_unknown-th unknown cell */
  int    flags;         /* must be 0 */
  int    pad;
  double reserved[4];
} vg_view_params;
typedef struct vg_view_rec {       /* 32 bytes, no implicit padding */
  int32_t ix, iy, status;          /* the viewpoint as given; VG_VIEW_* */
  int32_t n_visible;               /* cells of the visible set */
  int32_t n_unknown, n_free, n_occupied;  /* ... by class; they sum to n_visible */
  int32_t n_rays_open;             /* rays of the 8R that ended open */
} vg_view_rec;
typedef struct vg_view_summary {   /* 128 bytes, no implicit padding; every field is reproducible */
  int64_t n_views, n_ok, n_outside, n_blocked;  /* viewpoints; by status */
  int64_t rays;                    /* 8R per VG_VIEW_OK viewpoint */
  int64_t max_unknown_seen;        /* the largest n_unknown of an OK viewpoint; 0 without one */
  int64_t best_view;               /* the index of the viewpoint that has it, among equals the smallest index;
                                      -1 without an OK viewpoint */
  int64_t cells_seen, unknown_seen;  /* cells in at least one viewpoint's visible set; the unknown ones among
                                        them: the gain of the whole set, not the sum of the per-view gains */
  int64_t reserved[7];
} vg_view_summary;
#ifdef __cplusplus
static_assert(sizeof(vg_view_params) == 56 && sizeof(vg_view_rec) == 32 && sizeof(vg_view_summary) == 128,
              "the view records have no implicit padding");
#else
_Static_assert(sizeof(vg_view_params) == 56 && sizeof(vg_view_rec) == 32 && sizeof(vg_view_summary) == 128,
               "the view records have no implicit padding");
#endif
/* grid: nx ny int8 on the host, or NULL: the grid that the last vg_occupancy or
 * vg_terrain call on this context left on the device (VG_E_STATE when there was no such call or its nx,
 * ny differ from prm's). views: n_views pairs (ix, iy), 1 <= n_views <=
 * VG_NAV_MAX_POINTS; recs: one record per viewpoint, in the order given. A cell
 * named twice gets two records and counts twice in seen. seen: nx ny int32, or
 * NULL: not copied out; seen[i] is the number of VG_VIEW_OK viewpoints whose
 * visible set holds cell i. The counts are integer atomics: seen and the summary do
 * not depend on the order of the viewpoints, and the seen planes of two calls over
 * a split of the viewpoints add up to the plane of one call. All planes are device
 * buffers allocated on first use and re-used; only the records, seen (when asked
 * for) and the summary leave the device. NULL ctx, prm, views, recs or out; nx or
 * ny < 1 or > VG_CLR_MAX_SIDE, or nx ny > VG_OCC_MAX_CELLS; radius < 1 or >
 * VG_VIEW_MAX_RADIUS; max_unknown < 0; flags != 0; n_views < 1 or >
 * VG_NAV_MAX_POINTS: VG_E_ARG, and nothing is written. Legal where vg_clearance is:
 * completes outstanding work first; unsharded contexts only (VG_E_STATE with world
 * > 1). */
int vg_view_gain(vg_ctx* ctx, const int8_t* grid, const vg_view_params* prm, const int32_t* views, int n_views,
                 vg_view_rec* recs, int32_t* seen, vg_view_summary* out);

/* ---- Change layer: scan-vs-map evidence summed over many scans ----------------
 * One scan's classes do not say what changed: leaf planes reach to their cube's
 * faces past a real edge, so a static scene already shows some VANISHED. The
 * evidence that separates the two is per map leaf and per place, summed over many
 * scans and sensors. The layer is a side structure next to a frozen map, owned by
 * the context that owns the map; the map's bits never change.
 *   per node (int32): n_consistent, n_vanished, n_occluded, n_scans, last_epoch;
 *   a cell table for new surfaces: an open-addressed hash of 2^cell_hash_log2
 *     slots keyed by the packed integer cell of a world point w, k_j = floor(w_j /
 *     cell), |k_j| < 2^20, packed as root keys are; per slot int32 n_appeared,
 *     n_scans, last_epoch and int64 sum_q[3];
 *   totals (int64).
 * Per point of an accumulated scan, classified exactly as vg_scan_diff does, with
 * leaf the hit's node id: CONSISTENT n_consistent[leaf]++; VANISHED
 * n_vanished[leaf]++; APPEARED n_occluded[leaf]++ and the point is charged to the
 * cell of its world position w: n_appeared++, sum_q[j] += q_j, q_j =
 * clamp((int)floor((w_j - k_j cell) / cell * 65536), 0, 65535); UNKNOWN: the
 * totals only. Every accumulate call takes the next epoch (from 1); a leaf charged
 * CONSISTENT or VANISHED, and a cell charged a point, counts the call once in its
 * n_scans. Every sum is an integer sum, so the layer after a set of scans has the
 * same bits in whatever order, from whichever context and at whatever position in
 * the cloud the points arrived — as long as no point was dropped: a point whose
 * cell finds the table full (the probe is bounded by the table size) is dropped
 * and counted, and which points those are depends on the order. */
typedef struct vg_change_params {
  vg_diff_params diff;     /* zero fields: vg_scan_diff's defaults */
  double cell;             /* cell edge in metres; <= 0: voxel_size / 4 */
  int    cell_hash_log2;   /* <= 0: 20; at most 26 */
  int    pad;
  double reserved[4];
} vg_change_params;
typedef struct vg_change_query {
  int    min_obs;          /* <= 0: 5 */
  int    min_scans;        /* <= 0: 2 */
  double vanished_ratio;   /* <= 0: 0.8 */
  int    flags;            /* bit 0: every touched leaf / used cell, whether or not it meets its rule */
  int    pad;
  double reserved[4];
} vg_change_query;
typedef struct vg_change_leaf {   /* 112 bytes, no implicit padding */
  int32_t node, layer, n_consistent, n_vanished, n_occluded, n_scans;
  int32_t flags;                  /* bit 0: meets the removed rule */
  int32_t pad;
  double  voxel_center[3], quater_length, center[3], normal[3];  /* as vg_map_planes gives them */
} vg_change_leaf;
typedef struct vg_change_cell {   /* 56 bytes, no implicit padding */
  int32_t key[3];                 /* k_j */
  int32_t n_appeared, n_scans;
  int32_t flags;                  /* bit 0: meets the added rule */
  int32_t pad[2];
  double  centroid[3];            /* cell (k_j + (sum_q_j + 0.5 n_appeared) / (65536 n_appeared)) */
} vg_change_cell;
typedef struct vg_change_totals { /* 128 bytes */
  int64_t calls, points;          /* accumulate calls; their points */
  int64_t n[4];                   /* points per class, indexed by VG_DIFF_* */
  int64_t cells_used;             /* occupied slots of the cell table */
  int64_t dropped;                /* APPEARED points whose cell found the table full */
  int64_t out_of_range;           /* APPEARED points whose cell index left the key range */
  int64_t leaves_touched;         /* nodes with a non-zero counter */
  int64_t reserved[6];
} vg_change_totals;
/* vg_change_begin creates the layer (prm NULL: the defaults) on the context that
 * owns a frozen map. VG_E_STATE: mapping is on, the context is sharded, inside a
 * scan, itself attached, or has a layer already. VG_E_ARG: cell_hash_log2 > 26.
 * vg_change_accumulate* may be called on the owner and on any tracker attached to
 * it (a fleet's tracker between fleet steps included) and charges the owner's
 * layer; VG_E_STATE when the map it reads has no layer. Arguments as
 * vg_scan_diff's (pose12 NULL: the calling context's current state; out may be
 * NULL here), and per_point and *out have vg_scan_diff's bits for the same input.
 * The _dev form takes the cloud as three device arrays. Completes the calling
 * context's outstanding work first; synchronous; calls into one layer are
 * serialised inside the library, so they may come from several threads. n == 0 is
 * legal: it takes an epoch and counts a call. A call that fails takes no epoch
 * and leaves the totals as they were; after VG_E_HIP the layer's contents are
 * undefined (vg_change_clear). A call that another thread's vg_change_end
 * overtakes returns VG_E_STATE: the layer is looked up under the owner's lock.
 * vg_change_report (owner or attached tracker): the leaves that meet the removed
 * rule — n_vanished >= min_obs, n_scans >= min_scans and n_vanished >=
 * vanished_ratio (n_vanished + n_consistent) — in ascending node id, and the cells
 * that meet the added rule — n_appeared >= min_obs and n_scans >= min_scans — in
 * ascending packed key; with flags bit 0 every touched leaf and used cell, the
 * record's flags telling which meet the rule. min(count, cap) records are copied,
 * the counts always returned; NULL arrays query the counts. q NULL: the defaults.
 * totals may be NULL.
 * vg_change_clear zeroes the layer (the epochs restart at 1); vg_change_end frees
 * it. Both on the owner (VG_E_STATE without a layer).
 * While a layer exists node ids must not move and the map must not change: on the
 * owner vg_set_mapping(owner, 1), vg_reset, vg_checkpoint_load, vg_checkpoint_save
 * (it compacts), vg_release_far with the compaction flag, vg_shard_* and
 * vg_destroy return VG_E_STATE and change nothing. Frozen vg_step*, scoring,
 * relocalise, ray-casting, vg_scan_diff, attach, detach and fleets work as before.
 * The layer is not part of a checkpoint. */
int vg_change_begin(vg_ctx* ctx, const vg_change_params* prm);
int vg_change_accumulate(vg_ctx* ctx, const float* xyz, int n, const double* pose12,
                         vg_diff_point* per_point, vg_diff_summary* out);
int vg_change_accumulate_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int n,
                             const double* pose12, vg_diff_summary* out);
int vg_change_report(vg_ctx* ctx, const vg_change_query* q, vg_change_leaf* leaves, int leaf_cap, int* n_leaves,
                     vg_change_cell* cells, int cell_cap, int* n_cells, vg_change_totals* totals);
int vg_change_clear(vg_ctx* ctx);
int vg_change_end(vg_ctx* ctx);

/* ---- Live obstacle layer: what the sensor sees now, folded into the 2-D grid -------
 * vg_occupancy and vg_terrain give the grid of the saved map. A robot that localises
 * in it plans through a pallet or a person in the aisle unless what it sees now
 * reaches that grid. The layer is nav2's obstacle layer in integers: mark where
 * live returns fall, clear where live beams pass, forget after a while, and hand
 * vg_clearance and everything behind it one grid.
 *
 * State. A layer belongs to the context it was begun on. It holds its geometry
 * (x0, y0, res, nx, ny with vg_occ_params' meaning; nx ny <= VG_OCC_MAX_CELLS, each
 * side <= VG_CLR_MAX_SIDE), a private copy of a base grid (int8, VG_OCC_*), two
 * int32 planes hit and clear, and int64 totals. hit[i] is the largest stamp of a
 * scan that marked cell i, clear[i] the largest stamp of a scan whose beam crossed
 * it; 0: never.
 *
 * Per point of a marked scan. The point is classified exactly as vg_scan_diff
 * does: the same class bits, the same o, w and r. cell(v) = (floor((v_x - x0) /
 * res), floor((v_y - y0) / res)) in double, each index held to [-2^30, 2^30]. With
 * dz = w_z - o_z, and for a point whose o and w are finite (any other point marks
 * and clears nothing, and its record's flags and cells are 0):
 *   In band: z_lo <= dz <= z_hi.
 *   Obstacle point: the class is VG_DIFF_APPEARED (with params flags bit 0
 *     VG_DIFF_UNKNOWN too), the point is in band and r_min <= r <= mark_max. It sets
 *     hit[cell(w)] = max(hit[cell(w)], stamp).
 *   Clearing beam: every point with r > 0, whatever its class. t_b = r; where
 *     clear_max < t_b, t_b = clear_max (the beam is cut); then with t_z = z_hi r / dz
 *     for dz > 0 and z_lo r / dz for dz < 0, where t_z < t_b, t_b = t_z (the beam
 *     left the band; z_lo <= 0 <= z_hi, so it starts inside). e = o + (t_b / r)(w -
 *     o), a = cell(o), b = cell(e), n = max(|b_x - a_x|, |b_y - a_y|), s the signs of
 *     b - a. The beam's cells are the view gain's ray cells from a towards b,
 *       c_k = (a_x + s_x ((2 k |b_x - a_x| + n) div 2n), a_y + s_y ((2 k |b_y - a_y| + n) div 2n)),
 *     and cells k = 0 .. n - 1 get clear = max(clear, stamp): the end cell b is never
 *     cleared by its own beam, and a beam with a == b clears nothing. n <= 4097.
 *   Marks and clears outside the grid are dropped.
 * Stamp. Every vg_live_mark call carries an int32 stamp > 0, or 0 for the layer's
 * largest stamp so far + 1. Both planes are written by integer atomic maxima only:
 * the layer after a set of (scan, pose, stamp) triples has the same bytes in
 * whatever order, and at whatever position in its cloud, the points arrived.
 *
 * Live cell at time `now`: hit > 0 && hit >= clear && (persist == 0 || now - hit <
 * persist). A scan that both marks and crosses a cell leaves it occupied (nav2
 * marks after it clears).
 * Compose. out[i] = VG_OCC_OCCUPIED where cell i is live, else base[i]; with compose
 * flags bit 0 a cell that is not live and whose base is VG_OCC_UNKNOWN becomes
 * VG_OCC_FREE when clear > 0, clear > hit and (persist == 0 || now - clear <
 * persist). The composed grid is written where vg_occupancy / vg_terrain leave
 * theirs, with its shape, so that vg_clearance, vg_frontiers and vg_view_gain with
 * grid == NULL read it unchanged. The layer's base copy is never written: a second
 * compose does not compound, and a later vg_occupancy does not reach the base. */
typedef struct vg_live_params {    /* 224 bytes, no implicit padding */
  vg_diff_params diff;      /* zero fields: vg_scan_diff's defaults */
  double x0, y0, res;       /* as vg_occ_params */
  int    nx, ny;
  double z_lo, z_hi;        /* the band of dz; both 0: -1, 1. z_lo <= 0 <= z_hi, z_lo < z_hi */
  double r_min;             /* <= 0: 0 */
  double mark_max;          /* <= 0: no limit */
  double clear_max;         /* <= 0: 4096 res, or mark_max where that is set and smaller; clear_max / res <= 4096 */
  int    persist;           /* stamps a mark or a clearing lives; <= 0: 0, for ever */
  int    flags;             /* bit 0: VG_DIFF_UNKNOWN points mark too */
  double reserved[4];
} vg_live_params;
#define VG_LIVE_MARKS     1   /* vg_live_point.flags: an obstacle point */
#define VG_LIVE_CLEARS    2   /* a clearing beam */
#define VG_LIVE_IN_BAND   4   /* z_lo <= dz <= z_hi */
#define VG_LIVE_CUT       8   /* t_b = clear_max */
#define VG_LIVE_LEFT_BAND 16  /* t_b = t_z */
typedef struct vg_live_point {     /* 32 bytes, no implicit padding */
  int32_t cls;                     /* VG_DIFF_* */
  int32_t flags;                   /* VG_LIVE_* */
  int32_t ax, ay, bx, by;          /* cell(o), cell(e); 0 without a clearing beam */
  int32_t mx, my;                  /* cell(w) */
} vg_live_point;
typedef struct vg_live_summary {   /* 128 bytes, int64 only, no implicit padding */
  int64_t n[4];                    /* points per class, indexed by VG_DIFF_* */
  int64_t n_obstacle;              /* obstacle points */
  int64_t marks_dropped;           /* ... whose cell lies outside the grid */
  int64_t n_beams;                 /* clearing beams */
  int64_t cells_live;              /* mark: cells whose hit the call raised to its stamp; compose: live cells */
  int64_t cells_cleared;           /* mark: cells whose clear the call raised to its stamp; compose: cells that are
                                      not live with clear > hit, within persist */
  int64_t cells_free, cells_occupied, cells_unknown;  /* compose: cells by composed value (any other byte: free) */
  int64_t cells_raised;            /* compose: live cells whose base is not VG_OCC_OCCUPIED */
  int64_t stamp;                   /* mark: the stamp the call used; compose: now; totals: the largest stamp so far */
  int64_t calls;                   /* totals: vg_live_mark calls that succeeded; else 0 */
  int64_t reserved;
} vg_live_summary;
#ifdef __cplusplus
static_assert(sizeof(vg_live_params) == 224 && sizeof(vg_live_point) == 32 && sizeof(vg_live_summary) == 128,
              "the live layer's records have no implicit padding");
#else
_Static_assert(sizeof(vg_live_params) == 224 && sizeof(vg_live_point) == 32 && sizeof(vg_live_summary) == 128,
               "the live layer's records have no implicit padding");
#endif
/* vg_live_begin creates the layer. base_grid: nx ny int8 on the host, or NULL: a
 * copy of the grid the last vg_occupancy / vg_terrain / vg_live_compose call on this
 * context left on the device. VG_E_ARG (nothing is created): NULL ctx or prm; res
 * not finite or <= 0; x0 or y0 not finite; nx or ny < 1 or > VG_CLR_MAX_SIDE, or nx
 * ny > VG_OCC_MAX_CELLS; a band limit that is not finite, z_lo <= 0 <= z_hi or z_lo <
 * z_hi not true; clear_max / res > 4096; flags with a bit above 0. VG_E_STATE: the
 * context is sharded (world > 1), has a layer already, or base_grid is NULL and no
 * grid is held or its nx, ny differ from prm's.
 * vg_live_mark: xyz, n and pose12 as vg_scan_diff's (pose12 NULL: the context's
 * current state); stamp as above; per_point (may be NULL): n records; out (may be
 * NULL): the call's summary. The class of a record and n[] are vg_scan_diff's for
 * the same input. The _dev form takes the cloud as three device arrays. n == 0 is
 * legal and takes its stamp. VG_E_ARG (nothing is written, no stamp is taken):
 * NULL ctx, NULL xyz or device array with n > 0, n < 0 or above
 * max_points_per_scan, stamp < 0. VG_E_RANGE: stamp == 0 after the largest stamp
 * reached INT32_MAX. VG_E_STATE: no layer, or the context is sharded.
 * vg_live_compose: now > 0, or 0 for the layer's largest stamp so far; flags as
 * above; grid (may be NULL: the composed grid stays on the device only): nx ny
 * int8. VG_E_ARG: NULL ctx, now < 0, flags with a bit above 0. VG_E_STATE as above.
 * vg_live_info copies the planes (nx ny int32 each) and the totals: the sums of the
 * marks' summaries since the layer began or was cleared. vg_live_clear zeroes the
 * planes and the totals and restarts the stamps; the base stays. vg_live_end frees
 * the layer; vg_destroy and vg_reset free it too. VG_E_STATE without a layer.
 * Legal where vg_scan_diff is: completes outstanding work first; mapping on or off;
 * on an owner, an attached tracker and a fleet's tracker between fleet steps. The
 * calls read the map only. A fleet shares obstacles by marking every tracker's scan,
 * with that tracker's pose, into one context's layer; the calls into one layer come
 * from one thread at a time. The layer is not part of a checkpoint. */
int vg_live_begin(vg_ctx* ctx, const vg_live_params* prm, const int8_t* base_grid);
int vg_live_mark(vg_ctx* ctx, const float* xyz, int n, const double* pose12, int32_t stamp,
                 vg_live_point* per_point, vg_live_summary* out);
int vg_live_mark_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int n,
                     const double* pose12, int32_t stamp, vg_live_summary* out);
int vg_live_compose(vg_ctx* ctx, int32_t now, int flags, int8_t* grid, vg_live_summary* out);
int vg_live_info(vg_ctx* ctx, int32_t* hit, int32_t* clear, vg_live_summary* totals);
int vg_live_clear(vg_ctx* ctx);
int vg_live_end(vg_ctx* ctx);

/* ---- Place index: global relocalisation in a frozen map ------------------------
 * vg_relocalize needs a rough guess. The place index supplies one from a single
 * scan and the gravity direction: a side structure next to a frozen map (as the
 * change layer: owned by the context that owns the map, never part of a
 * checkpoint) that holds, per sample position ("place"), the polar range image
 * the map shows from there; a scan is binned into the same image, compared with
 * every place under every circular azimuth shift, and the best few (place, yaw)
 * pairs go to vg_relocalize's grid, scoring and refinement.
 *
 * The descriptor: n_az azimuth x n_el elevation bins, one uint16 per bin, range
 * in units of 1 / 512 m clipped to 65535, 0 = none; bin (e, a) is entry
 * e * n_az + a. The frame is (ex, ey, up): up = -g / |g| of the building
 * context's state, ex = world x made perpendicular to up (world y where |up.x|
 * >= 0.9), ey = up x ex. Azimuth bin a covers [a, a + 1) 2 pi / n_az from ex
 * towards ey, elevation bin e covers el_min + [e, e + 1) (el_max - el_min) /
 * n_el; a bin's centre direction is cos(el) (cos(az) ex + sin(az) ey) + sin(el)
 * up at the middle of both spans.
 *   Map side: bin (e, a) of a place is rint(512 range) of the vg_raycast ray from
 *   the place's position along the bin's centre direction over (ray.t_min,
 *   t_max]; a miss is 0.
 *   Scan side: a point x (LiDAR frame) is v = R_level ext_R x, R_level any
 *   rotation with the sensor's roll and pitch (its yaw is the unknown); r = |v|,
 *   q = rint(512 r), its bin from the azimuth atan2(v.ey, v.ex) and the elevation
 *   asin(v.up / r); points outside the elevation span or with r > t_max (or r =
 *   0) are dropped. A bin's value is (sum q + n / 2) / n over its n points in
 *   integer arithmetic, so it does not depend on the points' order.
 *   Match: score(place, s) = sum over the scan's non-empty bins (e, a) of
 *   min(|place[e][(a + s) mod n_az] - scan[e][a]|, clip_q), clip_q = rint(512
 *   clip), an empty place bin charged clip_q; int32. Shift s is the yaw 2 pi s /
 *   n_az about up: the sensor's rotation is Rz_up(yaw) R_level. */
typedef struct vg_places_params {
  int    n_az, n_el;       /* <= 0: 120, 12. At most 256 and 32, and n_az * n_el <= 4096 */
  double el_min, el_max;   /* radians, within [-pi/2, pi/2]; both 0: -+30 degrees */
  double t_max;            /* metres; <= 0: 60. Replaces ray.t_max */
  double clip;             /* metres; <= 0: 2 */
  int    min_bins;         /* a place with fewer hit bins is invalid; <= 0: n_az * n_el / 8 */
  int    pad;
  vg_ray_params ray;       /* t_min, min_cos, max_steps as vg_raycast takes them */
  double reserved[4];
} vg_places_params;
typedef struct vg_place_candidate {   /* 48 bytes, no implicit padding */
  int32_t place, shift;               /* index into the build's positions; azimuth shift in bins */
  int32_t score, n_valid;             /* the match's score; the scan's non-empty bins */
  double  pos[3];                     /* the place's position (a LiDAR origin, world) */
  double  yaw;                        /* 2 pi shift / n_az */
} vg_place_candidate;
/* The bin-centre directions in the descriptor's own frame (x = ex, y = ey, z =
 * up; the world frame where gravity is along -z), without a device: out (may be
 * NULL) cap x 3 doubles, entry e * n_az + a; *count = n_az * n_el. The index
 * casts exactly these (as ex, ey, up combinations). prm NULL: the defaults. A
 * limit exceeded, an empty or out-of-range elevation span, NULL count, cap < 0:
 * VG_E_ARG. */
int vg_places_dirs(const vg_places_params* prm, double* out, int cap, int* count);
/* Build the index over M positions (M x 3 doubles, LiDAR origins in the world)
 * on the context that owns a frozen map; an existing index is replaced. A
 * place's row depends on the place and the map alone (the same bytes at any M
 * and order). VG_E_STATE: mapping is on, the context is sharded, inside a scan,
 * or itself attached. VG_E_ARG: NULL, M <= 0, M * n_az * n_el >= 2^30, a limit
 * exceeded. Completes outstanding work; synchronous.
 * While an index exists the owner refuses what would change the map, as with a
 * change layer: vg_set_mapping(owner, 1), vg_reset, vg_checkpoint_load,
 * vg_checkpoint_save, vg_release_far with the compaction flag and vg_shard_*
 * return VG_E_STATE. vg_destroy ends the index. */
int vg_places_build(vg_ctx* ctx, const double* positions, int M, const vg_places_params* prm);
/* M, the number of valid places (hit_bins >= min_bins), and optionally the
 * descriptors (M * n_el * n_az uint16) and the per-place hit-bin counts. Every
 * pointer may be NULL. */
int vg_places_info(vg_ctx* ctx, int* M, int* n_valid, uint16_t* desc, int32_t* hit_bins);
/* The scan's descriptor alone: desc (n_el * n_az uint16) and n_per_bin (int32),
 * either may be NULL. R_level9: row-major rotation, NULL = the calling context's
 * current R. n == 0 gives an all-zero descriptor. */
int vg_places_scan(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, uint16_t* desc,
                   int32_t* n_per_bin);
/* Scan pass + match pass, then the top_k smallest records over every valid
 * place's two entries — its best shift (equal scores: the lower s) and its best
 * shift at least n_az / 4 bins (circularly) away from that one — ordered by
 * ascending score, then place, then shift. *n_out <= top_k records are written;
 * 0 when n == 0, the scan has no non-empty bin or no place is valid.
 * scores_all (may be NULL): M x n_az int32, INT32_MAX for invalid places.
 * The candidate's pose: R = Rz_up(yaw) R_level, p = pos - R ext_t. */
int vg_places_query(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, int top_k,
                    vg_place_candidate* out, int* n_out, int32_t* scores_all);
/* Frees the index (VG_E_STATE without one, or on an attached tracker). */
int vg_places_end(vg_ctx* ctx);
/* vg_places_query, then vg_relocalize's own grid, scoring and refinement around
 * each candidate's pose (at most 4096 candidates); a record that verifies
 * beats one that does not, among equals vg_relocalize's ranking decides, and
 * the winner is refined again from where it stands (a grid of one hypothesis,
 * at most 4 times) until it rests. prm NULL: half_xy = half the median nearest-neighbour spacing of the
 * places in the ex-ey plane at step 0.25 m, half_yaw = 1.5 azimuth bins at a
 * third of a bin, no z search, vg_relocalize's defaults for the rest. ok,
 * install, out_pose and out_score as vg_relocalize's; out_place (may be NULL):
 * the winning candidate. No candidate or a failed verification: VG_OK, *ok = 0,
 * the context's state untouched.
 * vg_places_info / _scan / _query and vg_relocalize_global may be called on the
 * owner and on any tracker attached to it (the owner's index; calls into one
 * index are serialised inside the library; a call that another thread's
 * vg_places_end overtakes returns VG_E_STATE). VG_E_ARG: NULL ctx, xyz (n > 0),
 * out / n_out / out_pose / ok, n < 0 or above max_points_per_scan, top_k <= 0.
 * Unsharded contexts, between scans. */
int vg_relocalize_global(vg_ctx* ctx, const float* xyz, int n, const double* R_level9, int top_k,
                         const vg_reloc_params* prm, int install, double* out_pose, vg_pose_score* out_score,
                         vg_place_candidate* out_place, int* ok);

/* ---- Map views: many sensors in one frozen map ------------------------------
 * vg_map_attach makes `tracker` a read-only view of `owner`'s map: every kernel
 * of the tracker that reads the map (the IEKF, vg_score_poses, vg_relocalize,
 * vg_map_planes) takes the owner's pointers, so B sensors localising in one
 * map hold it once. A tracker is an ordinary context and may be created with
 * tiny map capacities (e.g. max_nodes 1024, max_fix_points 1024, hash_log2
 * 10): it then costs its scan staging, IEKF work buffers and state, not a map.
 * Its own map stays allocated and comes back on the detach. A context that has
 * stepped scans before may attach: whatever it captured for its own map is
 * dropped on attach and on detach.
 * Attach requires (else VG_E_STATE, or VG_E_ARG where noted; vg_last_error of
 * either context names the failed check): the owner has mapping off; both
 * contexts on the same device (VG_E_ARG); both unsharded; neither inside a
 * scan; their vg_config equal byte for byte (VG_E_ARG); the tracker neither
 * attached already nor itself an owner; the owner not itself attached; the
 * owner's window fits the tracker's max_points_per_scan (VG_E_ARG).
 * Attach completes both contexts' outstanding work and installs the owner's
 * between-scans estimator into the tracker, through memory: afterwards the
 * tracker is what a context that loaded the owner's checkpoint and froze it
 * would be (state, window, last_pcl_end_time, trajectory and path rows,
 * vg_stats' nodes_used and fix_used; stats_log restarts), with mapping off.
 * vg_seed or vg_relocalize(install) then moves it to where its sensor is.
 * While attached, on the tracker: vg_step*, vg_seed, vg_score_poses,
 * vg_relocalize, vg_map_planes, the state / stats / trajectory / path / poll
 * accessors work as on a frozen context, and vg_release_far reports the census
 * only. VG_E_STATE: vg_set_mapping(tracker, 1), vg_checkpoint_save,
 * vg_checkpoint_load, vg_reset, vg_set_publish with either bit, vg_shard_*,
 * vg_profile with the per-stage bit (its P_k pass writes the map's stamps).
 * vg_destroy(tracker) detaches first.
 * While an owner has views these return VG_E_STATE and change nothing:
 * vg_set_mapping(owner, 1), vg_reset, vg_checkpoint_load, vg_checkpoint_save
 * (it compacts, so node ids move), vg_release_far with the compaction flag
 * (without it: the census only), vg_shard_*, vg_destroy. The owner may still
 * step frozen scans itself.
 * vg_map_detach (VG_E_STATE when not attached, inside a scan, or in a fleet)
 * completes the tracker's work and hands its own map back, empty, with the
 * context as after vg_reset and mapping still off: the window it followed
 * belongs to the owner's map. Read its trajectory before detaching. */
int vg_map_attach(vg_ctx* tracker, vg_ctx* owner);
int vg_map_detach(vg_ctx* tracker);

/* Window states x_buf (win_count x 250 doubles); returns win_count via *n. */
int vg_window_states(vg_ctx* ctx, double* out, int* n);

/* ---- Stage-level API ------------------------------------------------------
 * The steps vg_step composes, one entry per reference call of the steady-state
 * loop (local_mapping.cpp:389-547), for a caller that keeps the reference's
 * loop shape. Order per scan:
 *   vg_scan_load | vg_scan_bind_dev        deskewed scan -> HBM
 *   vg_propagate                           IMUEKF::process state/cov part (imu_ekf.cpp:28-94)
 *   vg_downsample_scan                     down_sampling_voxel + /2 fallback (point_utils.hpp:7-44; local_mapping.cpp:396-403)
 *   vg_lio_state_estimation                VINA_SLAM::VNC_lio -> LioStateEstimation (odometry.cpp:64-255)
 *   vg_window_push                         x_buf / pvec_buf / IMU_PRE push (local_mapping.cpp:434-441)
 *   vg_cut_voxel_multi                     pvec_update + cut_voxel_multi (point_utils.cpp:54-65; voxel_map.cpp:47-135)
 *   vg_multi_recut                         VINA_SLAM::multi_recut + tras_opt (local_mapping.cpp:144-201)
 *   if win_count >= win_size:
 *     vg_damping_iter   (if if_BA)         LI_BA_Optimizer::damping_iter (optimizers.cpp:430-517)
 *     vg_multi_margi                       x_curr <- x_buf.back(), multi_margi, slide (local_mapping.cpp:499-546)
 *   vg_step_end                            per-scan counters (vg_get_stats)
 * Every call returns VG_E_STATE when issued out of order. */
int vg_scan_load(vg_ctx* ctx, const float* xyz, const float* intensity, int n);
int vg_scan_bind_dev(vg_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, const float* d_intensity,
                     int n);
int vg_propagate(vg_ctx* ctx, const double* imu, int m, double pcl_beg_time, double pcl_end_time);
int vg_downsample_scan(vg_ctx* ctx, int* n_ds);
int vg_lio_state_estimation(vg_ctx* ctx, int* degenerate);
int vg_window_push(vg_ctx* ctx, const double* imu, int m);
int vg_cut_voxel_multi(vg_ctx* ctx);
int vg_multi_recut(vg_ctx* ctx, int* n_factors);
int vg_damping_iter(vg_ctx* ctx, int* lm_iters);
int vg_multi_margi(vg_ctx* ctx);
int vg_step_end(vg_ctx* ctx);
int vg_win_count(vg_ctx* ctx, int* n);

/* The TUM pose file's rows (FileReaderWriter::save_pose_tum, io.cpp:67-77,
 * called at local_mapping.cpp:430): the pose right after the IEKF of every
 * steady-state scan — none for the initialisation's scans (cold start).
 * n rows of 13 doubles [t, R row-major 9, p 3]. Copies min(n, cap) rows;
 * *n = total rows. out may be NULL to query. Completes outstanding work. */
int vg_trajectory(vg_ctx* ctx, double* out, int cap, int* n);

/* pub_localtraj / pub_localmap's path (pcl_path, publishers.cpp:65-131): one
 * row per pub_localtraj call (every stepped scan, the initialisation's
 * included, node.cpp:325 / local_mapping.cpp:427), n rows of 14 doubles
 * [t, R row-major 9, p 3, jour]. After every window BA pub_localmap re-writes
 * the positions of the window's rows with the refined x_buf[i].p
 * (publishers.cpp:121-129, local_mapping.cpp:505); system_reset clears it
 * (node.cpp:403). Completes outstanding work. */
int vg_path(vg_ctx* ctx, double* out, int cap, int* n);

/* Non-blocking: absorb every enqueued scan whose device results are already
 * published (no stream drain, no wait), then report how many scans are
 * complete and how many rows vg_poll_rows can copy. A node publishes from
 * here instead of draining after every scan. Any out-pointer may be NULL. */
int vg_poll(vg_ctx* ctx, int* n_scans, int* n_traj, int* n_path);
/* The rows absorbed so far (after vg_poll; no wait): TUM rows from row
 * traj_from on (at most traj_cap), and the first path_cap path rows. */
int vg_poll_rows(vg_ctx* ctx, double* traj, int traj_from, int traj_cap, double* path, int path_cap);

/* /map_cmap (pub_localmap, publishers.cpp:102-119,130): every third point of
 * the oldest window frame's downsampled cloud at that frame's pose after the
 * BA, x y z intensity per point, computed on the device after each window BA
 * while enabled (vg_set_publish bit 0; off by default: no cost to the scan).
 * Points follow the device's downsample order (first occurrence, DESIGN.md
 * section 3), so "every third" selects from that order. Completes outstanding
 * work; *n = points of the last window BA (0 if none ran while enabled). */
int vg_local_map(vg_ctx* ctx, float* out_xyzi, int cap, int* n);
/* Optional per-scan outputs: bit 0 = the /map_cmap cloud (vg_local_map),
 * bit 1 = the /voxel_plane + /voxel_normal marker events (vg_markers; the
 * reference's General.enable_visualization, node.cpp:99-100). While bit 1 is
 * set the steady state's one-launch scan graph is declined, as it is for
 * bit 0: the scan runs as the insert + recut graph, the collection kernel,
 * the LM graphs and the margi tail. With both bits clear nothing changes: the
 * same kernels, the same graphs, the same bits.
 * Bit 1 keeps the reference's per-plane publication flags (plane.hpp:18-21)
 * on the device only while it is set. Setting it starts from a blank slate:
 * nothing counts as published and nothing is pending, so a plane that exists
 * already appears at its next plane_update (octree.cpp:441-446); clearing it
 * drops every flag. This differs from the reference only for a caller that
 * enables after the first scan (the reference reads the parameter once, at
 * start-up).
 * In sharded mode (vg_shard_* with world > 1) a rank holds only its own
 * tiles' roots: setting bit 1 returns VG_E_STATE. */
int vg_set_publish(vg_ctx* ctx, int flags);

/* One record of the map's plane / normal markers (OctoTree::
 * collect_plane_markers / collect_normal_markers, octree.cpp:758-949). The two
 * MarkerArrays are always in step, so one record serves both: the CYLINDER of
 * /voxel_plane is (center, quat, plane_scale), the ARROW of /voxel_normal is
 * (center -> tip, normal_scale); both carry id and rgba. Fixed layout, 248
 * bytes, no implicit padding. For a DELETE only id, action, layer,
 * voxel_center and flags are meaningful (the rest is zero). */
typedef struct vg_plane_marker {
  double voxel_center[3]; /* OctoTree::voxel_center */
  double quater_length;   /* OctoTree::quater_length */
  double center[3];       /* plane.center: marker.pose.position / points[0] (octree.cpp:802-804, 901-904) */
  double normal[3];       /* plane.normal.normalized() (octree.cpp:806, 906) */
  double quat[4];         /* x y z w: FromTwoVectors(UnitZ, normal) (octree.cpp:807-811) */
  double plane_scale[3];  /* 3 sqrt(ev2), 3 sqrt(ev1), 2 sqrt(ev0), ev = max(0, eig_value) (octree.cpp:813-818) */
  double tip[3];          /* center + normal * 2 quater_length: points[1] (octree.cpp:907-910) */
  double normal_scale[3]; /* (0.1, 0.2, 0) * 2 quater_length (octree.cpp:915-917) */
  double eig[3];          /* OctoTree::eig_value as stored (not clamped) */
  double trace;           /* plane_var.block<3,3>(0,0).diagonal().sum() (octree.cpp:787-788) */
  float rgba[4];          /* map_jet(pow(min(trace, 0.25) / 0.25, 0.2)) bytes / 255.0f, alpha 0.8 (octree.cpp:789-795, 820-823) */
  int32_t id;             /* voxel_id_from_center(voxel_center, layer) (octree.cpp:11-21) */
  int32_t action;         /* visualization_msgs::Marker: 0 = ADD, 2 = DELETE */
  int32_t layer;
  int32_t flags;          /* bit 0 plane.is_plane, bit 1 octo_state, bit 2 the node's root is in surf_map_slide,
                             bit 3 is_update, bit 4 is_published (bits 3, 4: as the call found them) */
} vg_plane_marker;

/* The marker events of the last scan, collected on the device where the
 * reference collects them (local_mapping.cpp:455-470): after the scan's
 * multi_recut, before the window BA and multi_margi, on every steady-state
 * scan (also while the window is filling; none during the cold-start
 * initialisation) while vg_set_publish bit 1 is set. Per node of the
 * surf_map_slide subtrees the rule of octree.cpp:761-850: a leaf that lost
 * its plane, or a node that became internal, after it was published -> DELETE;
 * a plane leaf updated since its last publication -> ADD. Order unspecified
 * (the reference's is its unordered_map's). Every event is emitted: the
 * reference's used_ids de-duplication of colliding ids is the caller's
 * (vina::NodeCore does it).
 * *n = events that scan emitted; min(*n, cap) records are copied. *deferred =
 * events that did not fit the device buffer (vg_marker_capacity): their nodes'
 * flags were left untouched, so they come out on a later scan. Completes
 * outstanding work first, as vg_local_map does. */
int vg_markers(vg_ctx* ctx, vg_plane_marker* out, int cap, int* n, int* deferred);
/* Size of the device's event buffer, in records. Default 65536 (15.5 MiB of
 * HBM, allocated only while bit 1 is set). Call before enabling: VG_E_STATE
 * while bit 1 is set. */
int vg_marker_capacity(vg_ctx* ctx, int max_records);
/* Snapshot of the map in the same record type (action = 0): the user-facing
 * "give me the planes". Independent of vg_set_publish; changes no flag.
 * flags bit 0: only the subtrees of surf_map_slide's roots (default: the whole
 * map); bit 1: every node with layer <= max_layer (default: plane leaves only;
 * the marker fields of a node whose flags bit 0 is clear come from
 * its last plane record, zero if it never had one). out == NULL queries the
 * count; else min(*n, cap) records are copied, in unspecified order. Completes
 * outstanding work; may be called between scans, and in the stage API between
 * vg_multi_recut and vg_damping_iter / vg_multi_margi (the reference's
 * collection point). */
int vg_map_planes(vg_ctx* ctx, int flags, vg_plane_marker* out, int cap, int* n);

/* ---- Spatial-tile sharding (north_star: the voxel map shards by spatial tile
 * across the GPUs of one node, with an all-reduce of the normal equations).
 * One context per GPU runs the SAME sequence; each keeps only the root voxels
 * of its tiles (16^3 root voxels, owner = hash(tile) mod world) and sums only
 * its own points and factors. Per IEKF iteration the 34-value normal-equation
 * block is all-reduced, per LM iteration the 6W x 6W LiDAR Hessian + gradient
 * and the residual; three integer counts keep the reference's thread_num
 * quirks global. State and IMU factors are replicated, so every rank computes
 * the identical trajectory. Call once, before the first scan.
 *   vg_shard_rccl: RCCL communicator inside the library, collectives ordered on
 *                  the context stream (ncclAllReduce, no host synchronisation);
 *                  id128 from vg_rccl_unique_id on rank 0, broadcast by the caller.
 *   vg_shard_host: host callback fn(buf, count, dtype, user) summing `count`
 *                  elements of host memory in place across ranks (dtype 0 =
 *                  double, 1 = int32); the library stages through pinned memory
 *                  and synchronises the stream around each call (tests, CPU-
 *                  mediated transports). */
int vg_rccl_unique_id(void* id128);
int vg_shard_rccl(vg_ctx* ctx, int rank, int world, const void* id128);
int vg_shard_host(vg_ctx* ctx, int rank, int world, vg_host_allreduce_fn fn, void* user);

/* Stage timing with HIP events on the context stream (device time). stage:
 * 0 downsample, 1 IEKF point-loop kernel (k_iekf), 2 map insert, 3 recut +
 * factor extraction, 4 BA, 5 margi, 6 whole IEKF, 7 the LDL^T solve kernel
 * (k_ba_solve); 8..15 the HOST time of the stage calls (enqueue + waits):
 * propagate, downsample, IEKF, window push, insert, recut, BA, margi. `on`: 0 off, 1 the k_iekf and k_ba_solve launches only
 * (stages 1 and 7; cheap enough for a timed region), 3 every stage; bits 8-15
 * (n > 1) time k_ba_solve on every n-th BA run only; bit 2 (4): in-kernel
 * clocks of k_iekf and k_ba_solve (the device's constant-rate wall clock read
 * inside the kernels: kernel-only time of the executed launches, graph replays
 * included, no events in the stream), read as stages 16 (k_iekf), 17
 * (k_ba_solve), 18 (the recut's level kernels k_rc_level0 + k_rc_level, one
 * span per scan) and 19 (k_ba_hess), over the last <= 64 scans.
 * vg_profile resets the accumulators; vg_profile_read returns total ms and the
 * number of intervals. */
int vg_profile(vg_ctx* ctx, int on);
int vg_profile_read(vg_ctx* ctx, int stage, double* total_ms, int* count);

/* HIP stream the context enqueues on (hipStream_t as void*). */
void* vg_stream(vg_ctx* ctx);

/* How the host waits for device results: spin for spin_us, then poll every
 * sleep_us (sleep_us 0: spin only, the default and the lowest latency). Use
 * sleeping polls when several contexts run from their own threads. */
int vg_set_wait_policy(vg_ctx* ctx, int spin_us, int sleep_us);

/* Multi-sequence mode (BASELINE config 5): B independent sequences on one
 * GPU, each in its own context. vg_multi_create starts one native worker
 * thread per context (and sets their wait policy); vg_multi_step_dev queues
 * one scan per sequence (device-resident SoA, as vg_step_dev, or
 * vg_step_deskew_dev when d_time != NULL; the point buffers must stay valid
 * until vg_multi_sync, the IMU samples are copied) and returns — it blocks
 * only when a sequence has 4 scans queued; the workers run free, in order per
 * sequence. vg_multi_sync completes every queued scan. Each sequence's
 * results are exactly those of a lone context. vg_multi_step_dev queues all B
 * scans or none: after a worker's error it returns that status without
 * queuing (call vg_multi_sync before reading vg_last_error of the contexts).
 * With B > 1 the contexts run on one stream each while the multi object
 * exists; vg_multi_destroy gives each back its own stream, downsample stream
 * and the IEKF / margi overlap. Past four sequences they share four streams
 * (sequence b on stream b % 4, one worker thread per stream stepping its
 * sequences one scan each in turn): MI355X time-slices more than about four
 * busy hardware queues, and four shared streams keep B = 8 / 16 at B = 4's
 * rate. The environment variable VG_MULTI_STREAMS = G overrides
 * the count (G <= 0 or G >= B: one stream and one worker per sequence). */
typedef struct vg_scan_dev {
  const float *d_x, *d_y, *d_z, *d_intensity, *d_time;
  int n;
  double pcl_beg_time, pcl_end_time;
  const double* imu; /* host, m x 7 */
  int m;
} vg_scan_dev;
typedef struct vg_multi vg_multi;
vg_multi* vg_multi_create(vg_ctx** ctxs, int B, int spin_us, int sleep_us);
int vg_multi_step_dev(vg_multi* mv, const vg_scan_dev* scans);
/* At most `cap` sequences with device work in flight at once (0 or >= B: no
 * cap): sequence b runs in slot b % cap, one sequence per slot at a time, and
 * waits for its scan's device work before the slot passes on. Past about four
 * hardware queues per process the GPU time-slices them (every kernel >= ~47
 * us at B = 8, same L2 hit rates as B = 4), idle ones included, so pair the
 * cap with GPU_MAX_HW_QUEUES = cap (the B streams then share cap queues, slot
 * by slot). Between steps only (VG_E_STATE). */
int vg_multi_set_active(vg_multi* mv, int cap);
int vg_multi_sync(vg_multi* mv);
void vg_multi_destroy(vg_multi* mv);

/* The fleet: B trackers attached to one owner's map (vg_map_attach) stepped
 * together, one frozen scan each per step, in ten kernel launches on one
 * stream for any B (the opening, four IEKF point loops over a (blocks, B)
 * grid, four updates, the publication). Each tracker's results are a lone
 * frozen context's, bit for bit, whatever the batch.
 * vg_fleet_create: B >= 1; every tracker attached to `owner`, none inside a
 * scan or in another fleet, all with the same max_points_per_scan (one IEKF
 * grid, and with it one reduction tree, serves all); else VG_E_STATE / VG_E_ARG.
 * Completes the trackers' outstanding work. While the fleet exists its
 * trackers are stepped only through it: vg_step*, vg_propagate, vg_map_detach
 * and vg_destroy on them return VG_E_STATE; their accessors work as usual.
 * vg_fleet_step_dev: B records; n < 0: tracker b sits this step out (nothing of
 * it moves). d_time != NULL: the scan is deskewed first. Returns once the work
 * is enqueued; the scans' arrays must stay valid until the step's results are
 * read. n == 0 is an empty scan (its planes may be NULL): the tracker
 * propagates and its IEKF runs on no points. Queues every participating scan
 * or none: a bad record (VG_E_ARG, VG_E_CAPACITY) or a tracker's deferred error
 * is returned before anything is propagated or enqueued, and the fleet stays
 * usable. A failure past those checks (a HIP error, or a tracker's propagation
 * or deskew failing, e.g. more IMU segments than the deskew holds) cannot be
 * undone: nothing of the step is launched, but the trackers ahead of the
 * failing one have propagated (their opened scans are abandoned), so the fleet
 * is out of step; every later vg_fleet_step_dev and vg_fleet_sync returns that error,
 * and the way on is vg_fleet_destroy, then vg_map_detach + vg_map_attach of
 * each tracker (the detach resets it). A fleet step runs no downsample, nothing downstream of it existing
 * in a frozen map: for fleet-stepped scans vg_stats::n_ds is 0 and
 * vg_scan_points returns 0 points (vg_downsample gives the cloud). vg_profile's
 * in-kernel clocks and launch events do not cover fleet steps.
 * vg_fleet_sync completes every tracker's enqueued scans and returns the first
 * error. vg_fleet_destroy hands the trackers back, still attached. */
typedef struct vg_fleet vg_fleet;
int vg_fleet_create(vg_ctx* owner, vg_ctx** trackers, int B, vg_fleet** out);
int vg_fleet_step_dev(vg_fleet* f, const vg_scan_dev* scans);
int vg_fleet_sync(vg_fleet* f);
void vg_fleet_destroy(vg_fleet* f);

#ifdef __cplusplus
}
#endif
#endif /* VINA_GPU_H */
