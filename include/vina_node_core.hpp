// vina_node_core.hpp — the ROS-free core of the reference's ROS 2 node
// (SURVEY §8 row f4), header-only on the C-ABI (vina_gpu.h):
//   imu_handler / the point-cloud handlers (src/platform/ros2/node.cpp:153-170)
//     -> NodeCore::imu / NodeCore::scan (pcl_handler's decode runs at arrival,
//        lidar_decoder.cpp:7-43, on the device through vg_decode_scan);
//   sync_packages (src/sensor/sync.cpp:18-96) + the odometry thread's per-scan
//     step (local_mapping.cpp:389-547, deskew included) -> NodeCore::spin;
//   ResultOutput::pub_localtraj (publishers.cpp:65-97): the pose after the IEKF
//     (the TF camera_init -> aft_mapped, pub_odom_func 42-63), the path point
//     and the scan moved to the world (/map_scan) -> path() / scan_world();
//   ResultOutput::pub_localmap (publishers.cpp:99-131, local_mapping.cpp:505):
//     the path's window rows re-written with the BA-refined positions (in
//     path()) and the /map_cmap cloud -> local_map();
//   the /voxel_plane + /voxel_normal MarkerArrays of every steady-state scan
//     (General.enable_visualization, node.cpp:99-100; local_mapping.cpp:455-470,
//     OctoTree::collect_plane_markers / collect_normal_markers) ->
//     enable_visualization() / voxel_plane() / voxel_normal();
//   FileReaderWriter::save_pose_tum (io.cpp:67-77) -> tum_rows() / tum_line /
//     write_tum (steady-state scans only, as the reference's file).
// Outputs are refreshed without draining the device pipeline (vg_poll): a
// scan's rows appear once its results are published; scan_world(),
// local_map() and write_tum() complete outstanding work first.
// A ROS 2 wrapper (vina-slam_amd/ros2/vina_node.cpp, built when rclcpp is
// found) only converts messages to these calls and these outputs to messages.
#pragma once
#include <cmath>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <unordered_set>
#include <vector>
#include "vina_gpu.hpp"

namespace vina_gpu {

struct PoseStamped {
  double t;
  double R[9];  // row-major
  double p[3];
  double q[4];  // x, y, z, w
  double jour = 0;  // path points only: the journey (the PointType's curvature, publishers.cpp:88-92)
};

// Eigen::Quaterniond(const Matrix3d&): the trace branch, else the largest
// diagonal entry's branch
inline void quat_from_R(const double* R, double q[4]) {
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}

// one row of the TUM pose file: "t x y z qx qy qz qw", std::fixed, 9 decimals
inline std::string tum_line(const PoseStamped& s) {
  char b[320];
  snprintf(b, sizeof(b), "%.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", s.t, s.p[0], s.p[1], s.p[2], s.q[0], s.q[1],
           s.q[2], s.q[3]);
  return b;
}

// The node's localisation parameters (General.localization_mode,
// General.map_path): with the defaults the node maps as before
struct NodeParams {
  int localization_mode = 0;  // 1: load map_path and run with the map frozen (vg_set_mapping 0)
  std::string map_path;
};

// The 2-D navigation map of the node (nav_msgs/OccupancyGrid's content; vina_gpu.h "Occupancy grid")
struct OccupancyGridParams {
  double res = 0.1;      // cell edge, metres; the path's sensor origins are thinned to one per res
  double margin = 20.0;  // the grid reaches this far past the origins' bounds; the rays' t_max where occ.ray.t_max is 0
  int n_az = 360;        // the fan: n_az azimuths about the world's z at each elevation
  std::vector<double> elevations_deg = {-10.0, 0.0, 10.0};
  vg_occ_params occ = {};  // band (z_lo < z_hi not set: -0.3 .. 1.0), thresholds, flags, ray; the grid's fields are filled in
};
struct OccupancyGrid {
  double x0 = 0, y0 = 0, res = 0;
  int nx = 0, ny = 0;
  std::vector<int8_t> data;  // VG_OCC_*, row-major, cell (ix, iy) at iy nx + ix
  vg_occ_summary summary = {};
  std::vector<double> origins, dirs;  // what was cast: M x 3, D x 3
  vg_occ_params params = {};          // ... with these parameters
};
// map_server's pair: prefix.pgm (P5, the first row at the largest y; occupied 0, free 254, unknown 205) and prefix.yaml
inline bool write_occupancy_map(const std::string& prefix, const OccupancyGrid& g) {
  FILE* f = fopen((prefix + ".pgm").c_str(), "wb");
  if (!f) return false;
  fprintf(f, "P5\n%d %d\n255\n", g.nx, g.ny);
  std::vector<unsigned char> row((size_t)g.nx);
  for (int iy = g.ny - 1; iy >= 0; iy--) {
    for (int ix = 0; ix < g.nx; ix++) {
      const int8_t c = g.data[(size_t)iy * g.nx + ix];
      row[ix] = c == VG_OCC_OCCUPIED ? 0 : (c == VG_OCC_FREE ? 254 : 205);
    }
    if (fwrite(row.data(), 1, row.size(), f) != row.size()) {
      fclose(f);
      return false;
    }
  }
  if (fclose(f) != 0) return false;
  const size_t slash = prefix.find_last_of('/');
  f = fopen((prefix + ".yaml").c_str(), "w");
  if (!f) return false;
  fprintf(f, "image: %s.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n",
          prefix.substr(slash == std::string::npos ? 0 : slash + 1).c_str(), g.res, g.x0, g.y0);
  return fclose(f) == 0;
}
// The terrain layer of the node (vina_gpu.h "Terrain layer"): ground elevation, steps and the grid judged
// relative to the ground
struct TerrainGridParams {
  double res = 0.1;      // as OccupancyGridParams
  double margin = 20.0;  // as OccupancyGridParams
  int n_az = 360;
  std::vector<double> elevations_deg = {-30.0, -20.0, -10.0, 0.0, 10.0};  // a fan that reaches the floor
  vg_terrain_params ter = {};  // sensor_height, bands, thresholds, flags, ray; the grid's fields are filled in
};
struct TerrainGrid {
  double x0 = 0, y0 = 0, res = 0;
  int nx = 0, ny = 0;
  std::vector<int8_t> data;        // VG_OCC_*, row-major, cell (ix, iy) at iy nx + ix
  std::vector<int32_t> elev, step; // heights in units of z_res; elev VG_TER_NONE where there is none
  vg_terrain_summary summary = {};
  std::vector<double> origins, dirs;  // what was cast: M x 3, D x 3
  vg_terrain_params params = {};      // ... with these parameters
  double z_res() const { return params.z_res > 0.0 ? params.z_res : 0.001; }
  OccupancyGrid grid() const {        // the grid with its geometry, as occupancy_grid() would return it
    OccupancyGrid g;
    g.x0 = x0, g.y0 = y0, g.res = res, g.nx = nx, g.ny = ny;
    g.data = data;
    return g;
  }
};
// write_occupancy_map's pair for the grid, and the elevation beside it: prefix.elev (nx ny little-endian int32, row
// iy = 0 first) and prefix.elev.yaml (data, nx, ny, resolution, origin, z_res, none)
inline bool write_terrain_map(const std::string& prefix, const TerrainGrid& g) {
  if (!write_occupancy_map(prefix, g.grid())) return false;
  FILE* f = fopen((prefix + ".elev").c_str(), "wb");
  if (!f) return false;
  for (const int32_t e : g.elev) {
    const uint32_t u = (uint32_t)e;
    const unsigned char b[4] = {(unsigned char)u, (unsigned char)(u >> 8), (unsigned char)(u >> 16), (unsigned char)(u >> 24)};
    if (fwrite(b, 1, 4, f) != 4) {
      fclose(f);
      return false;
    }
  }
  if (fclose(f) != 0) return false;
  const size_t slash = prefix.find_last_of('/');
  f = fopen((prefix + ".elev.yaml").c_str(), "w");
  if (!f) return false;
  fprintf(f, "data: %s.elev\nnx: %d\nny: %d\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nz_res: %.17g\nnone: %d\n",
          prefix.substr(slash == std::string::npos ? 0 : slash + 1).c_str(), g.nx, g.ny, g.res, g.x0, g.y0, g.z_res(),
          (int)VG_TER_NONE);
  return fclose(f) == 0;
}
// The costmap of an OccupancyGrid (nav2's inflation layer; vina_gpu.h "Clearance field and costmap"), with the
// grid's geometry
struct Costmap {
  double x0 = 0, y0 = 0, res = 0;
  int nx = 0, ny = 0;
  std::vector<uint8_t> cost;   // VG_COST_*, row-major, cell (ix, iy) at iy nx + ix
  std::vector<int32_t> dist2;  // cells squared to the nearest obstacle; VG_CLR_NONE without any
  vg_clr_summary summary = {};
  vg_clr_params params = {};
};
// the cost's raw bytes as prefix.pgm (P5, the first row at the largest y, as write_occupancy_map flips it) and
// write_occupancy_map's prefix.yaml
inline bool write_costmap(const std::string& prefix, const Costmap& c) {
  FILE* f = fopen((prefix + ".pgm").c_str(), "wb");
  if (!f) return false;
  fprintf(f, "P5\n%d %d\n255\n", c.nx, c.ny);
  for (int iy = c.ny - 1; iy >= 0; iy--)
    if (fwrite(c.cost.data() + (size_t)iy * c.nx, 1, (size_t)c.nx, f) != (size_t)c.nx) {
      fclose(f);
      return false;
    }
  if (fclose(f) != 0) return false;
  const size_t slash = prefix.find_last_of('/');
  f = fopen((prefix + ".yaml").c_str(), "w");
  if (!f) return false;
  fprintf(f, "image: %s.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n",
          prefix.substr(slash == std::string::npos ? 0 : slash + 1).c_str(), c.res, c.x0, c.y0);
  return fclose(f) == 0;
}
// A planned path (NodeCore::plan): the world polyline through the centres of the path's cells, the start first
struct Plan {
  int status = VG_NAV_NO_PATH;   // VG_NAV_*
  int64_t cost = -1;             // the start's cost-to-go; -1 with VG_NAV_NO_PATH
  std::vector<int32_t> cells;    // linear indices iy nx + ix
  std::vector<double> xy;        // x, y per cell, metres
  std::vector<uint32_t> pot;     // the cost-to-go per cell of the path (plan() with want_pot; else empty)
  vg_nav_summary summary = {};
};

// Where to go next while the map is still growing (NodeCore::explore_goal)
struct ExploreGoal {
  bool found = false;            // a frontier the robot can reach exists
  vg_frontier_rec frontier = {}; // the chosen one: the first in LioCore::Frontiers::order()
  double goal_xy[2] = {0, 0};    // its best_cell's centre, metres
  Plan path;                     // from the goal's cell down to the robot's: reverse it to drive (the field is symmetric)
  LioCore::Frontiers frontiers;  // every kept frontier and the summary (labels only where asked for)
};

// The same, chosen by view gain (NodeCore::explore_goal_gain)
struct ExploreGoalGain {
  bool found = false;            // a reachable frontier from whose best_cell at least min_gain unknown cells show
  vg_frontier_rec frontier = {}; // the chosen one: frontiers.recs[order[0]]
  vg_view_rec view = {};         // what its best_cell sees: gain.recs[order[0]]
  double goal_xy[2] = {0, 0};    // that cell's centre, metres
  Plan path;                     // from the goal's cell down to the robot's, as ExploreGoal::path
  LioCore::Frontiers frontiers;  // every kept frontier
  LioCore::ViewGain gain;        // record k: the view from frontiers.recs[k].best_cell
  std::vector<int> order;        // LioCore::ViewGain::order() over the frontiers' best_pot
};

class NodeCore {
 public:
  // cfg.cold_start = 1 for a run from a bag (the node's initialization,
  // node.cpp:293-366); point_notime as the node's `point_notime` parameter
  NodeCore(const vg_config& cfg, const vg_capacity* cap, const vg_lidar_format& fmt, int point_notime = 0,
           int device = 0)
      : cfg_(cfg), fmt_(fmt), lio_(cfg, cap, device) {
    sync_ = vg_sync_create(point_notime);
    if (!sync_) throw Error(VG_E_ARG, "vg_sync_create");
  }
  ~NodeCore() { vg_sync_destroy(sync_); }
  NodeCore(const NodeCore&) = delete;
  NodeCore& operator=(const NodeCore&) = delete;

  // imu_handler: one sample (stamp, angular velocity, linear acceleration)
  void imu(double t, const double gyr[3], const double acc[3]) {
    const double s[7] = {t, gyr[0], gyr[1], gyr[2], acc[0], acc[1], acc[2]};
    check(vg_sync_push_imu(sync_, s), "vg_sync_push_imu");
  }

  // a point-cloud message: the sensor records and the header stamp; decoded
  // now, as pcl_handler does in the callback. fmt: this message's layout
  // (a PointCloud2's field offsets), else the constructor's
  void scan(double header_time, const void* records, int n, const vg_lidar_format* fmt = nullptr) {
    Scan& sc = scans_[next_id_];
    sc.xyz.resize((size_t)3 * (n + 2));
    sc.inten.resize(n + 2);
    sc.time.resize(n + 2);
    int m = 0;
    check(vg_decode_scan(lio_.raw(), records, n, fmt ? fmt : &fmt_, sc.xyz.data(), sc.inten.data(), sc.time.data(),
                         &m),
          "vg_decode_scan");
    sc.xyz.resize((size_t)3 * m);
    sc.inten.resize(m);
    sc.time.resize(m);
    const double last = m > 0 ? (double)sc.time[m - 1] : 0.0;
    check(vg_sync_push_scan(sync_, header_time, last, next_id_), "vg_sync_push_scan");
    next_id_++;
  }

  // sync_packages until it needs more data; one estimator step per package.
  // Returns the number of scans stepped.
  int spin() {
    int stepped = 0;
    std::vector<double> imu(7 * kImuCap);
    for (;;) {
      int id = -1, m = 0, ready = 0;
      double beg = 0, end = 0;
      check(vg_sync_pop(sync_, &id, &beg, &end, imu.data(), kImuCap, &m, &ready), "vg_sync_pop");
      if (ready == 0) {  // sync_packages came back empty: the idle branch (local_mapping.cpp:303-356)
        long long rel[6];
        check(vg_release_far(lio_.raw(), 0, rel), "vg_release_far");  // returns at once unless jour advanced
        break;
      }
      auto it = scans_.find(id);
      if (ready < 0) {  // too few IMU samples: the reference drops the scan
        if (it != scans_.end()) scans_.erase(it);
        continue;
      }
      if (it == scans_.end()) throw Error(VG_E_STATE, "sync_packages returned an unknown scan");
      packages_++;
      if (skip_ > 0) {  // resumed from a checkpoint: this package was consumed before the save
        skip_--;
        scans_.erase(it);
        continue;
      }
      Scan& sc = it->second;
      if (reloc_armed_) {  // the first scan after load_map: its pose in the map, from the guess or the place index
        double pose[12];
        if (reloc_global_)
          reloc_ok_ = lio_.relocalize_global(sc.xyz.data(), (int)sc.inten.size(), reloc_level_set_ ? reloc_guess_ : nullptr,
                                             reloc_top_k_, reloc_prm_set_ ? &reloc_prm_ : nullptr, true, pose, nullptr,
                                             &reloc_place_);
        else
          reloc_ok_ = lio_.relocalize(sc.xyz.data(), (int)sc.inten.size(), reloc_guess_, reloc_prm_, true, pose, nullptr);
        reloc_armed_ = false;
        reloc_done_ = true;
      }
      check(vg_step_deskew(lio_.raw(), sc.xyz.data(), sc.inten.data(), sc.time.data(), (int)sc.inten.size(), beg,
                           end, imu.data(), m),
            "vg_step_deskew");
      scans_.erase(it);
      stepped++;
      if (visualization_) take_markers();
      if (after_step_) after_step_();
      if (package_limit_ >= 0 && packages_ >= package_limit_) break;  // (the caller saves here, then spins on)
    }
    poll();
    return stepped;
  }

  // Non-blocking refresh of the outputs from every scan whose results the
  // device has published (vg_poll); returns true when something changed.
  bool poll() {
    int ns = 0, nt = 0, np = 0;
    check(vg_poll(lio_.raw(), &ns, &nt, &np), "vg_poll");
    return take_rows(ns, nt, np);
  }
  // Blocking: complete every enqueued scan, then refresh (end of a run).
  void finish() {
    int nt = 0;
    check(vg_trajectory(lio_.raw(), nullptr, 0, &nt), "vg_trajectory");  // completes outstanding work
    poll();
  }

  // Checkpoint and resume (vg_checkpoint_save / vg_checkpoint_load). Saving
  // completes the scans in flight first. Loading replaces the context's state
  // and then re-reads path() and tum_rows() from it — the TUM output continues
  // the saved rows — and empties the marker arrays (the per-scan used_ids rule
  // needs nothing older). The synchroniser's queues are not part of a
  // checkpoint: a caller replaying a log feeds it from the start and has the
  // first `skip_packages` packages dropped unstepped (vg_node_replay --resume).
  long long save_checkpoint(const std::string& file) {
    finish();
    return lio_.save_checkpoint(file);
  }
  void load_checkpoint(const std::string& file) {
    lio_.load_checkpoint(file);
    tum_.clear();
    path_.clear();
    clear_markers();
    scans_done_ = -1;  // (take_rows: read everything again)
    finish();
  }
  // Localisation in a saved map: load_map installs the checkpoint and turns
  // mapping off; relocalize(guess, ...) arms a relocalisation (vg_relocalize,
  // install = 1) on the first scan stepped after it, whose result
  // relocalized() / relocalize_ok() report. apply(params) does the first for
  // General.localization_mode = 1.
  void load_map(const std::string& file) {
    load_checkpoint(file);
    lio_.set_mapping(false);
  }
  void apply(const NodeParams& p) {
    if (p.localization_mode == 1) load_map(p.map_path);
  }
  void relocalize(const double guess_pose[12], const vg_reloc_params& prm) {
    for (int k = 0; k < 12; k++) reloc_guess_[k] = guess_pose[k];
    reloc_prm_ = prm;
    reloc_global_ = false;
    reloc_armed_ = true;
    reloc_done_ = false;
  }
  // The same without a position: the first scan stepped after it is relocalised through the place
  // index of the map (vg_relocalize_global, install = 1; lio().places_build first). R_level9: a
  // rotation with the sensor's roll and pitch, null: the state's R at that scan; prm null: the
  // default window around each candidate. relocalize_place() is the winning candidate.
  void relocalize_global(const double* R_level9 = nullptr, int top_k = 16, const vg_reloc_params* prm = nullptr) {
    reloc_level_set_ = R_level9 != nullptr;
    for (int k = 0; k < 9 && R_level9; k++) reloc_guess_[k] = R_level9[k];
    reloc_prm_set_ = prm != nullptr;
    if (prm) reloc_prm_ = *prm;
    reloc_top_k_ = top_k;
    reloc_global_ = true;
    reloc_armed_ = true;
    reloc_done_ = false;
  }
  const vg_place_candidate& relocalize_place() const { return reloc_place_; }
  bool relocalized() const { return reloc_done_; }
  bool relocalize_ok() const { return reloc_ok_; }
  // called after every stepped scan, before the next is taken: the caller reads what belongs to
  // that scan alone (vg_scan_points and the state for vg_scan_diff / vg_change_accumulate, which
  // complete the scan first)
  void set_after_step(std::function<void()> fn) { after_step_ = std::move(fn); }
  void skip_packages(int n) { skip_ = n; }
  void set_package_limit(int n) { package_limit_ = n; }  // spin() returns once this many packages were taken (-1: no limit)
  int packages() const { return packages_; }             // packages sync_packages has delivered, skipped ones included

  // save_pose_tum's rows: the pose after the IEKF of every steady-state scan
  const std::vector<PoseStamped>& tum_rows() const { return tum_; }
  // pcl_path (pub_localtraj's points, the initialisation's scans included,
  // cleared by system_reset, the window's positions re-written by
  // pub_localmap after each BA); R is the pose's rotation after its IEKF
  const std::vector<PoseStamped>& path() const { return path_; }

  // /map_cmap (pub_localmap): switch the device-side cloud on (from the next
  // window BA on) and read the last one: x y z intensity per point
  void enable_local_map(bool on) {
    publish_ = (publish_ & ~1) | (on ? 1 : 0);
    check(vg_set_publish(lio_.raw(), publish_), "vg_set_publish");
  }
  // General.enable_visualization (node.cpp:99-100): call before the first
  // scan, as the reference reads the parameter at start-up. While on, spin()
  // reads every stepped scan's marker events (which completes that scan) into
  // voxel_plane() / voxel_normal(): the two MarkerArrays the reference
  // publishes after the scan's multi_recut (local_mapping.cpp:455-470), each
  // holding the events of the scans stepped since clear_markers(). Within one
  // scan's array the first record of an id wins and later records with that id
  // are dropped — the reference's used_ids; a hash collision hides the second
  // leaf there too, which one follows its map order there and the device's
  // emission order here. One record serves both topics (vg_plane_marker), and
  // the two collectors see the same flags and ids, so the two arrays are one.
  void enable_visualization(bool on) {
    publish_ = (publish_ & ~2) | (on ? 2 : 0);
    check(vg_set_publish(lio_.raw(), publish_), "vg_set_publish");
    visualization_ = on;
  }
  const std::vector<vg_plane_marker>& voxel_plane() const { return markers_; }
  const std::vector<vg_plane_marker>& voxel_normal() const { return markers_; }
  // per steady-state scan stepped since clear_markers(): its record count
  const std::vector<int>& marker_scan_counts() const { return marker_counts_; }
  void clear_markers() {
    markers_.clear();
    marker_counts_.clear();
  }
  std::vector<float> local_map() {
    int n = 0;
    check(vg_local_map(lio_.raw(), nullptr, 0, &n), "vg_local_map");
    std::vector<float> out((size_t)4 * n);
    if (n > 0) check(vg_local_map(lio_.raw(), out.data(), n, &n), "vg_local_map");
    return out;
  }

  // the last scan's downsampled points in the world (pwld of pvec_update,
  // local_mapping.cpp:425-427): R (ext_R q + ext_t) + p at the scan's pose
  std::vector<float> scan_world() {
    finish();
    int n = 0;
    check(vg_scan_points(lio_.raw(), nullptr, 0, &n), "vg_scan_points");
    std::vector<float> body((size_t)3 * n), out;
    if (n == 0 || path_.empty()) return out;
    check(vg_scan_points(lio_.raw(), body.data(), n, &n), "vg_scan_points");
    // the pose pvec_update used: right after the IEKF (the TUM row; a path
    // row's position may since have been re-written by pub_localmap)
    const PoseStamped& s = (!tum_.empty() && tum_.back().t == path_.back().t) ? tum_.back() : path_.back();
    const double* E = cfg_.ext_R;
    out.resize((size_t)3 * n);
    for (int i = 0; i < n; i++) {
      const double x = body[3 * i], y = body[3 * i + 1], z = body[3 * i + 2];
      double b[3];
      for (int r = 0; r < 3; r++) b[r] = E[3 * r] * x + E[3 * r + 1] * y + E[3 * r + 2] * z + cfg_.ext_t[r];
      for (int r = 0; r < 3; r++)
        out[3 * i + r] = (float)(s.R[3 * r] * b[0] + s.R[3 * r + 1] * b[1] + s.R[3 * r + 2] * b[2] + s.p[r]);
    }
    return out;
  }

  // The occupancy grid cast from the node's own path (vg_occupancy): the sensor origins p + R ext_t of
  // path()'s rows — a loaded map's rows included, the only places from which free space is known —
  // thinned so that every kept origin is at least res from the one kept before it, on the grid that
  // covers their x, y bounds grown by margin (x0, y0 whole multiples of res). Completes outstanding work.
  OccupancyGrid occupancy_grid(const OccupancyGridParams& P = OccupancyGridParams()) {
    finish();
    OccupancyGrid g;
    vg_occ_params q = P.occ;
    if (!(q.z_lo < q.z_hi)) q.z_lo = -0.3, q.z_hi = 1.0;
    if (!(q.ray.t_max > 0.0) && P.margin > 0.0) q.ray.t_max = P.margin;
    cast_plan("occupancy_grid", P.res, P.margin, P.n_az, P.elevations_deg, g.origins, g.dirs, g.x0, g.y0, g.nx, g.ny);
    q.x0 = g.x0, q.y0 = g.y0, q.res = g.res = P.res, q.nx = g.nx, q.ny = g.ny;
    LioCore::Occupancy r = lio_.occupancy(g.origins.data(), (int)(g.origins.size() / 3), g.dirs.data(),
                                          (int)(g.dirs.size() / 3), q);
    g.data = std::move(r.grid);
    g.summary = r.summary;
    g.params = q;
    return g;
  }

  // The terrain layer cast from the node's own path (vg_terrain): occupancy_grid()'s origins, fan construction and
  // grid, with a fan that looks down. sensor_height is P.ter's: the sensor's height over the ground it drives on is
  // a property of the vehicle, not guessed from the first hits. g.grid() is an OccupancyGrid with the same geometry,
  // and the grid lies on the device where occupancy_grid() leaves its own: costmap(g.grid(), ..., true) prices it.
  // Completes outstanding work.
  TerrainGrid terrain_grid(const TerrainGridParams& P = TerrainGridParams()) {
    finish();
    TerrainGrid g;
    vg_terrain_params q = P.ter;
    if (!(q.ray.t_max > 0.0) && P.margin > 0.0) q.ray.t_max = P.margin;
    cast_plan("terrain_grid", P.res, P.margin, P.n_az, P.elevations_deg, g.origins, g.dirs, g.x0, g.y0, g.nx, g.ny);
    q.x0 = g.x0, q.y0 = g.y0, q.res = g.res = P.res, q.nx = g.nx, q.ny = g.ny;
    LioCore::Terrain r = lio_.terrain(g.origins.data(), (int)(g.origins.size() / 3), g.dirs.data(),
                                      (int)(g.dirs.size() / 3), q);
    g.data = std::move(r.grid);
    g.elev = std::move(r.elev);
    g.step = std::move(r.step);
    g.summary = r.summary;
    g.params = q;
    return g;
  }

  // The costmap of g (vg_clearance): cost and dist2 with g's geometry. inscribed, inflation: metres; scaling:
  // 1/m; flags bit 0: unknown cells are obstacles too. on_device: g is what occupancy_grid() returned last, or
  // terrain_grid()'s grid() (both leave their grid in the same device slot), and neither vg_occupancy nor vg_terrain
  // ran on the context since, so the grid is read where that call left it and nothing is uploaded.
  // Completes outstanding work.
  Costmap costmap(const OccupancyGrid& g, double inscribed, double inflation, double scaling, int flags = 0,
                  bool on_device = false) {
    finish();
    Costmap c;
    vg_clr_params q = {};
    q.nx = c.nx = g.nx, q.ny = c.ny = g.ny, q.res = c.res = g.res;
    c.x0 = g.x0, c.y0 = g.y0;
    q.flags = flags;
    q.inscribed_radius = inscribed, q.inflation_radius = inflation, q.cost_scaling = scaling;
    if (!on_device && g.data.size() != (size_t)g.nx * (size_t)g.ny) throw Error(VG_E_ARG, "costmap: the grid's data is not nx ny cells");
    LioCore::Clearance r = lio_.clearance(on_device ? nullptr : g.data.data(), q, true, false, true);
    c.cost = std::move(r.cost);
    c.dist2 = std::move(r.dist2);
    c.summary = r.summary;
    c.params = q;
    cm_x0_ = c.x0, cm_y0_ = c.y0, cm_res_ = c.res, cm_nx_ = c.nx, cm_ny_ = c.ny;
    return c;
  }

  // The live obstacle layer over g (vg_live_begin; vina_gpu.h "Live obstacle layer"): prm's band, ranges, persist,
  // flags and diff parameters, its geometry taken from g. on_device as costmap()'s: g is the grid that lies on the
  // device, which the layer copies there. Completes outstanding work.
  void live_begin(const OccupancyGrid& g, vg_live_params prm = vg_live_params(), bool on_device = false) {
    finish();
    prm.x0 = g.x0, prm.y0 = g.y0, prm.res = g.res, prm.nx = g.nx, prm.ny = g.ny;
    if (!on_device && g.data.size() != (size_t)g.nx * (size_t)g.ny) throw Error(VG_E_ARG, "live_begin: the grid's data is not nx ny cells");
    lio_.live_begin(prm, on_device ? nullptr : g.data.data());
    live_g_ = OccupancyGrid();
    live_g_.x0 = g.x0, live_g_.y0 = g.y0, live_g_.res = g.res, live_g_.nx = g.nx, live_g_.ny = g.ny;
  }
  void live_end() {
    finish();
    lio_.live_end();
    live_g_ = OccupancyGrid();
  }
  // What the planner gets of a scan: the scan (n points, LiDAR frame; pose12 null: the current state) marked into
  // the layer (vg_live_mark, stamp 0: the next), the layer composed at that stamp (vg_live_compose) and the composed
  // grid priced where it lies on the device (costmap(..., on_device)). plan() and frontiers() then read that costmap.
  struct LiveCostmap {
    OccupancyGrid grid;  // the composed grid, with the layer's geometry
    Costmap costmap;
    vg_live_summary mark = {}, compose = {};
  };
  LiveCostmap live_costmap(const float* xyz, int n, const double* pose12, double inscribed, double inflation,
                           double scaling, int32_t stamp = 0, int compose_flags = 0, int cost_flags = 0) {
    finish();
    if (!live_g_.nx) throw Error(VG_E_STATE, "live_costmap: no live_begin() on this node yet");
    LiveCostmap r;
    r.grid = live_g_;
    r.grid.data.resize((size_t)live_g_.nx * (size_t)live_g_.ny);
    r.mark = lio_.live_mark(xyz, n, pose12, stamp);
    r.compose = lio_.live_compose((int32_t)r.mark.stamp, compose_flags, r.grid.data.data());
    r.costmap = costmap(r.grid, inscribed, inflation, scaling, cost_flags, true);
    return r;
  }

  // The path from start_xy to goal_xy (world metres) over the last costmap() of this node, whose cost plane is read
  // where vg_clearance left it on the device (no vg_clearance may have run on the context since): vg_navfn towards
  // the goal's cell with prm's traversal table (null: nav2's defaults), then vg_nav_paths from the start's cell,
  // at most max_len cells. want_pot: the field is downloaded to fill Plan::pot. Further starts towards the same
  // goal: lio().nav_paths(). Completes outstanding work.
  Plan plan(const double goal_xy[2], const double start_xy[2], const vg_nav_params* prm = nullptr, int max_len = 65536,
            bool want_pot = false) {
    finish();
    if (!cm_nx_) throw Error(VG_E_STATE, "plan: no costmap() on this node yet");
    vg_nav_params q = {};
    if (prm) q = *prm;
    q.nx = cm_nx_, q.ny = cm_ny_;
    // the cell holding a world point; -1 (outside every grid) where the point is off the grid, far off or not a
    // number, so that no double beyond int32 is ever converted
    const auto index = [](double v, int n) { return v >= 0.0 && v < (double)n ? (int32_t)v : (int32_t)-1; };
    const auto cell = [&](const double* xy) {
      return std::vector<int32_t>{index(std::floor((xy[0] - cm_x0_) / cm_res_), cm_nx_),
                                  index(std::floor((xy[1] - cm_y0_) / cm_res_), cm_ny_)};
    };
    Plan p;
    const LioCore::NavField f = lio_.navfn(nullptr, q, cell(goal_xy), want_pot);
    p.summary = f.summary;
    const LioCore::NavPaths r = lio_.nav_paths(cell(start_xy), max_len);
    p.status = r.status[0], p.cost = r.cost[0];
    p.cells.assign(r.cells.begin(), r.cells.begin() + r.len[0]);
    for (const int32_t c : p.cells) {
      p.xy.push_back(cm_x0_ + (c % cm_nx_ + 0.5) * cm_res_);
      p.xy.push_back(cm_y0_ + (c / cm_nx_ + 0.5) * cm_res_);
      if (want_pot) p.pot.push_back(f.pot[(size_t)c]);
    }
    return p;
  }

  // The frontiers of the last occupancy_grid() over the last costmap() of this node, both read where they lie on
  // the device (no vg_occupancy or vg_clearance may have run on the context since): free cells beside unknown ones
  // whose cost is below cost_max (0: 253). use_pot: only cells that the field of the last plan() or navfn reaches,
  // and the records carry the cheapest cell of each. Completes outstanding work.
  LioCore::Frontiers frontiers(bool use_pot, int min_size = 0, int max_records = 4096, bool want_labels = false,
                               int cost_max = 0) {
    finish();
    if (!cm_nx_) throw Error(VG_E_STATE, "frontiers: no costmap() on this node yet");
    vg_frontier_params q = {};
    q.nx = cm_nx_, q.ny = cm_ny_, q.flags = 1 | (use_pot ? 2 : 0), q.cost_max = cost_max, q.min_size = min_size;
    return lio_.frontiers(nullptr, nullptr, q, max_records, want_labels);
  }
  // the centre of cell c of the last costmap(), metres
  void cell_xy(int32_t c, double xy[2]) const {
    xy[0] = cm_x0_ + (c % cm_nx_ + 0.5) * cm_res_, xy[1] = cm_y0_ + (c / cm_nx_ + 0.5) * cm_res_;
  }

  // The next goal of an exploring robot standing at robot_xy, without a plane leaving the device in between:
  // occupancy_grid(P) -> costmap() of it where it lies -> vg_navfn with the robot's own cell as the goal (w is
  // symmetric: the field is the cost from the robot to every cell) -> vg_frontiers with the cost and the reach
  // test -> the first frontier in order(), the cheapest to drive to, and its best_cell as a world point ->
  // vg_nav_paths from that cell, which descends to the robot: reverse ExploreGoal::path to drive. found is false
  // where no frontier of at least min_size cells can be reached.
  ExploreGoal explore_goal(const double robot_xy[2], const OccupancyGridParams& P, double inscribed, double inflation,
                           double scaling, int min_size = 0, const vg_nav_params* prm = nullptr, int max_len = 65536) {
    const OccupancyGrid g = occupancy_grid(P);
    costmap(g, inscribed, inflation, scaling, 0, true);
    vg_nav_params q = {};
    if (prm) q = *prm;
    q.nx = cm_nx_, q.ny = cm_ny_;
    const double fx = std::floor((robot_xy[0] - cm_x0_) / cm_res_), fy = std::floor((robot_xy[1] - cm_y0_) / cm_res_);
    const std::vector<int32_t> robot = {fx >= 0.0 && fx < (double)cm_nx_ ? (int32_t)fx : (int32_t)-1,
                                        fy >= 0.0 && fy < (double)cm_ny_ ? (int32_t)fy : (int32_t)-1};
    ExploreGoal e;
    e.path.summary = lio_.navfn(nullptr, q, robot, false).summary;
    e.frontiers = frontiers(true, min_size);
    if (e.frontiers.recs.empty()) return e;
    e.found = true;
    e.frontier = e.frontiers.recs[(size_t)e.frontiers.order()[0]];
    cell_xy(e.frontier.best_cell, e.goal_xy);
    const LioCore::NavPaths r = lio_.nav_paths({e.frontier.best_cell % cm_nx_, e.frontier.best_cell / cm_nx_}, max_len);
    e.path.status = r.status[0], e.path.cost = r.cost[0];
    e.path.cells.assign(r.cells.begin(), r.cells.begin() + r.len[0]);
    for (const int32_t c : e.path.cells) {
      double xy[2];
      cell_xy(c, xy);
      e.path.xy.push_back(xy[0]), e.path.xy.push_back(xy[1]);
    }
    return e;
  }

  // The view gain (vg_view_gain) at every frontier's best_cell, on the grid of the last occupancy_grid() where it
  // lies on the device (no vg_occupancy may have run on the context since): what a 2-D sensor of range radius_m
  // (rounded to whole cells of the last costmap(), 1 .. VG_VIEW_MAX_RADIUS) would see from where the robot would
  // stop. fs: frontiers(true, ...)'s, so that every record has its best_cell; record k belongs to fs.recs[k].
  // Completes outstanding work.
  LioCore::ViewGain frontier_gain(const LioCore::Frontiers& fs, double radius_m, int max_unknown = 0,
                                  bool want_seen = false) {
    finish();
    if (!cm_nx_) throw Error(VG_E_STATE, "frontier_gain: no costmap() on this node yet");
    vg_view_params q = {};
    const double cells = std::floor(radius_m / cm_res_ + 0.5);
    q.nx = cm_nx_, q.ny = cm_ny_, q.max_unknown = max_unknown;
    q.radius = !(cells >= 1.0) ? 1 : cells > (double)VG_VIEW_MAX_RADIUS ? VG_VIEW_MAX_RADIUS : (int)cells;
    std::vector<int32_t> views;
    for (const vg_frontier_rec& r : fs.recs) {
      if (r.best_cell < 0) throw Error(VG_E_ARG, "frontier_gain: a frontier without best_cell (frontiers(true) gives it)");
      views.push_back(r.best_cell % cm_nx_), views.push_back(r.best_cell / cm_nx_);
    }
    return lio_.view_gain(nullptr, q, views, want_seen);
  }
  // the frontier records' best_pot, as ViewGain::order() takes them
  static std::vector<uint32_t> frontier_pots(const LioCore::Frontiers& fs) {
    std::vector<uint32_t> p;
    for (const vg_frontier_rec& r : fs.recs) p.push_back(r.best_pot);
    return p;
  }

  // explore_goal() with the goal chosen by what the robot would learn there: its chain up to the frontiers, then
  // frontier_gain() at every kept frontier's best_cell, and the goal is the first in ViewGain::order(best_pot,
  // min_gain): the most unknown cells in view per cost to drive there. found is false where no reachable frontier
  // shows at least min_gain unknown cells. The path comes from vg_nav_paths as in explore_goal().
  ExploreGoalGain explore_goal_gain(const double robot_xy[2], const OccupancyGridParams& P, double inscribed,
                                    double inflation, double scaling, double radius_m, int min_gain = 1,
                                    int max_unknown = 0, int min_size = 0, const vg_nav_params* prm = nullptr,
                                    int max_len = 65536) {
    const OccupancyGrid g = occupancy_grid(P);
    costmap(g, inscribed, inflation, scaling, 0, true);
    vg_nav_params q = {};
    if (prm) q = *prm;
    q.nx = cm_nx_, q.ny = cm_ny_;
    const double fx = std::floor((robot_xy[0] - cm_x0_) / cm_res_), fy = std::floor((robot_xy[1] - cm_y0_) / cm_res_);
    const std::vector<int32_t> robot = {fx >= 0.0 && fx < (double)cm_nx_ ? (int32_t)fx : (int32_t)-1,
                                        fy >= 0.0 && fy < (double)cm_ny_ ? (int32_t)fy : (int32_t)-1};
    ExploreGoalGain e;
    e.path.summary = lio_.navfn(nullptr, q, robot, false).summary;
    e.frontiers = frontiers(true, min_size);
    if (e.frontiers.recs.empty()) return e;
    e.gain = frontier_gain(e.frontiers, radius_m, max_unknown);
    e.order = e.gain.order(frontier_pots(e.frontiers), min_gain);
    if (e.order.empty()) return e;
    e.found = true;
    e.frontier = e.frontiers.recs[(size_t)e.order[0]];
    e.view = e.gain.recs[(size_t)e.order[0]];
    cell_xy(e.frontier.best_cell, e.goal_xy);
    const LioCore::NavPaths r = lio_.nav_paths({e.frontier.best_cell % cm_nx_, e.frontier.best_cell / cm_nx_}, max_len);
    e.path.status = r.status[0], e.path.cost = r.cost[0];
    e.path.cells.assign(r.cells.begin(), r.cells.begin() + r.len[0]);
    for (const int32_t c : e.path.cells) {
      double xy[2];
      cell_xy(c, xy);
      e.path.xy.push_back(xy[0]), e.path.xy.push_back(xy[1]);
    }
    return e;
  }

  bool write_tum(const std::string& file) {
    finish();
    FILE* f = fopen(file.c_str(), "w");
    if (!f) return false;
    for (const PoseStamped& s : tum_) fputs(tum_line(s).c_str(), f);
    return fclose(f) == 0;
  }

  int init_phase() {
    vg_stats st;
    check(vg_get_stats(lio_.raw(), &st), "vg_get_stats");
    return st.init_phase;
  }
  LioCore& lio() { return lio_; }

 private:
  // What occupancy_grid() and terrain_grid() cast: the sensor origins of path()'s rows thinned to one per res, the
  // fan of n_az azimuths at each elevation, and the grid over the origins' bounds grown by margin
  void cast_plan(const char* who, double res, double margin, int n_az, const std::vector<double>& elevations_deg,
                 std::vector<double>& origins, std::vector<double>& dirs, double& x0, double& y0, int& gnx, int& gny) {
    if (!(res > 0.0) || !(margin >= 0.0) || n_az < 1 || elevations_deg.empty())
      throw Error(VG_E_ARG, std::string(who) + ": res, margin, n_az or the elevations");
    double lo[2] = {0, 0}, hi[2] = {0, 0};
    for (const PoseStamped& s : path_) {
      double o[3];
      for (int j = 0; j < 3; j++)
        o[j] = s.p[j] + s.R[3 * j] * cfg_.ext_t[0] + s.R[3 * j + 1] * cfg_.ext_t[1] + s.R[3 * j + 2] * cfg_.ext_t[2];
      const size_t m = origins.size();
      if (m && std::hypot(std::hypot(o[0] - origins[m - 3], o[1] - origins[m - 2]), o[2] - origins[m - 1]) < res)
        continue;
      for (int j = 0; j < 2; j++) {
        lo[j] = m && lo[j] < o[j] ? lo[j] : o[j];
        hi[j] = m && hi[j] > o[j] ? hi[j] : o[j];
      }
      origins.insert(origins.end(), o, o + 3);
    }
    if (origins.empty()) throw Error(VG_E_STATE, std::string(who) + ": the path is empty");
    for (const double e : elevations_deg)
      for (int a = 0; a < n_az; a++) {
        const double az = 2.0 * M_PI * a / n_az, el = e * M_PI / 180.0;
        const double d[3] = {std::cos(el) * std::cos(az), std::cos(el) * std::sin(az), std::sin(el)};
        dirs.insert(dirs.end(), d, d + 3);
      }
    const double kx = std::floor((lo[0] - margin) / res), ky = std::floor((lo[1] - margin) / res);
    const double nx = std::ceil((hi[0] + margin) / res) - kx, ny = std::ceil((hi[1] + margin) / res) - ky;
    if (!(nx * ny <= (double)VG_OCC_MAX_CELLS)) throw Error(VG_E_ARG, std::string(who) + ": more than 2^24 cells");
    x0 = kx * res, y0 = ky * res;
    gnx = nx < 1.0 ? 1 : (int)nx, gny = ny < 1.0 ? 1 : (int)ny;
  }

  static constexpr int kImuCap = 4096;
  struct Scan {
    std::vector<float> xyz, inten, time;
  };
  void check(int r, const char* what) {
    if (r != VG_OK) throw Error(r, std::string(what) + ": " + vg_last_error(lio_.raw()));
  }
  // one steady-state scan's events -> the arrays, under the used_ids rule. The
  // initialisation's scans publish nothing (the reference collects in the
  // steady-state branch only), so they add no array, not even an empty one.
  void take_markers() {
    vg_stats st;
    check(vg_get_stats(lio_.raw(), &st), "vg_get_stats");  // completes the scan
    if (st.init_phase != 0) return;
    if (marker_buf_.empty()) marker_buf_.resize(4096);
    int n = 0, deferred = 0;
    check(vg_markers(lio_.raw(), marker_buf_.data(), (int)marker_buf_.size(), &n, &deferred), "vg_markers");
    if (n > (int)marker_buf_.size()) {  // grown once to the scan's size, then one call per scan
      marker_buf_.resize((size_t)n);
      check(vg_markers(lio_.raw(), marker_buf_.data(), n, &n, &deferred), "vg_markers");
    }
    std::unordered_set<int> used_ids;
    int kept = 0;
    for (int i = 0; i < n; i++)
      if (used_ids.insert(marker_buf_[i].id).second) {
        markers_.push_back(marker_buf_[i]);
        kept++;
      }
    marker_counts_.push_back(kept);
  }
  static PoseStamped row_pose(const double* r) {
    PoseStamped s;
    s.t = r[0];
    for (int k = 0; k < 9; k++) s.R[k] = r[1 + k];
    for (int k = 0; k < 3; k++) s.p[k] = r[10 + k];
    quat_from_R(s.R, s.q);
    return s;
  }
  // TUM rows only grow; the path is re-read whenever more scans completed
  // (its window rows change after every BA, and a system_reset clears it)
  bool take_rows(int ns, int nt, int np) {
    if (ns == scans_done_ && nt == (int)tum_.size()) return false;
    scans_done_ = ns;
    const int nt_new = nt - (int)tum_.size();
    std::vector<double> t((size_t)13 * (nt_new > 0 ? nt_new : 0)), pth((size_t)14 * np);
    check(vg_poll_rows(lio_.raw(), t.data(), (int)tum_.size(), nt_new > 0 ? nt_new : 0, pth.data(), np),
          "vg_poll_rows");
    for (int i = 0; i < nt_new; i++) tum_.push_back(row_pose(&t[(size_t)13 * i]));
    path_.resize(np);
    for (int i = 0; i < np; i++) {
      path_[i] = row_pose(&pth[(size_t)14 * i]);
      path_[i].jour = pth[(size_t)14 * i + 13];
    }
    return true;
  }

  vg_config cfg_;
  vg_lidar_format fmt_;
  LioCore lio_;
  vg_sync* sync_ = nullptr;
  std::map<int, Scan> scans_;
  int next_id_ = 0;
  int scans_done_ = 0;
  int packages_ = 0, skip_ = 0, package_limit_ = -1;
  std::vector<PoseStamped> tum_, path_;
  bool reloc_armed_ = false, reloc_done_ = false, reloc_ok_ = false;
  double reloc_guess_[12] = {};
  vg_reloc_params reloc_prm_ = {};
  bool reloc_global_ = false, reloc_level_set_ = false, reloc_prm_set_ = false;
  int reloc_top_k_ = 16;
  vg_place_candidate reloc_place_ = {};
  int publish_ = 0;  // vg_set_publish flags
  double cm_x0_ = 0, cm_y0_ = 0, cm_res_ = 0;  // the last costmap()'s geometry (plan())
  int cm_nx_ = 0, cm_ny_ = 0;
  OccupancyGrid live_g_;  // the live layer's geometry (live_begin(); nx 0: none)
  bool visualization_ = false;
  std::function<void()> after_step_;
  std::vector<vg_plane_marker> markers_, marker_buf_;
  std::vector<int> marker_counts_;
};

}  // namespace vina_gpu
