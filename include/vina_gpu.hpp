// vina_gpu.hpp — header-only C++ face of the C-ABI (vina_gpu.h) for a caller
// shaped like the reference's VINA_SLAM (include/vina_slam/platform/ros2/node.hpp:27-96).
// Method names follow the reference calls they replace so that
// thd_odometry_localmapping (local_mapping.cpp:387-547) keeps its structure;
// see INTEGRATION.md for the line-by-line mapping. Errors become exceptions
// (the reference calls exit(), octree.cpp:407, optimizers.cpp:70).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>
#include "vina_gpu.h"

namespace vina_gpu {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

class LioCore {
 public:
  LioCore(const vg_config& cfg, const vg_capacity* cap = nullptr, int device = 0) {
    check(vg_create(&cfg, cap, device, &ctx_), "vg_create");
  }
  ~LioCore() { vg_destroy(ctx_); }
  LioCore(const LioCore&) = delete;
  LioCore& operator=(const LioCore&) = delete;

  // initialisation output (x_curr after Initialization::motion_init)
  void seed(const double* state250) { check(vg_seed(ctx_, state250), "vg_seed"); }
  // VINA_SLAM::system_reset (node.cpp:368-408)
  void system_reset() { check(vg_reset(ctx_), "vg_reset"); }

  // one scan (the whole steady-state branch, local_mapping.cpp:389-547)
  void process(const std::vector<float>& xyz, const std::vector<float>& intensity, double beg, double end,
               const std::vector<double>& imu7) {
    check(vg_step(ctx_, xyz.data(), intensity.empty() ? nullptr : intensity.data(), (int)(xyz.size() / 3), beg, end,
                  imu7.data(), (int)(imu7.size() / 7)),
          "vg_step");
  }
  // one raw sweep: IMUEKF::motion_blur's deskew (imu_ekf.cpp:114-144, row f1)
  // on the device, then the steady-state branch; time[i] = the point's offset
  // from beg in seconds (the reference's `curvature` field), ascending
  void process_raw(const std::vector<float>& xyz, const std::vector<float>& intensity, const std::vector<float>& time,
                   double beg, double end, const std::vector<double>& imu7) {
    check(vg_step_deskew(ctx_, xyz.data(), intensity.empty() ? nullptr : intensity.data(), time.data(),
                         (int)(xyz.size() / 3), beg, end, imu7.data(), (int)(imu7.size() / 7)),
          "vg_step_deskew");
  }

  // ---- the same, call by call (reference names) ----
  void load_scan(const float* xyz, const float* intensity, int n) { check(vg_scan_load(ctx_, xyz, intensity, n), "vg_scan_load"); }
  // odom_ekf.process(x_curr, *pcl_curr, imus)          local_mapping.cpp:389
  void odom_ekf_process(const double* imu7, int m, double beg, double end) {
    check(vg_propagate(ctx_, imu7, m, beg, end), "vg_propagate");
  }
  // down_sampling_voxel(pl_down, down_size) (+ /2)    local_mapping.cpp:396-403
  int down_sampling_voxel() {
    int n = 0;
    check(vg_downsample_scan(ctx_, &n), "vg_downsample_scan");
    return n;
  }
  // VNC_lio(no_ds_pptr)                                local_mapping.cpp:413
  bool VNC_lio() {
    int degenerate = 0;
    check(vg_lio_state_estimation(ctx_, &degenerate), "vg_lio_state_estimation");
    return degenerate == 0;
  }
  // x_buf.push_back / imu_pre_buf push_imu             local_mapping.cpp:434-441
  void push_window(const double* imu7, int m) { check(vg_window_push(ctx_, imu7, m), "vg_window_push"); }
  // cut_voxel_multi(surf_map, pvec_buf[..], ...)       local_mapping.cpp:448
  void cut_voxel_multi() { check(vg_cut_voxel_multi(ctx_), "vg_cut_voxel_multi"); }
  // multi_recut(surf_map_slide, win_count, x_buf, voxhess, ...)  local_mapping.cpp:451
  int multi_recut() {
    int nf = 0;
    check(vg_multi_recut(ctx_, &nf), "vg_multi_recut");
    return nf;
  }
  // LI_BA_Optimizer::damping_iter(x_buf, voxhess, imu_pre_buf, &hess)  local_mapping.cpp:496
  int damping_iter() {
    int it = 0;
    check(vg_damping_iter(ctx_, &it), "vg_damping_iter");
    return it;
  }
  // x_curr <- x_buf.back(); multi_margi(...); slide   local_mapping.cpp:499-546
  void multi_margi() { check(vg_multi_margi(ctx_), "vg_multi_margi"); }
  void end_scan() { check(vg_step_end(ctx_), "vg_step_end"); }
  int win_count() {
    int n = 0;
    check(vg_win_count(ctx_, &n), "vg_win_count");
    return n;
  }

  std::vector<double> x_curr() {
    std::vector<double> s(VG_STATE_LEN);
    check(vg_get_state(ctx_, s.data()), "vg_get_state");
    return s;
  }
  vg_stats stats() {
    vg_stats st;
    check(vg_get_stats(ctx_, &st), "vg_get_stats");
    return st;
  }
  // General.enable_visualization's collection (local_mapping.cpp:455-470): vg_set_publish
  // bit 1, then per scan the /voxel_plane + /voxel_normal events; map_planes: a snapshot
  void set_publish(int flags) { check(vg_set_publish(ctx_, flags), "vg_set_publish"); }
  // checkpoint and resume (vg_checkpoint_save / vg_checkpoint_load): returns the file's bytes
  long long save_checkpoint(const std::string& file) {
    long long bytes = 0;
    check(vg_checkpoint_save(ctx_, file.c_str(), &bytes), "vg_checkpoint_save");
    return bytes;
  }
  void load_checkpoint(const std::string& file) { check(vg_checkpoint_load(ctx_, file.c_str()), "vg_checkpoint_load"); }
  // localising in a saved map: the frozen-map switch, pose scoring, relocalisation (vina_gpu.h)
  void set_mapping(bool on) { check(vg_set_mapping(ctx_, on ? 1 : 0), "vg_set_mapping"); }
  std::vector<vg_pose_score> score_poses(const float* xyz, int n, const double* poses, int K,
                                         const double* pose_var = nullptr, vg_point_match* per_point = nullptr) {
    std::vector<vg_pose_score> out((size_t)(K > 0 ? K : 0));
    check(vg_score_poses(ctx_, xyz, n, poses, K, pose_var, out.data(), per_point), "vg_score_poses");
    return out;
  }
  // returns ok; out_pose: 12 doubles [R, p]; score may be null
  bool relocalize(const float* xyz, int n, const double* guess_pose, const vg_reloc_params& prm, bool install,
                  double* out_pose, vg_pose_score* score) {
    int ok = 0;
    check(vg_relocalize(ctx_, xyz, n, guess_pose, &prm, install ? 1 : 0, out_pose, score, &ok), "vg_relocalize");
    return ok != 0;
  }
  // ray-casting the map (vina_gpu.h): n rays -> n records; n_origins 1 (shared) or n; prm may be null
  std::vector<vg_ray_hit> raycast(const double* origins, int n_origins, const double* dirs, int n,
                                  const vg_ray_params* prm = nullptr) {
    std::vector<vg_ray_hit> out((size_t)(n > 0 ? n : 0));
    check(vg_raycast(ctx_, origins, n_origins, dirs, n, prm, out.data()), "vg_raycast");
    return out;
  }
  // a scan against the map's expected ranges; pose12 null: the current state; per_point may be null
  vg_diff_summary scan_diff(const float* xyz, int n, const double* pose12 = nullptr,
                            const vg_diff_params* prm = nullptr, vg_diff_point* per_point = nullptr) {
    vg_diff_summary out;
    check(vg_scan_diff(ctx_, xyz, n, pose12, prm, per_point, &out), "vg_scan_diff");
    return out;
  }
  // localisability (vina_gpu.h "Localisability"): one record per place over the shared D directions
  std::vector<vg_info_rec> localizability(const double* positions, int M, const double* dirs, int D,
                                          const vg_info_params* prm = nullptr) {
    std::vector<vg_info_rec> out((size_t)(M > 0 ? M : 0));
    check(vg_localizability(ctx_, positions, M, dirs, D, prm, out.data()), "vg_localizability");
    return out;
  }
  // a measured scan's record at pose12 (null: the current state); diff / prm null: the defaults
  vg_info_rec scan_info(const float* xyz, int n, const double* pose12 = nullptr, const vg_diff_params* diff = nullptr,
                        const vg_info_params* prm = nullptr) {
    vg_info_rec out;
    check(vg_scan_info(ctx_, xyz, n, pose12, diff, prm, &out), "vg_scan_info");
    return out;
  }
  // the occupancy grid (vina_gpu.h "Occupancy grid"): M origins x D shared directions rasterised on the
  // device; grid: nx ny cells of VG_OCC_*, row-major; counts (with_counts): n_free's plane, then n_occ's
  struct Occupancy {
    std::vector<int8_t> grid;
    std::vector<int32_t> counts;
    vg_occ_summary summary;
  };
  Occupancy occupancy(const double* positions, int M, const double* dirs, int D, const vg_occ_params& prm,
                      bool with_counts = false) {
    Occupancy r;
    const size_t cells = prm.nx > 0 && prm.ny > 0 ? (size_t)prm.nx * (size_t)prm.ny : 1;
    r.grid.resize(cells <= (size_t)VG_OCC_MAX_CELLS ? cells : 1);
    if (with_counts) r.counts.resize(2 * r.grid.size());
    check(vg_occupancy(ctx_, positions, M, dirs, D, &prm, r.grid.data(), with_counts ? r.counts.data() : nullptr,
                       &r.summary),
          "vg_occupancy");
    return r;
  }
  // the terrain layer (vina_gpu.h "Terrain layer"): the same rays cast twice, for the ground's elevation and then
  // for a grid judged relative to it; grid as occupancy()'s, left on the device in the same slot; elev (VG_TER_NONE:
  // none) and step: nx ny heights in units of z_res; counts (with_counts): n_free's plane, then n_occ's
  struct Terrain {
    std::vector<int8_t> grid;
    std::vector<int32_t> elev, step, counts;
    vg_terrain_summary summary;
  };
  Terrain terrain(const double* positions, int M, const double* dirs, int D, const vg_terrain_params& prm,
                  bool with_counts = false) {
    Terrain r;
    const size_t cells = prm.nx > 0 && prm.ny > 0 ? (size_t)prm.nx * (size_t)prm.ny : 1;
    r.grid.resize(cells <= (size_t)VG_OCC_MAX_CELLS ? cells : 1);
    r.elev.resize(r.grid.size());
    r.step.resize(r.grid.size());
    if (with_counts) r.counts.resize(2 * r.grid.size());
    check(vg_terrain(ctx_, positions, M, dirs, D, &prm, r.grid.data(), r.elev.data(), r.step.data(),
                     with_counts ? r.counts.data() : nullptr, &r.summary),
          "vg_terrain");
    return r;
  }
  // the clearance field and costmap (vina_gpu.h "Clearance field and costmap") of grid (nx ny cells of
  // VG_OCC_*; null: the grid the last occupancy() call left on the device); each output is filled only
  // where asked for
  struct Clearance {
    std::vector<int32_t> dist2, nearest;
    std::vector<uint8_t> cost;
    vg_clr_summary summary;
  };
  Clearance clearance(const int8_t* grid, const vg_clr_params& prm, bool want_dist2 = true, bool want_nearest = true,
                      bool want_cost = true) {
    Clearance r;
    size_t cells = prm.nx > 0 && prm.ny > 0 ? (size_t)prm.nx * (size_t)prm.ny : 1;
    if (cells > (size_t)VG_OCC_MAX_CELLS) cells = 1;
    if (want_dist2) r.dist2.resize(cells);
    if (want_nearest) r.nearest.resize(cells);
    if (want_cost) r.cost.resize(cells);
    check(vg_clearance(ctx_, grid, &prm, want_dist2 ? r.dist2.data() : nullptr, want_nearest ? r.nearest.data() : nullptr,
                       want_cost ? r.cost.data() : nullptr, &r.summary),
          "vg_clearance");
    return r;
  }
  // the navigation function (vina_gpu.h "Navigation function") over cost (nx ny cells of VG_COST_*; null: the plane
  // the last clearance() call left on the device) towards goals (ix, iy pairs); trav null: prm's default table
  struct NavField {
    std::vector<uint32_t> pot;  // filled only where asked for
    vg_nav_summary summary;
  };
  NavField navfn(const uint8_t* cost, const vg_nav_params& prm, const std::vector<int32_t>& goals, bool want_pot = true,
                 const uint16_t* trav = nullptr) {
    NavField r;
    size_t cells = prm.nx > 0 && prm.ny > 0 ? (size_t)prm.nx * (size_t)prm.ny : 1;
    if (cells > (size_t)VG_OCC_MAX_CELLS) cells = 1;
    if (want_pot) r.pot.resize(cells);
    check(vg_navfn(ctx_, cost, &prm, trav, goals.data(), (int)(goals.size() / 2), want_pot ? r.pot.data() : nullptr,
                   &r.summary),
          "vg_navfn");
    return r;
  }
  // the paths from starts (ix, iy pairs) down the field of the last navfn() call: max_len cells a row
  struct NavPaths {
    int max_len = 0;
    std::vector<int32_t> cells, len, status;  // cells: row s at s max_len, -1 past len[s]
    std::vector<int64_t> cost;                // pot[start]; -1 with VG_NAV_NO_PATH
  };
  NavPaths nav_paths(const std::vector<int32_t>& starts, int max_len) {
    NavPaths r;
    const size_t n = starts.size() / 2;
    const bool legal = n >= 1 && n <= (size_t)VG_NAV_MAX_POINTS && max_len >= 1 && n * (size_t)max_len <= (size_t)VG_NAV_MAX_PATH_CELLS;
    r.max_len = max_len;
    r.cells.resize(legal ? n * (size_t)max_len : 1);
    r.len.resize(n ? n : 1), r.status.resize(n ? n : 1), r.cost.resize(n ? n : 1);
    check(vg_nav_paths(ctx_, starts.data(), (int)n, max_len, r.cells.data(), r.len.data(), r.status.data(), r.cost.data()),
          "vg_nav_paths");
    return r;
  }
  // the exploration frontiers (vina_gpu.h "Exploration frontiers") of grid (nx ny cells of VG_OCC_*; null: the grid
  // the last occupancy() call left on the device); cost (flags bit 0) null: the plane the last clearance() call left
  // there; flags bit 1 reads the field of the last navfn() call. recs: the kept components in ascending label, at
  // most max_records
  struct Frontiers {
    std::vector<int32_t> labels;  // filled only where asked for
    std::vector<vg_frontier_rec> recs;
    vg_frontier_summary summary;
    // the indices of recs in the order to visit them: with best_cell >= 0 by ascending (best_pot, label), the
    // cheapest to drive to first; otherwise by descending size, then ascending label
    std::vector<int> order() const {
      std::vector<int> o(recs.size());
      for (size_t k = 0; k < o.size(); k++) o[k] = (int)k;
      bool best = !recs.empty();
      for (const vg_frontier_rec& r : recs) best = best && r.best_cell >= 0;
      std::sort(o.begin(), o.end(), [&](int a, int b) {
        const vg_frontier_rec &p = recs[a], &q = recs[b];
        if (best && p.best_pot != q.best_pot) return p.best_pot < q.best_pot;
        if (!best && p.size != q.size) return p.size > q.size;
        return p.label < q.label;
      });
      return o;
    }
  };
  Frontiers frontiers(const int8_t* grid, const uint8_t* cost, const vg_frontier_params& prm, int max_records = 4096,
                      bool want_labels = true) {
    Frontiers r;
    size_t cells = prm.nx > 0 && prm.ny > 0 ? (size_t)prm.nx * (size_t)prm.ny : 1;
    if (cells > (size_t)VG_OCC_MAX_CELLS) cells = 1;
    if (want_labels) r.labels.resize(cells);
    r.recs.resize(max_records > 0 && max_records <= VG_FRONTIER_MAX_RECORDS ? (size_t)max_records : 0);
    check(vg_frontiers(ctx_, grid, cost, &prm, want_labels ? r.labels.data() : nullptr,
                       r.recs.empty() ? nullptr : r.recs.data(), max_records, &r.summary),
          "vg_frontiers");
    r.recs.resize((size_t)r.summary.n_written);
    return r;
  }
  // the view gain (vina_gpu.h "View gain") from the cells views (ix, iy pairs) of grid (nx ny cells of VG_OCC_*;
  // null: the grid the last occupancy() call left on the device): one record per viewpoint in the order given
  struct ViewGain {
    std::vector<vg_view_rec> recs;
    std::vector<int32_t> seen;  // filled only where asked for
    vg_view_summary summary;
    // the indices of the recs worth visiting, best first: those with VG_VIEW_OK and n_unknown >= min_gain. With
    // pots (one per record, e.g. the frontier records' best_pot) a comes before b when n_unknown_a (pot_b + 1) >
    // n_unknown_b (pot_a + 1), exact in 64 bits (the products stay below 2^50); ties go to the smaller pot, then
    // the smaller index. Without pots (empty): by descending n_unknown, then index
    std::vector<int> order(const std::vector<uint32_t>& pots = {}, int min_gain = 1) const {
      std::vector<int> o;
      for (size_t k = 0; k < recs.size(); k++)
        if (recs[k].status == VG_VIEW_OK && recs[k].n_unknown >= min_gain) o.push_back((int)k);
      const bool use = pots.size() == recs.size() && !pots.empty();
      std::sort(o.begin(), o.end(), [&](int a, int b) {
        const int64_t ga = recs[a].n_unknown, gb = recs[b].n_unknown;
        if (!use) return ga != gb ? ga > gb : a < b;
        const int64_t lhs = ga * ((int64_t)pots[b] + 1), rhs = gb * ((int64_t)pots[a] + 1);
        if (lhs != rhs) return lhs > rhs;
        return pots[a] != pots[b] ? pots[a] < pots[b] : a < b;
      });
      return o;
    }
  };
  ViewGain view_gain(const int8_t* grid, const vg_view_params& prm, const std::vector<int32_t>& views,
                     bool want_seen = false) {
    ViewGain r;
    size_t cells = prm.nx > 0 && prm.ny > 0 ? (size_t)prm.nx * (size_t)prm.ny : 1;
    if (cells > (size_t)VG_OCC_MAX_CELLS) cells = 1;
    if (want_seen) r.seen.resize(cells);
    const size_t n = views.size() / 2;
    r.recs.resize(n ? n : 1);
    check(vg_view_gain(ctx_, grid, &prm, views.data(), (int)n, r.recs.data(), want_seen ? r.seen.data() : nullptr,
                       &r.summary),
          "vg_view_gain");
    r.recs.resize(n);
    return r;
  }
  // the change layer (vina_gpu.h "Change layer"): begin / end on the map's owner; accumulate on the
  // owner or any tracker attached to it; prm / q null: the defaults
  void change_begin(const vg_change_params* prm = nullptr) { check(vg_change_begin(ctx_, prm), "vg_change_begin"); }
  vg_diff_summary change_accumulate(const float* xyz, int n, const double* pose12 = nullptr,
                                    vg_diff_point* per_point = nullptr) {
    vg_diff_summary out;
    check(vg_change_accumulate(ctx_, xyz, n, pose12, per_point, &out), "vg_change_accumulate");
    return out;
  }
  vg_diff_summary change_accumulate_dev(const float* d_x, const float* d_y, const float* d_z, int n,
                                        const double* pose12 = nullptr) {
    vg_diff_summary out;
    check(vg_change_accumulate_dev(ctx_, d_x, d_y, d_z, n, pose12, &out), "vg_change_accumulate_dev");
    return out;
  }
  struct ChangeReport {
    std::vector<vg_change_leaf> leaves;  // ascending node id
    std::vector<vg_change_cell> cells;   // ascending packed key
    vg_change_totals totals;
  };
  ChangeReport change_report(const vg_change_query* q = nullptr) {
    ChangeReport r;
    int nl = 0, nc = 0;
    check(vg_change_report(ctx_, q, nullptr, 0, &nl, nullptr, 0, &nc, nullptr), "vg_change_report");
    r.leaves.resize((size_t)nl);
    r.cells.resize((size_t)nc);
    check(vg_change_report(ctx_, q, r.leaves.data(), nl, &nl, r.cells.data(), nc, &nc, &r.totals), "vg_change_report");
    r.leaves.resize((size_t)nl < r.leaves.size() ? (size_t)nl : r.leaves.size());
    r.cells.resize((size_t)nc < r.cells.size() ? (size_t)nc : r.cells.size());
    return r;
  }
  void change_clear() { check(vg_change_clear(ctx_), "vg_change_clear"); }
  void change_end() { check(vg_change_end(ctx_), "vg_change_end"); }
  // the live obstacle layer (vina_gpu.h "Live obstacle layer") of this context: base_grid null: a copy of the grid
  // the last occupancy() call left on the device; stamp 0: the largest so far + 1; now 0: the largest stamp
  void live_begin(const vg_live_params& prm, const int8_t* base_grid = nullptr) {
    check(vg_live_begin(ctx_, &prm, base_grid), "vg_live_begin");
  }
  vg_live_summary live_mark(const float* xyz, int n, const double* pose12 = nullptr, int32_t stamp = 0,
                            vg_live_point* per_point = nullptr) {
    vg_live_summary out;
    check(vg_live_mark(ctx_, xyz, n, pose12, stamp, per_point, &out), "vg_live_mark");
    return out;
  }
  vg_live_summary live_mark_dev(const float* d_x, const float* d_y, const float* d_z, int n,
                                const double* pose12 = nullptr, int32_t stamp = 0) {
    vg_live_summary out;
    check(vg_live_mark_dev(ctx_, d_x, d_y, d_z, n, pose12, stamp, &out), "vg_live_mark_dev");
    return out;
  }
  // grid null: the composed grid stays on the device, where clearance(nullptr, ...) reads it
  vg_live_summary live_compose(int32_t now = 0, int flags = 0, int8_t* grid = nullptr) {
    vg_live_summary out;
    check(vg_live_compose(ctx_, now, flags, grid, &out), "vg_live_compose");
    return out;
  }
  vg_live_summary live_info(int32_t* hit = nullptr, int32_t* clear = nullptr) {
    vg_live_summary out;
    check(vg_live_info(ctx_, hit, clear, &out), "vg_live_info");
    return out;
  }
  void live_clear() { check(vg_live_clear(ctx_), "vg_live_clear"); }
  void live_end() { check(vg_live_end(ctx_), "vg_live_end"); }
  // the place index (vina_gpu.h "Place index"): build / end on the map's owner; info, scan, query and
  // relocalize_global on the owner or any tracker attached to it. R_level9 null: the current R
  void places_build(const double* positions, int M, const vg_places_params* prm = nullptr) {
    check(vg_places_build(ctx_, positions, M, prm), "vg_places_build");
  }
  struct PlacesInfo {
    int M = 0, n_valid = 0;
    std::vector<int32_t> hit_bins;
  };
  PlacesInfo places_info() {
    PlacesInfo r;
    check(vg_places_info(ctx_, &r.M, &r.n_valid, nullptr, nullptr), "vg_places_info");
    r.hit_bins.resize((size_t)r.M);
    check(vg_places_info(ctx_, &r.M, &r.n_valid, nullptr, r.hit_bins.data()), "vg_places_info");
    return r;
  }
  // desc / n_per_bin: n_el * n_az entries each, either may be null
  void places_scan(const float* xyz, int n, const double* R_level9, uint16_t* desc, int32_t* n_per_bin) {
    check(vg_places_scan(ctx_, xyz, n, R_level9, desc, n_per_bin), "vg_places_scan");
  }
  std::vector<vg_place_candidate> places_query(const float* xyz, int n, const double* R_level9 = nullptr,
                                               int top_k = 16, int32_t* scores_all = nullptr) {
    std::vector<vg_place_candidate> out((size_t)(top_k > 0 ? top_k : 0));
    int n_out = 0;
    check(vg_places_query(ctx_, xyz, n, R_level9, top_k, out.data(), &n_out, scores_all), "vg_places_query");
    out.resize((size_t)n_out);
    return out;
  }
  void places_end() { check(vg_places_end(ctx_), "vg_places_end"); }
  // returns ok; prm null: the default window around each candidate; score / place may be null
  bool relocalize_global(const float* xyz, int n, const double* R_level9, int top_k, const vg_reloc_params* prm,
                         bool install, double* out_pose, vg_pose_score* score = nullptr,
                         vg_place_candidate* place = nullptr) {
    int ok = 0;
    check(vg_relocalize_global(ctx_, xyz, n, R_level9, top_k, prm, install ? 1 : 0, out_pose, score, place, &ok),
          "vg_relocalize_global");
    return ok != 0;
  }
  // map views (vina_gpu.h "Map views"): this context reads owner's frozen map. The owner
  // must outlive its views: destroy (or detach) the trackers first
  void attach(LioCore& owner) { check(vg_map_attach(ctx_, owner.ctx_), "vg_map_attach"); }
  void detach() { check(vg_map_detach(ctx_), "vg_map_detach"); }
  void marker_capacity(int max_records) { check(vg_marker_capacity(ctx_, max_records), "vg_marker_capacity"); }
  std::vector<vg_plane_marker> markers(int* deferred = nullptr) {
    int n = 0, d = 0;
    check(vg_markers(ctx_, nullptr, 0, &n, &d), "vg_markers");
    std::vector<vg_plane_marker> out((size_t)n);
    if (n > 0) check(vg_markers(ctx_, out.data(), n, &n, &d), "vg_markers");
    if (deferred) *deferred = d;
    return out;
  }
  std::vector<vg_plane_marker> map_planes(bool slide_only = false, bool all_nodes = false) {
    const int flags = (slide_only ? 1 : 0) | (all_nodes ? 2 : 0);
    int n = 0;
    check(vg_map_planes(ctx_, flags, nullptr, 0, &n), "vg_map_planes");
    std::vector<vg_plane_marker> out((size_t)(n > 0 ? n : 1));
    check(vg_map_planes(ctx_, flags, out.data(), n > 0 ? n : 1, &n), "vg_map_planes");
    out.resize((size_t)n < out.size() ? (size_t)n : out.size());
    return out;
  }
  vg_ctx* raw() { return ctx_; }

 private:
  void check(int r, const char* what) {
    if (r != VG_OK) throw Error(r, std::string(what) + ": " + vg_last_error(ctx_));
  }
  vg_ctx* ctx_ = nullptr;
};

// The fleet (vg_fleet_*): trackers attached to one owner's map, one frozen scan
// each per step in ten launches for any number of trackers. Destroy the fleet
// before its trackers.
class Fleet {
 public:
  Fleet(LioCore& owner, const std::vector<LioCore*>& trackers) {
    std::vector<vg_ctx*> c;
    for (LioCore* t : trackers) c.push_back(t->raw());
    const int r = vg_fleet_create(owner.raw(), c.data(), (int)c.size(), &f_);
    if (r != VG_OK) throw Error(r, std::string("vg_fleet_create: ") + vg_last_error(owner.raw()));
    first_ = c.empty() ? nullptr : c[0];
  }
  ~Fleet() { vg_fleet_destroy(f_); }
  Fleet(const Fleet&) = delete;
  Fleet& operator=(const Fleet&) = delete;
  // one record per tracker; n < 0: the tracker sits the step out
  void step(const std::vector<vg_scan_dev>& scans) { check(vg_fleet_step_dev(f_, scans.data()), "vg_fleet_step_dev"); }
  void sync() { check(vg_fleet_sync(f_), "vg_fleet_sync"); }

 private:
  void check(int r, const char* what) {
    if (r != VG_OK) throw Error(r, std::string(what) + ": " + vg_last_error(first_));
  }
  vg_fleet* f_ = nullptr;
  vg_ctx* first_ = nullptr;
};

}  // namespace vina_gpu
