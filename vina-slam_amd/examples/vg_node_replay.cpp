// vg_node_replay — runs a recorded sensor event log through vina_gpu::NodeCore,
// the ROS-free core of the reference's ROS 2 node (include/vina_node_core.hpp,
// SURVEY rows f3/f4): IMU samples and raw LiDAR messages in arrival order, as
// the node's subscriptions would deliver them (node.cpp:153-170), each
// followed by a spin of sync_packages + the estimator. Writes the TUM pose file
// of save_pose_tum (io.cpp:67-77) and prints one summary line.
//
// Event log (little-endian):
//   "VGEVENT1" | vg_config (sizeof) | vg_lidar_format (sizeof) | int32 point_notime
//   | int32 has_seed | double seed[VG_STATE_LEN] if has_seed
//   then events: int32 type; 0: double imu[7] (t, gyr 3, acc 3);
//                1: double header_time, int32 n, int32 stride, n*stride record bytes;
//                -1 or end of file: done
//
// usage: vg_node_replay <events.bin> <out_tum.txt> [device [out_path.txt [out_cmap.bin [out_markers.bin]]]]
//        [--checkpoint-out FILE --checkpoint-at N] [--resume FILE]
//        [--map FILE --localize [--guess "x y z yaw" | --global [--places-step S]] [--scan-diff] [--scan-info]
//         [--changes FILE [--changes-scans FILE]]
//         [--live [--live-persist N] [--live-scans FILE]]  (with --costmap)
//         [--terrain TPREFIX [--sensor-height H] [--step-max S] [--terrain-rays FILE]]
//         [--occupancy PREFIX [--occ-res R] [--occ-rays FILE]
//          [--costmap CPREFIX [--inscribed r] [--inflation R] [--cost-scaling s]
//           [--plan "gx gy" [--from "sx sy"] --path out.csv] [--frontiers out.csv
//           [--view-gain g.csv --view-radius METRES [--view-max-unknown N]]]]]]
// --checkpoint-out / --checkpoint-at: save a checkpoint (vg_checkpoint_save) once N packages have
// been stepped, beside it FILE.meta with N; --resume: load FILE before the first package and drop
// the packages it had consumed (the log is still read from its start: it feeds the synchroniser).
// --map FILE --localize: load the map FILE (a checkpoint), relocalise on the first scan around the
// guess (default: the map's saved pose; --guess: position and yaw about z, the saved roll / pitch kept;
// window +-2 m / 0.25 m, +-30 deg / 2.5 deg) and run with the map frozen; the TUM output is as always.
// --global (with --localize, not with --guess): no position is assumed. A place index (vg_places_build) is
// built from the map's own path rows, which the checkpoint carries — the LiDAR origins p + R ext_t, thinned to
// at least S metres apart (--places-step, default 1) — or, where the map has fewer than two rows, on a lattice of
// step S over the bounds of its plane leaves' voxel centres at the saved pose's height; the first scan is
// relocalised through it (vg_relocalize_global) with the saved attitude as R_level, and
//   relocalise: global place <i> yaw <deg> score <s>
// goes to stderr beside the relocalise line. The index is ended once the scan is placed.
// --scan-diff (with --localize): every localised scan's downsampled cloud is checked against the map at
// its IEKF pose (vg_scan_diff) and one line per scan goes to stdout ahead of the summary line:
//   scan_diff <scan index> <scan end time> <n_ds> <unknown> <consistent> <appeared> <vanished>
// --scan-info (with --localize): the expected pose information of every localised scan's downsampled cloud at
// the pose just estimated (vg_scan_info, its CONSISTENT points), one line per scan on stdout:
//   scan_info <scan index> <scan end time> <n_hits> <eig_t[0]> <dir_t x y z> <eig_r[0]>
// (doubles with 9 significant digits; the smallest eigenvalue of the translation information with the rotation
// marginalised, its direction in the world, and the rotation's).
// --changes FILE (with --localize): a change layer is begun on the loaded map, every localised scan's
// downsampled cloud accumulated at its IEKF pose (vg_change_accumulate; its summary feeds --scan-diff),
// and the report of everything touched (query flags 1, default rule) written as CSV at the end, doubles
// with 17 significant digits, one record per line by kind:
//   leaf,node,layer,n_consistent,n_vanished,n_occluded,n_scans,flags,vcx,vcy,vcz,quater_length,cx,cy,cz,nx,ny,nz
//   cell,kx,ky,kz,n_appeared,n_scans,flags,x,y,z
//   totals,calls,points,unknown,consistent,appeared,vanished,cells_used,dropped,out_of_range,leaves_touched
// (flags bit 0: the leaf meets the removed rule / the cell the added rule). --changes-scans FILE: what was
// accumulated, per scan int32 n, double pose[12], float xyz[3 n], to check the report against the API.
// --occupancy PREFIX (with --localize): at the end of the run the 2-D occupancy grid is cast from the node's
// path — the loaded map's rows and the localised scans' — (NodeCore::occupancy_grid: vg_occupancy on the
// sensor origins thinned to one per cell edge; --occ-res R metres, default 0.1) and written in map_server's
// form: PREFIX.pgm (P5, the first row at the largest y; occupied 0, free 254, unknown 205) and PREFIX.yaml
// (image, resolution, origin: [x0, y0, 0], negate: 0, occupied_thresh: 0.65, free_thresh: 0.196). Leaves
// without a plane are not obstacles in this grid. --occ-rays FILE: what was cast, int32 M, int32 D, the
// vg_occ_params used, double origins[3 M], double dirs[3 D], to check the grid against the API.
// --terrain TPREFIX (with --localize): the terrain layer cast from the same origins on the same grid
// (NodeCore::terrain_grid: vg_terrain with a fan of elevations -30 .. 10 degrees; --occ-res R; --sensor-height H
// metres, the sensor's height over the ground it drives on, default 0; --step-max S metres: cells with a larger
// step become occupied, flags bit 1). Written: the grid judged relative to the ground as TPREFIX.pgm and
// TPREFIX.yaml in --occupancy's form, and the elevation as TPREFIX.elev (nx ny little-endian int32 in units of
// z_res, row iy = 0 first, INT32_MIN where there is none) beside TPREFIX.elev.yaml (data, nx, ny, resolution,
// origin, z_res, none). It runs after --occupancy's cast where both are given, and --costmap (which goes with
// either) then prices the terrain grid: the one that lies on the device.
// --terrain-rays FILE: what was cast, int32 M, int32 D, the vg_terrain_params used, double origins[3 M], double
// dirs[3 D].
// --costmap CPREFIX (with --occupancy or --terrain): straight after the last cast the clearance field of that grid is
// taken where it lies on the device (NodeCore::costmap: vg_clearance with grid == NULL) with the robot's
// --inscribed r and --inflation R radii in metres (defaults 0.3, 1.0) and --cost-scaling s per metre (default
// 3.0; nav2's cost_scaling_factor), and its cost written as raw bytes (254 lethal, 253 inscribed, 252 .. 1 the
// skirt, 0 free, 255 no information) to CPREFIX.pgm, flipped as PREFIX.pgm is, with the same CPREFIX.yaml.
// --live (with --costmap; --live-persist N: the marks live N scans; --live-scans FILE: what was marked, in
// --changes-scans' form): every localised scan's downsampled cloud is kept with its IEKF pose; after everything
// --costmap brings, a live obstacle layer is begun over the grid --costmap priced, where it lies on the device
// (NodeCore::live_begin: band -0.5 .. 0.5 m about the sensor, marks between 0.5 and 8 m, beams cleared to 10 m,
// UNKNOWN points mark too), the scans are marked in order with stamps 1, 2, ..., and the last goes through
// NodeCore::live_costmap: the composed grid is written as CPREFIX.live.grid.pgm / .yaml in --occupancy's form, its
// cost as CPREFIX.live.pgm / .yaml in --costmap's, and one line goes to stdout: live: N scans, K cells live.
// --plan "gx gy" (with --costmap): the navigation function over that costmap where it lies on the device
// (NodeCore::plan: vg_navfn with cost == NULL, nav2's default traversal table) towards the cell holding the
// world point gx gy, and the path down it from the cell holding --from "sx sy" (default: the last pose), written
// to --path out.csv as one x,y,pot row per cell (the cell's centre in metres, its cost-to-go), the start first.
// One line on stdout: the status (REACHED, NO_PATH, TRUNCATED, STUCK), the number of cells and the start's cost.
// --frontiers out.csv (with --costmap): the exploration frontiers of that grid over that costmap, both where they
// lie on the device (NodeCore::frontiers: vg_frontiers with grid == NULL and cost == NULL), with --plan only those
// the plan's field reaches, ranked by it. One label,size,cx,cy,best_x,best_y,best_pot row per frontier in the
// order to visit them (cx, cy: the world centroid; best_x, best_y: the cheapest cell's centre, nan without
// --plan), and one line on stdout: frontiers: N kept of M, K cells.
// --view-gain g.csv --view-radius METRES (with --frontiers and --plan): what a 2-D sensor of that range, rounded to
// whole cells, sees of the grid from every frontier's best cell (NodeCore::frontier_gain: vg_view_gain with grid ==
// NULL; --view-max-unknown N ends a ray at its N-th unknown cell). One
// label,best_x,best_y,best_pot,n_unknown,n_free,n_occupied,n_rays_open row per frontier that shows an unknown cell,
// in the order of the gain per cost (LioCore::ViewGain::order over best_pot), and one line on stdout: view gain: N
// of M frontiers, radius R cells, K unknown cells in view. out.csv is what it is without these options.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/vina_node_core.hpp"

static bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc0, char** argv0) {
  std::vector<char*> pos;
  std::string ck_out, resume, map_file, guess_s, changes_file, changes_scans, occ_prefix, occ_rays, cm_prefix, plan_s, from_s,
      plan_csv, fr_csv, vg_csv, ter_prefix, ter_rays;
  double occ_res = 0.1, cm_inscribed = 0.3, cm_inflation = 1.0, cm_scaling = 3.0, view_radius = 0.0;
  double ter_height = 0.0, ter_step = -1.0;
  int ck_at = -1, view_max_unknown = 0;
  bool localize = false, scan_diff = false, scan_info = false, global = false, live = false;
  int live_persist = 0;
  std::string live_scans_file;
  double places_step = 1.0;
  for (int i = 0; i < argc0; i++) {
    const std::string a = argv0[i];
    if (i + 1 < argc0 && a == "--checkpoint-out") ck_out = argv0[++i];
    else if (i + 1 < argc0 && a == "--checkpoint-at") ck_at = atoi(argv0[++i]);
    else if (i + 1 < argc0 && a == "--resume") resume = argv0[++i];
    else if (i + 1 < argc0 && a == "--map") map_file = argv0[++i];
    else if (i + 1 < argc0 && a == "--guess") guess_s = argv0[++i];
    else if (i + 1 < argc0 && a == "--changes") changes_file = argv0[++i];
    else if (i + 1 < argc0 && a == "--changes-scans") changes_scans = argv0[++i];
    else if (i + 1 < argc0 && a == "--places-step") places_step = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--occupancy") occ_prefix = argv0[++i];
    else if (i + 1 < argc0 && a == "--occ-res") occ_res = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--occ-rays") occ_rays = argv0[++i];
    else if (i + 1 < argc0 && a == "--costmap") cm_prefix = argv0[++i];
    else if (i + 1 < argc0 && a == "--terrain") ter_prefix = argv0[++i];
    else if (i + 1 < argc0 && a == "--terrain-rays") ter_rays = argv0[++i];
    else if (i + 1 < argc0 && a == "--sensor-height") ter_height = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--step-max") ter_step = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--plan") plan_s = argv0[++i];
    else if (i + 1 < argc0 && a == "--from") from_s = argv0[++i];
    else if (i + 1 < argc0 && a == "--path") plan_csv = argv0[++i];
    else if (i + 1 < argc0 && a == "--frontiers") fr_csv = argv0[++i];
    else if (i + 1 < argc0 && a == "--view-gain") vg_csv = argv0[++i];
    else if (i + 1 < argc0 && a == "--view-radius") view_radius = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--view-max-unknown") view_max_unknown = atoi(argv0[++i]);
    else if (i + 1 < argc0 && a == "--inscribed") cm_inscribed = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--inflation") cm_inflation = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--cost-scaling") cm_scaling = atof(argv0[++i]);
    else if (i + 1 < argc0 && a == "--live-persist") live_persist = atoi(argv0[++i]);
    else if (i + 1 < argc0 && a == "--live-scans") live_scans_file = argv0[++i];
    else if (a == "--live") live = true;
    else if (a == "--localize") localize = true;
    else if (a == "--global") global = true;
    else if (a == "--scan-diff") scan_diff = true;
    else if (a == "--scan-info") scan_info = true;
    else pos.push_back(argv0[i]);
  }
  const int argc = (int)pos.size();
  char** argv = pos.data();
  const bool changes = !changes_file.empty();
  if ((scan_diff || scan_info || changes || !occ_prefix.empty() || !ter_prefix.empty()) && !localize) {
    fprintf(stderr, "%s: --scan-diff, --scan-info, --changes, --occupancy and --terrain need --map FILE --localize\n", argv0[0]);
    return 2;
  }
  if (ter_prefix.empty() ? (!ter_rays.empty() || ter_height != 0.0 || ter_step != -1.0) : (!(ter_height >= 0.0) || (ter_step != -1.0 && !(ter_step >= 0.0)))) {
    fprintf(stderr, "%s: --terrain-rays, --sensor-height H >= 0 and --step-max S >= 0 go with --terrain TPREFIX\n", argv0[0]);
    return 2;
  }
  if ((!occ_rays.empty() && occ_prefix.empty()) || !(occ_res > 0.0)) {
    fprintf(stderr, "%s: --occ-rays needs --occupancy PREFIX, --occ-res a positive edge\n", argv0[0]);
    return 2;
  }
  if (!cm_prefix.empty() && ((occ_prefix.empty() && ter_prefix.empty()) || !(cm_inscribed >= 0.0) || !(cm_inflation >= cm_inscribed) || !(cm_scaling >= 0.0))) {
    fprintf(stderr, "%s: --costmap needs --occupancy PREFIX or --terrain TPREFIX, 0 <= --inscribed <= --inflation and --cost-scaling >= 0\n", argv0[0]);
    return 2;
  }
  double plan_goal[2] = {0, 0}, plan_from[2] = {0, 0};
  if ((!plan_s.empty() || !from_s.empty() || !plan_csv.empty()) &&
      (cm_prefix.empty() || plan_csv.empty() || sscanf(plan_s.c_str(), "%lf %lf", &plan_goal[0], &plan_goal[1]) != 2 ||
       (!from_s.empty() && sscanf(from_s.c_str(), "%lf %lf", &plan_from[0], &plan_from[1]) != 2))) {
    fprintf(stderr, "%s: --plan \"gx gy\" needs --costmap CPREFIX and --path FILE; --from is \"sx sy\"\n", argv0[0]);
    return 2;
  }
  if (!fr_csv.empty() && cm_prefix.empty()) {
    fprintf(stderr, "%s: --frontiers FILE needs --costmap CPREFIX\n", argv0[0]);
    return 2;
  }
  if ((!vg_csv.empty() || view_radius != 0.0 || view_max_unknown != 0) &&
      (vg_csv.empty() || fr_csv.empty() || plan_s.empty() || !(view_radius > 0.0) || view_max_unknown < 0)) {
    fprintf(stderr, "%s: --view-gain FILE needs --frontiers FILE, --plan and a positive --view-radius METRES; --view-max-unknown N >= 0\n", argv0[0]);
    return 2;
  }
  if (global && (!localize || !guess_s.empty() || !(places_step > 0.0))) {
    fprintf(stderr, "%s: --global needs --map FILE --localize, a positive --places-step, and no --guess\n", argv0[0]);
    return 2;
  }
  if (live ? (cm_prefix.empty() || live_persist < 0) : (live_persist != 0 || !live_scans_file.empty())) {
    fprintf(stderr, "%s: --live needs --costmap CPREFIX; --live-persist N >= 0 and --live-scans FILE go with --live\n", argv0[0]);
    return 2;
  }
  if (!changes_scans.empty() && !changes) {
    fprintf(stderr, "%s: --changes-scans needs --changes FILE\n", argv0[0]);
    return 2;
  }
  if (argc < 3 || (ck_out.empty() != (ck_at < 0)) || (localize != !map_file.empty())) {
    fprintf(stderr, "usage: %s events.bin out_tum.txt [device [out_path.txt [out_cmap.bin [out_markers.bin]]]]\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror("events");
    return 1;
  }
  char magic[8];
  vg_config cfg;
  vg_lidar_format fmt;
  int point_notime = 0, has_seed = 0;
  double seed[VG_STATE_LEN];
  if (!rd(f, magic, 8) || memcmp(magic, "VGEVENT1", 8) != 0 || !rd(f, &cfg, sizeof(cfg)) ||
      !rd(f, &fmt, sizeof(fmt)) || !rd(f, &point_notime, 4) || !rd(f, &has_seed, 4) ||
      (has_seed && !rd(f, seed, sizeof(seed)))) {
    fprintf(stderr, "bad event log header\n");
    return 1;
  }
  try {
    vg_capacity cap = {0, 0, 0, 0};
    cap.max_points_per_scan = 400000;
    vina_gpu::NodeCore node(cfg, &cap, fmt, point_notime, argc > 3 ? atoi(argv[3]) : 0);
    if (has_seed) node.lio().seed(seed);
    if (argc > 5) node.enable_local_map(true);  // /map_cmap after every window BA
    // /voxel_plane + /voxel_normal (General.enable_visualization): per stepped scan an int32 record
    // count, then that scan's vg_plane_marker records (one record serves both topics)
    FILE* fm = nullptr;
    size_t n_markers = 0;
    if (argc > 6) {
      fm = fopen(argv[6], "wb");
      if (!fm) {
        perror("markers");
        return 1;
      }
      node.enable_visualization(true);
    }
    if (!resume.empty()) {
      int consumed = -1;
      FILE* fmeta = fopen((resume + ".meta").c_str(), "r");
      if (!fmeta || fscanf(fmeta, "%d", &consumed) != 1 || consumed < 0) {
        fprintf(stderr, "vg_node_replay: cannot read %s.meta\n", resume.c_str());
        return 1;
      }
      fclose(fmeta);
      node.load_checkpoint(resume);
      node.skip_packages(consumed);
    }
    if (localize) {
      vina_gpu::NodeParams np;
      np.localization_mode = 1;
      np.map_path = map_file;
      node.apply(np);
      double st[VG_STATE_LEN], g[12];
      if (vg_get_state(node.lio().raw(), st) != VG_OK) return 1;
      memcpy(g, st + 1, sizeof(g));
      double x, y, z, yaw;
      if (!guess_s.empty()) {
        if (sscanf(guess_s.c_str(), "%lf %lf %lf %lf", &x, &y, &z, &yaw) != 4) {
          fprintf(stderr, "vg_node_replay: --guess wants \"x y z yaw\"\n");
          return 2;
        }
        const double c = cos(yaw), s = sin(yaw), y0 = atan2(g[3], g[0]);
        const double c0 = cos(-y0), s0 = sin(-y0);  // Rz(yaw) Rz(-yaw0) R: the saved roll / pitch under the new yaw
        double R1[9], R2[9];
        for (int k = 0; k < 3; k++) {
          R1[k] = c0 * g[k] - s0 * g[3 + k], R1[3 + k] = s0 * g[k] + c0 * g[3 + k], R1[6 + k] = g[6 + k];
        }
        for (int k = 0; k < 3; k++) {
          R2[k] = c * R1[k] - s * R1[3 + k], R2[3 + k] = s * R1[k] + c * R1[3 + k], R2[6 + k] = R1[6 + k];
        }
        memcpy(g, R2, sizeof(R2));
        g[9] = x, g[10] = y, g[11] = z;
      }
      if (global) {
        std::vector<double> places;
        vg_ctx* c = node.lio().raw();
        int rows = 0;
        if (vg_path(c, nullptr, 0, &rows) != VG_OK) return 1;
        if (rows >= 2) {
          std::vector<double> path((size_t)rows * 14);
          if (vg_path(c, path.data(), rows, &rows) != VG_OK) return 1;
          for (int r = 0; r < rows; r++) {
            const double* R = &path[(size_t)r * 14 + 1];
            const double* p = R + 9;
            double o[3];
            for (int j = 0; j < 3; j++)
              o[j] = p[j] + R[3 * j] * cfg.ext_t[0] + R[3 * j + 1] * cfg.ext_t[1] + R[3 * j + 2] * cfg.ext_t[2];
            const size_t m = places.size();
            if (m == 0 || hypot(hypot(o[0] - places[m - 3], o[1] - places[m - 2]), o[2] - places[m - 1]) >= places_step)
              places.insert(places.end(), o, o + 3);
          }
        } else {
          const std::vector<vg_plane_marker> pl = node.lio().map_planes();
          if (pl.empty()) {
            fprintf(stderr, "vg_node_replay: --global: the map has neither path rows nor planes\n");
            return 1;
          }
          double lo[2] = {pl[0].voxel_center[0], pl[0].voxel_center[1]}, hi[2] = {lo[0], lo[1]};
          for (const vg_plane_marker& m : pl)
            for (int j = 0; j < 2; j++) {
              lo[j] = m.voxel_center[j] < lo[j] ? m.voxel_center[j] : lo[j];
              hi[j] = m.voxel_center[j] > hi[j] ? m.voxel_center[j] : hi[j];
            }
          for (double y = lo[1]; y <= hi[1] + 1e-9; y += places_step)
            for (double x = lo[0]; x <= hi[0] + 1e-9; x += places_step) {
              const double o[3] = {x, y, g[11]};
              places.insert(places.end(), o, o + 3);
            }
        }
        node.lio().places_build(places.data(), (int)(places.size() / 3));
        fprintf(stderr, "places: %d from %s\n", (int)(places.size() / 3), rows >= 2 ? "the map's path" : "a lattice");
        node.relocalize_global(g, 16, nullptr);  // R_level: the saved attitude
      } else {
        vg_reloc_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.half_xy = 2.0, prm.step_xy = 0.25;
        prm.half_yaw = 30 * M_PI / 180, prm.step_yaw = 2.5 * M_PI / 180;
        node.relocalize(g, prm);
      }
    }
    // --scan-diff / --changes: after every localised scan, its downsampled cloud against the map at its IEKF pose
    FILE* fscans = nullptr;
    int n_diffed = 0;
    std::vector<float> ds;
    if (changes) {
      node.lio().change_begin();
      if (!changes_scans.empty() && !(fscans = fopen(changes_scans.c_str(), "wb"))) {
        perror("changes-scans");
        return 1;
      }
    }
    struct LiveScan {
      std::vector<float> xyz;
      double pose[12];
    };
    std::vector<LiveScan> live_scans;  // --live: every localised scan, marked at the end of the run
    if (scan_diff || scan_info || changes || live)
      node.set_after_step([&]() {
        vg_ctx* c = node.lio().raw();
        int n = 0;
        double st[VG_STATE_LEN];
        if (vg_scan_points(c, nullptr, 0, &n) != VG_OK || vg_get_state(c, st) != VG_OK)
          throw vina_gpu::Error(VG_E_STATE, std::string("after the scan: ") + vg_last_error(c));
        ds.resize((size_t)3 * (n > 0 ? n : 1));
        if (n > 0 && vg_scan_points(c, ds.data(), n, &n) != VG_OK)
          throw vina_gpu::Error(VG_E_STATE, std::string("vg_scan_points: ") + vg_last_error(c));
        const double* pose = st + 1;  // R row-major, p: the pose after the scan's IEKF
        if (live) {
          LiveScan ls;
          ls.xyz.assign(ds.begin(), ds.begin() + (size_t)3 * n);
          memcpy(ls.pose, pose, sizeof(ls.pose));
          live_scans.push_back(std::move(ls));
        }
        if (scan_info) {
          const vg_info_rec r = node.lio().scan_info(ds.data(), n, pose);
          printf("scan_info %d %.9f %d %.9g %.9g %.9g %.9g %.9g\n", n_diffed, st[0], r.n_hits, r.eig_t[0], r.dir_t[0],
                 r.dir_t[1], r.dir_t[2], r.eig_r[0]);
        }
        if (!scan_diff && !changes) {
          n_diffed++;
          return;
        }
        const vg_diff_summary sm = changes ? node.lio().change_accumulate(ds.data(), n, pose)
                                           : node.lio().scan_diff(ds.data(), n, pose);
        if (fscans) {
          const int32_t n32 = n;
          if (fwrite(&n32, sizeof(n32), 1, fscans) != 1 || fwrite(pose, sizeof(double), 12, fscans) != 12 ||
              fwrite(ds.data(), sizeof(float), (size_t)3 * n, fscans) != (size_t)3 * n)
            throw vina_gpu::Error(VG_E_STATE, "writing the --changes-scans file failed");
        }
        if (scan_diff)
          printf("scan_diff %d %.9f %d %d %d %d %d\n", n_diffed, st[0], n, sm.n[VG_DIFF_UNKNOWN], sm.n[VG_DIFF_CONSISTENT],
                 sm.n[VG_DIFF_APPEARED], sm.n[VG_DIFF_VANISHED]);
        n_diffed++;
      });
    if (ck_at >= 0) node.set_package_limit(ck_at);
    std::vector<unsigned char> rec;
    int n_imu = 0, n_msg = 0, n_step = 0;
    bool reloc_said = false;
    for (;;) {
      int type = -1;
      if (!rd(f, &type, 4) || type < 0) break;
      if (type == 0) {
        double s[7];
        if (!rd(f, s, sizeof(s))) break;
        node.imu(s[0], s + 1, s + 4);
        n_imu++;
      } else {
        double stamp;
        int n, stride;
        if (!rd(f, &stamp, 8) || !rd(f, &n, 4) || !rd(f, &stride, 4) || n < 0 || stride <= 0) break;
        rec.resize((size_t)n * stride);
        if (!rd(f, rec.data(), rec.size())) break;
        node.scan(stamp, rec.data(), n);
        n_msg++;
      }
      n_step += node.spin();
      if (localize && node.relocalized() && !reloc_said) {
        fprintf(stderr, "relocalise: %s\n", node.relocalize_ok() ? "ok" : "failed (the guess's pose stays)");
        if (global) {
          const vg_place_candidate& pc = node.relocalize_place();
          fprintf(stderr, "relocalise: global place %d yaw %.3f score %d\n", pc.place, pc.yaw * 180.0 / M_PI, pc.score);
          node.lio().places_end();  // (a later --checkpoint-out would be refused while it stands)
        }
        reloc_said = true;
      }
      if (ck_at >= 0 && node.packages() >= ck_at) {
        const long long bytes = node.save_checkpoint(ck_out);
        FILE* fmeta = fopen((ck_out + ".meta").c_str(), "w");
        if (!fmeta || fprintf(fmeta, "%d\n", node.packages()) < 0 || fclose(fmeta) != 0) {
          perror("checkpoint meta");
          return 1;
        }
        fprintf(stderr, "checkpoint: %lld bytes after %d packages\n", bytes, node.packages());
        ck_at = -1;
        node.set_package_limit(-1);
        n_step += node.spin();  // the packages the limit held back
      }
      if (fm) {
        size_t at = 0;
        for (const int cnt : node.marker_scan_counts()) {
          const int32_t c = cnt;
          if (fwrite(&c, sizeof(c), 1, fm) != 1 ||
              fwrite(node.voxel_plane().data() + at, sizeof(vg_plane_marker), (size_t)cnt, fm) != (size_t)cnt) {
            perror("markers");
            return 1;
          }
          at += (size_t)cnt;
        }
        n_markers += at;
        node.clear_markers();
      }
    }
    if (fm) fclose(fm);
    if (fscans && fclose(fscans) != 0) {
      perror("changes-scans");
      return 1;
    }
    if (changes) {  // everything the layer holds, the records' flags telling what meets the default rule
      vg_change_query q;
      memset(&q, 0, sizeof(q));
      q.flags = 1;
      const vina_gpu::LioCore::ChangeReport r = node.lio().change_report(&q);
      node.lio().change_end();
      FILE* fc = fopen(changes_file.c_str(), "w");
      if (!fc) {
        perror("changes");
        return 1;
      }
      for (const vg_change_leaf& l : r.leaves)
        fprintf(fc, "leaf,%d,%d,%d,%d,%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n", l.node, l.layer,
                l.n_consistent, l.n_vanished, l.n_occluded, l.n_scans, l.flags, l.voxel_center[0], l.voxel_center[1],
                l.voxel_center[2], l.quater_length, l.center[0], l.center[1], l.center[2], l.normal[0], l.normal[1],
                l.normal[2]);
      for (const vg_change_cell& c : r.cells)
        fprintf(fc, "cell,%d,%d,%d,%d,%d,%d,%.17g,%.17g,%.17g\n", c.key[0], c.key[1], c.key[2], c.n_appeared, c.n_scans,
                c.flags, c.centroid[0], c.centroid[1], c.centroid[2]);
      const vg_change_totals& t = r.totals;
      fprintf(fc, "totals,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld,%lld\n", (long long)t.calls, (long long)t.points,
              (long long)t.n[0], (long long)t.n[1], (long long)t.n[2], (long long)t.n[3], (long long)t.cells_used,
              (long long)t.dropped, (long long)t.out_of_range, (long long)t.leaves_touched);
      if (fclose(fc) != 0) {
        perror("changes");
        return 1;
      }
    }
    // --terrain: after --occupancy's cast, so that the grid left on the device is the terrain's; grid_out: that grid
    const auto run_terrain = [&](vina_gpu::OccupancyGrid& grid_out) -> bool {
      vina_gpu::TerrainGridParams tp;
      tp.res = occ_res;
      tp.ter.sensor_height = ter_height;
      if (ter_step >= 0.0) tp.ter.flags |= 2, tp.ter.step_max = ter_step;
      const vina_gpu::TerrainGrid tg = node.terrain_grid(tp);
      if (!vina_gpu::write_terrain_map(ter_prefix, tg)) {
        perror("terrain");
        return false;
      }
      const vg_terrain_summary& sm = tg.summary;
      fprintf(stderr, "terrain: %d x %d cells of %g m from %d origins x %d directions: %lld ground hits on %lld cells, max step %d, %lld occupied (%lld by their step), %lld free, %lld unknown\n",
              tg.nx, tg.ny, tg.res, (int)(tg.origins.size() / 3), (int)(tg.dirs.size() / 3), (long long)sm.n_ground_hits,
              (long long)sm.cells_ground, (int)sm.max_step, (long long)sm.cells_occupied, (long long)sm.cells_step_lethal,
              (long long)sm.cells_free, (long long)sm.cells_unknown);
      if (!ter_rays.empty()) {
        const int32_t md[2] = {(int32_t)(tg.origins.size() / 3), (int32_t)(tg.dirs.size() / 3)};
        FILE* fr = fopen(ter_rays.c_str(), "wb");
        if (!fr || fwrite(md, sizeof(md), 1, fr) != 1 || fwrite(&tg.params, sizeof(tg.params), 1, fr) != 1 ||
            fwrite(tg.origins.data(), sizeof(double), tg.origins.size(), fr) != tg.origins.size() ||
            fwrite(tg.dirs.data(), sizeof(double), tg.dirs.size(), fr) != tg.dirs.size() || fclose(fr) != 0) {
          perror("terrain-rays");
          return false;
        }
      }
      grid_out = tg.grid();
      return true;
    };
    vina_gpu::OccupancyGrid nav;  // the grid --costmap prices: --terrain's where given, else --occupancy's (the last cast: it lies on the device)
    if (!occ_prefix.empty()) {
      vina_gpu::OccupancyGridParams op;
      op.res = occ_res;
      const vina_gpu::OccupancyGrid og = node.occupancy_grid(op);
      if (!vina_gpu::write_occupancy_map(occ_prefix, og)) {
        perror("occupancy");
        return 1;
      }
      const vg_occ_summary& sm = og.summary;
      fprintf(stderr, "occupancy: %d x %d cells of %g m from %d origins x %d directions: %lld occupied, %lld free, %lld unknown\n",
              og.nx, og.ny, og.res, (int)(og.origins.size() / 3), (int)(og.dirs.size() / 3), (long long)sm.cells_occupied,
              (long long)sm.cells_free, (long long)sm.cells_unknown);
      if (!occ_rays.empty()) {
        const int32_t md[2] = {(int32_t)(og.origins.size() / 3), (int32_t)(og.dirs.size() / 3)};
        FILE* fr = fopen(occ_rays.c_str(), "wb");
        if (!fr || fwrite(md, sizeof(md), 1, fr) != 1 || fwrite(&og.params, sizeof(og.params), 1, fr) != 1 ||
            fwrite(og.origins.data(), sizeof(double), og.origins.size(), fr) != og.origins.size() ||
            fwrite(og.dirs.data(), sizeof(double), og.dirs.size(), fr) != og.dirs.size() || fclose(fr) != 0) {
          perror("occ-rays");
          return 1;
        }
      }
      nav = og;
    }
    if (!ter_prefix.empty() && !run_terrain(nav)) return 1;
    if (!cm_prefix.empty()) {
      const vina_gpu::Costmap cm = node.costmap(nav, cm_inscribed, cm_inflation, cm_scaling, 0, true);
      if (!vina_gpu::write_costmap(cm_prefix, cm)) {
        perror("costmap");
        return 1;
      }
      const vg_clr_summary& cs = cm.summary;
      fprintf(stderr, "costmap: inscribed %g m, inflation %g m, scaling %g /m: %lld obstacles, %lld lethal, %lld inscribed, %lld inflated, %lld free, %lld no information; max dist2 %lld\n",
              cm_inscribed, cm_inflation, cm_scaling, (long long)cs.n_obstacles, (long long)cs.cells_lethal,
              (long long)cs.cells_inscribed, (long long)cs.cells_inflated, (long long)cs.cells_free,
              (long long)cs.cells_no_info, (long long)cs.max_dist2);
      if (!plan_s.empty()) {
        if (from_s.empty()) {
          if (node.tum_rows().empty()) {
            fprintf(stderr, "plan: no pose to start from; give --from\n");
            return 1;
          }
          plan_from[0] = node.tum_rows().back().p[0], plan_from[1] = node.tum_rows().back().p[1];
        }
        const vina_gpu::Plan pl = node.plan(plan_goal, plan_from, nullptr, cm.nx * cm.ny < 65536 ? cm.nx * cm.ny : 65536, true);
        FILE* fp = fopen(plan_csv.c_str(), "w");
        if (!fp) {
          perror("path");
          return 1;
        }
        for (size_t k = 0; k < pl.cells.size(); k++)
          fprintf(fp, "%.17g,%.17g,%u\n", pl.xy[2 * k], pl.xy[2 * k + 1], pl.pot[k]);
        if (fclose(fp) != 0) {
          perror("path");
          return 1;
        }
        static const char* const names[] = {"REACHED", "NO_PATH", "TRUNCATED", "STUCK"};
        printf("plan: %s, %d cells, cost %lld, from %.17g %.17g to %.17g %.17g; %lld of %lld passable cells reached\n",
               names[pl.status & 3], (int)pl.cells.size(), (long long)pl.cost, plan_from[0], plan_from[1], plan_goal[0],
               plan_goal[1], (long long)pl.summary.cells_reached, (long long)pl.summary.cells_passable);
      }
      if (!fr_csv.empty()) {
        const vina_gpu::LioCore::Frontiers fs = node.frontiers(!plan_s.empty());
        FILE* ff = fopen(fr_csv.c_str(), "w");
        if (!ff) {
          perror("frontiers");
          return 1;
        }
        for (const int k : fs.order()) {
          const vg_frontier_rec& r = fs.recs[(size_t)k];
          double best[2] = {NAN, NAN};
          if (r.best_cell >= 0) node.cell_xy(r.best_cell, best);
          fprintf(ff, "%d,%d,%.17g,%.17g,%.17g,%.17g,%u\n", r.label, r.size,
                  cm.x0 + ((double)r.sum_x / r.size + 0.5) * cm.res, cm.y0 + ((double)r.sum_y / r.size + 0.5) * cm.res,
                  best[0], best[1], r.best_pot);
        }
        if (fclose(ff) != 0) {
          perror("frontiers");
          return 1;
        }
        printf("frontiers: %lld kept of %lld, %lld cells\n", (long long)fs.summary.n_kept,
               (long long)fs.summary.n_components, (long long)fs.summary.n_frontier_cells);
        if (!vg_csv.empty()) {
          FILE* fv = fopen(vg_csv.c_str(), "w");
          if (!fv) {
            perror("view-gain");
            return 1;
          }
          size_t rows = 0;
          long long in_view = 0;
          int radius = 0;
          if (!fs.recs.empty()) {  // (vg_view_gain takes at least one viewpoint)
            const vina_gpu::LioCore::ViewGain vw = node.frontier_gain(fs, view_radius, view_max_unknown);
            for (const int k : vw.order(vina_gpu::NodeCore::frontier_pots(fs))) {
              const vg_frontier_rec& r = fs.recs[(size_t)k];
              const vg_view_rec& v = vw.recs[(size_t)k];
              double best[2];
              node.cell_xy(r.best_cell, best);
              fprintf(fv, "%d,%.17g,%.17g,%u,%d,%d,%d,%d\n", r.label, best[0], best[1], r.best_pot, v.n_unknown, v.n_free,
                      v.n_occupied, v.n_rays_open);
              rows++;
            }
            in_view = (long long)vw.summary.unknown_seen;
            radius = (int)(vw.summary.n_ok ? vw.summary.rays / vw.summary.n_ok / 8 : 0);
          }
          if (fclose(fv) != 0) {
            perror("view-gain");
            return 1;
          }
          printf("view gain: %zu of %zu frontiers, radius %d cells, %lld unknown cells in view\n", rows, fs.recs.size(),
                 radius, in_view);
        }
      }
    }
    if (live) {
      vg_live_params lp = {};
      lp.z_lo = -0.5, lp.z_hi = 0.5, lp.r_min = 0.5, lp.mark_max = 8.0, lp.clear_max = 10.0;
      lp.persist = live_persist, lp.flags = 1;
      node.live_begin(nav, lp, true);
      vina_gpu::NodeCore::LiveCostmap lc;
      FILE* fl = live_scans_file.empty() ? nullptr : fopen(live_scans_file.c_str(), "wb");
      if (!live_scans_file.empty() && !fl) {
        perror("live-scans");
        return 1;
      }
      for (size_t k = 0; k < live_scans.size(); k++) {
        const LiveScan& ls = live_scans[k];
        const int32_t n32 = (int32_t)(ls.xyz.size() / 3);
        if (fl && (fwrite(&n32, sizeof(n32), 1, fl) != 1 || fwrite(ls.pose, sizeof(double), 12, fl) != 12 ||
                   fwrite(ls.xyz.data(), sizeof(float), ls.xyz.size(), fl) != ls.xyz.size())) {
          perror("live-scans");
          return 1;
        }
        if (k + 1 < live_scans.size()) node.lio().live_mark(ls.xyz.data(), n32, ls.pose);
        else lc = node.live_costmap(ls.xyz.data(), n32, ls.pose, cm_inscribed, cm_inflation, cm_scaling);
      }
      if (fl && fclose(fl) != 0) {
        perror("live-scans");
        return 1;
      }
      if (live_scans.empty()) lc = node.live_costmap(nullptr, 0, nullptr, cm_inscribed, cm_inflation, cm_scaling);
      node.live_end();
      if (!vina_gpu::write_occupancy_map(cm_prefix + ".live.grid", lc.grid) || !vina_gpu::write_costmap(cm_prefix + ".live", lc.costmap)) {
        perror("live");
        return 1;
      }
      printf("live: %d scans, %lld cells live, %lld raised over the grid\n", (int)live_scans.size(),
             (long long)lc.compose.cells_live, (long long)lc.compose.cells_raised);
    }
    const std::vector<float> w = node.scan_world();
    if (!node.write_tum(argv[2])) {
      perror("tum");
      return 1;
    }
    if (argc > 4) {  // pcl_path after the run: t x y z jour per row (the BA re-writes included)
      FILE* fp = fopen(argv[4], "w");
      if (!fp) {
        perror("path");
        return 1;
      }
      for (const vina_gpu::PoseStamped& s : node.path())
        fprintf(fp, "%.9f %.12f %.12f %.12f %.12f\n", s.t, s.p[0], s.p[1], s.p[2], s.jour);
      fclose(fp);
    }
    size_t ncmap = 0;
    if (argc > 5) {  // the last /map_cmap cloud, float32 x y z intensity
      const std::vector<float> c = node.local_map();
      ncmap = c.size() / 4;
      FILE* fc = fopen(argv[5], "wb");
      if (!fc || fwrite(c.data(), sizeof(float), c.size(), fc) != c.size()) {
        perror("cmap");
        return 1;
      }
      fclose(fc);
    }
    printf("{\"imu\": %d, \"scans\": %d, \"stepped\": %d, \"poses\": %zu, \"path\": %zu, "
           "\"last_scan_world_points\": %zu, \"cmap_points\": %zu, \"marker_records\": %zu}\n",
           n_imu, n_msg, n_step, node.tum_rows().size(), node.path().size(), w.size() / 3, ncmap, n_markers);
  } catch (const vina_gpu::Error& e) {
    fprintf(stderr, "vg_node_replay: %s (code %d)\n", e.what(), e.code);
    return 1;
  }
  fclose(f);
  return 0;
}
