"""ctypes binding of the product C-ABI (include/vina_gpu.h, lib/libvina_gpu.so).

This is the Python face of the drop-in boundary used by tests/ and bench.py. It
loads ONLY the in-tree HIP library; there is no CPU fallback — if the library
or a GPU is missing every call raises.
"""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np

from vgconfig import CConfig

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
REPO = os.path.dirname(PKG)
LIB = os.environ.get("VINA_GPU_LIB") or os.path.join(PKG, "lib", "libvina_gpu.so")
HEADER = os.path.join(REPO, "include", "vina_gpu.h")
STATE_LEN = 250
XC_LEN = 249       # a frame state (24) and its 15 x 15 covariance (DState::xc)
PROP_MAX = 48      # kPropMax: IMU samples k_scan_prop's arguments hold
MAX_WIN = 32       # kMaxWin: slots of the IMU record ring
IMU_REC = 289      # kBaImuRec
BA_MAX_W = 16      # kMaxW: rows of imuout / imures


class Capacity(ctypes.Structure):
    _fields_ = [("max_points_per_scan", ctypes.c_int), ("max_nodes", ctypes.c_int),
                ("max_fix_points", ctypes.c_int), ("hash_log2", ctypes.c_int)]


class LidarFormat(ctypes.Structure):
    """vg_lidar_format."""
    _fields_ = [("kind", ctypes.c_int), ("stride", ctypes.c_int), ("off_x", ctypes.c_int), ("off_y", ctypes.c_int),
                ("off_z", ctypes.c_int), ("off_intensity", ctypes.c_int), ("off_time", ctypes.c_int),
                ("point_filter_num", ctypes.c_int), ("blind", ctypes.c_double), ("omega_l", ctypes.c_double),
                ("time_base", ctypes.c_double)]


class ScanDev(ctypes.Structure):
    _fields_ = [("d_x", ctypes.c_void_p), ("d_y", ctypes.c_void_p), ("d_z", ctypes.c_void_p),
                ("d_intensity", ctypes.c_void_p), ("d_time", ctypes.c_void_p), ("n", ctypes.c_int),
                ("pcl_beg_time", ctypes.c_double), ("pcl_end_time", ctypes.c_double),
                ("imu", ctypes.POINTER(ctypes.c_double)), ("m", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [("n_raw", ctypes.c_int), ("n_ds", ctypes.c_int), ("iekf_iters", ctypes.c_int),
                ("iekf_matches", ctypes.c_int * 4), ("roots_new", ctypes.c_int), ("n_slide", ctypes.c_int),
                ("n_factors", ctypes.c_int), ("ba_iters", ctypes.c_int), ("degenerate", ctypes.c_int),
                ("nodes_used", ctypes.c_int), ("fix_used", ctypes.c_int), ("plane_updates", ctypes.c_int),
                ("fix_full", ctypes.c_int), ("iekf_planes", ctypes.c_int * 4), ("v_ins", ctypes.c_int),
                ("ba_hess", ctypes.c_int), ("init_phase", ctypes.c_int), ("init_rounds", ctypes.c_int),
                ("init_valid", ctypes.c_int), ("iekf_points", ctypes.c_int)]


class VgPlaneMarker(ctypes.Structure):
    """vg_plane_marker (include/vina_gpu.h): one record of the /voxel_plane + /voxel_normal markers."""
    _fields_ = [("voxel_center", ctypes.c_double * 3), ("quater_length", ctypes.c_double),
                ("center", ctypes.c_double * 3), ("normal", ctypes.c_double * 3), ("quat", ctypes.c_double * 4),
                ("plane_scale", ctypes.c_double * 3), ("tip", ctypes.c_double * 3),
                ("normal_scale", ctypes.c_double * 3), ("eig", ctypes.c_double * 3), ("trace", ctypes.c_double),
                ("rgba", ctypes.c_float * 4), ("id", ctypes.c_int32), ("action", ctypes.c_int32),
                ("layer", ctypes.c_int32), ("flags", ctypes.c_int32)]


class PoseScore(ctypes.Structure):
    """vg_pose_score (include/vina_gpu.h): one hypothesis' record, 80 bytes."""
    _fields_ = [("matches", ctypes.c_int32), ("in_map", ctypes.c_int32), ("cost", ctypes.c_double),
                ("sum_abs", ctypes.c_double), ("nn", ctypes.c_double * 6), ("reserved", ctypes.c_double)]


class PointMatch(ctypes.Structure):
    """vg_point_match: vg_score_poses' per-point record, 24 bytes."""
    _fields_ = [("leaf", ctypes.c_int32), ("flag", ctypes.c_int32), ("r", ctypes.c_double),
                ("sigma_d", ctypes.c_double)]


class RelocParams(ctypes.Structure):
    """vg_reloc_params."""
    _fields_ = [("half_xy", ctypes.c_double), ("step_xy", ctypes.c_double), ("half_z", ctypes.c_double),
                ("step_z", ctypes.c_double), ("half_yaw", ctypes.c_double), ("step_yaw", ctypes.c_double),
                ("refine_top", ctypes.c_int), ("refine_iters", ctypes.c_int), ("min_match_ratio", ctypes.c_double),
                ("reserved", ctypes.c_double * 4)]


POSE_SCORE_DTYPE = np.dtype([("matches", "<i4"), ("in_map", "<i4"), ("cost", "<f8"), ("sum_abs", "<f8"),
                             ("nn", "<f8", 6), ("reserved", "<f8")])
POINT_MATCH_DTYPE = np.dtype([("leaf", "<i4"), ("flag", "<i4"), ("r", "<f8"), ("sigma_d", "<f8")])
SCORE_MAX_POSES = 65536


class RayParams(ctypes.Structure):
    """vg_ray_params."""
    _fields_ = [("t_min", ctypes.c_double), ("t_max", ctypes.c_double), ("min_cos", ctypes.c_double),
                ("max_steps", ctypes.c_int), ("pad", ctypes.c_int), ("reserved", ctypes.c_double * 4)]


class RayHit(ctypes.Structure):
    """vg_ray_hit: one ray's record, 64 bytes."""
    _fields_ = [("range", ctypes.c_double), ("var", ctypes.c_double), ("normal", ctypes.c_double * 3),
                ("ndotd", ctypes.c_double), ("leaf", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("reserved", ctypes.c_double)]


class DiffParams(ctypes.Structure):
    """vg_diff_params."""
    _fields_ = [("ray", RayParams), ("gate_sigma", ctypes.c_double), ("gate_floor", ctypes.c_double),
                ("reserved", ctypes.c_double * 4)]


class DiffPoint(ctypes.Structure):
    """vg_diff_point: vg_scan_diff's per-point record, 32 bytes."""
    _fields_ = [("cls", ctypes.c_int32), ("leaf", ctypes.c_int32), ("r_meas", ctypes.c_double),
                ("r_map", ctypes.c_double), ("gate", ctypes.c_double)]


class DiffSummary(ctypes.Structure):
    """vg_diff_summary."""
    _fields_ = [("n", ctypes.c_int32 * 4), ("n_truncated", ctypes.c_int32), ("n_occupied_unknown", ctypes.c_int32),
                ("sum_abs_consistent", ctypes.c_double), ("reserved", ctypes.c_double * 3)]


class InfoParams(ctypes.Structure):
    """vg_info_params, 112 bytes."""
    _fields_ = [("ray", RayParams), ("floor_var", ctypes.c_double), ("min_hits", ctypes.c_int), ("pad", ctypes.c_int),
                ("reserved", ctypes.c_double * 4)]


class InfoRec(ctypes.Structure):
    """vg_info_rec: one place's (one scan's) information record, 416 bytes."""
    _fields_ = [("H", ctypes.c_double * 36), ("eig_t", ctypes.c_double * 3), ("eig_r", ctypes.c_double * 3),
                ("dir_t", ctypes.c_double * 3), ("dir_r", ctypes.c_double * 3), ("sum_w", ctypes.c_double),
                ("reserved", ctypes.c_double), ("n_rays", ctypes.c_int32), ("n_hits", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("pad", ctypes.c_int32)]


class OccParams(ctypes.Structure):
    """vg_occ_params, 176 bytes."""
    _fields_ = [("ray", RayParams), ("x0", ctypes.c_double), ("y0", ctypes.c_double), ("res", ctypes.c_double),
                ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("z_lo", ctypes.c_double), ("z_hi", ctypes.c_double),
                ("free_on_miss", ctypes.c_double), ("min_occ", ctypes.c_int), ("min_free", ctypes.c_int),
                ("occ_ratio", ctypes.c_double), ("flags", ctypes.c_int), ("pad", ctypes.c_int),
                ("reserved", ctypes.c_double * 4)]


class OccSummary(ctypes.Structure):
    """vg_occ_summary, 128 bytes."""
    _fields_ = [("n_rays", ctypes.c_int64), ("n_hits", ctypes.c_int64), ("n_hits_in_band", ctypes.c_int64),
                ("n_truncated", ctypes.c_int64), ("n_occupied_unknown", ctypes.c_int64), ("n_invalid", ctypes.c_int64),
                ("free_marks", ctypes.c_int64), ("occ_marks", ctypes.c_int64), ("cells_free", ctypes.c_int64),
                ("cells_occupied", ctypes.c_int64), ("cells_unknown", ctypes.c_int64), ("reserved", ctypes.c_int64 * 5)]


class TerrainParams(ctypes.Structure):
    """vg_terrain_params, 224 bytes."""
    _fields_ = [("ray", RayParams), ("x0", ctypes.c_double), ("y0", ctypes.c_double), ("res", ctypes.c_double),
                ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("free_on_miss", ctypes.c_double),
                ("min_occ", ctypes.c_int), ("min_free", ctypes.c_int), ("occ_ratio", ctypes.c_double),
                ("flags", ctypes.c_int), ("min_ground", ctypes.c_int), ("z_res", ctypes.c_double),
                ("up_min", ctypes.c_double), ("g_lo", ctypes.c_double), ("g_hi", ctypes.c_double),
                ("clear_lo", ctypes.c_double), ("clear_hi", ctypes.c_double), ("sensor_height", ctypes.c_double),
                ("step_max", ctypes.c_double), ("reserved", ctypes.c_double * 4)]


class TerrainSummary(ctypes.Structure):
    """vg_terrain_summary, 128 bytes."""
    _fields_ = [("n_rays", ctypes.c_int64), ("n_hits", ctypes.c_int64), ("n_hits_in_band", ctypes.c_int64),
                ("n_truncated", ctypes.c_int64), ("n_occupied_unknown", ctypes.c_int64), ("n_invalid", ctypes.c_int64),
                ("n_ground_hits", ctypes.c_int64), ("n_out_of_range", ctypes.c_int64), ("cells_ground", ctypes.c_int64),
                ("max_step", ctypes.c_int32), ("max_spread", ctypes.c_int32), ("cells_step_lethal", ctypes.c_int64),
                ("free_marks", ctypes.c_int64), ("occ_marks", ctypes.c_int64), ("cells_free", ctypes.c_int64),
                ("cells_occupied", ctypes.c_int64), ("cells_unknown", ctypes.c_int64)]


class ClrParams(ctypes.Structure):
    """vg_clr_params, 80 bytes."""
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("res", ctypes.c_double), ("flags", ctypes.c_int),
                ("pad", ctypes.c_int), ("inscribed_radius", ctypes.c_double), ("inflation_radius", ctypes.c_double),
                ("cost_scaling", ctypes.c_double), ("reserved", ctypes.c_double * 4)]


class ClrSummary(ctypes.Structure):
    """vg_clr_summary, 128 bytes."""
    _fields_ = [("n_obstacles", ctypes.c_int64), ("n_unknown", ctypes.c_int64), ("cells_lethal", ctypes.c_int64),
                ("cells_inscribed", ctypes.c_int64), ("cells_inflated", ctypes.c_int64), ("cells_free", ctypes.c_int64),
                ("cells_no_info", ctypes.c_int64), ("max_dist2", ctypes.c_int64), ("reserved", ctypes.c_int64 * 8)]


class NavParams(ctypes.Structure):
    """vg_nav_params, 64 bytes."""
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("flags", ctypes.c_int), ("neutral", ctypes.c_int),
                ("lethal_from", ctypes.c_int), ("unknown_as", ctypes.c_int), ("factor", ctypes.c_double),
                ("reserved", ctypes.c_double * 4)]


class NavSummary(ctypes.Structure):
    """vg_nav_summary, 128 bytes."""
    _fields_ = [("n_goals_used", ctypes.c_int64), ("n_goals_ignored", ctypes.c_int64), ("cells_passable", ctypes.c_int64),
                ("cells_reached", ctypes.c_int64), ("cells_saturated", ctypes.c_int64), ("max_pot", ctypes.c_int64),
                ("rounds", ctypes.c_int64), ("tile_runs", ctypes.c_int64), ("reserved", ctypes.c_int64 * 8)]


class FrontierParams(ctypes.Structure):
    """vg_frontier_params, 56 bytes."""
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("flags", ctypes.c_int), ("cost_max", ctypes.c_int),
                ("min_size", ctypes.c_int), ("pad", ctypes.c_int), ("reserved", ctypes.c_double * 4)]


class FrontierRec(ctypes.Structure):
    """vg_frontier_rec, 64 bytes (FRONTIER_REC is the same layout as a numpy dtype)."""
    _fields_ = [("label", ctypes.c_int32), ("size", ctypes.c_int32), ("x_min", ctypes.c_int32), ("y_min", ctypes.c_int32),
                ("x_max", ctypes.c_int32), ("y_max", ctypes.c_int32), ("sum_x", ctypes.c_int64), ("sum_y", ctypes.c_int64),
                ("best_cell", ctypes.c_int32), ("best_pot", ctypes.c_uint32), ("reserved", ctypes.c_int64 * 2)]


class FrontierSummary(ctypes.Structure):
    """vg_frontier_summary, 128 bytes."""
    _fields_ = [("n_frontier_cells", ctypes.c_int64), ("n_components", ctypes.c_int64), ("n_kept", ctypes.c_int64),
                ("n_written", ctypes.c_int64), ("max_size", ctypes.c_int64), ("cells_free", ctypes.c_int64),
                ("cells_unknown", ctypes.c_int64), ("n_rejected_cost", ctypes.c_int64),
                ("n_rejected_unreached", ctypes.c_int64), ("reserved", ctypes.c_int64 * 7)]


FRONTIER_REC = np.dtype([("label", "<i4"), ("size", "<i4"), ("x_min", "<i4"), ("y_min", "<i4"), ("x_max", "<i4"),
                         ("y_max", "<i4"), ("sum_x", "<i8"), ("sum_y", "<i8"), ("best_cell", "<i4"), ("best_pot", "<u4"),
                         ("reserved", "<i8", (2,))])
FRONTIER_MAX_RECORDS = 65536


class ViewParams(ctypes.Structure):
    """vg_view_params, 56 bytes."""
    _fields_ = [("nx", ctypes.c_int), ("ny", ctypes.c_int), ("radius", ctypes.c_int), ("max_unknown", ctypes.c_int),
                ("flags", ctypes.c_int), ("pad", ctypes.c_int), ("reserved", ctypes.c_double * 4)]


class ViewRec(ctypes.Structure):
    """vg_view_rec, 32 bytes (VIEW_REC is the same layout as a numpy dtype)."""
    _fields_ = [("ix", ctypes.c_int32), ("iy", ctypes.c_int32), ("status", ctypes.c_int32), ("n_visible", ctypes.c_int32),
                ("n_unknown", ctypes.c_int32), ("n_free", ctypes.c_int32), ("n_occupied", ctypes.c_int32),
                ("n_rays_open", ctypes.c_int32)]


class ViewSummary(ctypes.Structure):
    """vg_view_summary, 128 bytes."""
    _fields_ = [("n_views", ctypes.c_int64), ("n_ok", ctypes.c_int64), ("n_outside", ctypes.c_int64),
                ("n_blocked", ctypes.c_int64), ("rays", ctypes.c_int64), ("max_unknown_seen", ctypes.c_int64),
                ("best_view", ctypes.c_int64), ("cells_seen", ctypes.c_int64), ("unknown_seen", ctypes.c_int64),
                ("reserved", ctypes.c_int64 * 7)]


VIEW_REC = np.dtype([("ix", "<i4"), ("iy", "<i4"), ("status", "<i4"), ("n_visible", "<i4"), ("n_unknown", "<i4"),
                     ("n_free", "<i4"), ("n_occupied", "<i4"), ("n_rays_open", "<i4")])
VIEW_MAX_RADIUS = 255
VIEW_OK, VIEW_OUTSIDE, VIEW_BLOCKED = 0, 1, 2
NAV_SAT,NAV_UNREACHED = 0xFFFFFFFE, 0xFFFFFFFF
NAV_K_ORTHO, NAV_K_DIAG = 12, 17
NAV_MAX_POINTS, NAV_MAX_PATH_CELLS = 65536, 1 << 27
NAV_REACHED, NAV_NO_PATH, NAV_TRUNCATED, NAV_STUCK = 0, 1, 2, 3
NAV_SCHEDULING = ("rounds", "tile_runs")    # the summary's fields that depend on scheduling
CLR_NONE = 2 ** 31 - 1
CLR_MAX_SIDE = 32768
COST_FREE, COST_INSCRIBED, COST_LETHAL, COST_NO_INFO = 0, 253, 254, 255
OCC_UNKNOWN, OCC_FREE, OCC_OCCUPIED = -1, 0, 100
OCC_MAX_CELLS = 1 << 24
OCC_PGM = {OCC_OCCUPIED: 0, OCC_FREE: 254, OCC_UNKNOWN: 205}   # map_server's grey levels


def occ_params(x0=0.0, y0=0.0, res=0.0, nx=0, ny=0, z_lo=-0.3, z_hi=1.0, free_on_miss=0.0, min_occ=0, min_free=0,
               occ_ratio=0.0, flags=0, **ray):
    """vg_occ_params; the band defaults to 0.3 m below .. 1 m above the sensor, zeros elsewhere take the
    library's defaults (one mark classifies a cell, no ratio test, a miss marks nothing)."""
    p = OccParams()
    p.ray = ray_params(**ray)
    p.x0, p.y0, p.res, p.nx, p.ny = x0, y0, res, nx, ny
    p.z_lo, p.z_hi, p.free_on_miss = z_lo, z_hi, free_on_miss
    p.min_occ, p.min_free, p.occ_ratio, p.flags = min_occ, min_free, occ_ratio, flags
    return p


TER_NONE = -2 ** 31


def terrain_params(x0=0.0, y0=0.0, res=0.0, nx=0, ny=0, free_on_miss=0.0, min_occ=0, min_free=0, occ_ratio=0.0,
                   flags=0, min_ground=0, z_res=0.0, up_min=0.0, g_lo=0.0, g_hi=0.0, clear_lo=0.0, clear_hi=0.0,
                   sensor_height=0.0, step_max=0.0, **ray):
    """vg_terrain_params; zeros take the library's defaults (a 1 mm height quantum, planes within 35 degrees of
    level as ground, ground hits 3 m .. 0.1 m below the sensor, obstacles 0.15 .. 1.5 m above the ground)."""
    p = TerrainParams()
    p.ray = ray_params(**ray)
    p.x0, p.y0, p.res, p.nx, p.ny = x0, y0, res, nx, ny
    p.free_on_miss, p.min_occ, p.min_free, p.occ_ratio = free_on_miss, min_occ, min_free, occ_ratio
    p.flags, p.min_ground, p.z_res, p.up_min = flags, min_ground, z_res, up_min
    p.g_lo, p.g_hi, p.clear_lo, p.clear_hi = g_lo, g_hi, clear_lo, clear_hi
    p.sensor_height, p.step_max = sensor_height, step_max
    return p


def write_terrain(prefix, elev, x0, y0, res, z_res):
    """The elevation (int32 [ny, nx], TER_NONE where there is none) as raw little-endian int32 in prefix.elev,
    row iy first as in memory, beside prefix.elev.yaml with the grid's shape, origin, res and z_res (a
    height in metres is elev z_res)."""
    e = np.ascontiguousarray(elev, dtype="<i4")
    with open(prefix + ".elev", "wb") as f:
        f.write(e.tobytes())
    with open(prefix + ".elev.yaml", "w") as f:
        f.write("data: %s\nnx: %d\nny: %d\nresolution: %r\norigin: [%r, %r, 0]\nz_res: %r\nnone: %d\n"
                % (os.path.basename(prefix) + ".elev", e.shape[1], e.shape[0], float(res), float(x0), float(y0),
                   float(z_res), TER_NONE))


def read_terrain(prefix):
    """(elev int32 [ny, nx], x0, y0, res, z_res) back from write_terrain's (or vg_node_replay --terrain's) pair."""
    meta = {}
    for ln in open(prefix + ".elev.yaml"):
        k, _, v = ln.partition(":")
        meta[k.strip()] = v.strip()
    org = [float(x) for x in meta["origin"].strip("[]").split(",")]
    nx, ny = int(meta["nx"]), int(meta["ny"])
    raw = open(os.path.join(os.path.dirname(prefix), meta["data"]), "rb").read()
    e = np.frombuffer(raw, dtype="<i4", count=nx * ny).reshape(ny, nx).astype(np.int32)
    return e, org[0], org[1], float(meta["resolution"]), float(meta["z_res"])


def occupancy_dirs(n_az=360, elevations_deg=(-10, 0, 10)):
    """(len(elevations_deg) * n_az, 3) unit directions, entry e * n_az + a: azimuth 2 pi a / n_az about the
    world's z at each elevation: the horizontal-biased fan Context.occupancy casts by default (no device)."""
    az = 2.0 * np.pi * np.arange(int(n_az)) / int(n_az)
    el = np.deg2rad(np.asarray(elevations_deg, dtype=np.float64).reshape(-1))
    E, A = np.meshgrid(el, az, indexing="ij")
    return np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)


def grid_around(positions, res, margin):
    """(x0, y0, nx, ny) of the grid of cell edge res that covers the positions' x, y bounds grown by margin
    on every side; x0 and y0 are whole multiples of res."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        raise ValueError("grid_around: no positions")
    lo, hi = p[:, :2].min(axis=0) - margin, p[:, :2].max(axis=0) + margin
    k0 = np.floor(lo / res)
    n = np.maximum(np.ceil(hi / res) - k0, 1.0)
    return float(k0[0] * res), float(k0[1] * res), int(n[0]), int(n[1])


def write_occupancy(prefix, grid, x0, y0, res):
    """The grid (int8 [ny, nx], OCC_*) as map_server's pair: prefix.pgm (P5, the first row at the largest y,
    occupied 0 / free 254 / unknown 205) and prefix.yaml."""
    g = np.asarray(grid, dtype=np.int8)
    px = np.full(g.shape, OCC_PGM[OCC_UNKNOWN], dtype=np.uint8)
    px[g == OCC_FREE] = OCC_PGM[OCC_FREE]
    px[g == OCC_OCCUPIED] = OCC_PGM[OCC_OCCUPIED]
    with open(prefix + ".pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]))
        f.write(np.ascontiguousarray(px[::-1]).tobytes())
    with open(prefix + ".yaml", "w") as f:
        f.write("image: %s\nresolution: %r\norigin: [%r, %r, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
                % (os.path.basename(prefix) + ".pgm", float(res), float(x0), float(y0)))


def write_costmap(prefix, cost, x0, y0, res):
    """The cost (uint8 [ny, nx], COST_*) as raw bytes in prefix.pgm (P5, the first row at the largest y) and
    write_occupancy's prefix.yaml."""
    c = np.asarray(cost, dtype=np.uint8)
    with open(prefix + ".pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (c.shape[1], c.shape[0]))
        f.write(np.ascontiguousarray(c[::-1]).tobytes())
    with open(prefix + ".yaml", "w") as f:
        f.write("image: %s\nresolution: %r\norigin: [%r, %r, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
                % (os.path.basename(prefix) + ".pgm", float(res), float(x0), float(y0)))


def nav_trav_table(flags=0, neutral=0, lethal_from=0, unknown_as=0, factor=0.0):
    """vg_navfn's default traversal table (uint16 [256], 0 impassable) of these parameters, zeros taking nav2's
    values, as the library fills it (no device); ValueError where the library returns VG_E_ARG."""
    if (flags & ~1 or neutral < 0 or not 0 <= lethal_from <= 255 or not 0 <= unknown_as <= 254
            or not (factor >= 0.0 and math.isfinite(factor))):
        raise ValueError("nav_trav_table: a parameter out of range")
    neutral, lethal_from, factor = neutral or 50, lethal_from or 253, factor or 0.8
    t = [neutral + int(math.floor(factor * c)) if c < min(lethal_from, 255) else 0 for c in range(256)]
    if max(t) > 65535:
        raise ValueError("nav_trav_table: an entry overflows uint16")
    if flags & 1:
        t[255] = t[unknown_as]
    return np.array(t, dtype=np.uint16)


def frontier_order(recs):
    """The indices of the frontier records (FRONTIER_REC) in the order to visit them: with best_cell >= 0 (the
    reach test was on) by ascending (best_pot, label), the cheapest to drive to first; otherwise by descending
    size, then ascending label."""
    r = np.asarray(recs)
    if r.size and (r["best_cell"] >= 0).all():
        return np.lexsort((r["label"], r["best_pot"]))
    return np.lexsort((r["label"], -r["size"].astype(np.int64)))


def view_order(view_recs, pots=None, min_gain=1):
    """The indices of the view records (VIEW_REC) worth visiting, best first: those with status VIEW_OK and
    n_unknown >= min_gain. With pots (uint32 per record, e.g. the frontier records' best_pot) a comes before b when
    n_unknown_a (pot_b + 1) > n_unknown_b (pot_a + 1), the gain per cost in exact integers (the products stay
    below 2^50); ties go to the smaller pot, then the smaller index. Without pots: by descending n_unknown, then
    index."""
    r = np.asarray(view_recs)
    keep = [int(i) for i in np.flatnonzero((r["status"] == VIEW_OK) & (r["n_unknown"] >= min_gain))]
    gain = [int(v) for v in r["n_unknown"]]
    if pots is None:
        return np.array(sorted(keep, key=lambda i: (-gain[i], i)), dtype=np.int64)
    pot = [int(v) for v in np.asarray(pots, dtype=np.uint32).reshape(-1)]
    if len(pot) != len(gain):
        raise ValueError("view_order: one pot per record")

    def cmp(a, b):
        lhs, rhs = gain[a] * (pot[b] + 1), gain[b] * (pot[a] + 1)
        if lhs != rhs:
            return -1 if lhs > rhs else 1
        return -1 if (pot[a], a) < (pot[b], b) else 1

    return np.array(sorted(keep, key=functools.cmp_to_key(cmp)), dtype=np.int64)


def cells_to_world(cells, nx, x0, y0, res):
    """(n, 2) world x, y of the centres of the cells with linear indices `cells` (iy nx + ix) of a grid whose
    cell (0, 0) has its corner at (x0, y0)."""
    c = np.asarray(cells, dtype=np.int64).reshape(-1)
    return np.stack([x0 + (c % nx + 0.5) * res, y0 + (c // nx + 0.5) * res], axis=1)


def read_costmap(prefix):
    """(cost uint8 [ny, nx], x0, y0, res) back from write_costmap's (or vg_node_replay --costmap's) pair."""
    meta = {}
    for ln in open(prefix + ".yaml"):
        k, _, v = ln.partition(":")
        meta[k.strip()] = v.strip()
    org = [float(x) for x in meta["origin"].strip("[]").split(",")]
    raw = open(os.path.join(os.path.dirname(prefix), meta["image"]), "rb").read()
    m = re.match(rb"P5\s+(\d+)\s+(\d+)\s+255\s", raw)
    nx, ny = int(m.group(1)), int(m.group(2))
    c = np.frombuffer(raw, dtype=np.uint8, offset=m.end(), count=nx * ny).reshape(ny, nx)[::-1]
    return np.ascontiguousarray(c), org[0], org[1], float(meta["resolution"])


def read_occupancy(prefix):
    """(grid int8 [ny, nx], x0, y0, res) back from write_occupancy's (or vg_node_replay --occupancy's) pair."""
    meta = {}
    for ln in open(prefix + ".yaml"):
        k, _, v = ln.partition(":")
        meta[k.strip()] = v.strip()
    org = [float(x) for x in meta["origin"].strip("[]").split(",")]
    raw = open(os.path.join(os.path.dirname(prefix), meta["image"]), "rb").read()
    m = re.match(rb"P5\s+(\d+)\s+(\d+)\s+255\s", raw)
    nx, ny = int(m.group(1)), int(m.group(2))
    px = np.frombuffer(raw, dtype=np.uint8, offset=m.end(), count=nx * ny).reshape(ny, nx)[::-1]
    g = np.full((ny, nx), OCC_UNKNOWN, dtype=np.int8)
    g[px == OCC_PGM[OCC_FREE]] = OCC_FREE
    g[px == OCC_PGM[OCC_OCCUPIED]] = OCC_OCCUPIED
    return g, org[0], org[1], float(meta["resolution"])


class ChangeParams(ctypes.Structure):
    """vg_change_params."""
    _fields_ = [("diff", DiffParams), ("cell", ctypes.c_double), ("cell_hash_log2", ctypes.c_int),
                ("pad", ctypes.c_int), ("reserved", ctypes.c_double * 4)]


class ChangeQuery(ctypes.Structure):
    """vg_change_query."""
    _fields_ = [("min_obs", ctypes.c_int), ("min_scans", ctypes.c_int), ("vanished_ratio", ctypes.c_double),
                ("flags", ctypes.c_int), ("pad", ctypes.c_int), ("reserved", ctypes.c_double * 4)]


class ChangeTotals(ctypes.Structure):
    """vg_change_totals, 128 bytes."""
    _fields_ = [("calls", ctypes.c_int64), ("points", ctypes.c_int64), ("n", ctypes.c_int64 * 4),
                ("cells_used", ctypes.c_int64), ("dropped", ctypes.c_int64), ("out_of_range", ctypes.c_int64),
                ("leaves_touched", ctypes.c_int64), ("reserved", ctypes.c_int64 * 6)]


class LiveParams(ctypes.Structure):
    """vg_live_params, 224 bytes."""
    _fields_ = [("diff", DiffParams), ("x0", ctypes.c_double), ("y0", ctypes.c_double), ("res", ctypes.c_double),
                ("nx", ctypes.c_int), ("ny", ctypes.c_int), ("z_lo", ctypes.c_double), ("z_hi", ctypes.c_double),
                ("r_min", ctypes.c_double), ("mark_max", ctypes.c_double), ("clear_max", ctypes.c_double),
                ("persist", ctypes.c_int), ("flags", ctypes.c_int), ("reserved", ctypes.c_double * 4)]


class LiveSummary(ctypes.Structure):
    """vg_live_summary, 128 bytes."""
    _fields_ = [("n", ctypes.c_int64 * 4), ("n_obstacle", ctypes.c_int64), ("marks_dropped", ctypes.c_int64),
                ("n_beams", ctypes.c_int64), ("cells_live", ctypes.c_int64), ("cells_cleared", ctypes.c_int64),
                ("cells_free", ctypes.c_int64), ("cells_occupied", ctypes.c_int64), ("cells_unknown", ctypes.c_int64),
                ("cells_raised", ctypes.c_int64), ("stamp", ctypes.c_int64), ("calls", ctypes.c_int64),
                ("reserved", ctypes.c_int64)]


# vg_live_point (32 bytes) as a numpy record type, and its flags
LIVE_POINT_DTYPE = np.dtype([("cls", "<i4"), ("flags", "<i4"), ("ax", "<i4"), ("ay", "<i4"), ("bx", "<i4"),
                             ("by", "<i4"), ("mx", "<i4"), ("my", "<i4")])
LIVE_MARKS, LIVE_CLEARS, LIVE_IN_BAND, LIVE_CUT, LIVE_LEFT_BAND = 1, 2, 4, 8, 16


def live_params(x0=0.0, y0=0.0, res=0.0, nx=0, ny=0, z_lo=0.0, z_hi=0.0, r_min=0.0, mark_max=0.0, clear_max=0.0,
                persist=0, flags=0, **diff):
    """vg_live_params; zeros take the defaults (band -1 .. 1 m about the sensor, no range limits on marks, beams
    cleared to 4096 cells or mark_max, marks kept for ever); diff: diff_params."""
    p = LiveParams()
    p.diff = diff_params(**diff)
    p.x0, p.y0, p.res, p.nx, p.ny = x0, y0, res, nx, ny
    p.z_lo, p.z_hi, p.r_min, p.mark_max, p.clear_max = z_lo, z_hi, r_min, mark_max, clear_max
    p.persist, p.flags = persist, flags
    return p


def _live_summary(s):
    return {k: (list(getattr(s, k)) if k == "n" else int(getattr(s, k))) for k, _ in LiveSummary._fields_
            if k != "reserved"}


class PlacesParams(ctypes.Structure):
    """vg_places_params, 144 bytes."""
    _fields_ = [("n_az", ctypes.c_int), ("n_el", ctypes.c_int), ("el_min", ctypes.c_double),
                ("el_max", ctypes.c_double), ("t_max", ctypes.c_double), ("clip", ctypes.c_double),
                ("min_bins", ctypes.c_int), ("pad", ctypes.c_int), ("ray", RayParams),
                ("reserved", ctypes.c_double * 4)]


# vg_place_candidate (48 bytes)
PLACE_CANDIDATE_DTYPE = np.dtype([("place", "<i4"), ("shift", "<i4"), ("score", "<i4"), ("n_valid", "<i4"),
                                  ("pos", "<f8", 3), ("yaw", "<f8")])
PLACE_NONE = 2 ** 31 - 1  # an invalid place's score


def places_params(n_az=0, n_el=0, el_min=0.0, el_max=0.0, t_max=0.0, clip=0.0, min_bins=0, **ray):
    """vg_places_params; zeros take the defaults (120 x 12 bins, -+30 degrees, 60 m, clip 2 m, n_az n_el / 8)."""
    p = PlacesParams()
    p.n_az, p.n_el, p.el_min, p.el_max, p.t_max, p.clip, p.min_bins = n_az, n_el, el_min, el_max, t_max, clip, min_bins
    p.ray = ray_params(**ray)
    return p


def places_dirs(**params):
    """vg_places_dirs: the bin-centre directions (n_el * n_az, 3), entry e * n_az + a, in the descriptor's frame
    (no device). Raises VgError (-1) where a limit is exceeded."""
    p = places_params(**params)
    n = ctypes.c_int(0)
    r = lib().vg_places_dirs(ctypes.byref(p), None, 0, ctypes.byref(n))
    if r != 0:
        raise VgError("vg_places_dirs failed (%d)" % r)
    out = np.zeros((n.value, 3))
    r = lib().vg_places_dirs(ctypes.byref(p), _d(out), n.value, ctypes.byref(n))
    if r != 0:
        raise VgError("vg_places_dirs failed (%d)" % r)
    return out


def place_lattice(lo, hi, step, z):
    """(M, 3) positions on a lattice over [lo[0], hi[0]] x [lo[1], hi[1]] (both ends where the step fits) at
    height z, x fastest: sample positions for Context.places_build."""
    nx = int(np.floor((hi[0] - lo[0]) / step + 1e-9)) + 1
    ny = int(np.floor((hi[1] - lo[1]) / step + 1e-9)) + 1
    gx, gy = np.meshgrid(lo[0] + step * np.arange(nx), lo[1] + step * np.arange(ny), indexing="xy")
    return np.stack([gx.reshape(-1), gy.reshape(-1), np.full(nx * ny, float(z))], axis=1)


# vg_change_leaf (112 bytes) and vg_change_cell (56 bytes) as numpy record types
CHANGE_LEAF_DTYPE = np.dtype([("node", "<i4"), ("layer", "<i4"), ("n_consistent", "<i4"), ("n_vanished", "<i4"),
                              ("n_occluded", "<i4"), ("n_scans", "<i4"), ("flags", "<i4"), ("pad", "<i4"),
                              ("voxel_center", "<f8", 3), ("quater_length", "<f8"), ("center", "<f8", 3),
                              ("normal", "<f8", 3)])
CHANGE_CELL_DTYPE = np.dtype([("key", "<i4", 3), ("n_appeared", "<i4"), ("n_scans", "<i4"), ("flags", "<i4"),
                              ("pad", "<i4", 2), ("centroid", "<f8", 3)])

RAY_HIT_DTYPE = np.dtype([("range", "<f8"), ("var", "<f8"), ("normal", "<f8", 3), ("ndotd", "<f8"), ("leaf", "<i4"),
                          ("flags", "<i4"), ("reserved", "<f8")])
DIFF_POINT_DTYPE = np.dtype([("cls", "<i4"), ("leaf", "<i4"), ("r_meas", "<f8"), ("r_map", "<f8"), ("gate", "<f8")])
RAY_HIT, RAY_TRUNCATED, RAY_OCCUPIED, RAY_LEFT_RANGE, RAY_INVALID = 1, 2, 4, 8, 16
DIFF_UNKNOWN, DIFF_CONSISTENT, DIFF_APPEARED, DIFF_VANISHED = 0, 1, 2, 3


INFO_REC_DTYPE = np.dtype([("H", "<f8", (6, 6)), ("eig_t", "<f8", 3), ("eig_r", "<f8", 3), ("dir_t", "<f8", 3),
                           ("dir_r", "<f8", 3), ("sum_w", "<f8"), ("reserved", "<f8"), ("n_rays", "<i4"),
                           ("n_hits", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
INFO_VALID, INFO_ROT_DEGENERATE, INFO_TRANS_DEGENERATE, INFO_RAY_ENDED = 1, 2, 4, 8
INFO_MAX_DIRS = 4096


def ray_params(t_min=0.0, t_max=0.0, min_cos=0.0, max_steps=0):
    """vg_ray_params; zeros take the defaults (100 m, 0.05, 4096)."""
    p = RayParams()
    p.t_min, p.t_max, p.min_cos, p.max_steps = t_min, t_max, min_cos, max_steps
    return p


def diff_params(gate_sigma=0.0, gate_floor=0.0, **ray):
    """vg_diff_params; zeros take the defaults (3 sigma, no floor)."""
    p = DiffParams()
    p.ray = ray_params(**ray)
    p.gate_sigma, p.gate_floor = gate_sigma, gate_floor
    return p


def info_params(floor_var=0.0, min_hits=0, **ray):
    """vg_info_params; zeros take the defaults (no floor, 16 hits, ray_params' defaults)."""
    p = InfoParams()
    p.ray = ray_params(**ray)
    p.floor_var, p.min_hits = floor_var, min_hits
    return p


def reloc_params(half_xy=0.0, step_xy=0.0, half_z=0.0, step_z=0.0, half_yaw=0.0, step_yaw=0.0, refine_top=8,
                 refine_iters=8, min_match_ratio=0.5):
    p = RelocParams()
    p.half_xy, p.step_xy, p.half_z, p.step_z, p.half_yaw, p.step_yaw = half_xy, step_xy, half_z, step_z, half_yaw, step_yaw
    p.refine_top, p.refine_iters, p.min_match_ratio = refine_top, refine_iters, min_match_ratio
    return p


def reloc_grid(**params):
    """vg_reloc_grid: the hypothesis offsets (K, 4) [dx, dy, dz, dyaw] of vg_relocalize, in dispatch order
    (no device). Raises VgError (-1) for a bad window or more than 65,536 hypotheses."""
    p = reloc_params(**params)
    n = ctypes.c_int(0)
    r = lib().vg_reloc_grid(ctypes.byref(p), None, 0, ctypes.byref(n))
    if r != 0:
        raise VgError("vg_reloc_grid failed (%d)" % r)
    out = np.zeros((n.value, 4))
    r = lib().vg_reloc_grid(ctypes.byref(p), _d(out), n.value, ctypes.byref(n))
    if r != 0:
        raise VgError("vg_reloc_grid failed (%d)" % r)
    return out


# the same layout as a numpy record type (what the marker calls return)
MARKER_DTYPE = np.dtype([("voxel_center", "<f8", 3), ("quater_length", "<f8"), ("center", "<f8", 3),
                         ("normal", "<f8", 3), ("quat", "<f8", 4), ("plane_scale", "<f8", 3), ("tip", "<f8", 3),
                         ("normal_scale", "<f8", 3), ("eig", "<f8", 3), ("trace", "<f8"), ("rgba", "<f4", 4),
                         ("id", "<i4"), ("action", "<i4"), ("layer", "<i4"), ("flags", "<i4")])
MARKER_EVAL_IN = 15  # vgx_marker_eval: voxel_center 3, layer, quater_length, center 3, normal 3, trace, eig 3


def _stats_dict(s):
    return {k: (list(getattr(s, k)) if k in ("iekf_matches", "iekf_planes") else getattr(s, k))
            for k, _ in Stats._fields_}


# vg_host_allreduce_fn: int (*)(void* buf, int count, int dtype, void* user)
HOST_ALLREDUCE = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p)


def rccl_unique_id():
    buf = ctypes.create_string_buffer(128)
    r = lib().vg_rccl_unique_id(buf)
    if r != 0:
        raise VgError("vg_rccl_unique_id failed (%d)" % r)
    return buf.raw


def build(jobs=8):
    subprocess.check_call(["make", "-s", "-j%d" % jobs, "-C", PKG])


def header_symbols():
    """Every function the C-ABI header declares."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:int|void\*?|const char\*|vg_\w+\*)\s+(vg_\w+)\s*\(", txt, re.M)))


_lib = None


def _torch_first():
    """PyTorch-ROCm carries its own HIP runtime beside /opt/rocm's (which the
    library links). Both share the process's device address space, but the
    one that opens the GPU second must not be torch's: its init then reports
    "No HIP GPUs are available". Callers hand torch device buffers to the
    library, so open torch's runtime first whenever torch is installed."""
    try:
        import torch
    except ImportError:
        return
    if torch.cuda.is_available():
        torch.cuda.init()


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            raise RuntimeError("libvina_gpu.so not built: run `make -C vina-slam_amd` (no CPU fallback exists)")
        _torch_first()
        L = ctypes.CDLL(LIB)
        P = ctypes.c_void_p
        dp = ctypes.POINTER(ctypes.c_double)
        fp = ctypes.POINTER(ctypes.c_float)
        ip = ctypes.POINTER(ctypes.c_int)
        L.vg_create.argtypes = [ctypes.POINTER(CConfig), ctypes.POINTER(Capacity), ctypes.c_int, ctypes.POINTER(P)]
        L.vg_destroy.argtypes = [P]
        L.vg_last_error.argtypes = [P]
        L.vg_last_error.restype = ctypes.c_char_p
        L.vg_reset.argtypes = [P]
        L.vg_downsample.argtypes = [P, fp, fp, ctypes.c_int, ctypes.c_double, fp, ip]
        L.vg_downsample_close.argtypes = [P, fp, fp, ctypes.c_int, ctypes.c_double, fp, ip]
        L.vg_seed.argtypes = [P, dp]
        L.vg_lio_kdtree.argtypes = [P, fp, ctypes.c_int, dp, ip, ip]
        L.vg_kdmap_get.argtypes = [P, fp, ctypes.c_int, ip]
        L.vg_decode_scan.argtypes = [P, P, ctypes.c_int, ctypes.POINTER(LidarFormat), fp, fp, fp, ip]
        L.vg_sync_create.argtypes = [ctypes.c_int]
        L.vg_sync_create.restype = P
        L.vg_sync_destroy.argtypes = [P]
        L.vg_sync_push_scan.argtypes = [P, ctypes.c_double, ctypes.c_double, ctypes.c_int]
        L.vg_sync_push_imu.argtypes = [P, dp]
        L.vg_sync_pop.argtypes = [P, ip, dp, dp, dp, ctypes.c_int, ip, ip]
        L.vg_step.argtypes = [P, fp, fp, ctypes.c_int, ctypes.c_double, ctypes.c_double, dp, ctypes.c_int]
        L.vg_step_dev.argtypes = [P, P, P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_double, dp, ctypes.c_int]
        L.vg_step_deskew.argtypes = [P, fp, fp, fp, ctypes.c_int, ctypes.c_double, ctypes.c_double, dp, ctypes.c_int]
        L.vg_step_deskew_dev.argtypes = [P, P, P, P, P, P, ctypes.c_int, ctypes.c_double, ctypes.c_double, dp,
                                         ctypes.c_int]
        L.vg_get_state.argtypes = [P, dp]
        L.vg_scan_points.argtypes = [P, fp, ctypes.c_int, ip]
        L.vg_get_stats.argtypes = [P, ctypes.POINTER(Stats)]
        L.vg_stats_log.argtypes = [P, ctypes.POINTER(Stats), ctypes.c_int, ip]
        L.vg_release_far.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]
        L.vg_window_states.argtypes = [P, dp, ip]
        L.has_checkpoint = hasattr(L, "vg_checkpoint_save")  # a build older than the checkpoint (A/B runs)
        if L.has_checkpoint:
            L.vg_checkpoint_save.argtypes = [P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
            L.vg_checkpoint_load.argtypes = [P, ctypes.c_char_p]
            L.vgx_checkpoint_timed.argtypes = [P, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), dp]
        L.has_localize = hasattr(L, "vg_score_poses")  # a build older than the localisation calls (A/B runs)
        if L.has_localize:
            L.vg_set_mapping.argtypes = [P, ctypes.c_int]
            L.vg_score_poses.argtypes = [P, fp, ctypes.c_int, dp, ctypes.c_int, dp, P, P]
            L.vg_reloc_grid.argtypes = [ctypes.POINTER(RelocParams), dp, ctypes.c_int, ip]
            L.vg_relocalize.argtypes = [P, fp, ctypes.c_int, dp, ctypes.POINTER(RelocParams), ctypes.c_int, dp,
                                        ctypes.POINTER(PoseScore), ip]
            L.vgx_score_ms.argtypes = [P, dp]
        L.has_fleet = hasattr(L, "vg_fleet_create")  # a build older than the map views and the fleet (A/B runs)
        if L.has_fleet:
            L.vg_map_attach.argtypes = [P, P]
            L.vg_map_detach.argtypes = [P]
            L.vg_fleet_create.argtypes = [P, ctypes.POINTER(P), ctypes.c_int, ctypes.POINTER(P)]
            L.vg_fleet_step_dev.argtypes = [P, ctypes.POINTER(ScanDev)]
            L.vg_fleet_sync.argtypes = [P]
            L.vg_fleet_destroy.argtypes = [P]
            L.vg_fleet_destroy.restype = None
        L.has_raycast = hasattr(L, "vg_raycast")  # a build older than the ray-casting calls (A/B runs)
        if L.has_raycast:
            L.vg_raycast.argtypes = [P, dp, ctypes.c_int, dp, ctypes.c_int, ctypes.POINTER(RayParams), P]
            L.vg_scan_diff.argtypes = [P, fp, ctypes.c_int, dp, ctypes.POINTER(DiffParams), P,
                                       ctypes.POINTER(DiffSummary)]
            L.vgx_ray_ms.argtypes = [P, dp]
        L.has_info = hasattr(L, "vg_localizability")  # a build older than the localisability calls (A/B runs)
        if L.has_info:
            L.vg_localizability.argtypes = [P, dp, ctypes.c_int, dp, ctypes.c_int, ctypes.POINTER(InfoParams), P]
            L.vg_scan_info.argtypes = [P, fp, ctypes.c_int, dp, ctypes.POINTER(DiffParams),
                                       ctypes.POINTER(InfoParams), P]
            L.vgx_info_ms.argtypes = [P, dp]
            L.vgx_info_slab.argtypes = [P, ctypes.c_int]
        L.has_occupancy = hasattr(L, "vg_occupancy")  # a build older than the occupancy grid (A/B runs)
        if L.has_occupancy:
            L.vg_occupancy.argtypes = [P, dp, ctypes.c_int, dp, ctypes.c_int, ctypes.POINTER(OccParams), P, P,
                                       ctypes.POINTER(OccSummary)]
            L.vgx_occ_ms.argtypes = [P, dp]
        L.has_terrain = hasattr(L, "vg_terrain")  # a build older than the terrain layer (A/B runs)
        if L.has_terrain:
            L.vg_terrain.argtypes = [P, dp, ctypes.c_int, dp, ctypes.c_int, ctypes.POINTER(TerrainParams), P, P, P, P,
                                     ctypes.POINTER(TerrainSummary)]
            L.vgx_ter_ground.argtypes = [P, ctypes.c_int, ctypes.c_int, P, P, P, P]
            L.vgx_ter_cells.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P, P, P, P, P, P]
            L.vgx_ter_ms.argtypes = [P, dp]
        L.has_clearance = hasattr(L, "vg_clearance")  # a build older than the clearance field (A/B runs)
        if L.has_clearance:
            L.vg_clearance.argtypes = [P, P, ctypes.POINTER(ClrParams), P, P, P, ctypes.POINTER(ClrSummary)]
            L.vgx_clr_ms.argtypes = [P, dp]
        L.has_navfn = hasattr(L, "vg_navfn")  # a build older than the navigation function (A/B runs)
        if L.has_navfn:
            L.vg_navfn.argtypes = [P, P, ctypes.POINTER(NavParams), P, P, ctypes.c_int, P, ctypes.POINTER(NavSummary)]
            L.vg_nav_paths.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P, P, P, P]
            L.vgx_nav_ms.argtypes = [P, dp]
        L.has_frontiers = hasattr(L, "vg_frontiers")  # a build older than the exploration frontiers (A/B runs)
        if L.has_frontiers:
            L.vg_frontiers.argtypes = [P, P, P, ctypes.POINTER(FrontierParams), P, P, ctypes.c_int,
                                       ctypes.POINTER(FrontierSummary)]
            L.vgx_frontier_ms.argtypes = [P, dp]
            L.vgx_frontier_combine.argtypes = [P, ctypes.c_int]
        L.has_view_gain = hasattr(L, "vg_view_gain")  # a build older than the view gain (A/B runs)
        if L.has_view_gain:
            L.vg_view_gain.argtypes = [P, P, ctypes.POINTER(ViewParams), P, ctypes.c_int, P, P, ctypes.POINTER(ViewSummary)]
            L.vgx_view_ms.argtypes = [P, dp]
            L.vgx_view_stage.argtypes = [P, ctypes.c_int]
        L.has_live = hasattr(L, "vg_live_begin")  # a build older than the live obstacle layer (A/B runs)
        if L.has_live:
            ls = ctypes.POINTER(LiveSummary)
            L.vg_live_begin.argtypes = [P, ctypes.POINTER(LiveParams), P]
            L.vg_live_mark.argtypes = [P, fp, ctypes.c_int, dp, ctypes.c_int32, P, ls]
            L.vg_live_mark_dev.argtypes = [P, P, P, P, ctypes.c_int, dp, ctypes.c_int32, ls]
            L.vg_live_compose.argtypes = [P, ctypes.c_int32, ctypes.c_int, P, ls]
            L.vg_live_info.argtypes = [P, P, P, ls]
            L.vg_live_clear.argtypes = [P]
            L.vg_live_end.argtypes = [P]
            L.vgx_live_walk.argtypes = [P, P, ctypes.c_int, ctypes.c_int32]
            L.vgx_live_ms.argtypes = [P, dp]
        L.has_change = hasattr(L, "vg_change_begin")  # a build older than the change layer (A/B runs)
        if L.has_change:
            L.vg_change_begin.argtypes = [P, ctypes.POINTER(ChangeParams)]
            L.vg_change_accumulate.argtypes = [P, fp, ctypes.c_int, dp, P, ctypes.POINTER(DiffSummary)]
            L.vg_change_accumulate_dev.argtypes = [P, P, P, P, ctypes.c_int, dp, ctypes.POINTER(DiffSummary)]
            L.vg_change_report.argtypes = [P, ctypes.POINTER(ChangeQuery), P, ctypes.c_int, ip, P, ctypes.c_int, ip,
                                           ctypes.POINTER(ChangeTotals)]
            L.vg_change_clear.argtypes = [P]
            L.vg_change_end.argtypes = [P]
        L.has_places = hasattr(L, "vg_places_build")  # a build older than the place index (A/B runs)
        if L.has_places:
            pp = ctypes.POINTER(PlacesParams)
            L.vg_places_dirs.argtypes = [pp, dp, ctypes.c_int, ip]
            L.vg_places_build.argtypes = [P, dp, ctypes.c_int, pp]
            L.vg_places_info.argtypes = [P, ip, ip, P, P]
            L.vg_places_scan.argtypes = [P, fp, ctypes.c_int, dp, P, P]
            L.vg_places_query.argtypes = [P, fp, ctypes.c_int, dp, ctypes.c_int, P, ip, P]
            L.vg_places_end.argtypes = [P]
            L.vg_relocalize_global.argtypes = [P, fp, ctypes.c_int, dp, ctypes.c_int, ctypes.POINTER(RelocParams),
                                               ctypes.c_int, dp, ctypes.POINTER(PoseScore), P, ip]
            L.vgx_places_ms.argtypes = [P, dp, dp]
        L.vg_trajectory.argtypes = [P, dp, ctypes.c_int, ip]
        L.vg_path.argtypes = [P, dp, ctypes.c_int, ip]
        L.vg_poll.argtypes = [P, ip, ip, ip]
        L.vg_poll_rows.argtypes = [P, dp, ctypes.c_int, ctypes.c_int, dp, ctypes.c_int]
        L.vg_local_map.argtypes = [P, fp, ctypes.c_int, ip]
        L.vg_set_publish.argtypes = [P, ctypes.c_int]
        L.has_markers = hasattr(L, "vg_markers")  # a build older than the markers (A/B runs): _need_markers says so
        if L.has_markers:
            mp = ctypes.POINTER(VgPlaneMarker)
            L.vg_markers.argtypes = [P, mp, ctypes.c_int, ip, ip]
            L.vg_marker_capacity.argtypes = [P, ctypes.c_int]
            L.vg_map_planes.argtypes = [P, ctypes.c_int, mp, ctypes.c_int, ip]
            L.vgx_marker_eval.argtypes = [P, dp, ctypes.c_int, mp]
            L.vgx_marker_sizeof.argtypes = []
        L.vg_scan_load.argtypes = [P, fp, fp, ctypes.c_int]
        L.vg_scan_bind_dev.argtypes = [P, P, P, P, P, ctypes.c_int]
        L.vg_propagate.argtypes = [P, dp, ctypes.c_int, ctypes.c_double, ctypes.c_double]
        L.vg_downsample_scan.argtypes = [P, ip]
        L.vg_lio_state_estimation.argtypes = [P, ip]
        L.vg_window_push.argtypes = [P, dp, ctypes.c_int]
        L.vg_cut_voxel_multi.argtypes = [P]
        L.vg_multi_recut.argtypes = [P, ip]
        L.vg_damping_iter.argtypes = [P, ip]
        L.vg_multi_margi.argtypes = [P]
        L.vg_step_end.argtypes = [P]
        L.vg_win_count.argtypes = [P, ip]
        L.vg_profile.argtypes = [P, ctypes.c_int]
        L.vg_profile_read.argtypes = [P, ctypes.c_int, dp, ip]
        L.vg_rccl_unique_id.argtypes = [ctypes.c_char_p]
        L.vg_shard_rccl.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
        L.vg_shard_host.argtypes = [P, ctypes.c_int, ctypes.c_int, HOST_ALLREDUCE, P]
        L.vg_stream.argtypes = [P]
        L.vg_stream.restype = P
        L.vg_set_wait_policy.argtypes = [P, ctypes.c_int, ctypes.c_int]
        L.vg_multi_create.argtypes = [ctypes.POINTER(P), ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.vg_multi_create.restype = P
        L.vg_multi_step_dev.argtypes = [P, ctypes.POINTER(ScanDev)]
        L.vg_multi_sync.argtypes = [P]
        L.vg_multi_set_active.argtypes = [P, ctypes.c_int]
        L.vg_multi_destroy.argtypes = [P]
        L.vgx_debug.argtypes = [P, ctypes.c_int, ctypes.c_int]
        L.vgx_downsample_hashed.argtypes = [P, fp, fp, ctypes.c_int, ctypes.c_double, fp, ip]
        L.vgx_ba_capture.argtypes = [P, dp, ctypes.c_int, ip]
        if hasattr(L, "vgx_ba_solve"):  # absent from builds older than the test entry (A/B runs)
            L.vgx_ba_solve.argtypes = [P, dp, dp, dp]
        if hasattr(L, "vgx_ba_step"):
            L.vgx_ba_step.argtypes = [P, dp, dp, dp, dp, ctypes.c_double, ctypes.c_double, ctypes.c_int, dp, dp, dp,
                                      dp, ip, dp, dp]
            L.vgx_ba_control.argtypes = [P, dp, ip, dp, dp, ctypes.c_int, dp, dp, dp, ip]
        if hasattr(L, "vgx_ba_factors"):
            L.vgx_ba_factors.argtypes = [P, ctypes.c_int, ip, ctypes.c_int, ip, dp, dp, dp, ip, ctypes.c_int,
                                         ctypes.c_int, dp, dp, dp, dp]
        if hasattr(L, "vgx_memo_probe"):
            L.vgx_memo_probe.argtypes = [P, ip]
        if hasattr(L, "vgx_map_nodes"):
            l64 = ctypes.POINTER(ctypes.c_int64)
            L.vgx_map_nodes.argtypes = [P, dp, ctypes.c_int, dp, l64, dp, l64, l64]
        if hasattr(L, "vgx_roots"):
            L.vgx_roots.argtypes = [P, ctypes.POINTER(ctypes.c_longlong), dp, ip, ip, ip, ctypes.c_int, ip]
        if hasattr(L, "vgx_la_eval"):
            L.vgx_la_eval.argtypes = [P, ctypes.c_int, dp, ctypes.c_int, dp, ctypes.c_int, ctypes.c_int]
        if hasattr(L, "vgx_iekf_update"):
            L.vgx_iekf_update.argtypes = [P, ctypes.c_int, dp, ctypes.c_int, dp, dp, ctypes.c_int, ctypes.c_int, dp,
                                          dp, ip]
        if hasattr(L, "vgx_scan_prop"):
            L.vgx_scan_prop.argtypes = [P, dp, ctypes.c_int, dp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        dp, dp, dp]
            L.vgx_ba_imu.argtypes = [P, ctypes.c_int, dp, dp, dp, dp, ctypes.c_double, dp, dp, dp, dp]
            L.vgx_imu_record.argtypes = [dp, dp, dp, ctypes.c_int, ctypes.c_double, dp, dp, dp]
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _f(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


class VgError(RuntimeError):
    pass


def _plane_arg(who, name, arr, dtype, nx, ny):
    """A 2-D query's plane argument: (arr as a contiguous dtype [ny, nx] array, or None: the plane a call before left
    on the device; nx; ny). An array brings its shape, which nx and ny may repeat; None needs both."""
    if arr is None:
        if nx is None or ny is None:
            raise ValueError("%s: %s=None needs nx and ny" % (who, name))
        return None, nx, ny
    a = np.ascontiguousarray(arr, dtype=dtype)
    if a.ndim != 2 or (nx not in (None, a.shape[1])) or (ny not in (None, a.shape[0])):
        raise ValueError("%s: %s is [ny, nx]" % (who, name))
    return a, a.shape[1], a.shape[0]


def _grid_legal(nx, ny):
    """The library's shape check of the 2-D query layers: outputs are sized by nx, ny only where it passes."""
    return 1 <= nx <= CLR_MAX_SIDE and 1 <= ny <= CLR_MAX_SIDE and nx * ny <= OCC_MAX_CELLS


def _summary(s):
    """A summary structure as a dict of ints, without its reserved field."""
    return {f: int(getattr(s, f)) for f, _ in s._fields_ if f != "reserved"}


class Context:
    """One device-resident LIO sequence (vg_ctx)."""

    def __init__(self, cconfig, device=0, max_points=2_000_000, max_nodes=0, max_fix_points=0, hash_log2=0):
        self.h = ctypes.c_void_p()
        cap = Capacity(max_points, max_nodes, max_fix_points, hash_log2)
        r = lib().vg_create(ctypes.byref(cconfig), ctypes.byref(cap), device, ctypes.byref(self.h))
        if r != 0:
            raise VgError("vg_create failed (%d)" % r)
        self._fn_step = lib().vg_step_dev
        self._cfg = cconfig
        self._live_shape = (1, 1)  # [ny, nx] of the live layer (live_begin); without one the library reports the state

    def _chk(self, r, what):
        if r != 0:
            raise VgError("%s failed (%d): %s" % (what, r, lib().vg_last_error(self.h).decode()))

    def _ms(self, fn, name):
        """A measurement hook's one value: fn(ctx, double*) named `name`."""
        ms = ctypes.c_double(0)
        self._chk(fn(self.h, ctypes.byref(ms)), name)
        return ms.value

    def close(self):
        """vg_destroy; refused (VgError -5, the context stays) while contexts are attached to
        this one's map or a fleet steps it. An attached tracker detaches first. Close in this
        order, explicitly: the Fleet, its trackers (or detach them), then the owner. Dropping the
        objects instead leaves the order to the collector: __del__ swallows a refused close and
        does not try again, so an owner collected before its trackers keeps its device memory
        until the process ends."""
        if self.h:
            self._chk(lib().vg_destroy(self.h), "vg_destroy")
            self.h = None
            self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def attach(self, owner):
        """vg_map_attach: this context becomes a read-only view of owner's frozen map and takes
        owner's between-scans estimator; seed() or relocalize(install=True) then places it."""
        self._chk(lib().vg_map_attach(self.h, owner.h), "vg_map_attach")
        self._owner = owner  # the owner outlives its views

    def detach(self):
        """vg_map_detach: this context's own (empty) map back, the context as after reset()."""
        self._chk(lib().vg_map_detach(self.h), "vg_map_detach")
        self._owner = None

    def downsample(self, xyz, inten, size):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        inten = np.ascontiguousarray(inten, dtype=np.float32)
        out = np.zeros((max(xyz.shape[0], 1), 5), dtype=np.float32)
        n = ctypes.c_int(0)
        self._chk(lib().vg_downsample(self.h, _f(xyz), _f(inten), xyz.shape[0], size, _f(out), ctypes.byref(n)),
                  "vg_downsample")
        return out[: n.value]

    def downsample_hashed(self, xyz, inten, size, fallback=False):
        """The per-scan pipeline's downsample (test hook): (m,5) in first-occurrence order;
        fallback: with the /2 pass below 2000 voxels (local_mapping.cpp:399-403)."""
        if fallback:
            size = -size
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        inten = np.ascontiguousarray(inten, dtype=np.float32)
        out = np.zeros((max(xyz.shape[0], 1), 5), dtype=np.float32)
        n = ctypes.c_int(0)
        self._chk(lib().vgx_downsample_hashed(self.h, _f(xyz), _f(inten), xyz.shape[0], size, _f(out),
                                              ctypes.byref(n)), "vgx_downsample_hashed")
        return out[: n.value]

    def downsample_close(self, xyz, times, size):
        """down_sampling_close + the init's time sort: (m,4) [x,y,z,t]."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        t = None if times is None else np.ascontiguousarray(times, dtype=np.float32)
        out = np.zeros((max(xyz.shape[0], 1), 4), dtype=np.float32)
        n = ctypes.c_int(0)
        self._chk(lib().vg_downsample_close(self.h, _f(xyz), None if t is None else _f(t), xyz.shape[0], size,
                                            _f(out), ctypes.byref(n)), "vg_downsample_close")
        return out[: n.value]

    def reset(self):
        """Drop the map and the window (vg_reset, the reference's system_reset)."""
        self._chk(lib().vg_reset(self.h), "vg_reset")

    def seed(self, state):
        s = np.ascontiguousarray(state, dtype=np.float64)
        self._chk(lib().vg_seed(self.h, _d(s)), "vg_seed")

    def step(self, xyz, inten, beg, end, imu):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        inten = np.ascontiguousarray(inten, dtype=np.float32)
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        self._chk(lib().vg_step(self.h, _f(xyz), _f(inten), xyz.shape[0], beg, end, _d(imu), imu.shape[0]),
                  "vg_step")

    def step_deskew(self, xyz, inten, times, beg, end, imu):
        """One scan of raw (not motion-compensated) points with per-point times (row f1)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        inten = np.ascontiguousarray(inten, dtype=np.float32)
        times = np.ascontiguousarray(times, dtype=np.float32)
        imu = np.ascontiguousarray(imu, dtype=np.float64)
        self._chk(lib().vg_step_deskew(self.h, _f(xyz), _f(inten), _f(times), xyz.shape[0], beg, end, _d(imu),
                                       imu.shape[0]), "vg_step_deskew")

    def step_deskew_dev(self, dx, dy, dz, di, dt, n, beg, end, imu):
        imu = np.ascontiguousarray(imu, dtype=np.float64)
        self._chk(lib().vg_step_deskew_dev(self.h, ctypes.c_void_p(dx), ctypes.c_void_p(dy), ctypes.c_void_p(dz),
                                           ctypes.c_void_p(di), ctypes.c_void_p(dt), n, beg, end, _d(imu),
                                           imu.shape[0]), "vg_step_deskew_dev")

    def step_dev(self, dx, dy, dz, di, n, beg, end, imu):
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        self._chk(lib().vg_step_dev(self.h, ctypes.c_void_p(dx), ctypes.c_void_p(dy), ctypes.c_void_p(dz),
                                    ctypes.c_void_p(di), n, beg, end, _d(imu), imu.shape[0]), "vg_step_dev")

    def prep_step_dev(self, dx, dy, dz, di, n, beg, end, imu):
        """vg_step_dev's arguments converted once (a caller that holds its
        scans resident passes them straight on, as a C++ caller would)."""
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        return (imu, (ctypes.c_void_p(dx), ctypes.c_void_p(dy), ctypes.c_void_p(dz), ctypes.c_void_p(di),
                      ctypes.c_int(n), ctypes.c_double(beg), ctypes.c_double(end), _d(imu), ctypes.c_int(imu.shape[0])))

    def step_prepped(self, p):
        r = self._fn_step(self.h, *p[1])
        if r != 0:
            self._chk(r, "vg_step_dev")

    def scan_points(self):
        """vg_scan_points: the last completed scan's downsampled cloud (n, 3); empty after a fleet step."""
        n = ctypes.c_int(0)
        self._chk(lib().vg_scan_points(self.h, None, 0, ctypes.byref(n)), "vg_scan_points")
        out = np.zeros((max(n.value, 1), 3), dtype=np.float32)
        self._chk(lib().vg_scan_points(self.h, _f(out), n.value, ctypes.byref(n)), "vg_scan_points")
        return out[: n.value]

    def state(self):
        s = np.zeros(STATE_LEN)
        self._chk(lib().vg_get_state(self.h, _d(s)), "vg_get_state")
        return s

    def lio_kdtree(self, xyz, state):
        """SURVEY A14 (init-phase LIO against the kNN map): returns (state,
        valid correspondences or -1 when the scan only seeded the map, IEKF
        iterations). xyz: the scan downsampled at max(down_size, 0.5)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        st = np.array(state, dtype=np.float64, copy=True)
        v = ctypes.c_int(0)
        it = ctypes.c_int(0)
        self._chk(lib().vg_lio_kdtree(self.h, _f(xyz), xyz.shape[0], _d(st), ctypes.byref(v), ctypes.byref(it)),
                  "vg_lio_kdtree")
        return st, v.value, it.value

    def decode_scan(self, records, fmt):
        """Sensor records -> time-ordered scan: (xyz (m, 3), intensity, time)."""
        buf = np.frombuffer(bytes(records), dtype=np.uint8)
        f = LidarFormat(**{k: fmt.get(k, 3610.0 if k == "omega_l" else 0.0) for k, _ in LidarFormat._fields_})
        n = buf.size // f.stride
        xyz = np.zeros((n + 2, 3), dtype=np.float32)
        it = np.zeros(n + 2, dtype=np.float32)
        tm = np.zeros(n + 2, dtype=np.float32)
        m = ctypes.c_int(0)
        self._chk(lib().vg_decode_scan(self.h, buf.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(f), _f(xyz),
                                       _f(it), _f(tm), ctypes.byref(m)), "vg_decode_scan")
        return xyz[: m.value], it[: m.value], tm[: m.value]

    def kdmap(self):
        n = ctypes.c_int(0)
        self._chk(lib().vg_kdmap_get(self.h, None, 0, ctypes.byref(n)), "vg_kdmap_get")
        out = np.zeros((max(n.value, 1), 3), dtype=np.float32)
        self._chk(lib().vg_kdmap_get(self.h, _f(out), n.value, ctypes.byref(n)), "vg_kdmap_get")
        return out[: n.value]

    def stats(self):
        s = Stats()
        self._chk(lib().vg_get_stats(self.h, ctypes.byref(s)), "vg_get_stats")
        return _stats_dict(s)

    def stats_log(self):
        """Counters of every completed scan (drains the stream once)."""
        n = ctypes.c_int(0)
        self._chk(lib().vg_stats_log(self.h, None, 0, ctypes.byref(n)), "vg_stats_log")
        arr = (Stats * max(n.value, 1))()
        self._chk(lib().vg_stats_log(self.h, arr, n.value, ctypes.byref(n)), "vg_stats_log")
        return [_stats_dict(s) for s in arr[: n.value]]

    def release_far(self, compact=False, census=True):
        """The idle branch's journey release + pool compaction (vg_release_far): [roots erased (-1: none
        pending), nodes erased, roots, nodes, point_fix points held, point_fix arena used]; census=False:
        the caller's idle-branch call (returns at once with -1s when no release is pending)."""
        out = (ctypes.c_longlong * 6)()
        self._chk(lib().vg_release_far(self.h, (1 if compact else 0) | (2 if census else 0), out), "vg_release_far")
        return list(out)

    def set_mapping(self, on):
        """vg_set_mapping: False freezes the map (localisation only), True maps again. Between scans."""
        self._chk(lib().vg_set_mapping(self.h, 1 if on else 0), "vg_set_mapping")

    def score_poses(self, xyz, poses, pose_var=None, per_point=False):
        """vg_score_poses: the scan xyz (n, 3; LiDAR frame) under the K poses (K, 12) [R row-major, p].
        Returns the K records (POSE_SCORE_DTYPE); with per_point (K = 1) also the n POINT_MATCH_DTYPE records."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
        pv = None if pose_var is None else np.ascontiguousarray(pose_var, dtype=np.float64).reshape(18)
        out = np.zeros(max(poses.shape[0], 1), dtype=POSE_SCORE_DTYPE)
        pp = np.zeros(max(xyz.shape[0], 1), dtype=POINT_MATCH_DTYPE) if per_point else None
        self._chk(lib().vg_score_poses(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0], _d(poses),
                                       poses.shape[0], None if pv is None else _d(pv), out.ctypes.data,
                                       None if pp is None else pp.ctypes.data), "vg_score_poses")
        out = out[: poses.shape[0]]
        return (out, pp[: xyz.shape[0]]) if per_point else out

    def score_ms(self):
        """Device time of the last score_poses call's kernels (HIP events on the context stream), ms."""
        return self._ms(lib().vgx_score_ms, "vgx_score_ms")

    def relocalize(self, xyz, guess, install=False, **params):
        """vg_relocalize: (pose (12,), the refined winner's record, ok). guess: (12,) [R, p]; params: reloc_params."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        g = np.ascontiguousarray(guess, dtype=np.float64).reshape(12)
        p = reloc_params(**params)
        pose = np.zeros(12)
        sc = PoseScore()
        ok = ctypes.c_int(0)
        self._chk(lib().vg_relocalize(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0], _d(g), ctypes.byref(p),
                                      1 if install else 0, _d(pose), ctypes.byref(sc), ctypes.byref(ok)),
                  "vg_relocalize")
        rec = {"matches": sc.matches, "in_map": sc.in_map, "cost": sc.cost, "sum_abs": sc.sum_abs, "nn": list(sc.nn)}
        return pose, rec, bool(ok.value)

    def raycast(self, origins, dirs, **params):
        """vg_raycast: rays from origins ((3,) shared by all, or (n, 3)) along dirs (n, 3), world frame, to
        the first plane of the map; params: ray_params. Returns the n records (RAY_HIT_DTYPE)."""
        o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        p = ray_params(**params)
        out = np.zeros(max(d.shape[0], 1), dtype=RAY_HIT_DTYPE)
        self._chk(lib().vg_raycast(self.h, _d(o) if o.shape[0] else None, o.shape[0], _d(d) if d.shape[0] else None,
                                   d.shape[0], ctypes.byref(p), out.ctypes.data), "vg_raycast")
        return out[: d.shape[0]]

    def scan_diff(self, xyz, pose=None, per_point=False, **params):
        """vg_scan_diff: the scan xyz (n, 3; LiDAR frame) against the map's expected ranges at pose (12,)
        [R row-major, p] (None: the context's state); params: diff_params. Returns the summary as a dict
        (n: the four class counts by DIFF_*); with per_point also the n DIFF_POINT_DTYPE records."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        g = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        p = diff_params(**params)
        pp = np.zeros(max(xyz.shape[0], 1), dtype=DIFF_POINT_DTYPE) if per_point else None
        s = DiffSummary()
        self._chk(lib().vg_scan_diff(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                     None if g is None else _d(g), ctypes.byref(p),
                                     None if pp is None else pp.ctypes.data, ctypes.byref(s)), "vg_scan_diff")
        rec = {"n": list(s.n), "n_truncated": s.n_truncated, "n_occupied_unknown": s.n_occupied_unknown,
               "sum_abs_consistent": s.sum_abs_consistent}
        return (rec, pp[: xyz.shape[0]]) if per_point else rec

    # ---- localisability (vina_gpu.h "Localisability")
    def localizability(self, positions, dirs, **prm):
        """vg_localizability: one INFO_REC_DTYPE record per place. positions (M, 3): LiDAR origins in the
        world; dirs (D, 3), 1 <= D <= 4096: world-frame directions shared by all places (places_dirs()
        gives a suitable set); prm: info_params."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        p = info_params(**prm)
        out = np.zeros(max(pos.shape[0], 1), dtype=INFO_REC_DTYPE)
        self._chk(lib().vg_localizability(self.h, _d(pos) if pos.shape[0] else None, pos.shape[0],
                                          _d(d) if d.shape[0] else None, d.shape[0], ctypes.byref(p),
                                          out.ctypes.data), "vg_localizability")
        return out[: pos.shape[0]]

    def scan_info(self, xyz, pose=None, floor_var=0.0, min_hits=0, **diff):
        """vg_scan_info: the information record (an INFO_REC_DTYPE scalar) of the scan xyz (n, 3; LiDAR
        frame) at pose (12,) [R row-major, p] (None: the context's state), over its CONSISTENT points;
        diff: diff_params, as scan_diff takes them."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        g = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        dq = diff_params(**diff)
        p = info_params(floor_var=floor_var, min_hits=min_hits)
        out = np.zeros(1, dtype=INFO_REC_DTYPE)
        self._chk(lib().vg_scan_info(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                     None if g is None else _d(g), ctypes.byref(dq), ctypes.byref(p),
                                     out.ctypes.data), "vg_scan_info")
        return out[0]

    def info_ms(self):
        """Device time (ms) of the last localizability call's kernels, summed over its slabs, or of the
        last scan_info call's (HIP events on the context stream)."""
        return self._ms(lib().vgx_info_ms, "vgx_info_ms")

    def info_slab(self, places):
        """Test hook: the places per launch of localizability from the next call on (<= 0: the default)."""
        self._chk(lib().vgx_info_slab(self.h, places), "vgx_info_slab")

    # ---- the occupancy grid (vina_gpu.h "Occupancy grid")
    def occupancy(self, positions, dirs=None, counts=False, **params):
        """vg_occupancy: the 2-D occupancy grid ray-cast from positions (M, 3), the sensor origins in the
        world, along dirs (D, 3) shared by all of them (None: occupancy_dirs()). params: occ_params (x0, y0,
        res, nx, ny and the rest) or prm=a filled OccParams. Returns (grid int8 [ny, nx] of OCC_*, counts int32 [2, ny, nx] (n_free,
        n_occ) or None, the summary as a dict)."""
        if not lib().has_occupancy:
            raise VgError("this libvina_gpu.so has no occupancy grid (vg_occupancy): rebuild it")
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(occupancy_dirs() if dirs is None else dirs, dtype=np.float64).reshape(-1, 3)
        p = params["prm"] if "prm" in params else occ_params(**params)   # prm: a filled OccParams
        cells = p.nx * p.ny if 1 <= p.nx and 1 <= p.ny and p.nx * p.ny <= OCC_MAX_CELLS else 1
        grid = np.zeros(cells, dtype=np.int8)
        cnt = np.zeros(2 * cells, dtype=np.int32) if counts else None
        s = OccSummary()
        self._chk(lib().vg_occupancy(self.h, _d(pos) if pos.shape[0] else None, pos.shape[0],
                                     _d(d) if d.shape[0] else None, d.shape[0], ctypes.byref(p), grid.ctypes.data,
                                     None if cnt is None else cnt.ctypes.data, ctypes.byref(s)), "vg_occupancy")
        return grid.reshape(p.ny, p.nx), None if cnt is None else cnt.reshape(2, p.ny, p.nx), _summary(s)

    def occ_ms(self):
        """Device time (ms) of the last occupancy call's kernels, summed over its slabs and the classification."""
        return self._ms(lib().vgx_occ_ms, "vgx_occ_ms")

    # ---- the terrain layer (vina_gpu.h "Terrain layer")
    def terrain(self, positions, dirs=None, **params):
        """vg_terrain: ground elevation, steps and the ground-relative grid ray-cast from positions (M, 3) along
        dirs (D, 3) shared by all of them (None: occupancy_dirs()). params: terrain_params (x0, y0, res, nx, ny and
        the rest) or prm=a filled TerrainParams. Returns (grid int8 [ny, nx] of OCC_*, elev int32 [ny, nx] (TER_NONE:
        none), step int32 [ny, nx], counts int32 [2, ny, nx] (n_free, n_occ), the summary as a dict). The grid stays
        on the device where occupancy() leaves its own."""
        if not lib().has_terrain:
            raise VgError("this libvina_gpu.so has no terrain layer (vg_terrain): rebuild it")
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        d = np.ascontiguousarray(occupancy_dirs() if dirs is None else dirs, dtype=np.float64).reshape(-1, 3)
        p = params["prm"] if "prm" in params else terrain_params(**params)   # prm: a filled TerrainParams
        cells = p.nx * p.ny if 1 <= p.nx and 1 <= p.ny and p.nx * p.ny <= OCC_MAX_CELLS else 1
        grid = np.zeros(cells, dtype=np.int8)
        elev, step = np.zeros(cells, dtype=np.int32), np.zeros(cells, dtype=np.int32)
        cnt = np.zeros(2 * cells, dtype=np.int32)
        s = TerrainSummary()
        self._chk(lib().vg_terrain(self.h, _d(pos) if pos.shape[0] else None, pos.shape[0],
                                   _d(d) if d.shape[0] else None, d.shape[0], ctypes.byref(p), grid.ctypes.data,
                                   elev.ctypes.data, step.ctypes.data, cnt.ctypes.data, ctypes.byref(s)), "vg_terrain")
        return (grid.reshape(p.ny, p.nx), elev.reshape(p.ny, p.nx), step.reshape(p.ny, p.nx),
                cnt.reshape(2, p.ny, p.nx), _summary(s))

    def terrain_ground(self, nx, ny):
        """Test hook (vgx_ter_ground): the four ground planes the last terrain() call left on the device, (g_n
        int32, g_sum int64, g_min int32, g_max int32), [ny, nx] each; nx, ny other than that call's is refused."""
        g_n, g_min, g_max = (np.zeros((ny, nx), dtype=np.int32) for _ in range(3))
        g_sum = np.zeros((ny, nx), dtype=np.int64)
        self._chk(lib().vgx_ter_ground(self.h, nx, ny, g_n.ctypes.data, g_sum.ctypes.data, g_min.ctypes.data,
                                       g_max.ctypes.data), "vgx_ter_ground")
        return g_n, g_sum, g_min, g_max

    def terrain_cells(self, g_n, g_sum, g_min, g_max, min_ground=1):
        """Test hook (vgx_ter_cells): the per-cell stage alone on ground planes [ny, nx]. Returns (elev, step int32
        [ny, nx], (cells_ground, max_step, max_spread))."""
        g_n, g_min, g_max = (np.ascontiguousarray(a, dtype=np.int32) for a in (g_n, g_min, g_max))
        g_sum = np.ascontiguousarray(g_sum, dtype=np.int64)
        ny, nx = g_n.shape
        assert g_sum.shape == g_min.shape == g_max.shape == (ny, nx)
        elev, step = np.zeros((ny, nx), dtype=np.int32), np.zeros((ny, nx), dtype=np.int32)
        out = np.zeros(3, dtype=np.int64)
        self._chk(lib().vgx_ter_cells(self.h, nx, ny, min_ground, g_n.ctypes.data, g_sum.ctypes.data, g_min.ctypes.data,
                                      g_max.ctypes.data, elev.ctypes.data, step.ctypes.data, out.ctypes.data),
                  "vgx_ter_cells")
        return elev, step, tuple(int(v) for v in out)

    def ter_ms(self):
        """Device time (ms) of the last terrain() call's kernels: (k_ter_ground, k_ter_cells, k_ter_marks,
        k_ter_classify), the ray kernels summed over their slabs."""
        ms = (ctypes.c_double * 4)()
        self._chk(lib().vgx_ter_ms(self.h, ms), "vgx_ter_ms")
        return tuple(ms)

    # ---- the clearance field and costmap (vina_gpu.h "Clearance field and costmap")
    def clearance(self, grid=None, *, nx=None, ny=None, res, flags=0, inscribed_radius=0.0, inflation_radius=0.0,
                  cost_scaling=0.0, want=("dist2", "nearest", "cost")):
        """vg_clearance of grid (int8 [ny, nx] of OCC_*; None: the grid the last occupancy() call on this
        context left on the device, nx and ny naming its shape). want: which of dist2 (int32, cells squared,
        CLR_NONE without any obstacle), nearest (int32, the obstacle's linear index, -1 without any) and cost
        (uint8, COST_*) leave the device. Returns ({name: array [ny, nx]}, the summary as a dict)."""
        if not lib().has_clearance:
            raise VgError("this libvina_gpu.so has no clearance field (vg_clearance): rebuild it")
        g, nx, ny = _plane_arg("clearance", "grid", grid, np.int8, nx, ny)
        unknown = [w for w in want if w not in ("dist2", "nearest", "cost")]
        if unknown:
            raise ValueError("clearance: want holds %r" % unknown)
        p = ClrParams()
        p.nx, p.ny, p.res, p.flags = int(nx), int(ny), res, flags
        p.inscribed_radius, p.inflation_radius, p.cost_scaling = inscribed_radius, inflation_radius, cost_scaling
        legal = _grid_legal(p.nx, p.ny)
        shape = (p.ny, p.nx) if legal else (1, 1)
        out = {w: np.zeros(shape, dtype=np.uint8 if w == "cost" else np.int32) for w in ("dist2", "nearest", "cost")
               if w in want}
        s = ClrSummary()
        self._chk(lib().vg_clearance(self.h, None if g is None else g.ctypes.data, ctypes.byref(p),
                                     *[out[w].ctypes.data if w in out else None for w in ("dist2", "nearest", "cost")],
                                     ctypes.byref(s)), "vg_clearance")
        return out, _summary(s)

    def clearance_ms(self):
        """Device time (ms) of the last clearance call's two kernels."""
        return self._ms(lib().vgx_clr_ms, "vgx_clr_ms")

    # ---- the navigation function (vina_gpu.h "Navigation function")
    def navfn(self, cost=None, goals=(), *, nx=None, ny=None, want_pot=True, trav=None, **params):
        """vg_navfn over cost (uint8 [ny, nx] of COST_*; None: the cost plane the last clearance() call on this
        context left on the device, nx and ny naming its shape) towards goals ((G, 2) cells ix, iy). trav: an
        explicit uint16 [256] table, or None: nav_trav_table(**params) as the library builds it from params
        (flags, neutral, lethal_from, unknown_as, factor). Returns (pot uint32 [ny, nx] of cost-to-go, NAV_SAT,
        NAV_UNREACHED, or None without want_pot; the summary as a dict). The field stays on the device for
        nav_paths()."""
        if not lib().has_navfn:
            raise VgError("this libvina_gpu.so has no navigation function (vg_navfn): rebuild it")
        c, nx, ny = _plane_arg("navfn", "cost", cost, np.uint8, nx, ny)
        g = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        t = None
        if trav is not None:
            t = np.ascontiguousarray(trav, dtype=np.uint16)
            if t.shape != (256,):
                raise ValueError("navfn: trav is uint16 [256]")
        p = NavParams()
        p.nx, p.ny = int(nx), int(ny)
        for k, v in params.items():
            if k not in ("flags", "neutral", "lethal_from", "unknown_as", "factor"):
                raise ValueError("navfn: no parameter %r" % k)
            setattr(p, k, v)
        legal = _grid_legal(p.nx, p.ny)
        pot = np.zeros((p.ny, p.nx) if legal else (1, 1), dtype=np.uint32) if want_pot else None
        s = NavSummary()
        self._chk(lib().vg_navfn(self.h, None if c is None else c.ctypes.data, ctypes.byref(p),
                                 None if t is None else t.ctypes.data, g.ctypes.data, g.shape[0],
                                 None if pot is None else pot.ctypes.data, ctypes.byref(s)), "vg_navfn")
        return pot, _summary(s)

    def nav_paths(self, starts, max_len):
        """vg_nav_paths from starts ((S, 2) cells ix, iy) down the field of the last navfn() call. Returns
        (cells int32 [S, max_len] of linear indices, -1 past a path's end; len int32 [S]; status int32 [S] of
        NAV_REACHED, NAV_NO_PATH, NAV_TRUNCATED, NAV_STUCK; path_cost int64 [S]: pot[start], -1 with NAV_NO_PATH)."""
        if not lib().has_navfn:
            raise VgError("this libvina_gpu.so has no navigation function (vg_nav_paths): rebuild it")
        st = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 2)
        n, m = st.shape[0], int(max_len)
        legal = 1 <= n <= NAV_MAX_POINTS and m >= 1 and n * m <= NAV_MAX_PATH_CELLS
        cells = np.zeros((n, m) if legal else (1, 1), dtype=np.int32)
        ln, status = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        pc = np.zeros(max(n, 1), dtype=np.int64)
        self._chk(lib().vg_nav_paths(self.h, st.ctypes.data, n, m, cells.ctypes.data, ln.ctypes.data, status.ctypes.data,
                                     pc.ctypes.data), "vg_nav_paths")
        return cells, ln, status, pc

    def navfn_ms(self):
        """Device time (ms) of the last navfn() or nav_paths() call's kernels."""
        return self._ms(lib().vgx_nav_ms, "vgx_nav_ms")

    # ---- exploration frontiers (vina_gpu.h "Exploration frontiers")
    def frontiers(self, grid=None, *, nx=None, ny=None, cost=None, use_cost=False, use_pot=False, cost_max=0,
                  min_size=0, max_records=4096, want_labels=True):
        """vg_frontiers of grid (int8 [ny, nx] of OCC_*; None: the grid the last occupancy() call on this context
        left on the device, nx and ny naming its shape). use_cost: only cells with cost < cost_max (0: 253), cost a
        uint8 [ny, nx] plane or None: the one the last clearance() call left on the device (giving cost implies
        use_cost). use_pot: only cells the field of the last navfn() call reaches; the records then carry the
        cheapest cell. Returns (labels int32 [ny, nx], -1 off the frontier, or None without want_labels; the
        records of the components with size >= min_size as a FRONTIER_REC array in ascending label, at most
        max_records; the summary as a dict)."""
        if not lib().has_frontiers:
            raise VgError("this libvina_gpu.so has no exploration frontiers (vg_frontiers): rebuild it")
        g, nx, ny = _plane_arg("frontiers", "grid", grid, np.int8, nx, ny)
        c = None
        if cost is not None:
            c = np.ascontiguousarray(cost, dtype=np.uint8)
            if c.shape != (ny, nx):
                raise ValueError("frontiers: cost is [ny, nx]")
            use_cost = True
        p = FrontierParams()
        p.nx, p.ny, p.flags = int(nx), int(ny), (1 if use_cost else 0) | (2 if use_pot else 0)
        p.cost_max, p.min_size = cost_max, min_size
        legal = _grid_legal(p.nx, p.ny)
        labels = np.zeros((p.ny, p.nx) if legal else (1, 1), dtype=np.int32) if want_labels else None
        m = int(max_records)
        recs = np.zeros(min(max(m, 0), FRONTIER_MAX_RECORDS), dtype=FRONTIER_REC)
        s = FrontierSummary()
        self._chk(lib().vg_frontiers(self.h, None if g is None else g.ctypes.data, None if c is None else c.ctypes.data,
                                     ctypes.byref(p), None if labels is None else labels.ctypes.data,
                                     recs.ctypes.data if recs.size else None, m, ctypes.byref(s)), "vg_frontiers")
        return labels, recs[:s.n_written], _summary(s)

    def frontiers_ms(self):
        """Device time (ms) of the last frontiers() call's kernels."""
        return self._ms(lib().vgx_frontier_ms, "vgx_frontier_ms")

    # ---- view gain (vina_gpu.h "View gain")
    def view_gain(self, views, radius, grid=None, *, nx=None, ny=None, max_unknown=0, want_seen=False):
        """vg_view_gain from the cells `views` ((n, 2) int32 of ix, iy) of grid (int8 [ny, nx] of OCC_*; None: the
        grid the last occupancy() call on this context left on the device, nx and ny naming its shape): what a 2-D
        sensor of range `radius` cells sees from each; max_unknown > 0 ends a ray at that many unknown cells.
        Returns (the records as a VIEW_REC array, one per viewpoint in the order given; seen int32 [ny, nx], the
        OK viewpoints that see each cell, or None without want_seen; the summary as a dict)."""
        if not lib().has_view_gain:
            raise VgError("this libvina_gpu.so has no view gain (vg_view_gain): rebuild it")
        g, nx, ny = _plane_arg("view_gain", "grid", grid, np.int8, nx, ny)
        v = np.ascontiguousarray(views, dtype=np.int32).reshape(-1, 2)
        p = ViewParams()
        p.nx, p.ny, p.radius, p.max_unknown = int(nx), int(ny), int(radius), int(max_unknown)
        legal = _grid_legal(p.nx, p.ny)
        seen = np.zeros((p.ny, p.nx) if legal else (1, 1), dtype=np.int32) if want_seen else None
        recs = np.zeros(max(v.shape[0], 1), dtype=VIEW_REC)
        s = ViewSummary()
        self._chk(lib().vg_view_gain(self.h, None if g is None else g.ctypes.data, ctypes.byref(p), v.ctypes.data,
                                     v.shape[0], recs.ctypes.data, None if seen is None else seen.ctypes.data,
                                     ctypes.byref(s)), "vg_view_gain")
        return recs[:v.shape[0]], seen, _summary(s)

    def view_gain_ms(self):
        """Device time (ms) of the last view_gain() call's kernels."""
        return self._ms(lib().vgx_view_ms, "vgx_view_ms")

    # ---- the change layer (vina_gpu.h "Change layer")
    def change_begin(self, cell=0.0, cell_hash_log2=0, **diff):
        """vg_change_begin on the context that owns a frozen map; diff: diff_params; zeros take the
        defaults (cell = voxel_size / 4, 2^20 slots)."""
        p = ChangeParams()
        p.diff = diff_params(**diff)
        p.cell, p.cell_hash_log2 = cell, cell_hash_log2
        self._chk(lib().vg_change_begin(self.h, ctypes.byref(p)), "vg_change_begin")

    @staticmethod
    def _summary(s):
        return {"n": list(s.n), "n_truncated": s.n_truncated, "n_occupied_unknown": s.n_occupied_unknown,
                "sum_abs_consistent": s.sum_abs_consistent}

    def change_accumulate(self, xyz, pose=None, per_point=False):
        """vg_change_accumulate: scan_diff's arguments and returns, and the scan's evidence charged to the
        layer of the map this context reads (its own, or its owner's when attached)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        g = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        pp = np.zeros(max(xyz.shape[0], 1), dtype=DIFF_POINT_DTYPE) if per_point else None
        s = DiffSummary()
        self._chk(lib().vg_change_accumulate(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                             None if g is None else _d(g), None if pp is None else pp.ctypes.data,
                                             ctypes.byref(s)), "vg_change_accumulate")
        rec = self._summary(s)
        return (rec, pp[: xyz.shape[0]]) if per_point else rec

    def change_accumulate_dev(self, dx, dy, dz, n, pose=None):
        """vg_change_accumulate_dev: the cloud as three device arrays (addresses) of n floats."""
        g = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        s = DiffSummary()
        self._chk(lib().vg_change_accumulate_dev(self.h, ctypes.c_void_p(dx), ctypes.c_void_p(dy), ctypes.c_void_p(dz),
                                                 n, None if g is None else _d(g), ctypes.byref(s)),
                  "vg_change_accumulate_dev")
        return self._summary(s)

    def change_report(self, min_obs=0, min_scans=0, vanished_ratio=0.0, flags=0):
        """vg_change_report: (leaves (CHANGE_LEAF_DTYPE, ascending node id), cells (CHANGE_CELL_DTYPE,
        ascending packed key), totals as a dict). Zeros take the defaults (5, 2, 0.8); flags bit 0: every
        touched leaf and used cell, the records' flags telling which meet their rule."""
        q = ChangeQuery()
        q.min_obs, q.min_scans, q.vanished_ratio, q.flags = min_obs, min_scans, vanished_ratio, flags
        nl, nc = ctypes.c_int(0), ctypes.c_int(0)
        t = ChangeTotals()
        self._chk(lib().vg_change_report(self.h, ctypes.byref(q), None, 0, ctypes.byref(nl), None, 0, ctypes.byref(nc),
                                         None), "vg_change_report")
        leaves = np.zeros(max(nl.value, 1), dtype=CHANGE_LEAF_DTYPE)
        cells = np.zeros(max(nc.value, 1), dtype=CHANGE_CELL_DTYPE)
        self._chk(lib().vg_change_report(self.h, ctypes.byref(q), leaves.ctypes.data, nl.value, ctypes.byref(nl),
                                         cells.ctypes.data, nc.value, ctypes.byref(nc), ctypes.byref(t)),
                  "vg_change_report")
        tot = {k: (list(getattr(t, k)) if k == "n" else getattr(t, k)) for k, _ in ChangeTotals._fields_
               if k != "reserved"}
        return leaves[: nl.value], cells[: nc.value], tot

    def change_clear(self):
        """vg_change_clear: the layer zeroed, the epochs restart."""
        self._chk(lib().vg_change_clear(self.h), "vg_change_clear")

    def change_end(self):
        """vg_change_end: the layer freed."""
        self._chk(lib().vg_change_end(self.h), "vg_change_end")

    # ---- the live obstacle layer (vina_gpu.h "Live obstacle layer")
    def live_begin(self, base=None, **params):
        """vg_live_begin: params: live_params (the geometry x0, y0, res, nx, ny at least); base: int8 [ny, nx] of
        OCC_*, or None: a copy of the grid the last occupancy() / terrain() / live_compose() left on the device."""
        if not lib().has_live:
            raise VgError("this libvina_gpu.so has no live obstacle layer (vg_live_begin): rebuild it")
        p = live_params(**params)
        b = None
        if base is not None:
            b = np.ascontiguousarray(base, dtype=np.int8)
            if b.shape != (p.ny, p.nx):
                raise ValueError("live_begin: base is [ny, nx]")
        self._chk(lib().vg_live_begin(self.h, ctypes.byref(p), None if b is None else b.ctypes.data), "vg_live_begin")
        self._live_shape = (p.ny, p.nx)

    def live_mark(self, xyz, pose=None, stamp=0, per_point=False):
        """vg_live_mark: the scan xyz (n, 3; LiDAR frame) at pose (12,) (None: the context's state) marked and
        cleared into the layer at `stamp` (0: the largest so far + 1). Returns the summary as a dict; with per_point
        also the n LIVE_POINT_DTYPE records."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        g = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        pp = np.zeros(max(xyz.shape[0], 1), dtype=LIVE_POINT_DTYPE) if per_point else None
        s = LiveSummary()
        self._chk(lib().vg_live_mark(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                     None if g is None else _d(g), stamp, None if pp is None else pp.ctypes.data,
                                     ctypes.byref(s)), "vg_live_mark")
        rec = _live_summary(s)
        return (rec, pp[: xyz.shape[0]]) if per_point else rec

    def live_mark_dev(self, dx, dy, dz, n, pose=None, stamp=0):
        """vg_live_mark_dev: the cloud as three device arrays (addresses) of n floats."""
        g = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        s = LiveSummary()
        self._chk(lib().vg_live_mark_dev(self.h, ctypes.c_void_p(dx), ctypes.c_void_p(dy), ctypes.c_void_p(dz), n,
                                         None if g is None else _d(g), stamp, ctypes.byref(s)), "vg_live_mark_dev")
        return _live_summary(s)

    def live_compose(self, now=0, flags=0, want_grid=True):
        """vg_live_compose at `now` (0: the layer's largest stamp): (the composed grid int8 [ny, nx], or None with
        want_grid False: it stays on the device for clearance(grid=None); the summary as a dict). flags bit 0: a
        base-unknown cell a beam crossed becomes free."""
        grid = np.zeros(self._live_shape, dtype=np.int8) if want_grid else None
        s = LiveSummary()
        self._chk(lib().vg_live_compose(self.h, now, flags, None if grid is None else grid.ctypes.data,
                                        ctypes.byref(s)), "vg_live_compose")
        return grid, _live_summary(s)

    def live_info(self):
        """vg_live_info: (hit int32 [ny, nx], clear int32 [ny, nx], the totals as a dict)."""
        hit, clear = np.zeros(self._live_shape, dtype=np.int32), np.zeros(self._live_shape, dtype=np.int32)
        s = LiveSummary()
        self._chk(lib().vg_live_info(self.h, hit.ctypes.data, clear.ctypes.data, ctypes.byref(s)), "vg_live_info")
        return hit, clear, _live_summary(s)

    def live_clear(self):
        """vg_live_clear: the planes and the totals zeroed, the stamps restart; the base stays."""
        self._chk(lib().vg_live_clear(self.h), "vg_live_clear")

    def live_end(self):
        """vg_live_end: the layer freed."""
        self._chk(lib().vg_live_end(self.h), "vg_live_end")

    def live_walk(self, recs, stamp):
        """vgx_live_walk (test hook): k_live_walk alone on LIVE_POINT_DTYPE records at `stamp`, into the layer."""
        r = np.ascontiguousarray(recs, dtype=LIVE_POINT_DTYPE)
        self._chk(lib().vgx_live_walk(self.h, r.ctypes.data if r.shape[0] else None, r.shape[0], stamp), "vgx_live_walk")

    def live_ms(self):
        """Device time (ms) of the last live_mark()'s kernels, of its k_live_walk, and of the last live_compose()."""
        ms = (ctypes.c_double * 3)()
        self._chk(lib().vgx_live_ms(self.h, ms), "vgx_live_ms")
        return tuple(ms)

    # ---- the place index (vina_gpu.h "Place index")
    def places_build(self, positions, **params):
        """vg_places_build on the context that owns a frozen map: positions (M, 3), LiDAR origins in the
        world; params: places_params. Replaces an existing index."""
        pos = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        p = places_params(**params)
        self._chk(lib().vg_places_build(self.h, _d(pos) if pos.shape[0] else None, pos.shape[0], ctypes.byref(p)),
                  "vg_places_build")
        self._places_shape = (p.n_el or 12, p.n_az or 120)

    def _places_bins(self):
        o = getattr(self, "_owner", None) or self
        return getattr(o, "_places_shape", (12, 120))

    def places_info(self, desc=False):
        """vg_places_info: {M, n_valid, hit_bins (M,)} and, with desc, the descriptors (M, n_el, n_az) uint16."""
        m, nv = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(lib().vg_places_info(self.h, ctypes.byref(m), ctypes.byref(nv), None, None), "vg_places_info")
        E, A = self._places_bins()
        hit = np.zeros(max(m.value, 1), dtype=np.int32)
        d = np.zeros((max(m.value, 1), E, A), dtype=np.uint16) if desc else None
        self._chk(lib().vg_places_info(self.h, ctypes.byref(m), ctypes.byref(nv), None if d is None else d.ctypes.data,
                                       hit.ctypes.data), "vg_places_info")
        out = {"M": m.value, "n_valid": nv.value, "hit_bins": hit[: m.value]}
        if desc:
            out["desc"] = d[: m.value]
        return out

    def places_scan(self, xyz, R_level=None):
        """vg_places_scan: the scan's descriptor (n_el, n_az) uint16 and its points per bin (int32). R_level:
        (3, 3) or (9,), a rotation with the sensor's roll and pitch; None: the context's current R."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        R = None if R_level is None else np.ascontiguousarray(R_level, dtype=np.float64).reshape(9)
        E, A = self._places_bins()
        d = np.zeros((E, A), dtype=np.uint16)
        n = np.zeros((E, A), dtype=np.int32)
        self._chk(lib().vg_places_scan(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                       None if R is None else _d(R), d.ctypes.data, n.ctypes.data), "vg_places_scan")
        return d, n

    def places_query(self, xyz, R_level=None, top_k=16, scores=False):
        """vg_places_query: the candidates (PLACE_CANDIDATE_DTYPE, ascending score, then place, then shift);
        with scores also the full (M, n_az) int32 table (PLACE_NONE rows for invalid places)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        R = None if R_level is None else np.ascontiguousarray(R_level, dtype=np.float64).reshape(9)
        out = np.zeros(max(top_k, 1), dtype=PLACE_CANDIDATE_DTYPE)
        n = ctypes.c_int(0)
        sc = None
        if scores:
            sc = np.zeros((self.places_info()["M"], self._places_bins()[1]), dtype=np.int32)
        self._chk(lib().vg_places_query(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                        None if R is None else _d(R), top_k, out.ctypes.data, ctypes.byref(n),
                                        None if sc is None else sc.ctypes.data), "vg_places_query")
        return (out[: n.value], sc) if scores else out[: n.value]

    def places_end(self):
        """vg_places_end: the index freed."""
        self._chk(lib().vg_places_end(self.h), "vg_places_end")

    def places_from_path(self, spacing, **params):
        """Build the index from this context's own path rows (vg_path): the LiDAR origins p + R ext_t of
        the rows (ext_t: the configuration's), thinned so that every kept origin is at least `spacing`
        from the one kept before it. Returns the positions used."""
        ext_t = np.array(list(self._cfg.ext_t), dtype=np.float64)
        rows = self.path()
        keep = []
        for row in rows:
            o = row[10:13] + row[1:10].reshape(3, 3) @ ext_t
            if not keep or np.linalg.norm(o - keep[-1]) >= spacing:
                keep.append(o)
        pos = np.array(keep).reshape(-1, 3)
        self.places_build(pos, **params)
        return pos

    def relocalize_global(self, xyz, R_level=None, top_k=16, install=False, **params):
        """vg_relocalize_global: (pose (12,), the refined winner's record, the winning candidate
        (PLACE_CANDIDATE_DTYPE scalar), ok). No params: the default window around each candidate
        (half the places' spacing, +-1.5 azimuth bins); else reloc_params."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        R = None if R_level is None else np.ascontiguousarray(R_level, dtype=np.float64).reshape(9)
        p = reloc_params(**params) if params else None
        pose = np.zeros(12)
        sc = PoseScore()
        cand = np.zeros(1, dtype=PLACE_CANDIDATE_DTYPE)
        ok = ctypes.c_int(0)
        self._chk(lib().vg_relocalize_global(self.h, _f(xyz) if xyz.shape[0] else None, xyz.shape[0],
                                             None if R is None else _d(R), top_k,
                                             None if p is None else ctypes.byref(p), 1 if install else 0, _d(pose),
                                             ctypes.byref(sc), cand.ctypes.data, ctypes.byref(ok)),
                  "vg_relocalize_global")
        rec = {"matches": sc.matches, "in_map": sc.in_map, "cost": sc.cost, "sum_abs": sc.sum_abs, "nn": list(sc.nn)}
        return pose, rec, cand[0], bool(ok.value)

    def places_ms(self):
        """Device time (ms) of the index's build kernel and of the last query's kernels (HIP events)."""
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._chk(lib().vgx_places_ms(self.h, ctypes.byref(a), ctypes.byref(b)), "vgx_places_ms")
        return a.value, b.value

    def ray_ms(self):
        """Device time of the last raycast slab's / scan_diff call's kernels (HIP events on the context stream), ms."""
        return self._ms(lib().vgx_ray_ms, "vgx_ray_ms")

    def _need_checkpoint(self):
        if not lib().has_checkpoint:
            raise VgError("this libvina_gpu.so has no checkpoint support (vg_checkpoint_save): rebuild it")

    def checkpoint_save(self, path):
        """Everything that outlives a scan to one file (vg_checkpoint_save; compacts first); returns its bytes."""
        self._need_checkpoint()
        n = ctypes.c_longlong(0)
        self._chk(lib().vg_checkpoint_save(self.h, os.fsencode(path), ctypes.byref(n)), "vg_checkpoint_save")
        return n.value

    def checkpoint_load(self, path):
        """Install a checkpoint into this context (vg_reset semantics first). A rejected file raises
        VgError with the code (-1 VG_E_ARG, -3 VG_E_CAPACITY) and leaves the context as it was."""
        self._need_checkpoint()
        self._chk(lib().vg_checkpoint_load(self.h, os.fsencode(path)), "vg_checkpoint_load")

    def checkpoint_timed(self, path, load=False):
        """scripts/probe_checkpoint.py: (bytes, [4 phase times in ms]) of one save or load."""
        self._need_checkpoint()
        n = ctypes.c_longlong(0)
        ms = np.zeros(4)
        self._chk(lib().vgx_checkpoint_timed(self.h, os.fsencode(path), 1 if load else 0, ctypes.byref(n), _d(ms)),
                  "vgx_checkpoint_timed")
        return n.value, ms

    def window_states(self):
        out = np.zeros((64, STATE_LEN))
        n = ctypes.c_int(0)
        self._chk(lib().vg_window_states(self.h, _d(out), ctypes.byref(n)), "vg_window_states")
        return out[: n.value]

    def trajectory(self):
        n = ctypes.c_int(0)
        self._chk(lib().vg_trajectory(self.h, None, 0, ctypes.byref(n)), "vg_trajectory")
        out = np.zeros((max(n.value, 1), 13))
        self._chk(lib().vg_trajectory(self.h, _d(out), n.value, ctypes.byref(n)), "vg_trajectory")
        return out[: n.value]

    def path(self):
        """pcl_path rows (vg_path): t, R(9), p(3), jour; the window's positions re-written after each BA."""
        n = ctypes.c_int(0)
        self._chk(lib().vg_path(self.h, None, 0, ctypes.byref(n)), "vg_path")
        out = np.zeros((max(n.value, 1), 14))
        self._chk(lib().vg_path(self.h, _d(out), n.value, ctypes.byref(n)), "vg_path")
        return out[: n.value]

    def poll(self):
        """Non-blocking (vg_poll): (scans complete, TUM rows, path rows) absorbed so far."""
        a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._chk(lib().vg_poll(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "vg_poll")
        return a.value, b.value, c.value

    def set_publish(self, flags):
        self._chk(lib().vg_set_publish(self.h, flags), "vg_set_publish")

    def _need_markers(self):
        if not lib().has_markers:
            raise VgError("%s has no marker entry points (vg_markers, vg_map_planes): rebuild it" % LIB)

    def marker_capacity(self, max_records):
        """Size of the device's marker event buffer (vg_marker_capacity); before set_publish(2)."""
        self._need_markers()
        self._chk(lib().vg_marker_capacity(self.h, max_records), "vg_marker_capacity")

    def markers(self):
        """The last scan's /voxel_plane + /voxel_normal events (vg_markers): (records as a MARKER_DTYPE
        array, events deferred to a later scan because the device buffer was full)."""
        self._need_markers()
        n, d = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(lib().vg_markers(self.h, None, 0, ctypes.byref(n), ctypes.byref(d)), "vg_markers")
        out = np.zeros(max(n.value, 1), dtype=MARKER_DTYPE)
        self._chk(lib().vg_markers(self.h, out.ctypes.data_as(ctypes.POINTER(VgPlaneMarker)), n.value,
                                   ctypes.byref(n), ctypes.byref(d)), "vg_markers")
        return out[: n.value], d.value

    def map_planes(self, slide_only=False, all_nodes=False):
        """Snapshot of the map's planes (vg_map_planes) as a MARKER_DTYPE array: plane leaves, or with
        all_nodes every node down to max_layer; slide_only: under surf_map_slide's roots only."""
        self._need_markers()
        flags = (1 if slide_only else 0) | (2 if all_nodes else 0)
        n = ctypes.c_int(0)
        self._chk(lib().vg_map_planes(self.h, flags, None, 0, ctypes.byref(n)), "vg_map_planes")
        out = np.zeros(max(n.value, 1), dtype=MARKER_DTYPE)
        self._chk(lib().vg_map_planes(self.h, flags, out.ctypes.data_as(ctypes.POINTER(VgPlaneMarker)), n.value,
                                      ctypes.byref(n)), "vg_map_planes")
        return out[: n.value]

    def marker_eval(self, inputs):
        """Test hook (vgx_marker_eval): the device's marker math on (n, 15) inputs -> n records."""
        self._need_markers()
        a = np.ascontiguousarray(inputs, dtype=np.float64).reshape(-1, MARKER_EVAL_IN)
        out = np.zeros(a.shape[0], dtype=MARKER_DTYPE)
        self._chk(lib().vgx_marker_eval(self.h, _d(a), a.shape[0], out.ctypes.data_as(ctypes.POINTER(VgPlaneMarker))),
                  "vgx_marker_eval")
        return out

    def local_map(self):
        """/map_cmap of the last window BA (vg_local_map): (n, 4) float32 x, y, z, intensity."""
        n = ctypes.c_int(0)
        self._chk(lib().vg_local_map(self.h, None, 0, ctypes.byref(n)), "vg_local_map")
        out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._chk(lib().vg_local_map(self.h, _f(out), n.value, ctypes.byref(n)), "vg_local_map")
        return out[: n.value]

    # ---- stage-level API (reference call order, include/vina_gpu.h) ----
    def scan_load(self, xyz, inten):
        self._xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        self._inten = np.ascontiguousarray(inten, dtype=np.float32)
        self._chk(lib().vg_scan_load(self.h, _f(self._xyz), _f(self._inten), self._xyz.shape[0]), "vg_scan_load")

    def propagate(self, imu, beg, end):
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        self._chk(lib().vg_propagate(self.h, _d(imu), imu.shape[0], beg, end), "vg_propagate")

    def _int_call(self, fn, name):
        v = ctypes.c_int(0)
        self._chk(fn(self.h, ctypes.byref(v)), name)
        return v.value

    def downsample_scan(self):
        return self._int_call(lib().vg_downsample_scan, "vg_downsample_scan")

    def lio_state_estimation(self):
        return self._int_call(lib().vg_lio_state_estimation, "vg_lio_state_estimation")

    def window_push(self, imu):
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        self._chk(lib().vg_window_push(self.h, _d(imu), imu.shape[0]), "vg_window_push")

    def cut_voxel_multi(self):
        self._chk(lib().vg_cut_voxel_multi(self.h), "vg_cut_voxel_multi")

    def multi_recut(self):
        return self._int_call(lib().vg_multi_recut, "vg_multi_recut")

    def damping_iter(self):
        return self._int_call(lib().vg_damping_iter, "vg_damping_iter")

    def multi_margi(self):
        self._chk(lib().vg_multi_margi(self.h), "vg_multi_margi")

    def step_end(self):
        self._chk(lib().vg_step_end(self.h), "vg_step_end")

    def win_count(self):
        return self._int_call(lib().vg_win_count, "vg_win_count")

    PROFILE_STAGES = ["downsample", "iekf", "insert", "recut", "ba", "margi", "iekf_total", "ba_solve",
                      "host_propagate", "host_downsample", "host_iekf", "host_push", "host_insert", "host_recut",
                      "host_ba", "host_margi", "k_iekf_clock", "k_ba_solve_clock", "k_rc_clock", "k_ba_hess_clock"]

    def profile(self, on=True, stages=False, every=1, clock=False):
        """on: k_iekf / k_ba_solve launch events (the solve's on every `every`-th
        BA run) and host stage timers; stages: per-stage events as well; clock:
        the in-kernel clocks of k_iekf / k_ba_solve (kernel-only time, graphs
        kept; replaces the solve's events)."""
        flags = (1 if on else 0) | (2 if stages else 0) | (4 if clock else 0) | ((max(1, min(255, every)) & 0xff) << 8)
        self._chk(lib().vg_profile(self.h, flags), "vg_profile")

    def profile_read(self):
        out = {}
        for i, name in enumerate(self.PROFILE_STAGES):
            ms = ctypes.c_double(0)
            n = ctypes.c_int(0)
            self._chk(lib().vg_profile_read(self.h, i, ctypes.byref(ms), ctypes.byref(n)), "vg_profile_read")
            out[name] = {"ms": ms.value, "launches": n.value}
        return out

    def shard_rccl(self, rank, world, uid):
        """Spatial-tile sharding over `world` contexts, RCCL inside the library."""
        self._chk(lib().vg_shard_rccl(self.h, rank, world, uid), "vg_shard_rccl")

    def shard_host(self, rank, world, allreduce):
        """Spatial-tile sharding with a host all-reduce: allreduce(np.ndarray) sums
        the array in place across ranks (e.g. torch.distributed gloo)."""
        def cb(buf, count, dtype, user):
            try:
                ct = ctypes.c_double if dtype == 0 else ctypes.c_int32
                arr = np.ctypeslib.as_array(ctypes.cast(buf, ctypes.POINTER(ct)), shape=(count,))
                allreduce(arr)
                return 0
            except Exception:  # noqa: BLE001 - reported to the library as a failed exchange
                import traceback
                traceback.print_exc()
                return 1
        self._cb = HOST_ALLREDUCE(cb)  # keep alive
        self._chk(lib().vg_shard_host(self.h, rank, world, self._cb, None), "vg_shard_host")

    def stream(self):
        return lib().vg_stream(self.h)

    # ---- test-only knobs (vgx_*, not part of include/vina_gpu.h)
    def debug(self, key, value):
        self._chk(lib().vgx_debug(self.h, key, value), "vgx_debug")

    def memo_probe(self):
        """The IEKF memo at internal nodes' centre planes (vgx_memo_probe):
        samples, mismatches of OctoTree::inside's box, mismatches of the descent
        region k_iekf uses, samples whose plane separates two leaves."""
        out = np.zeros(4, np.int32)
        self._chk(lib().vgx_memo_probe(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))), "vgx_memo_probe")
        return [int(v) for v in out]

    def roots(self):
        """Every root voxel of the device map (vgx_roots): {(x, y, z): (jour stamp,
        flags 1 in slide | 2 isexist, subtree nodes, point_fix points)} — the
        shape of the oracle's Pipeline.roots()."""
        def call(key, jour, flags, nodes, nfix, cap):
            n = ctypes.c_int(0)
            self._chk(lib().vgx_roots(self.h, key, jour, flags, nodes, nfix, cap, ctypes.byref(n)), "vgx_roots")
            return n.value
        n = call(None, None, None, None, None, 0)
        key = np.zeros((max(n, 1), 3), dtype=np.int64)
        jour = np.zeros(max(n, 1))
        arr = [np.zeros(max(n, 1), dtype=np.int32) for _ in range(3)]
        ip = ctypes.POINTER(ctypes.c_int)
        m = call(key.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)), _d(jour), *[a.ctypes.data_as(ip) for a in arr], n)
        assert m == n, (m, n)
        return {tuple(int(v) for v in key[i]): (float(jour[i]), int(arr[0][i]), int(arr[1][i]), int(arr[2][i]))
                for i in range(n)}

    def map_nodes(self):
        """The device map node for node (vgx_map_nodes: a count call, then a data call), as the raw dump of the
        oracle's Pipeline.map_nodes(): "rec" (one record per node, layout in oracle/vina_oracle.h),
        "fixp" / "fix_off" (point_fix per node), "winp" / "win_off" (window points per node and
        physical slot), "win_count", "W" and the ring "mp". Between scans, or inside a stage-level
        scan wherever map_planes may be called; nothing on the device changes."""
        lp = ctypes.POINTER(ctypes.c_int64)
        info = np.zeros(5 + 32, dtype=np.int64)
        self._chk(lib().vgx_map_nodes(self.h, None, 0, None, None, None, None, info.ctypes.data_as(lp)),
                  "vgx_map_nodes")
        n, nf, nw, W = (int(info[i]) for i in (0, 1, 2, 4))
        rec = np.zeros((max(n, 1), 131 + 11 * W))
        fixp, winp = np.zeros((max(nf, 1), 12)), np.zeros((max(nw, 1), 12))
        fix_off, win_off = np.zeros(n + 1, dtype=np.int64), np.zeros(n * W + 1, dtype=np.int64)
        self._chk(lib().vgx_map_nodes(self.h, _d(rec), n, _d(fixp), fix_off.ctypes.data_as(lp), _d(winp),
                                      win_off.ctypes.data_as(lp), info.ctypes.data_as(lp)), "vgx_map_nodes")
        return {"rec": rec[:n], "fixp": fixp[:nf], "winp": winp[:nw], "fix_off": fix_off, "win_off": win_off,
                "win_count": int(info[3]), "W": W, "mp": [int(v) for v in info[5: 5 + W]]}

    def capture_arm(self):
        """Capture the next LM run's first Hessian pass (vgx_debug 5)."""
        self.debug(5, 1)

    def capture_get(self):
        n = ctypes.c_int(0)
        self._chk(lib().vgx_ba_capture(self.h, None, 0, ctypes.byref(n)), "vgx_ba_capture")
        out = np.zeros(max(n.value, 1))
        self._chk(lib().vgx_ba_capture(self.h, _d(out), n.value, ctypes.byref(n)), "vgx_ba_capture")
        return out[: n.value]

    def ba_solve(self, A, b):
        """k_ba_solve on a (15W-15)-unknown symmetric system in identity pivot order."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros(b.shape[0])
        self._chk(lib().vgx_ba_solve(self.h, _d(A), _d(b), _d(x)), "vgx_ba_solve")
        return x

    def ba_step(self, W, hl, imuout, xs, bias, u, v=2.0, calc_hess=1):
        """One LM step's k_ba_prep + k_ba_solve (vgx_ba_step) on the LiDAR system hl (packed lower
        6W x 6W, 6W gradient, residual), the IMU blocks imuout (W-1, 931), the window states xs
        (W, 24) and the bias records (W-1, 12). W is the context's win_size. Returns a dict: dxi,
        xt, bias, q1, res1, ipg, Hcalc (packed lower 15W x 15W), Jcalc. The context must not be
        stepped afterwards."""
        n, L = 15 * W, 6 * W
        hl = np.ascontiguousarray(hl, dtype=np.float64)
        imuout = np.ascontiguousarray(imuout, dtype=np.float64)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        bias = np.ascontiguousarray(bias, dtype=np.float64)
        assert hl.size == L * (L + 1) // 2 + L + 1 and imuout.size == (W - 1) * 931
        assert xs.size == W * 24 and bias.size == (W - 1) * 12
        o = {"dxi": np.zeros(n), "xt": np.zeros((W, 24)), "bias": np.zeros((W - 1, 12)),
             "ipg": np.zeros(n - 15, dtype=np.int32), "Hcalc": np.zeros(n * (n + 1) // 2), "Jcalc": np.zeros(n)}
        qr = np.zeros(2)
        self._chk(lib().vgx_ba_step(self.h, _d(hl), _d(imuout), _d(xs), _d(bias), u, v, calc_hess, _d(o["dxi"]),
                                    _d(o["xt"]), _d(o["bias"]), _d(qr),
                                    o["ipg"].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _d(o["Hcalc"]),
                                    _d(o["Jcalc"])), "vgx_ba_step")
        o["q1"], o["res1"] = float(qr[0]), float(qr[1])
        return o

    BA_STATE_D = ("u", "v", "res1", "res2", "q1")
    BA_STATE_I = ("calc_hess", "done", "iters", "nhess", "fin", "skip")

    def ba_control(self, W, state, imures, rpart, xs, xt, bias):
        """One k_ba_control launch (vgx_ba_control) on the LM state `state` (a dict over BA_STATE_D
        and BA_STATE_I), the IMU residuals (W-1), the residual partials rpart, xs, xt (W, 24) and
        the bias records (W-1, 12). Returns (state, xs, bias, accept) after the launch; accept is
        1, 0, or -1 when the LM had already ended. The context must not be stepped afterwards."""
        sd = np.array([state[k] for k in self.BA_STATE_D], dtype=np.float64)
        si = np.array([state[k] for k in self.BA_STATE_I], dtype=np.int32)
        imures = np.ascontiguousarray(imures, dtype=np.float64)
        rpart = np.ascontiguousarray(rpart, dtype=np.float64)
        xs = np.array(xs, dtype=np.float64).reshape(W, 24)
        xt = np.ascontiguousarray(xt, dtype=np.float64)
        bias = np.array(bias, dtype=np.float64).reshape(W - 1, 12)
        assert imures.size == W - 1 and xt.size == W * 24
        acc = ctypes.c_int(0)
        ip = ctypes.POINTER(ctypes.c_int)
        self._chk(lib().vgx_ba_control(self.h, _d(sd), si.ctypes.data_as(ip), _d(imures), _d(rpart), rpart.size,
                                       _d(xs), _d(xt), _d(bias), ctypes.byref(acc)), "vgx_ba_control")
        out = {k: float(sd[i]) for i, k in enumerate(self.BA_STATE_D)}
        out.update({k: int(si[i]) for i, k in enumerate(self.BA_STATE_I)})
        return out, xs, bias, acc.value

    def ba_factors(self, W, fac_node, nodes, clus, fix, poses, mp_ring, G=0, nrb=0):
        """The LM's LiDAR factor passes on given factors (vgx_ba_factors): the residual pass
        (k_ba_resid), then the Hessian pass (k_ba_hess, k_ba_hfinal) at the same poses. fac_node
        (nf,): each factor's node id; nodes (nn,) with clus (nn, W, 10) by physical slot [P xx xy xz
        yy yz zz, v 3, N] and fix (nn, 10); poses (W, 24); mp_ring (W,): frame -> slot; G / nrb: the
        passes' workgroup counts (0: the LM's own). Returns a dict: H (packed lower 6W x 6W), g (6W),
        res (the Hessian pass's residual), resid (the residual pass's), eig (nf, 12), pcr (nf, 10).
        The context must not be stepped afterwards."""
        ip = ctypes.POINTER(ctypes.c_int)
        fac_node = np.ascontiguousarray(fac_node, dtype=np.int32).reshape(-1)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        clus = np.ascontiguousarray(clus, dtype=np.float64)
        fix = np.ascontiguousarray(fix, dtype=np.float64)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        mp_ring = np.ascontiguousarray(mp_ring, dtype=np.int32)
        nf, nn, L = fac_node.size, nodes.size, 6 * W
        assert clus.size == nn * W * 10 and fix.size == nn * 10 and poses.size == W * 24 and mp_ring.size == W
        nl = L * (L + 1) // 2
        hl, resid = np.zeros(nl + L + 1), np.zeros(1)
        eig, pcr = np.zeros((max(nf, 1), 12)), np.zeros((max(nf, 1), 10))
        self._chk(lib().vgx_ba_factors(self.h, nf, fac_node.ctypes.data_as(ip), nn, nodes.ctypes.data_as(ip),
                                       _d(clus), _d(fix), _d(poses), mp_ring.ctypes.data_as(ip), G, nrb, _d(hl),
                                       _d(resid), _d(eig), _d(pcr)), "vgx_ba_factors")
        return {"H": hl[:nl], "g": hl[nl: nl + L], "res": float(hl[nl + L]), "resid": float(resid[0]),
                "eig": eig[:nf], "pcr": pcr[:nf]}

    LA_OPS = {"eig3": (0, 9, 12), "exp": (1, 3, 9), "exp_dt": (2, 4, 9), "log": (3, 9, 3), "jr": (4, 3, 9),
              "jr_inv": (5, 9, 9), "inverse6": (6, 36, 36), "inverse15": (7, 225, 225), "colpiv_qr": (8, 33, 3),
              "clu_cov": (9, 10, 9), "clu_transform": (10, 22, 10)}

    def la_eval(self, op, x):
        """vg_la.h on the device, one item per row of x (vgx_la_eval, la_probe.hip): (n, in) -> (n, out)."""
        code, nin, nout = self.LA_OPS[op]
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, nin)
        out = np.zeros((x.shape[0], nout))
        self._chk(lib().vgx_la_eval(self.h, code, _d(x), nin, _d(out), nout, x.shape[0]), "vgx_la_eval")
        return out

    def iekf_update(self, partials, n_points, x_curr, x_prop, it, rematch, reduce=False):
        """One k_iekf_update launch (vgx_iekf_update) on the 34 final sums, or with
        reduce on (nb, 34) block partials. Returns x_curr after the update (250),
        G6 (15, 6), nnt (6) and [iters, matches[it], rematch, done]. The context
        must not be stepped afterwards."""
        p = np.ascontiguousarray(partials, dtype=np.float64)
        nb = p.reshape(-1, 34).shape[0] if reduce else -1
        assert reduce or p.size == 34
        xc = np.ascontiguousarray(x_curr, dtype=np.float64)
        xp = np.ascontiguousarray(x_prop, dtype=np.float64)
        assert xc.size == STATE_LEN and xp.size == STATE_LEN
        xo, g = np.zeros(STATE_LEN), np.zeros(96)
        fl = np.zeros(4, dtype=np.int32)
        self._chk(lib().vgx_iekf_update(self.h, nb, _d(p), n_points, _d(xc), _d(xp), it, rematch, _d(xo), _d(g),
                                        fl.ctypes.data_as(ctypes.POINTER(ctypes.c_int))), "vgx_iekf_update")
        return xo, g[:90].reshape(15, 6), g[90:], fl

    def scan_prop(self, x_in, imu, last_end, beg, end):
        """k_scan_prop alone (vgx_scan_prop) on the x_curr block x_in (249: frame state 24, cov 225)
        and the samples imu (n, 7: t, gyr, acc), n <= PROP_MAX (more: VgError -1 before any launch);
        the noises and the gravity scale are the context's. Returns (xc, xp, host): DState::xc and
        xp after the launch and the host propagate()'s block of the same inputs. The context must
        not be stepped afterwards."""
        x_in = np.ascontiguousarray(x_in, dtype=np.float64)
        imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
        assert x_in.size == XC_LEN
        xc, xp, host = np.zeros(XC_LEN), np.zeros(XC_LEN), np.zeros(XC_LEN)
        buf = imu if imu.size else np.zeros((1, 7))
        self._chk(lib().vgx_scan_prop(self.h, _d(x_in), imu.shape[0], _d(buf), last_end, beg, end, _d(xc), _d(xp),
                                      _d(host)), "vgx_scan_prop")
        return xc, xp, host

    def ba_imu(self, W, head, rec, bias, xs, xt, poison=np.nan):
        """The IMU factor workgroups of the LM's factor passes on given records (vgx_ba_imu): rec
        (W-1, 289) in ring slots (head + k) % MAX_WIN, bias (W-1, 12), xs and xt (W, 24); W is the
        context's win_size. Returns a dict of whole buffers, rows past W-1 still `poison`: hess
        (16, 931: k_ba_hess at xs), resid (16: k_ba_resid at xt), rh_out and rh_res (k_ba_resid_hess
        at xt). The context must not be stepped afterwards."""
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        bias = np.ascontiguousarray(bias, dtype=np.float64)
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        xt = np.ascontiguousarray(xt, dtype=np.float64)
        assert rec.size == (W - 1) * IMU_REC and bias.size == (W - 1) * 12 and xs.size == W * 24 and xt.size == W * 24
        o = {"hess": np.zeros((BA_MAX_W, 931)), "resid": np.zeros(BA_MAX_W), "rh_out": np.zeros((BA_MAX_W, 931)),
             "rh_res": np.zeros(BA_MAX_W)}
        self._chk(lib().vgx_ba_imu(self.h, head, _d(rec), _d(bias), _d(xs), _d(xt), poison, _d(o["hess"]),
                                   _d(o["resid"]), _d(o["rh_out"]), _d(o["rh_res"])), "vgx_ba_imu")
        return o


def imu_record(bg, ba, imu, sg, noise_meas, noise_walk):
    """HImuPre::push_imu + record() on the host (vgx_imu_record; no context, no device): biases,
    samples (n, 7), the gravity scale and the 6 x 6 noises -> the 289-double record."""
    bg = np.ascontiguousarray(bg, dtype=np.float64)
    ba = np.ascontiguousarray(ba, dtype=np.float64)
    imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
    nm = np.ascontiguousarray(noise_meas, dtype=np.float64)
    nw = np.ascontiguousarray(noise_walk, dtype=np.float64)
    assert bg.size == 3 and ba.size == 3 and nm.size == 36 and nw.size == 36
    rec = np.zeros(IMU_REC)
    r = lib().vgx_imu_record(_d(bg), _d(ba), _d(imu), imu.shape[0], sg, _d(nm), _d(nw), _d(rec))
    if r != 0:
        raise VgError("vgx_imu_record failed (%d)" % r)
    return rec


class Sync:
    """sync_packages (replay side): host packager of scans and IMU samples."""

    def __init__(self, point_notime=0):
        self.h = lib().vg_sync_create(point_notime)

    def close(self):
        if self.h:
            lib().vg_sync_destroy(self.h)
            self.h = None

    def push_scan(self, header_time, last_point_time, scan_id):
        lib().vg_sync_push_scan(self.h, header_time, last_point_time, scan_id)

    def push_imu(self, imu7):
        a = np.ascontiguousarray(imu7, dtype=np.float64)
        lib().vg_sync_push_imu(self.h, _d(a))

    def pop(self, cap=4096):
        """(scan_id, beg, end, imu (m, 7)), "dropped" (a scan with <= 4 IMU samples was
        consumed), or None (wait for data); VgError when the IMU stream ran dry."""
        sid, m, rd = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        b, e = ctypes.c_double(0), ctypes.c_double(0)
        out = np.zeros((cap, 7))
        r = lib().vg_sync_pop(self.h, ctypes.byref(sid), ctypes.byref(b), ctypes.byref(e), _d(out), cap,
                              ctypes.byref(m), ctypes.byref(rd))
        if r != 0:
            raise VgError("vg_sync_pop: IMU stream ran dry (%d)" % r)
        if rd.value < 0:
            return "dropped"
        return (sid.value, b.value, e.value, out[: m.value].copy()) if rd.value else None


class Multi:
    """Multi-sequence mode (vg_multi_*): B contexts stepped together, one
    native worker thread each."""

    def __init__(self, contexts, spin_us=20, sleep_us=20):
        self.contexts = list(contexts)
        arr = (ctypes.c_void_p * len(self.contexts))(*[c.h.value for c in self.contexts])
        self.h = lib().vg_multi_create(arr, len(self.contexts), spin_us, sleep_us)
        if not self.h:
            raise VgError("vg_multi_create failed")
        self._keep = []

    def step_dev(self, scans):
        """scans: per context (d_x, d_y, d_z, d_intensity, d_time or 0, n, beg, end, imu (m,7) float64)."""
        B = len(self.contexts)
        arr = (ScanDev * B)()
        keep = []
        for b, (x, y, z, i, t, n, beg, end, imu) in enumerate(scans):
            imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
            keep.append(imu)
            arr[b] = ScanDev(x, y, z, i, t or None, n, beg, end, _d(imu), imu.shape[0])
        r = lib().vg_multi_step_dev(self.h, arr)
        if r != 0:
            lib().vg_multi_sync(self.h)  # the workers are idle before their error strings are read
            raise VgError("vg_multi_step_dev failed (%d): %s" % (
                r, "; ".join(lib().vg_last_error(c.h).decode() for c in self.contexts)))

    def set_active(self, cap):
        """At most `cap` sequences on the device at once (vg_multi_set_active)."""
        r = lib().vg_multi_set_active(self.h, int(cap))
        if r != 0:
            raise VgError("vg_multi_set_active failed (%d)" % r)

    def sync(self):
        r = lib().vg_multi_sync(self.h)
        if r != 0:
            raise VgError("vg_multi_sync failed (%d)" % r)

    def close(self):
        if self.h:
            lib().vg_multi_destroy(self.h)
            self.h = None


class Fleet:
    """The fleet (vg_fleet_*): B trackers attached to one owner's map, one frozen scan each per
    step in ten launches for any B. Close order: this Fleet first, then its trackers, then the
    owner (Context.close refuses the other orders; see its docstring). The Fleet holds references
    to all of them, so none is collected before it."""

    def __init__(self, owner, trackers):
        self.owner = owner
        self.trackers = list(trackers)
        arr = (ctypes.c_void_p * len(self.trackers))(*[c.h.value for c in self.trackers])
        self.h = ctypes.c_void_p()
        r = lib().vg_fleet_create(owner.h, arr, len(self.trackers), ctypes.byref(self.h))
        if r != 0:
            self.h = None
            raise VgError("vg_fleet_create failed (%d): %s" % (r, lib().vg_last_error(owner.h).decode()))
        self._keep = None

    def step_dev(self, scans):
        """scans: per tracker (d_x, d_y, d_z, d_intensity, d_time or 0, n, beg, end, imu (m,7) float64),
        or None (n < 0): the tracker sits this step out."""
        B = len(self.trackers)
        arr = (ScanDev * B)()
        keep = []
        for b, sc in enumerate(scans):
            if sc is None:
                arr[b] = ScanDev(None, None, None, None, None, -1, 0.0, 0.0, None, 0)
                continue
            x, y, z, i, t, n, beg, end, imu = sc
            imu = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 7)
            keep.append(imu)
            arr[b] = ScanDev(x or None, y or None, z or None, i or None, t or None, n, beg, end, _d(imu), imu.shape[0])
        r = lib().vg_fleet_step_dev(self.h, arr)
        if r != 0:
            raise VgError("vg_fleet_step_dev failed (%d): %s" % (
                r, "; ".join(lib().vg_last_error(c.h).decode() for c in self.trackers)))

    def sync(self):
        r = lib().vg_fleet_sync(self.h)
        if r != 0:
            raise VgError("vg_fleet_sync failed (%d): %s" % (
                r, "; ".join(lib().vg_last_error(c.h).decode() for c in self.trackers)))

    def close(self):
        if self.h:
            lib().vg_fleet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
