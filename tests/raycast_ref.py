"""Brute-force numpy restatement of the ray-cast's hit definition (vina_gpu.h
"Ray-casting the map") over Context.map_planes() records, and of vg_scan_diff's
rule on top of ray records; plus the shared GPU workload of test_raycast_gpu and
test_scan_diff_gpu (computed once per process, read-only afterwards).

The snapshot normalises the plane normal, which moves t by rounding only: the
GPU comparison therefore carries a tolerance (1e-9 m) and may leave out rays
whose candidates graze a cube face (near below)."""
import math

import numpy as np

FACE_EPS = 1e-7   # a candidate this close to its cube's surface may fall on either side by rounding
T_MAX, MIN_COS = 100.0, 0.05   # the defaults of vg_ray_params
DEPT = float(np.float32(0.02))                                   # MP::dept (Odometry.dept_err as a float)
BEAM_DV = math.sin(float(np.float32(0.05)) * math.pi / 180.0) ** 2   # MP::beam_dv


def cast(planes, origins, dirs, t_min=0.0, t_max=T_MAX, min_cos=MIN_COS, chunk=32):
    """For every ray the min-t candidate over every plane leaf. Returns (t (inf: none), index into
    planes (-1: none), near: some candidate intersection with t <= the winner's t + FACE_EPS (t_max
    where there is no winner) lies within FACE_EPS of its cube's surface, inside or outside)."""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(np.asarray(origins, dtype=np.float64).reshape(-1, 3), d.shape)
    vc = np.asarray(planes["voxel_center"], dtype=np.float64).reshape(-1, 3)
    hl = 2.0 * np.asarray(planes["quater_length"], dtype=np.float64).reshape(-1)
    c = np.asarray(planes["center"], dtype=np.float64).reshape(-1, 3)
    nrm = np.asarray(planes["normal"], dtype=np.float64).reshape(-1, 3)
    n = d.shape[0]
    t_out, i_out, near = np.full(n, np.inf), np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=bool)
    if vc.shape[0] == 0:
        return t_out, i_out, near
    t_lo = max(t_min, 0.0)
    cn = np.einsum("ij,ij->i", c, nrm)
    with np.errstate(divide="ignore", invalid="ignore"):
        for a in range(0, n, chunk):
            dd, oo = d[a:a + chunk], o[a:a + chunk]
            nd = dd @ nrm.T
            t = (cn[None, :] - oo @ nrm.T) / nd
            ok = (np.abs(nd) >= min_cos) & (t > t_lo) & (t <= t_max)
            ri, li = np.nonzero(ok)
            tt = t[ri, li]
            h = oo[ri] + tt[:, None] * dd[ri]
            lo, hi = vc[li] - hl[li, None], vc[li] + hl[li, None]
            ins = np.all((h >= lo) & (h <= hi), axis=1)
            cheb = np.abs(h - vc[li]).max(axis=1)
            tw = np.full(dd.shape[0], np.inf)
            np.minimum.at(tw, ri[ins], tt[ins])
            win = ins & (tt == tw[ri])
            t_out[a + ri[win]] = tt[win]
            i_out[a + ri[win]] = li[win]
            lim = np.where(np.isfinite(tw), tw, t_max) + FACE_EPS
            graze = (np.abs(cheb - hl[li]) <= FACE_EPS) & (tt <= lim[ri])
            near[a + ri[graze]] = True
    return t_out, i_out, near


def diff_rule(hits, r, gate_sigma=3.0, gate_floor=0.0, min_cos=MIN_COS, t_max=T_MAX):
    """vg_scan_diff's rule on the records of rays cast to t_max along the points' beams (r: the
    measured ranges). Returns (cls, leaf, r_map, gate, margin = |r_map - r| - gate, nan where no hit)."""
    r = np.asarray(r, dtype=np.float64)
    mc2 = min_cos * min_cos
    reach = np.minimum(r + (gate_sigma * np.sqrt(DEPT * DEPT + r * r * BEAM_DV * (1.0 - mc2) / mc2) + 1.0), t_max)
    hit = ((hits["flags"] & 1) != 0) & (hits["range"] <= reach)
    c2 = np.where(hit, hits["ndotd"] ** 2, 1.0)
    g2 = gate_sigma * gate_sigma * (np.where(hit, hits["var"], 0.0) + DEPT * DEPT + r * r * BEAM_DV * (1.0 - c2) / c2)
    gate = np.sqrt(np.maximum(g2, gate_floor * gate_floor))
    diff = hits["range"] - r
    cls = np.zeros(r.shape[0], dtype=np.int32)
    cls[hit & (np.abs(diff) <= gate)] = 1
    cls[hit & (diff > gate)] = 2
    cls[hit & (diff < -gate)] = 3
    return (cls, np.where(hit, hits["leaf"], -1).astype(np.int32), np.where(hit, hits["range"], 0.0),
            np.where(hit, gate, 0.0), np.where(hit, np.abs(diff) - gate, np.nan))


def beams(xyz, pose, ext_R, ext_t):
    """The beams vg_scan_diff casts: (sensor origin (3,), w - o (n, 3), r (n,)) of LiDAR-frame points at pose (12,)."""
    R, p = np.asarray(pose[:9], dtype=np.float64).reshape(3, 3), np.asarray(pose[9:12], dtype=np.float64)
    o = R @ ext_t + p
    w = (np.asarray(xyz, dtype=np.float64) @ ext_R.T + ext_t) @ R.T + p
    dv = w - o
    return o, dv, np.linalg.norm(dv, axis=1)


# ---- the GPU tests' shared workload (tests/loc_common.py: the map after scan 30)
_cache = {}


def fan(pose, ext_t, n_az=64, n_el=32, el_deg=25.0, az0_deg=0.37):
    """(origin, dirs (n_az * n_el, 3)): full circle by +-el_deg from the sensor origin at pose."""
    R, p = np.asarray(pose[:9]).reshape(3, 3), np.asarray(pose[9:12])
    az = np.deg2rad(az0_deg) + np.linspace(0.0, 2.0 * np.pi, n_az, endpoint=False)
    el = np.deg2rad(np.linspace(-el_deg, el_deg, n_el))
    E, A = np.meshgrid(el, az, indexing="xy")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    return R @ ext_t + p, d


def workload():
    """{M: the frozen loaded context (never closed: shared), planes: its plane leaves, o, d: the fan
    of scan 30's pose, hits: M.raycast(o, d), ref: cast(planes, o, d)}."""
    if not _cache:
        import loc_common as lc
        b = lc.base()
        M = lc.loaded(mapping=False)
        planes = M.map_planes()
        o, d = fan(lc.pose_of_row(b["traj"][lc.K0 - 1]), lc.ext()[1])
        _cache.update(M=M, planes=planes, o=o, d=d, hits=M.raycast(o, d), ref=cast(planes, o, d))
    return _cache
