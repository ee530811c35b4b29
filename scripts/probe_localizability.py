"""Localisability: the device time of vg_localizability against the two routes
that existed before it.

The localisation tests' workload (16-line sequence 3, mid360) maps --map-scans
scans and freezes the map; the places are the first --places nodes of a 0.375 m
lattice over x in [-18, 18], y in [-8, 8] at z = 1.5, the directions
vg_places_dirs' default table (120 x 12 = 1440), every ray cast to 60 m (the
place index's t_max). Median of --reps calls after 3 warm-up calls:

  vg_localizability, HIP events around k_info_places (vgx_info_ms);
  vg_places_build at the same M and D, HIP events around k_place_cast
    (vgx_places_ms): the same rays without the reduction;
  the route without the call: vg_raycast of the same M D rays in chunks of 256
    places and the numpy sum of w J J^T over the 64-byte records, wall time
    (median of --ref-reps runs), and the part of it spent inside the
    vg_raycast calls;

and vg_scan_info of the next scan's downsampled cloud at its true pose beside
vg_scan_diff of the same cloud (vgx_info_ms, vgx_ray_ms). One JSON document on
stdout, and in --out when given.

    python scripts/probe_localizability.py [--map-scans 31] [--places 4096] [--reps 11] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vina-slam_amd", "py"))

import numpy as np  # noqa: E402
import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

T_MAX = 60.0
DEPT = float(np.float32(0.02))
BEAM_DV = float(np.sin(float(np.float32(0.05)) * np.pi / 180.0) ** 2)


def stat(ms, warm=3):
    return {"median": statistics.median(ms[warm:]), "min": min(ms[warm:]), "max": max(ms[warm:])}


def numpy_route(ctx, pos, dirs, chunk=256):
    """(H (M, 6, 6), seconds inside vg_raycast, bytes of records moved)."""
    D = dirs.shape[0]
    H = np.zeros((pos.shape[0], 6, 6))
    t_cast, moved = 0.0, 0
    for a in range(0, pos.shape[0], chunk):
        p = pos[a:a + chunk]
        t0 = time.perf_counter()
        h = ctx.raycast(np.repeat(p, D, axis=0), np.tile(dirs, (p.shape[0], 1)), t_max=T_MAX)
        t_cast += time.perf_counter() - t0
        moved += h.nbytes
        hit = (h["flags"] & vgpu.RAY_HIT) != 0
        c2 = np.where(hit, h["ndotd"] ** 2, 1.0)
        r = h["range"]
        s2 = c2 * (h["var"] + DEPT * DEPT + (r * r * BEAM_DV) * (1.0 - c2) / c2)
        w = np.where(hit & (s2 > 0), 1.0 / np.where(s2 > 0, s2, 1.0), 0.0)
        n = h["normal"]
        J = np.concatenate([n, np.cross(r[:, None] * np.tile(dirs, (p.shape[0], 1)), n)], axis=1)
        H[a:a + chunk] = np.einsum("pd,pdi,pdj->pij", w.reshape(-1, D), J.reshape(-1, D, 6), J.reshape(-1, D, 6))
    return H, t_cast, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=31)
    ap.add_argument("--places", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ref-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 3, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    ctx = vgpu.Context(vgconfig.to_c(p), device=0, max_points=100_000, max_nodes=400_000, max_fix_points=2_000_000,
                       hash_log2=18)
    ctx.seed(seq.gt_state(0))
    for k in range(args.map_scans):
        xyz, it, b, e = seq.scan(k)
        ctx.step(xyz, it, b, e, seq.imu(k))
    ctx.set_mapping(False)
    lattice = vgpu.place_lattice((-18.0, -8.0), (18.0, 8.0), 0.375, 1.5)[: args.places]
    dirs = vgpu.places_dirs()
    M, D = int(lattice.shape[0]), int(dirs.shape[0])
    out = {"map_scans": args.map_scans, "reps": args.reps, "places": M, "dirs": D, "rays": M * D, "t_max": T_MAX,
           "nodes_used": ctx.stats()["nodes_used"]}
    ms = []
    for r in range(args.reps + 3):
        rec = ctx.localizability(lattice, dirs, t_max=T_MAX)
        ms.append(ctx.info_ms())
    out["localizability_ms"] = stat(ms)
    out["record_bytes"] = int(rec.nbytes)
    out["valid_places"] = int(((rec["flags"] & vgpu.INFO_VALID) != 0).sum())
    out["hit_share"] = float(rec["n_hits"].sum()) / (M * D)
    wall = []
    for r in range(5):
        t0 = time.perf_counter()
        ctx.localizability(lattice, dirs, t_max=T_MAX)
        wall.append(1e3 * (time.perf_counter() - t0))
    out["localizability_wall_ms"] = stat(wall, 1)
    ms = []
    for r in range(args.reps + 3):
        ctx.places_build(lattice)
        ms.append(ctx.places_ms()[0])
    ctx.places_end()
    out["places_build_ms"] = stat(ms)
    out["overhead_over_places_build"] = out["localizability_ms"]["median"] / out["places_build_ms"]["median"]
    wall, cast = [], []
    for r in range(args.ref_reps + 1):
        t0 = time.perf_counter()
        H, t_cast, moved = numpy_route(ctx, lattice, dirs)
        wall.append(1e3 * (time.perf_counter() - t0))
        cast.append(1e3 * t_cast)
    out["raycast_numpy_wall_ms"] = stat(wall, 1)
    out["raycast_calls_wall_ms"] = stat(cast, 1)
    out["raycast_record_bytes"] = int(moved)
    out["raycast_numpy_over_localizability"] = out["raycast_numpy_wall_ms"]["median"] / out["localizability_wall_ms"]["median"]
    scale = np.sqrt(np.einsum("pii,pjj->pij", rec["H"], rec["H"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        out["max_rel_diff_to_numpy"] = float(np.nanmax(np.where(scale > 0, np.abs(H - rec["H"]) / scale, 0.0)))
    # the scan form beside vg_scan_diff
    k = args.map_scans
    xyz, it = seq.scan(k)[:2]
    ds = np.ascontiguousarray(ctx.downsample(xyz, it, 0.1)[:, :3])
    R, t = seq.gt_pose(k)
    pose = np.concatenate([R.reshape(9), t])
    a, b = [], []
    for r in range(args.reps + 3):
        sr = ctx.scan_info(ds, pose)
        a.append(ctx.info_ms())
        ctx.scan_diff(ds, pose)
        b.append(ctx.ray_ms())
    out["scan_points"] = int(ds.shape[0])
    out["scan_info_ms"] = stat(a)
    out["scan_diff_ms"] = stat(b)
    out["scan_info"] = {"n_hits": int(sr["n_hits"]), "eig_t": sr["eig_t"].tolist(), "eig_r": sr["eig_r"].tolist()}
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
