"""Clearance field: the device time of vg_clearance against the route that
existed before it.

The localisation tests' workload (16-line sequence 3, mid360) maps --map-scans
scans and freezes the map; vg_occupancy casts vgpu.occupancy_dirs()'s 1,080
directions to 20 m from the first 256 nodes of probe_occupancy's 0.375 m lattice
into a square grid of n x n cells over the same 51.2 m x 51.2 m, n = 1024 (0.05 m
cells) and n = 4096 (0.0125 m cells). A third grid is the search's worst case:
4096 x 4096 free cells and one obstacle in a corner, so that every cell's row
search runs to the obstacle's column. The robot: inscribed 0.3 m, inflation 1.0 m,
cost scaling 3 / m. Per grid:

  vg_clearance of the host grid with all three outputs downloaded: HIP events
    around k_clr_cols and k_clr_rows (vgx_clr_ms) and the call's wall time,
    medians of --reps calls after 3 warm-up calls;
  vg_clearance with grid == NULL (the grid where vg_occupancy left it; for the
    synthetic grid a host grid, nothing of the kind being on the device) and only
    `cost` downloaded: the same two figures;
  the route without it, on the grid vg_occupancy already returned:
    scipy.ndimage.distance_transform_edt with return_indices=True and the numpy
    cost of tests/clr_ref.py, wall time, median of --host-reps runs;
  whether the two routes' dist2 and cost agree in every cell.

One JSON document on stdout, and in --out when given.

    python scripts/probe_clearance.py [--map-scans 31] [--reps 9] [--host-reps 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vina-slam_amd", "py"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import clr_ref as cr  # noqa: E402
import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

T_MAX, SPAN = 20.0, 51.2
BAND = dict(z_lo=-0.3, z_hi=1.0)
ROBOT = dict(inscribed_radius=0.3, inflation_radius=1.0, cost_scaling=3.0)


def stat(ms, warm=3):
    return {"median": statistics.median(ms[warm:]), "min": min(ms[warm:]), "max": max(ms[warm:])}


def device(ctx, reps, grid, res, want, **shape):
    ms, wall = [], []
    for r in range(reps + 3):
        t0 = time.perf_counter()
        out, s = ctx.clearance(grid, res=res, want=want, **shape, **ROBOT)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(ctx.clearance_ms())
    return out, s, stat(ms), stat(wall)


def host(grid, res, reps):
    from scipy import ndimage
    wall = []
    for r in range(reps):
        t0 = time.perf_counter()
        obst = grid == vgpu.OCC_OCCUPIED
        edt, idx = ndimage.distance_transform_edt(~obst, return_indices=True)
        dist2 = np.rint(edt * edt).astype(np.int32)
        nearest = (idx[0] * grid.shape[1] + idx[1]).astype(np.int32)
        cost = cr.cost(grid, dist2, res=res, **ROBOT)
        wall.append(1e3 * (time.perf_counter() - t0))
    return dist2, nearest, cost, {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=31)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 3, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    ctx = vgpu.Context(vgconfig.to_c(p), device=0, max_points=300_000, max_nodes=400_000, max_fix_points=2_000_000,
                       hash_log2=18)
    ctx.seed(seq.gt_state(0))
    for k in range(args.map_scans):
        xyz, it, b, e = seq.scan(k)
        ctx.step(xyz, it, b, e, seq.imu(k))
    ctx.set_mapping(False)
    pos = vgpu.place_lattice((-18.0, -8.0), (18.0, 8.0), 0.375, 1.5)[:256]
    dirs = vgpu.occupancy_dirs()
    out = {"map_scans": args.map_scans, "reps": args.reps, "host_reps": args.host_reps, "robot": ROBOT,
           "places": int(pos.shape[0]), "dirs": int(dirs.shape[0]), "runs": []}
    cases = [("occupancy", 1024), ("occupancy", 4096), ("one obstacle", 4096)]
    for kind, n in cases:
        res = SPAN / n
        run = {"grid": kind, "nx": n, "ny": n, "res": res}
        if kind == "occupancy":
            # (moved off the lattice's lines, where a ray's cells are ambiguous, as probe_occupancy does)
            geom = dict(x0=-0.5 * SPAN - 0.0371 * res, y0=-0.5 * SPAN - 0.0173 * res, res=res, nx=n, ny=n)
            grid, _, so = ctx.occupancy(pos, dirs, t_max=T_MAX, **geom, **BAND)
            run["occupancy_ms"] = ctx.occ_ms()
            run["occupancy_summary"] = so
            chained = dict(grid=None, nx=n, ny=n)
        else:
            grid = np.zeros((n, n), dtype=np.int8)
            grid[0, 0] = vgpu.OCC_OCCUPIED
            chained = dict(grid=grid)
        full, s, ms, wall = device(ctx, args.reps, grid, res, ("dist2", "nearest", "cost"))
        run["summary"] = s
        run["all_outputs_ms"], run["all_outputs_wall_ms"] = ms, wall
        only, s1, ms, wall = device(ctx, args.reps, chained.pop("grid"), res, ("cost",), **chained)
        run["cost_only_chained_ms"], run["cost_only_chained_wall_ms"] = ms, wall
        dist2, nearest, cost, hw = host(grid, res, args.host_reps)
        run["host_route_wall_ms"] = hw
        run["host_over_device_wall_all_outputs"] = hw["median"] / run["all_outputs_wall_ms"]["median"]
        run["host_over_device_wall_cost_only"] = hw["median"] / run["cost_only_chained_wall_ms"]["median"]
        run["cells_differing_dist2"] = int((full["dist2"] != dist2).sum())
        run["cells_differing_cost"] = int((full["cost"] != cost).sum())
        run["cost_only_equals_all_outputs"] = bool(only["cost"].tobytes() == full["cost"].tobytes() and s1 == s)
        # scipy breaks ties its own way: only that its obstacle is as near is checked
        iy, ix = np.divmod(np.arange(n * n, dtype=np.int64), n)
        nn = nearest.ravel().astype(np.int64)
        run["scipy_nearest_attains_dist2"] = bool(np.array_equal((ix - nn % n) ** 2 + (iy - nn // n) ** 2,
                                                                 full["dist2"].ravel()))
        out["runs"].append(run)
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
