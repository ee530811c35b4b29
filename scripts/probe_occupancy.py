"""Occupancy grid: the device time of vg_occupancy against the only route that
existed before it.

The localisation tests' workload (16-line sequence 3, mid360) maps --map-scans
scans and freezes the map; the origins are the first M nodes of a 0.375 m
lattice over x in [-18, 18], y in [-8, 8] at z = 1.5 (probe_localizability's),
the directions vgpu.occupancy_dirs()'s 1,080, every ray cast to 20 m on a 0.1 m
grid that reaches 20 m past the origins. Per M in --places:

  vg_occupancy: HIP events around k_occ_cast and k_occ_classify (vgx_occ_ms,
    median of --reps calls after 3 warm-up calls) and the call's wall time;
  the route without it: vg_raycast of the same M D rays to the host in chunks of
    256 origins and the numpy rasteriser of tests/occ_ref.py over the 64-byte
    records, wall time (once: it takes minutes at the larger M), the part inside
    the vg_raycast calls, and whether the two grids' counts agree;
  the bytes that leave the device on each route, the atomics per ray (marks inside
    the grid / rays), and vg_localizability of the same rays (vgx_info_ms): the
    same traces followed by a reduction in registers and LDS where vg_occupancy
    walks the lattice, so the difference is what the walk and its atomics cost
    (one workgroup per place there: a fair comparison only where M fills the device).

One JSON document on stdout, and in --out when given.

    python scripts/probe_occupancy.py [--map-scans 31] [--places 64,1024] [--reps 9] [--out FILE]
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
import occ_ref as oc  # noqa: E402
import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

T_MAX, RES, MARGIN = 20.0, 0.1, 20.0
BAND = dict(z_lo=-0.3, z_hi=1.0)
ENDED = vgpu.RAY_TRUNCATED | vgpu.RAY_LEFT_RANGE | vgpu.RAY_INVALID


def stat(ms, warm=3):
    return {"median": statistics.median(ms[warm:]), "min": min(ms[warm:]), "max": max(ms[warm:])}


def host_route(ctx, pos, dirs, geom, chunk=256):
    """(counts, seconds inside vg_raycast, bytes of records moved)."""
    D = dirs.shape[0]
    counts = np.zeros((2, geom["ny"], geom["nx"]), dtype=np.int64)
    t_cast, moved, n_unc = 0.0, 0, 0
    for a in range(0, pos.shape[0], chunk):
        p = pos[a:a + chunk]
        O, Dd = np.repeat(p, D, axis=0), np.tile(dirs, (p.shape[0], 1))
        t0 = time.perf_counter()
        h = ctx.raycast(O, Dd, t_max=T_MAX)
        t_cast += time.perf_counter() - t0
        moved += h.nbytes
        r = np.where((h["flags"] & vgpu.RAY_HIT) != 0, h["range"], np.inf)
        c, unc, _ = oc.marks(O, Dd, r, ended=(h["flags"] & ENDED) != 0, **geom, **BAND)
        counts += c
        n_unc += int(unc.sum())
    return counts, t_cast, moved, n_unc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=31)
    ap.add_argument("--places", default="64,1024")
    ap.add_argument("--reps", type=int, default=9)
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
    lattice = vgpu.place_lattice((-18.0, -8.0), (18.0, 8.0), 0.375, 1.5)
    dirs = vgpu.occupancy_dirs()
    D = int(dirs.shape[0])
    out = {"map_scans": args.map_scans, "reps": args.reps, "dirs": D, "t_max": T_MAX, "res": RES,
           "nodes_used": ctx.stats()["nodes_used"], "runs": []}
    for M in [int(x) for x in args.places.split(",")]:
        pos = lattice[:M]
        x0, y0, nx, ny = vgpu.grid_around(pos, RES, MARGIN)
        # (the lattice's nodes lie on multiples of res: moved off the lines, where a ray's cells are ambiguous)
        geom = dict(x0=x0 - 0.0371, y0=y0 - 0.0173, res=RES, nx=nx + 1, ny=ny + 1)
        run = {"places": int(pos.shape[0]), "rays": int(pos.shape[0]) * D, "nx": geom["nx"], "ny": geom["ny"]}
        ms, wall = [], []
        for r in range(args.reps + 3):
            t0 = time.perf_counter()
            grid, counts, s = ctx.occupancy(pos, dirs, counts=True, t_max=T_MAX, **geom, **BAND)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(ctx.occ_ms())
        run["occupancy_ms"] = stat(ms)
        run["occupancy_wall_ms"] = stat(wall)
        run["summary"] = s
        run["atomics_per_ray"] = (s["free_marks"] + s["occ_marks"]) / s["n_rays"]
        run["device_route_bytes"] = int(grid.nbytes + 128 + pos.nbytes + dirs.nbytes)
        run["device_route_bytes_with_counts"] = run["device_route_bytes"] + int(counts.nbytes)
        ms = []
        for r in range(args.reps + 3):
            ctx.localizability(pos, dirs, t_max=T_MAX)
            ms.append(ctx.info_ms())
        run["localizability_ms"] = stat(ms)
        run["walk_share_of_device_time"] = 1.0 - run["localizability_ms"]["median"] / run["occupancy_ms"]["median"]
        t0 = time.perf_counter()
        ref, t_cast, moved, n_unc = host_route(ctx, pos, dirs, geom)
        run["host_route_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        run["host_route_raycast_ms"] = 1e3 * t_cast
        run["host_route_bytes"] = int(moved + 2 * 24 * pos.shape[0] * D)   # records back, origins and directions up
        run["host_over_device_wall"] = run["host_route_wall_ms"] / run["occupancy_wall_ms"]["median"]
        run["uncertain_rays"] = n_unc
        run["cells_differing_from_numpy"] = int((ref != counts).any(axis=0).sum())
        out["runs"].append(run)
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
