"""Terrain layer: the device time of vg_terrain and its per-kernel split against
vg_occupancy on the same rays and against the host route.

probe_occupancy's workload (16-line sequence 3, mid360, --map-scans scans, frozen;
the first M nodes of the 0.375 m lattice at z = 1.5; vgpu.occupancy_dirs()'s fan
with two rows that reach the floor added, every ray cast to 20 m) on a grid of
4096 x 4096 cells of 0.1 m centred on the origins. Per M in --places:

  vg_terrain: HIP events around each kernel (vgx_ter_ms: k_ter_ground, k_ter_cells,
    k_ter_marks, k_ter_classify; median of --reps calls after 3 warm-up calls) and
    the call's wall time;
  vg_occupancy of the same rays on the same grid (vgx_occ_ms): the expectation is
    two of its casts plus a per-cell pass; and vg_occupancy with no origin at all
    on that grid, which is k_occ_classify alone (one lane per cell, one atomic per
    wave and class: what k_ter_classify's strided form is set against);
  the host route, for M <= --host-places: vg_raycast of the rays to the host in
    chunks of 64 origins and tests/terrain_ref.py over the records, wall time
    (once), and in how many cells its elevation and counts differ.

One JSON document on stdout, and in --out when given.

    python scripts/probe_terrain.py [--map-scans 31] [--places 64,1024] [--host-places 64] [--reps 9] [--out FILE]
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
import synth  # noqa: E402
import terrain_ref as tr  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

T_MAX, RES, N = 20.0, 0.1, 4096
BAND = dict(z_lo=-0.3, z_hi=1.0)
PRM = dict(sensor_height=1.4987)   # (1.5 would put every origin's reference on a whole millimetre: uncertain)
ENDED = vgpu.RAY_TRUNCATED | vgpu.RAY_LEFT_RANGE | vgpu.RAY_INVALID
KERNELS = ("k_ter_ground", "k_ter_cells", "k_ter_marks", "k_ter_classify")


def stat(ms, warm=3):
    return {"median": statistics.median(ms[warm:]), "min": min(ms[warm:]), "max": max(ms[warm:])}


def host_route(ctx, pos, dirs, geom, chunk=64):
    """terrain_ref over vg_raycast's records: (result, seconds inside vg_raycast, bytes of records moved)."""
    D = dirs.shape[0]
    O, Dd = np.repeat(pos, D, axis=0), np.tile(dirs, (pos.shape[0], 1))
    t_cast, recs = 0.0, []
    for a in range(0, O.shape[0], chunk * D):
        t0 = time.perf_counter()
        recs.append(ctx.raycast(O[a:a + chunk * D], Dd[a:a + chunk * D], t_max=T_MAX))
        t_cast += time.perf_counter() - t0
    h = np.concatenate(recs)
    r = np.where((h["flags"] & vgpu.RAY_HIT) != 0, h["range"], np.inf)
    ref = tr.terrain(O, Dd, r, h["normal"][:, 2], tr.defaults(**geom, **PRM), ended=(h["flags"] & ENDED) != 0, chunk=256)
    return ref, t_cast, h.nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=31)
    ap.add_argument("--places", default="64,1024")
    ap.add_argument("--host-places", type=int, default=64)
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
    dirs = vgpu.occupancy_dirs(elevations_deg=(-30, -20, -10, 0, 10))
    D = int(dirs.shape[0])
    out = {"map_scans": args.map_scans, "reps": args.reps, "dirs": D, "t_max": T_MAX, "res": RES, "nx": N, "ny": N,
           "nodes_used": ctx.stats()["nodes_used"], "kernels": KERNELS, "runs": []}
    for M in [int(x) for x in args.places.split(",")]:
        pos = lattice[:M]
        c = 0.5 * (pos[:, :2].min(axis=0) + pos[:, :2].max(axis=0))
        # (moved off the lattice's lines, where a ray's cells are ambiguous, as probe_occupancy does)
        geom = dict(x0=float(c[0]) - 0.5 * N * RES - 0.0371, y0=float(c[1]) - 0.5 * N * RES - 0.0173, res=RES, nx=N, ny=N)
        run = {"places": int(pos.shape[0]), "rays": int(pos.shape[0]) * D}
        ms, wall = [], []
        for r in range(args.reps + 3):
            t0 = time.perf_counter()
            grid, elev, step, counts, s = ctx.terrain(pos, dirs, t_max=T_MAX, **geom, **PRM)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(ctx.ter_ms())
        run["terrain_ms"] = {k: stat([m[i] for m in ms]) for i, k in enumerate(KERNELS)}
        run["terrain_ms"]["total"] = stat([sum(m) for m in ms])
        run["terrain_wall_ms"] = stat(wall)
        run["summary"] = s
        ms = []
        for r in range(args.reps + 3):
            ctx.occupancy(pos, dirs, t_max=T_MAX, **geom, **BAND)
            ms.append(ctx.occ_ms())
        run["occupancy_ms"] = stat(ms)
        ms = []
        for r in range(args.reps + 3):
            ctx.occupancy(np.zeros((0, 3)), dirs, t_max=T_MAX, **geom, **BAND)
            ms.append(ctx.occ_ms())
        run["occupancy_classify_only_ms"] = stat(ms)
        run["classify_waves"] = (N * N + 63) // 64
        run["terrain_over_occupancy"] = run["terrain_ms"]["total"]["median"] / run["occupancy_ms"]["median"]
        if M <= args.host_places:
            t0 = time.perf_counter()
            ref, t_cast, moved = host_route(ctx, pos, dirs, geom)
            run["host_route_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            run["host_route_raycast_ms"] = 1e3 * t_cast
            run["host_route_bytes"] = int(moved + 2 * 24 * pos.shape[0] * D)
            run["host_over_device_wall"] = run["host_route_wall_ms"] / run["terrain_wall_ms"]["median"]
            run["uncertain_rays"] = int(ref["uncertain"].sum())
            run["cells_elev_differing_from_numpy"] = int((ref["elev"] != elev).sum())
            run["cells_counts_differing_from_numpy"] = int((ref["counts"] != counts).any(axis=0).sum())
        out["runs"].append(run)
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
