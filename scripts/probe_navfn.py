"""Navigation function: the device time of vg_navfn and vg_nav_paths against the
route that existed before them.

probe_clearance.py's scenes: the localisation tests' workload (16-line sequence
3, mid360) maps --map-scans scans and freezes the map; vg_occupancy casts 1,080
directions to 20 m from 256 lattice nodes into n x n cells over 51.2 m x 51.2 m, n
= 1024 and n = 4096; vg_clearance (inscribed 0.3 m, inflation 1.0 m, scaling 3 /
m) leaves the cost plane on the device. The goal is the passable cell nearest
the grid's centre. A third plane is a 4096 x 4096 maze: free corridors 32 cells
wide between lethal walls 32 cells thick, each wall open for 32 cells at one end,
the ends alternating, the goal in the first corridor's closed corner: the field
has to run the whole serpentine, 64 corridors of 4096 cells. Per plane:

  vg_navfn with cost == NULL (the maze: a host plane) and the field left on the
    device: HIP events from the field's fill to the summary kernel (vgx_nav_ms;
    the host's reads of the round counters lie inside), the call's wall time, and
    the rounds and tile runs it took, medians of --reps calls after 2 warm-up
    calls; the same with the field downloaded;
  an estimate of the rounds the scheme needs: one more than the tile borders
    crossed by the path vg_nav_paths takes from the cell of max_pot. No bound:
    another shortest path may cross fewer borders, another cell may need more;
  vg_nav_paths of 256 starts drawn from the reached cells, max_len 65536: device
    and wall time;
  the route without it, on the downloaded cost: scipy.sparse.csgraph.dijkstra
    over the same graph, wall time of building the graph and of the search;
  whether the two fields agree in every cell.

One JSON document on stdout, and in --out when given.

    python scripts/probe_navfn.py [--map-scans 31] [--reps 5] [--sizes 1024,4096] [--no-maze] [--out FILE]
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
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

T_MAX, SPAN = 20.0, 51.2
BAND = dict(z_lo=-0.3, z_hi=1.0)
ROBOT = dict(inscribed_radius=0.3, inflation_radius=1.0, cost_scaling=3.0)
WARM = 2


def stat(v):
    v = v[WARM:]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def maze(n, pitch=32):
    """uint8 [n, n]: corridors `pitch` rows high between lethal walls `pitch` rows thick, each wall open over its
    last (even walls) or first (odd walls) `pitch` columns."""
    c = np.zeros((n, n), dtype=np.uint8)
    for k, y in enumerate(range(pitch, n, 2 * pitch)):
        c[y:y + pitch] = vgpu.COST_LETHAL
        if k % 2 == 0:
            c[y:y + pitch, n - pitch:] = 0
        else:
            c[y:y + pitch, :pitch] = 0
    return c


def host(cost, trav, goal):
    """(pot uint32 [ny, nx], seconds building the graph, seconds searching it) by scipy."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    t0 = time.perf_counter()
    ny, nx = cost.shape
    t = trav.astype(np.int64)[cost]
    ok = t > 0
    idx = np.arange(nx * ny, dtype=np.int32).reshape(ny, nx)
    rows, cols, wts = [], [], []
    for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 1)):                 # each undirected edge once
        a = (slice(0, ny - dy), slice(max(0, -dx), nx - max(0, dx)))
        b = (slice(dy, ny), slice(max(0, dx), nx + min(0, dx)))
        e = ok[a] & ok[b]
        if dx and dy:
            e &= ok[a[0], b[1]] & ok[b[0], a[1]]
        rows.append(idx[a][e])
        cols.append(idx[b][e])
        wts.append(((17 if dx and dy else 12) * (t[a] + t[b]))[e].astype(np.float64))
    m = coo_matrix((np.concatenate(wts), (np.concatenate(rows), np.concatenate(cols))), shape=(nx * ny, nx * ny)).tocsr()
    t1 = time.perf_counter()
    d = dijkstra(m, directed=False, indices=[goal[1] * nx + goal[0]], min_only=True)
    t2 = time.perf_counter()
    pot = np.where(np.isinf(d), vgpu.NAV_UNREACHED, np.minimum(d, vgpu.NAV_SAT)).astype(np.uint32).reshape(ny, nx)
    return pot, t1 - t0, t2 - t1


def field(ctx, reps, cost, goal, want_pot, **shape):
    ms, wall, rounds, runs = [], [], [], []
    for r in range(reps + WARM):
        t0 = time.perf_counter()
        pot, s = ctx.navfn(cost, [goal], want_pot=want_pot, **shape)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(ctx.navfn_ms())
        rounds.append(s["rounds"])
        runs.append(s["tile_runs"])
    return pot, s, {"ms": stat(ms), "wall_ms": stat(wall), "rounds": stat(rounds), "tile_runs": stat(runs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=31)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--no-maze", action="store_true")
    ap.add_argument("--no-host", action="store_true")
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
    trav = vgpu.nav_trav_table()
    out = {"map_scans": args.map_scans, "reps": args.reps, "warm": WARM, "robot": ROBOT, "tile": 64, "runs": []}
    cases = [("costmap", int(n)) for n in args.sizes.split(",") if n] + ([] if args.no_maze else [("maze", 4096)])
    for kind, n in cases:
        res = SPAN / n
        run = {"plane": kind, "nx": n, "ny": n, "res": res}
        if kind == "costmap":
            geom = dict(x0=-0.5 * SPAN - 0.0371 * res, y0=-0.5 * SPAN - 0.0173 * res, res=res, nx=n, ny=n)
            ctx.occupancy(pos, dirs, t_max=T_MAX, **geom, **BAND)
            o, _ = ctx.clearance(None, nx=n, ny=n, res=res, want=("cost",), **ROBOT)
            cost = o["cost"]
            run["clearance_ms"] = ctx.clearance_ms()
            iy, ix = np.nonzero(trav[cost] > 0)
            j = int(np.argmin((ix - n // 2) ** 2 + (iy - n // 2) ** 2))
            goal = [int(ix[j]), int(iy[j])]
            chained = dict(cost=None, nx=n, ny=n)
        else:
            cost = maze(n)
            goal = [0, 0]
            chained = dict(cost=cost)
        run["goal"] = goal
        _, s, run["field_on_device"] = field(ctx, args.reps, chained.pop("cost"), goal, False, **chained)
        pot, s, run["field_downloaded"] = field(ctx, args.reps, cost, goal, True)
        run["summary"] = {k: v for k, v in s.items() if k not in vgpu.NAV_SCHEDULING}
        # the longest shortest path, and the tile borders it crosses
        far = int(np.argmax(np.where(pot >= vgpu.NAV_SAT, 0, pot)))
        cells, ln, status, _ = ctx.nav_paths([[far % n, far // n]], 1 << 24)
        c = cells[0, :ln[0]].astype(np.int64)
        tiles = (c // n // 64) * ((n + 63) // 64) + c % n // 64
        run["longest_path"] = {"cells": int(ln[0]), "status": int(status[0]), "tile_borders": int((np.diff(tiles) != 0).sum()),
                               "device_ms": ctx.navfn_ms()}
        run["rounds_needed_estimate"] = run["longest_path"]["tile_borders"] + 1
        # 256 paths
        ry, rx = np.nonzero(pot < vgpu.NAV_SAT)
        pick = np.random.default_rng(1).choice(rx.size, size=256, replace=False)
        starts = np.stack([rx[pick], ry[pick]], axis=1).astype(np.int32)
        ms, wall = [], []
        for r in range(args.reps + WARM):
            t0 = time.perf_counter()
            cells, ln, status, pc = ctx.nav_paths(starts, 65536)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms.append(ctx.navfn_ms())
        run["paths_256"] = {"ms": stat(ms), "wall_ms": stat(wall), "reached": int((status == vgpu.NAV_REACHED).sum()),
                            "truncated": int((status == vgpu.NAV_TRUNCATED).sum()), "mean_len": float(ln.mean()),
                            "max_len": int(ln.max())}
        if not args.no_host:
            ref, t_build, t_search = host(cost, trav, goal)
            run["host_dijkstra"] = {"build_graph_s": t_build, "search_s": t_search}
            run["cells_differing"] = int((ref != pot).sum())
            run["host_search_over_device_wall"] = 1e3 * t_search / run["field_on_device"]["wall_ms"]["median"]
        out["runs"].append(run)
        print(json.dumps(run), file=sys.stderr, flush=True)
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
