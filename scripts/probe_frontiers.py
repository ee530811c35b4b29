"""Exploration frontiers: the device time of vg_frontiers against one vg_navfn on
the same plane and against the route that existed before it.

Two grids at n x n cells, n from --sizes: tests/frontier_ref.py's rooms(n, n, 1)
(unknown discs in free space: mid-sized frontiers) and its serpentine tiled up
to n x n (corridors of free cells between unknown walls: long thin frontiers that
change tile at every border). Per grid:

  vg_frontiers of the host grid, labels left on the device: HIP events around
    its kernels (vgx_frontier_ms; the host's read of the component count lies
    inside) and the call's wall time, medians of --reps calls after 2 warm-up
    calls, once with k_fr_stats combining the lanes of a wave that lie in one
    component and once with every lane adding for itself (vgx_frontier_combine);
    the same with the labels downloaded;
  vgx_nav_ms of one vg_navfn over the plane that prices a free cell 0 and every
    other cell lethal, from the first free cell: what labelling by navfn-style
    rounds would cost at the least, and the rounds it took;
  the route without it: the download of the grid's n n bytes (timed as a device
    to host copy of that size through torch, null without torch) plus the
    frontier mask in numpy and scipy.ndimage.label with a 3 x 3 structure, wall
    time; and whether scipy finds the same number of components.

One JSON document on stdout, and in --out when given.

    python scripts/probe_frontiers.py [--reps 5] [--sizes 512,2048,4096] [--no-host] [--no-navfn] [--out FILE]
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
import frontier_ref as fr  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

WARM = 2


def stat(v):
    v = v[WARM:]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(ctx, reps, grid, want_labels):
    ms, wall = [], []
    for r in range(reps + WARM):
        t0 = time.perf_counter()
        _, _, s = ctx.frontiers(grid, want_labels=want_labels, max_records=vgpu.FRONTIER_MAX_RECORDS)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(ctx.frontiers_ms())
    return s, {"ms": stat(ms), "wall_ms": stat(wall)}


def download_ms(n_bytes, reps):
    try:
        import torch
    except ImportError:
        return None
    t = torch.zeros(n_bytes, dtype=torch.int8, device="cuda")
    v = []
    for r in range(reps + WARM):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.cpu()
        v.append(1e3 * (time.perf_counter() - t0))
    return stat(v)


def host(grid):
    from scipy import ndimage
    t0 = time.perf_counter()
    m, _, _ = fr.mask(grid)
    t1 = time.perf_counter()
    _, n = ndimage.label(m, structure=np.ones((3, 3), dtype=int))
    t2 = time.perf_counter()
    return n, 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="512,2048,4096")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-navfn", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), device=0, max_points=100_000, max_nodes=1024,
                       max_fix_points=1024, hash_log2=10)
    out = {"reps": args.reps, "warm": WARM, "tile": 64, "runs": []}
    for n in [int(v) for v in args.sizes.split(",") if v]:
        s0 = fr.serpentine_grid()
        tiled = np.tile(s0, (n // s0.shape[0] + 1, n // s0.shape[1] + 1))[:n, :n]
        for kind, grid in (("rooms", fr.rooms(n, n, 1)), ("serpentine", np.ascontiguousarray(tiled))):
            run = {"grid": kind, "nx": n, "ny": n}
            for name, on in (("combined", 1), ("per_lane", 0)):
                vgpu.lib().vgx_frontier_combine(ctx.h, on)
                s, run["on_device_" + name] = timed(ctx, args.reps, grid, False)
            vgpu.lib().vgx_frontier_combine(ctx.h, 1)
            s, run["labels_downloaded"] = timed(ctx, args.reps, grid, True)
            run["summary"] = s
            if not args.no_navfn:
                cost = np.where(grid == fr.FREE, 0, vgpu.COST_LETHAL).astype(np.uint8)
                iy, ix = [int(v[0]) for v in np.nonzero(cost == 0)]
                t0 = time.perf_counter()
                _, sn = ctx.navfn(cost, [[ix, iy]], want_pot=False)
                run["navfn_once"] = {"ms": ctx.navfn_ms(), "wall_ms": 1e3 * (time.perf_counter() - t0), "rounds": sn["rounds"],
                                     "cells_reached": sn["cells_reached"]}
            if not args.no_host:
                n_comp, t_mask, t_label = host(grid)
                run["host"] = {"download_ms": download_ms(n * n, args.reps), "mask_ms": t_mask, "label_ms": t_label,
                               "same_component_count": n_comp == s["n_components"]}
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
