"""View gain: the device time of vg_view_gain against the route that existed
before it, downloading the grid and casting the rays on the host.

One grid of n x n cells (--size, default 4096): tests/frontier_ref.py's
rooms(n, n, 1), unknown discs in free space with few occupied cells, so that
almost every ray runs its full length. The viewpoints: the smallest-index cell of
each of the --views (default 512) largest frontiers vg_frontiers finds on it; the
number of frontiers it finds is recorded beside them. Per radius of --radii:

  vg_view_gain of the grid where a vg_occupancy-style upload left it (the host
    grid is uploaded by the call; the upload lies outside the timed span): HIP
    events around the two memsets and the two kernels (vgx_view_ms) and the
    call's wall time, medians of --reps calls after 2 warm-up calls, once with
    the window's classes read from the grid through the caches and once staged
    in LDS (vgx_view_stage; above R = 208 the two are the same kernel); the same
    with the seen plane downloaded;
  the route without it: the download of the grid's n n bytes (timed as a device
    to host copy of that size through torch, null without torch) plus
    tests/view_ref.py's view_gain on the host, which is vectorised numpy: all
    rays of a batch of viewpoints advance together, one numpy step per ray cell.
    Wall time of one run; and whether its records equal the device's.

One JSON document on stdout, and in --out when given.

    python scripts/probe_view.py [--reps 5] [--size 4096] [--views 512] [--radii 32,128,255] [--no-host] [--out FILE]
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
import view_ref as vr  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

WARM = 2


def stat(v):
    v = v[WARM:]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(ctx, reps, grid, views, R, want_seen):
    ms, wall = [], []
    for r in range(reps + WARM):
        t0 = time.perf_counter()
        rec, _, s = ctx.view_gain(views, R, grid, want_seen=want_seen)
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(ctx.view_gain_ms())
    return rec, s, {"ms": stat(ms), "wall_ms": stat(wall)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--views", type=int, default=512)
    ap.add_argument("--radii", default="32,128,255")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), device=0, max_points=100_000, max_nodes=1024,
                       max_fix_points=1024, hash_log2=10)
    n = args.size
    grid = fr.rooms(n, n, 1)
    _, frec, fs = ctx.frontiers(grid, want_labels=False, max_records=vgpu.FRONTIER_MAX_RECORDS)
    top = frec[np.argsort(-frec["size"].astype(np.int64), kind="stable")[:args.views]]
    views = np.stack([top["label"] % n, top["label"] // n], axis=1).astype(np.int32)
    out = {"reps": args.reps, "warm": WARM, "nx": n, "ny": n, "grid": "rooms", "n_frontiers": int(fs["n_kept"]),
           "n_views": int(views.shape[0]), "host_route": "tests/view_ref.py (vectorised numpy)",
           "download_ms": None if args.no_host else download_ms(n * n, args.reps), "runs": []}
    for R in [int(v) for v in args.radii.split(",") if v]:
        run = {"radius": R, "rays_per_view": 8 * R, "bitmap_bytes": 4 * (((2 * R + 1) ** 2 + 31) // 32)}
        for name, on in (("from_grid", 0), ("staged", 1)):
            vgpu.lib().vgx_view_stage(ctx.h, on)
            rec, s, run["on_device_" + name] = timed(ctx, args.reps, grid, views, R, False)
        vgpu.lib().vgx_view_stage(ctx.h, 0)
        rec, s, run["seen_downloaded"] = timed(ctx, args.reps, grid, views, R, True)
        run["summary"] = s
        if not args.no_host:
            t0 = time.perf_counter()
            want = vr.view_gain(grid, views, R)
            run["host"] = {"view_gain_ms": 1e3 * (time.perf_counter() - t0), "same_records": want[0].tobytes() == rec.tobytes(),
                           "same_summary": want[2] == s}
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
