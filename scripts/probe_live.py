"""Live obstacle layer: the device time of vg_live_mark and vg_live_compose on
one scan of the 64-line synthetic sequence and a 1024 x 1024 grid of 0.1 m cells,
against vg_scan_diff alone on the same scan and against the route that existed
before: download the per-point records, rasterise on the host (tests/live_ref.py,
vectorised numpy) and upload a grid.

A context maps the sequence's first scans, freezes the map, and marks the next
scan (its raw points, as the bench steps them) at the ground-truth pose:
  mark:      vgx_live_ms[0]: HIP events round the two memsets, k_live_points and
             k_live_walk; [1] k_live_walk alone;
  scan_diff: vgx_ray_ms: k_scan_diff and k_diff_sum on the same cloud;
  compose:   vgx_live_ms[2]: k_live_compose over the 2^20 cells;
  host:      wall time of vg_live_mark with per_point (the records' download),
             live_ref.planes + live_ref.compose, and the grid's upload through
             vg_clearance's own path being left out (it is the same either way).
Medians of --reps calls after 2 warm-up calls (the host route: 3 after 2); the planes of the device and of the
host route are compared byte for byte.

    python scripts/probe_live.py [--reps 5] [--size 1024] [--map-scans 12] [--no-host] [--out FILE]
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
import live_ref as lr  # noqa: E402
import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402

WARM = 2


def stat(v):
    v = v[WARM:]
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--res", type=float, default=0.1)
    ap.add_argument("--map-scans", type=int, default=12)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("64line", 3, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    K = args.map_scans
    xyz = np.ascontiguousarray(seq.scan(K)[0], dtype=np.float32)
    ctx = vgpu.Context(vgconfig.to_c(p), device=0, max_points=xyz.shape[0] + 200_000, max_nodes=600_000,
                       max_fix_points=2_000_000, hash_log2=20)
    ctx.seed(seq.gt_state(0))
    for k in range(K):
        s = seq.scan(k)
        ctx.step(s[0], s[1], s[2], s[3], seq.imu(k))
    ctx.set_mapping(False)
    R, t = seq.gt_pose(K)
    pose = np.concatenate([np.asarray(R).reshape(9), np.asarray(t)])
    n, res = args.size, args.res
    o = np.asarray(R) @ np.asarray(g["extrinsic_tran"], dtype=np.float64) + np.asarray(t)
    geom = dict(x0=float(o[0] - 0.5 * n * res - 0.37 * res), y0=float(o[1] - 0.5 * n * res - 0.61 * res), res=res,
                nx=n, ny=n)
    prm = dict(z_lo=-0.5, z_hi=0.5, r_min=0.5, mark_max=30.0, clear_max=40.0, flags=1)
    base = np.full((n, n), -1, dtype=np.int8)
    ctx.live_begin(base, **geom, **prm)
    mark, walk, comp, diff, host_dl = [], [], [], [], []
    for r in range(args.reps + WARM):
        ctx.live_clear()
        s = ctx.live_mark(xyz, pose, stamp=1)
        ms = ctx.live_ms()
        mark.append(ms[0]), walk.append(ms[1])
        ctx.live_compose(want_grid=False)
        comp.append(ctx.live_ms()[2])
        ctx.scan_diff(xyz, pose)
        diff.append(ctx.ray_ms())
    hit, clear, _ = ctx.live_info()
    out = {"reps": args.reps, "warm": WARM, "lidar": "64line", "scan": K, "points": int(xyz.shape[0]), "nx": n, "ny": n,
           "res": res, "params": prm, "summary": s,
           "cells_hit": int((hit > 0).sum()), "cells_cleared": int((clear > 0).sum()),
           "kernels": {"vg_live_mark (memsets, k_live_points, k_live_walk)": stat(mark), "k_live_walk": stat(walk),
                       "vg_scan_diff (k_scan_diff, k_diff_sum)": stat(diff), "k_live_compose": stat(comp)}}
    if not args.no_host:
        ras = []
        for r in range(3 + WARM):  # (numpy takes seconds a run: three measured runs)
            ctx.live_clear()
            t0 = time.perf_counter()
            _, rec = ctx.live_mark(xyz, pose, stamp=1, per_point=True)
            t1 = time.perf_counter()
            h, c, _ = lr.planes(rec, 1, n, n)
            grid = lr.compose(base, h, c, 1)
            t2 = time.perf_counter()
            host_dl.append(1e3 * (t1 - t0)), ras.append(1e3 * (t2 - t1))
        dev_grid, _ = ctx.live_compose()
        out["host"] = {"route": "vg_live_mark with per_point (records downloaded), tests/live_ref.py planes + compose",
                       "mark_with_records_wall_ms": stat(host_dl), "rasterise_ms": stat(ras),
                       "same_planes": h.tobytes() == hit.tobytes() and c.tobytes() == clear.tobytes(),
                       "same_grid": grid.tobytes() == dev_grid.tobytes()}
    m = out["kernels"]
    med = lambda k: m[k]["median"]  # noqa: E731
    out["ratios"] = {"mark_over_scan_diff": med("vg_live_mark (memsets, k_live_points, k_live_walk)") /
                     med("vg_scan_diff (k_scan_diff, k_diff_sum)"),
                     "walk_share_of_mark": med("k_live_walk") / med("vg_live_mark (memsets, k_live_points, k_live_walk)"),
                     "compose_over_mark": med("k_live_compose") / med("vg_live_mark (memsets, k_live_points, k_live_walk)")}
    if "host" in out:
        out["ratios"]["host_rasterise_over_device_walk_and_compose"] = out["host"]["rasterise_ms"]["median"] / (
            med("k_live_walk") + med("k_live_compose"))
    ctx.live_end()
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
