"""The place index: device times of its build and of a query, against brute force.

The localisation tests' workload (16-line sequence 3, mid360) maps --map-scans
scans and freezes the map; the index is the 1 m lattice over x in [-18, 18], y
in [-8, 8] at z = 1.5 (629 places, 120 x 12 bins). Timed with HIP events around
the launches (vgx_places_ms, vgx_score_ms; median of --reps calls after 3
warm-up calls each):

  vg_places_build of the lattice (k_place_cast);
  vg_places_query of the next scan, its true attitude re-yawed by 137 degrees
    (k_place_scan, k_place_scan_finish, k_place_match);
  the comparator: vg_score_poses over the same 629 x 120 (place, yaw)
    hypotheses on the same cloud, in dispatches of up to 65,536 poses;

and the wall time of vg_relocalize_global end to end. One JSON document on
stdout, and in --out when given.

    python scripts/probe_places.py [--map-scans 31] [--reps 21] [--out FILE]
"""
import argparse
import json
import math
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


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def stat(ms):
    return {"median": statistics.median(ms[3:]), "min": min(ms[3:]), "max": max(ms[3:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=31)
    ap.add_argument("--reps", type=int, default=21)
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
    k = args.map_scans
    xyz = seq.scan(k)[0]
    R, t = seq.gt_pose(k)
    ext_t = np.array(g["extrinsic_tran"])
    R_level = rot_z(math.radians(137.0)) @ R
    lattice = vgpu.place_lattice((-18.0, -8.0), (18.0, 8.0), 1.0, 1.5)
    out = {"map_scans": args.map_scans, "reps": args.reps, "scan_points": int(xyz.shape[0]),
           "places": int(lattice.shape[0]), "nodes_used": ctx.stats()["nodes_used"]}
    ms = []
    for r in range(args.reps + 3):
        ctx.places_build(lattice)
        ms.append(ctx.places_ms()[0])
    out["build_ms"] = stat(ms)
    info = ctx.places_info()
    out["valid_places"] = info["n_valid"]
    out["rays"] = int(lattice.shape[0]) * 1440
    out["hit_share"] = float(info["hit_bins"].sum()) / out["rays"]
    ms = []
    for r in range(args.reps + 3):
        cand = ctx.places_query(xyz, R_level, top_k=16)
        ms.append(ctx.places_ms()[1])
    out["query_ms"] = stat(ms)
    org = t + R @ ext_t
    near = int(np.argmin(np.linalg.norm(lattice[:, :2] - org[:2], axis=1)))
    out["true_node"] = near
    out["true_node_rank"] = next((i + 1 for i, c in enumerate(cand) if c["place"] == near), None)
    # brute force: every (place, yaw) hypothesis through vg_score_poses
    A = 120
    poses = np.zeros((lattice.shape[0], A, 12))
    for s in range(A):
        Rs = rot_z(2.0 * math.pi * s / A) @ R_level
        poses[:, s, :9] = Rs.reshape(9)
        poses[:, s, 9:] = lattice - Rs @ ext_t
    poses = poses.reshape(-1, 12)
    ms = []
    for r in range(args.reps + 3):
        tot, best = 0.0, None
        for i0 in range(0, poses.shape[0], vgpu.SCORE_MAX_POSES):
            sc = ctx.score_poses(xyz, poses[i0:i0 + vgpu.SCORE_MAX_POSES])
            tot += ctx.score_ms()
            j = int(np.argmax(sc["matches"]))
            if best is None or sc["matches"][j] > best[0]:
                best = (int(sc["matches"][j]), i0 + j)
        ms.append(tot)
    out["brute_force_ms"] = stat(ms)
    out["brute_force_poses"] = int(poses.shape[0])
    out["brute_force_best"] = {"matches": best[0], "place": best[1] // A, "shift": best[1] % A}
    out["brute_over_query"] = out["brute_force_ms"]["median"] / out["query_ms"]["median"]
    wall = []
    for r in range(5):
        t0 = time.perf_counter()
        pose, rec, c, ok = ctx.relocalize_global(xyz, R_level, top_k=16)
        wall.append(1e3 * (time.perf_counter() - t0))
    out["relocalize_global_wall_ms"] = {"median": statistics.median(wall), "min": min(wall), "max": max(wall)}
    out["relocalize_global"] = {"ok": ok, "matches": rec["matches"], "place": int(c["place"]), "shift": int(c["shift"]),
                                "position_error_to_truth_m": float(np.linalg.norm(pose[9:] - t))}
    ctx.places_end()
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
