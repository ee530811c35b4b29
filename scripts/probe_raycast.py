"""Ray-casting the map: device times of vg_scan_diff and vg_raycast.

The bench workload (64-line, mid360) maps --map-scans scans, freezes the map,
then times (HIP events around the launches, vgx_ray_ms; median of --reps calls
after 3 warm-up calls each):

  scan_diff of the next scan's downsampled cloud at the run's pose for it;
  raycast of a 64 x 32 fan (2,048 rays) from that pose's sensor origin;

and, for scale, k_iekf's per-launch time over the mapped scans (vg_profile's
in-kernel clock). With a VG_PROBE library (make probe; VINA_GPU_LIB=
vina-slam_amd/lib_probe/libvina_gpu.so) the records' reserved field carries the
cells + nodes a ray visited: their mean is reported. One JSON document on
stdout, and in --out when given.

    python scripts/probe_raycast.py [--map-scans 60] [--reps 21] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vina-slam_amd", "py"))

import numpy as np  # noqa: E402
import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map-scans", type=int, default=60)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--lidar", default="64line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence(args.lidar, 0, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    ctx = vgpu.Context(vgconfig.to_c(p), device=0, max_points=300_000)
    ctx.seed(seq.gt_state(0))
    ctx.profile(on=True, clock=True)
    for k in range(args.map_scans):
        xyz, it, b, e = seq.scan(k)
        ctx.step(xyz, it, b, e, seq.imu(k))
    prof = ctx.profile_read()
    ctx.profile(on=False)
    ctx.set_mapping(False)
    k = args.map_scans
    xyz, it, b, e = seq.scan(k)
    ds = np.ascontiguousarray(ctx.downsample(xyz, it, p["Odometry"]["down_size"])[:, :3])
    ctx.step(xyz, it, b, e, seq.imu(k))   # a frozen scan: the pose of scan k in the map
    pose = ctx.state()[1:13]
    R, t = pose[:9].reshape(3, 3), pose[9:]
    az = np.deg2rad(0.37) + np.linspace(0.0, 2.0 * np.pi, 64, endpoint=False)
    el = np.deg2rad(np.linspace(-25.0, 25.0, 32))
    E, A = np.meshgrid(el, az, indexing="xy")
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
    o = R @ np.array(g["extrinsic_tran"]) + t
    out = {"lidar": args.lidar, "map_scans": args.map_scans, "reps": args.reps, "scan_points": int(ds.shape[0]),
           "nodes_used": ctx.stats()["nodes_used"], "probe_build": "lib_probe" in vgpu.LIB}
    ms = []
    for r in range(args.reps + 3):
        summ, pp = ctx.scan_diff(ds, pose, per_point=True)
        ms.append(ctx.ray_ms())
    out["scan_diff_ms"] = {"median": statistics.median(ms[3:]), "min": min(ms[3:]), "max": max(ms[3:])}
    out["scan_diff_summary"] = summ
    ms = []
    for r in range(args.reps + 3):
        hits = ctx.raycast(o, d)
        ms.append(ctx.ray_ms())
    out["raycast_2048_ms"] = {"median": statistics.median(ms[3:]), "min": min(ms[3:]), "max": max(ms[3:])}
    out["raycast_hits"] = int(((hits["flags"] & 1) != 0).sum())
    if out["probe_build"]:
        out["mean_steps_raycast"] = float(hits["reserved"].mean())
        out["max_steps_raycast"] = float(hits["reserved"].max())
        w = (ds.astype(np.float64) @ np.array(g["extrinsic_rota"]).reshape(3, 3).T + np.array(g["extrinsic_tran"])) @ R.T + t
        beams = ctx.raycast(o, w - o)   # the scan's beams, cast to 100 m (scan_diff stops ~1-2 m past the point)
        out["mean_steps_scan_beams_100m"] = float(beams["reserved"].mean())
    out["k_iekf"] = {k: prof[k] for k in ("iekf_kernel", "k_iekf_clock") if k in prof}   # vg_profile_read's pairs
    ctx.close()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
