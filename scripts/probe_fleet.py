"""Many sensors in one frozen map: the fleet against what came before it.

The bench workload (64-line, mid360) maps --warmup + --map-scans scans
(probe_checkpoint's recipe) and saves a checkpoint; then --scans frozen scans
per sequence, every sequence replaying the same device-resident scans, at each
B of --batches, two ways:

  (a) B contexts that each load the file, mapping off, stepped by
      vg_multi_step_dev (all a build without map views can do);
  (b) one owner that loads the file and B trackers with tiny maps attached to
      it, stepped by vg_fleet_step_dev.

(a) and (b) alternate for --rounds rounds (as scripts/ab.sh alternates builds);
every round starts from the file's state (a reload, a re-attach). Reported per B
and side: whole-job scans/s of every round, the median, the spread (max - min)
/ median, and the HBM the contexts took (the device's free memory before and
after creating them). GPU_MAX_HW_QUEUES is left as the machine sets it. One JSON
document on stdout, and in --out when given.

    python scripts/probe_fleet.py [--scans 200] [--batches 1,4,8,16] [--rounds 3] [--out FILE]
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

TINY = dict(max_nodes=1024, max_fix_points=1024, hash_log2=10)


def free_bytes(torch):
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--map-scans", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--lidar", default="64line")
    ap.add_argument("--batches", default="1,4,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--file", default="/tmp/probe_fleet.vgck")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence(args.lidar, 0, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    n_map = args.warmup + args.map_scans
    n_all = n_map + args.scans
    scans = [seq.scan(k) for k in range(n_all)]
    max_points = max(s[0].shape[0] for s in scans) + 16
    cfg = vgconfig.to_c(p)
    A = vgpu.Context(cfg, max_points=max_points)
    A.seed(seq.gt_state(0))
    for k in range(n_map):
        xyz, it, b, e = scans[k]
        A.step(xyz, it, b, e, seq.imu(k))
    st = A.stats()
    file_bytes = A.checkpoint_save(args.file)
    A.close()
    frozen = []
    for k in range(n_map, n_all):
        xyz, it, b, e = scans[k]
        t = torch.from_numpy(np.ascontiguousarray(np.concatenate([xyz.T, it[None]], 0).astype(np.float32))).to(dev)
        frozen.append((t, xyz.shape[0], b, e, seq.imu(k)))

    def records(B, k):
        t, n, b, e, imu = frozen[k]
        return [(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 0, n, b, e, imu)] * B

    def run(stepper, B):
        t0 = time.perf_counter()
        for k in range(args.scans):
            stepper.step_dev(records(B, k))
        stepper.sync()
        return B * args.scans / (time.perf_counter() - t0)

    out = {"lidar": args.lidar, "map_scans": n_map, "frozen_scans": args.scans, "rounds": args.rounds,
           "file_bytes": file_bytes, "nodes_used": st["nodes_used"], "fix_used": st["fix_used"],
           "env": {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)")}, "by_B": {}}
    for B in [int(v) for v in args.batches.split(",")]:
        # (a): B private copies
        f0 = free_bytes(torch)
        copies = [vgpu.Context(cfg, max_points=max_points) for _ in range(B)]
        for c in copies:
            c.checkpoint_load(args.file)
            c.set_mapping(False)
        hbm_a = f0 - free_bytes(torch)
        # (b): one owner, B trackers
        f0 = free_bytes(torch)
        M = vgpu.Context(cfg, max_points=max_points)
        M.checkpoint_load(args.file)
        M.set_mapping(False)
        f1 = free_bytes(torch)
        trk = [vgpu.Context(cfg, max_points=max_points, **TINY) for _ in range(B)]
        for t in trk:
            t.attach(M)
        f2 = free_bytes(torch)
        ra, rb = [], []
        for r in range(args.rounds):
            if r > 0:  # back to the file's state
                for c in copies:
                    c.checkpoint_load(args.file)
                for t in trk:
                    t.detach()
                    t.attach(M)
            mv = vgpu.Multi(copies)
            ra.append(run(mv, B))
            mv.close()
            fl = vgpu.Fleet(M, trk)
            rb.append(run(fl, B))
            fl.close()
        same = all(np.array_equal(copies[0].trajectory()[-args.scans:], t.trajectory()[-args.scans:]) for t in trk)

        def summ(v):
            m = statistics.median(v)
            return {"scans_per_s": [round(x, 1) for x in v], "median": round(m, 1),
                    "spread": round((max(v) - min(v)) / m, 4)}
        out["by_B"][str(B)] = {
            "multi_private_copies": dict(summ(ra), hbm_bytes=hbm_a),
            "fleet": dict(summ(rb), hbm_bytes=f0 - f2, hbm_owner_bytes=f0 - f1, hbm_per_tracker_bytes=(f1 - f2) // B),
            "fleet_over_multi": round(statistics.median(rb) / statistics.median(ra), 3),
            "trajectories_equal": bool(same)}
        for c in trk + copies:
            c.close()
        M.close()
        print("B = %d done" % B, json.dumps(out["by_B"][str(B)]), file=sys.stderr, flush=True)
    os.remove(args.file)
    doc = json.dumps(out, indent=1)
    print(doc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
