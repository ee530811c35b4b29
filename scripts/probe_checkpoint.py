"""What a checkpoint costs: the bench workload (64-line, mid360) for --scans
scans after the warm-up, then one vg_checkpoint_save and one
vg_checkpoint_load into a second context, each split into its phases (host
clocks around stream-synchronised steps, csrc/checkpoint.hip). Prints one
JSON line: the file's bytes beside nodes_used / fix_used, and the milliseconds

    save: compaction + root collection + leaf-run scan | pack + checksum | device -> pinned host | file write
    load: file read + table checks | host -> device | checksum | reset + unpack + hash rebuild

    python scripts/probe_checkpoint.py [--scans 200] [--warmup 12] [--file /tmp/probe.vgck]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vina-slam_amd", "py"))

import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--lidar", default="64line")
    ap.add_argument("--file", default="/tmp/probe_checkpoint.vgck")
    args = ap.parse_args()
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence(args.lidar, 0, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    n = args.warmup + args.scans
    scans = [seq.scan(k) for k in range(n)]
    cap = dict(max_points=max(s[0].shape[0] for s in scans) + 16)
    ctx = vgpu.Context(vgconfig.to_c(p), **cap)
    ctx.seed(seq.gt_state(0))
    for k in range(n):
        xyz, it, b, e = scans[k]
        ctx.step(xyz, it, b, e, seq.imu(k))
    st = ctx.stats()
    t0 = time.perf_counter()
    nbytes, save_ms = ctx.checkpoint_timed(args.file)
    save_wall = (time.perf_counter() - t0) * 1e3
    after = ctx.release_far(census=True)
    ctx.close()
    ctx2 = vgpu.Context(vgconfig.to_c(p), **cap)
    t0 = time.perf_counter()
    _, load_ms = ctx2.checkpoint_timed(args.file, load=True)
    load_wall = (time.perf_counter() - t0) * 1e3
    ctx2.close()
    os.remove(args.file)
    print(json.dumps({
        "lidar": args.lidar, "scans": n, "file_bytes": nbytes, "nodes_used_before": st["nodes_used"],
        "fix_used_before": st["fix_used"], "nodes_after_compaction": after[3], "fix_used_after_compaction": after[5],
        "save_ms": {"compact_roots_runs": round(save_ms[0], 2), "pack_checksum": round(save_ms[1], 2),
                    "d2h": round(save_ms[2], 2), "file_write": round(save_ms[3], 2), "wall": round(save_wall, 2)},
        "load_ms": {"file_read_checks": round(load_ms[0], 2), "h2d": round(load_ms[1], 2),
                    "checksum": round(load_ms[2], 2), "reset_unpack_hash": round(load_ms[3], 2),
                    "wall": round(load_wall, 2)}}))


if __name__ == "__main__":
    main()
