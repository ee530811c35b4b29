"""Cost of the /voxel_plane + /voxel_normal markers on the 64-line mid360
workload: scans/s with vg_set_publish bit 1 set and vg_markers read after
every scan (which completes the scan), beside the same loop with the markers
off and no read. The collection kernel's own span comes from a kernel trace
of this script:

    rocprofv3 --kernel-trace --stats -d prof_out -- python scripts/probe_markers.py --on-only
    (k_mk_collect's row of the *_kernel_stats.csv it writes)
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vina-slam_amd", "py"))

import synth  # noqa: E402
import vgconfig  # noqa: E402
import vgpu  # noqa: E402


def run(seq, p, scans, on, nscan, warm):
    ctx = vgpu.Context(vgconfig.to_c(p), device=0)
    if on:
        ctx.set_publish(2)
    ctx.seed(seq.gt_state(0))
    events = 0
    t0 = None
    for k in range(nscan):
        if k == warm:
            ctx.stats()  # completes the warm-up scans
            t0 = time.perf_counter()
        xyz, it, b, e, imu = scans[k]
        ctx.step(xyz, it, b, e, imu)
        if on:
            ev, _ = ctx.markers()
            events += ev.shape[0] if k >= warm else 0
    ctx.stats()
    dt = time.perf_counter() - t0
    ctx.close()
    n = nscan - warm
    return {"markers": bool(on), "scans": n, "scans_per_s": n / dt, "ms_per_scan": 1e3 * dt / n,
            "events_per_scan": events / n}


def main():
    nscan, warm = 60, 20
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("64line", 0, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    scans = [seq.scan(k) + (seq.imu(k),) for k in range(nscan)]
    out = []
    if "--on-only" not in sys.argv:
        out.append(run(seq, p, scans, False, nscan, warm))
    out.append(run(seq, p, scans, True, nscan, warm))
    for r in out:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
