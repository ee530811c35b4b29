"""End-to-end parity of the device pipeline (vg_step) against the oracle's
restatement of thd_odometry_localmapping (local_mapping.cpp:389-547) on the same
synthetic sequence, on every BASELINE config's parameter set:

* every per-scan integer counter agrees exactly: raw / downsampled points, IEKF
  iterations and per-iteration match counts, new roots, slide-map size, factor
  count, LM iterations, the degeneracy flag, and margi's branch counters
  (plane_update calls, leaves past max_points — octree.cpp:441-469);
* poses: the north-star bar ATE <= 1 cm, and a tight bound at what is observed
  (per-scan position difference <= 1e-9 m; observed ~1e-14 m: the device keeps
  the reference's fp64 arithmetic and per-leaf accumulation order, so only the
  summation order of reductions differs).
"""
import numpy as np
import pytest

import oracle
import synth
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

COUNTERS = ("n_raw", "n_ds", "iekf_iters", "iekf_matches", "roots_new", "n_slide", "n_factors", "ba_iters",
            "degenerate", "plane_updates", "fix_full")
TIGHT_M = 1e-9   # per-scan position bound (observed ~1e-14 m)
ATE_M = 0.01     # north star: ATE within 1 cm of the CPU reference


def run_pair(cfgname, lidar, nscan, seq_id=0, max_points=1_100_000, resident=False, nodrain=False, shrink=0):
    """resident: the scans go to the device first and the GPU side runs
    vg_step_dev (no stream drain between scans, as in the bench), so the next
    scan's IEKF overlaps the previous margi's remainder (map_margi).
    nodrain: host buffers through vg_step without reading stats between scans
    (the in-flight upload slots, vina_gpu.cpp upload_scan). shrink: the first
    `shrink` scans keep only their first third of points (both sides), so the
    upload slots grow mid-sequence."""
    p = vgconfig.load(cfgname)
    g = p["General"]
    seq = synth.Sequence(lidar, seq_id, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0))
    gpu = vgpu.Context(vgconfig.to_c(p), max_points=max_points, max_nodes=1_500_000, max_fix_points=6_000_000,
                       hash_log2=21)
    s0 = seq.gt_state(0)
    orc.seed(s0)
    gpu.seed(s0)
    so, sg = [], []
    dev = []
    if resident:
        import torch
        for k in range(nscan):
            xyz, it, b, e = seq.scan(k)
            dev.append(torch.from_numpy(np.ascontiguousarray(np.concatenate([xyz.T, it[None]], 0).astype(np.float32)))
                       .to("cuda:0"))
    for k in range(nscan):
        xyz, it, b, e = seq.scan(k)
        if k < shrink:
            xyz, it = np.ascontiguousarray(xyz[: xyz.shape[0] // 3]), np.ascontiguousarray(it[: it.shape[0] // 3])
        imu = seq.imu(k)
        orc.step(xyz, it, b, e, imu)
        if resident:
            t = dev[k]
            gpu.step_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), xyz.shape[0], b, e, imu)
        else:
            gpu.step(xyz, it, b, e, imu)
        so.append(orc.stats())
        sg.append(gpu.stats() if not (resident or nodrain) else None)
    if resident or nodrain:  # stats of every scan, read only now (no drain while stepping)
        sg = gpu.stats_log()
    return seq, orc, gpu, so, sg


def check_pair(so, sg, to, tg, wo, wg):
    assert len(so) == len(sg)
    for k, (a, b) in enumerate(zip(so, sg)):
        for key in COUNTERS:
            assert a[key] == b[key], (k, key, a[key], b[key])
    assert to.shape == tg.shape and wo.shape == wg.shape
    dpos = np.linalg.norm(to[:, 10:13] - tg[:, 10:13], axis=1)
    drot = np.abs(to[:, 1:10] - tg[:, 1:10]).max()
    print("max dpos %.3e m, max dR %.3e, ATE %.3e m" % (dpos.max(), drot, synth.ate(to, tg)))
    assert synth.ate(to, tg) < ATE_M
    assert dpos.max() < TIGHT_M and drot < TIGHT_M
    assert np.abs(wo[:, 1:25] - wg[:, 1:25]).max() < TIGHT_M  # window states R, p, v, bg, ba, g


# (config, lidar, scans): BASELINE configs[0..4]'s parameter sets. The window
# fills at scan 9 (W = 10): the LM (mid360) and margi run from there, and the
# IEKF matches against planes that margi's plane_update published.
CASES = [
    ("mid360", "16line", 16),
    ("HILTI", "16line", 12),
    ("mid360", "64line", 30),     # the bench workload (BASELINE metric config), margi's max_points branch
    ("HILTI", "64line", 15),      # dense voxel map (voxel 1.0, max_layer 2, BA off)
    ("robosense", "128line", 14),  # 128-line / 200 k rays (voxel 1.0, max_layer 2, BA off)
    ("mid360", "128line", 14),    # the north star's 128-line target on mid360 parameters
    ("mid360", "1M", 11),          # 1,000,064 rays (~870 k points after the blind filter)
    ("velodyne", "16line", 16),   # configs[0]'s parameter set: voxel 1.0, max_layer 3, BA on, blind 0, rotated
                                  # extrinsic (no VLP-16 bag exists here; the same loop the CPU path runs)
]


@pytest.mark.parametrize("cfgname,lidar,nscan", CASES)
def test_pipeline_matches_oracle(oracle_lib, cfgname, lidar, nscan):
    seq, orc, gpu, so, sg = run_pair(cfgname, lidar, nscan)
    check_case(cfgname, lidar, nscan, orc, gpu, so, sg)


def test_resident_pipeline_matches_oracle(oracle_lib):
    """The bench's way of stepping (device-resident scans, vg_step_dev, no
    drain): the overlapped IEKF / margi path, every counter exact."""
    seq, orc, gpu, so, sg = run_pair("mid360", "64line", 30, resident=True)
    check_case("mid360", "64line", 30, orc, gpu, so, sg)


def test_host_input_nodrain_matches_oracle(oracle_lib):
    """Host buffers through vg_step with nothing read back between scans: the
    two in-flight upload slots (pinned copy, DMA, device unpack) are reused
    every other scan and grow at scan 3, the IEKF of an uploaded scan overlaps
    the previous margi remainder; every counter exact."""
    seq, orc, gpu, so, sg = run_pair("mid360", "64line", 30, nodrain=True, shrink=3)
    check_case("mid360", "64line", 30, orc, gpu, so, sg)


def check_case(cfgname, lidar, nscan, orc, gpu, so, sg):
    for k, b in enumerate(sg):
        print(k, {key: b[key] for key in COUNTERS})
    check_pair(so, sg, orc.trajectory(), gpu.trajectory(), orc.window_states(), gpu.window_states())
    W = vgconfig.load(cfgname)["LocalBA"]["win_size"]
    if nscan > W:
        assert sum(s["plane_updates"] for s in sg) > 0
        assert max(s["iekf_matches"][0] for s in sg[W:]) > 0
    if (cfgname, lidar) == ("mid360", "64line"):
        # margi's pcr_fix.N >= max_points branch (octree.cpp:461-469) and the LM were exercised
        assert sum(s["fix_full"] for s in sg) > 0
        assert min(s["ba_iters"] for s in sg[W - 1:]) > 0
        # Hessian passes per scan (the oracle's divide_thread count): ba_iters - ba_hess steps were
        # rejected and retried. No suite workload rejects one (tests/test_ba_step_gpu.py lists the counts)
        assert [s["ba_hess"] for s in sg] == [s["ba_hess"] for s in so]
    gpu.close()
    orc.close()


def test_gravity_scale_matches_oracle(oracle_lib):
    """An IMU reporting in g (Livox Mid-360) with scale_gravity = 9.8: every
    accelerometer sample is scaled in the propagation (imu_ekf.cpp:51) and the
    preintegration (imu_preintegration.cpp:51) on both sides; counters exact,
    poses tight, and the trajectory tracks ground truth."""
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 4, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"],
                         imu_in_g=True)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0, scale_gravity=9.8))
    gpu = vgpu.Context(vgconfig.to_c(p, scale_gravity=9.8), max_points=100_000, max_nodes=500_000,
                       max_fix_points=2_000_000, hash_log2=20)
    s0 = seq.gt_state(0)
    orc.seed(s0)
    gpu.seed(s0)
    so, sg = [], []
    for k in range(14):
        xyz, it, b, e = seq.scan(k)
        imu = seq.imu(k)
        orc.step(xyz, it, b, e, imu)
        gpu.step(xyz, it, b, e, imu)
        so.append(orc.stats())
        sg.append(gpu.stats())
    tg = gpu.trajectory()
    check_pair(so, sg, orc.trajectory(), tg, orc.window_states(), gpu.window_states())
    gt = np.array([seq.gt_pose(k)[1] for k in range(tg.shape[0])])
    assert np.linalg.norm(tg[:, 10:13] - gt, axis=1).max() < 0.05
    gpu.close()
    orc.close()


def test_long_sequence_matches_oracle(oracle_lib):
    """240 scans (24 window lengths) of the 16-line sequence: every counter
    exact and poses tight at every scan, through the node pool's and the
    point_fix arena's growth (reported), long after the window first filled."""
    seq, orc, gpu, so, sg = run_pair("mid360", "16line", 240, seq_id=7, max_points=100_000)
    check_pair(so, sg, orc.trajectory(), gpu.trajectory(), orc.window_states(), gpu.window_states())
    for k in range(39, 240, 40):
        print("scan %d: nodes %d, point_fix %d, slide %d" % (k, sg[k]["nodes_used"], sg[k]["fix_used"],
                                                          sg[k]["n_slide"]))
    assert sum(s["fix_full"] for s in sg) > 0
    gpu.close()
    orc.close()


def test_path_and_local_map_match_oracle(oracle_lib):
    """pub_localtraj / pub_localmap outputs (publishers.cpp:65-131,
    local_mapping.cpp:427,505): the path with the window's BA re-writes, and the
    /map_cmap cloud of the last window BA (vg_set_publish bit 0), against the
    oracle; vg_poll never waits and ends at the full count once the device is
    done."""
    from test_node_core import check_path_and_cmap
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 5, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0))
    gpu = vgpu.Context(vgconfig.to_c(p), max_points=100_000, max_nodes=500_000, max_fix_points=2_000_000,
                       hash_log2=20)
    gpu.set_publish(1)
    orc.seed(seq.gt_state(0))
    gpu.seed(seq.gt_state(0))
    polled = []
    for k in range(16):
        xyz, it, b, e = seq.scan(k)
        orc.step(xyz, it, b, e, seq.imu(k))
        gpu.step(xyz, it, b, e, seq.imu(k))
        polled.append(gpu.poll()[0])
    assert all(0 <= n <= k + 1 for k, n in enumerate(polled)) and polled == sorted(polled)
    path = gpu.path()
    assert gpu.poll() == (16, 16, 16)
    ref = dict(path=orc.path(), cmap=orc.local_map(), cmap_all=orc.local_map(all_points=True))
    gp = np.concatenate([path[:, :1], path[:, 10:13], path[:, 13:14]], 1)
    check_path_and_cmap(gp, gpu.local_map(), ref, TIGHT_M)
    # the re-write moved the window's rows off the post-IEKF poses (the TUM rows)
    tr = gpu.trajectory()
    assert np.abs(path[-10:, 10:13] - tr[-10:, 10:13]).max() > 1e-6
    assert np.array_equal(path[:-10, 1:10], tr[:-10, 1:10])
    gpu.close()
    orc.close()
