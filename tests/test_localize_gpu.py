"""Frozen-map (localisation) mode, vg_set_mapping: a context that loaded a
checkpoint steps scans with the map read-only. No oracle (the reference is
single-session): the checks lean on the mapping run of the same build, the map
snapshot and the checkpoint's section table. Workload: tests/loc_common.py."""
import os

import numpy as np
import pytest

import loc_common as lc
import synth
import vgckpt
import vgpu

pytestmark = pytest.mark.gpu

# Test 3's margin. Measured on the MI355X (frozen-map mode): over
# scans 31..50 the mapping run's ATE against the synthetic ground truth is
# 1.511 mm and the frozen run's 1.705 mm (ratio 1.13; largest position
# difference between the two runs 1.056 mm); over scans 32..41 after a
# relocalisation 1.474 mm and 1.726 mm (ratio 1.17). The frozen run matches
# against a map up to 20 scans staler and has no BA behind it, so some loss is
# expected. 1.5 is the measured pair's ratio with room for the staleness to
# cost half of A's own error (about three times the measured loss); the 1 cm
# north-star bar caps the frozen ATE regardless.
ATE_MARGIN = 1.5
ATE_BAR = 0.01


def _frozen_run(B, s, k0, k1):
    for k in range(k0, k1):
        lc.step(B, s, k)
    return B.trajectory()


def test_first_frozen_scan_equals_mapping_scan():
    """1: B (frozen) and C (mapping) load the file and step scan 31: n_raw,
    n_ds, the IEKF's counters, degenerate and the new TUM row are equal bit for
    bit (the IEKF runs before anything touches the map); B's map counters read
    0 and its pool counts are unchanged."""
    b = lc.base()
    s = b["seq"]
    B, C = lc.loaded(mapping=False), lc.loaded()
    before = B.release_far()
    lc.step(B, s, lc.K0)
    lc.step(C, s, lc.K0)
    sb, sc = B.stats(), C.stats()
    for key in ("n_raw", "n_ds", "iekf_iters", "iekf_matches", "degenerate"):
        assert sb[key] == sc[key], (key, sb[key], sc[key])
    tb, tc = B.trajectory(), C.trajectory()
    assert tb.shape == tc.shape == (lc.K0 + 1, 13) and np.array_equal(tb[-1], tc[-1])
    assert np.array_equal(tc[-1], b["traj"][lc.K0])  # C is the uninterrupted run's scan as well
    for key in ("roots_new", "n_slide", "n_factors", "ba_iters", "plane_updates", "fix_full", "v_ins"):
        assert sb[key] == 0, (key, sb[key])
    pb, pc = B.path(), C.path()
    assert pb.shape[0] == lc.K0 + 1 and pb[-1, 13] == pc[-1, 13]  # the row carries the last value of jour
    assert np.array_equal(pb[-1, :13], tb[-1])
    assert np.array_equal(B.state()[1:13], tb[-1, 1:13])  # x_curr is the IEKF's result
    lc.step(B, s, lc.K0 + 1)
    s2 = B.stats()
    assert s2["nodes_used"] == sb["nodes_used"] > 0 and s2["fix_used"] == sb["fix_used"] > 0
    assert before[2:] == B.release_far()[2:]
    B.close()
    C.close()


def test_map_does_not_move(tmp_path):
    """2: after 10 frozen scans B's map is the loaded file's: roots, every
    node's snapshot record, the census, the window states; and a checkpoint
    saved from B has the same map, window and slide sections."""
    b = lc.base()
    s = b["seq"]
    B, D = lc.loaded(mapping=False), lc.loaded()
    for k in range(lc.K0, lc.K0 + 10):
        lc.step(B, s, k)
    lc.same_map(B, lc.roots(D), lc.planes(D))
    assert np.array_equal(B.window_states(), D.window_states())
    assert B.win_count() == D.win_count()
    cb = B.release_far(census=True)
    assert cb[0] == -1 and cb[1] <= 0
    assert cb[2:] == D.release_far(census=True)[2:]
    out = str(tmp_path / "frozen.vgck")
    B.checkpoint_save(out)
    sa, sb = vgckpt.verify(b["path"])[1], vgckpt.verify(out)[1]
    assert set(sa) == set(sb)
    for name in sa:
        if name in ("dstate", "host"):  # the estimator state and the host mirror moved on
            continue
        assert sa[name][1:] == sb[name][1:], name
    lc.same_map(B, lc.roots(D), lc.planes(D))  # (the save itself changed nothing)
    # mapping resumes from the frozen window
    B.set_mapping(True)
    lc.step(B, s, lc.K0 + 10)
    st = B.stats()
    assert st["n_ds"] > 0 and st["v_ins"] > 0 and st["n_factors"] > 0 and st["ba_iters"] > 0
    B.close()
    D.close()


def test_tracking_stays_close_to_mapping_run():
    """3: B steps scans 31..50 frozen, A stepped them mapping. B's ATE against
    the synthetic ground truth is bounded by A's times ATE_MARGIN and by the
    1 cm bar. Measured on the MI355X: see DESIGN.md §5 (frozen-map mode)."""
    b = lc.base()
    s = b["seq"]
    B = lc.loaded(mapping=False)
    tb = _frozen_run(B, s, lc.K0, lc.K1)[lc.K0:lc.K1]
    B.close()
    ta = b["traj"][lc.K0:lc.K1]
    gt = lc.gt_traj(s, lc.K0, lc.K1)
    dmax = np.linalg.norm(tb[:, 10:13] - ta[:, 10:13], axis=1).max()
    ate_a, ate_b = synth.ate(ta, gt), synth.ate(tb, gt)
    print("frozen vs mapping: max |dp| %.6f m, ATE mapping %.6f m, ATE frozen %.6f m" % (dmax, ate_a, ate_b))
    assert ate_b <= ate_a * ATE_MARGIN, (ate_a, ate_b)
    assert ate_b <= ATE_BAR, ate_b


def _refused(fn, word):
    with pytest.raises(vgpu.VgError) as ei:
        fn()
    assert "(-5)" in str(ei.value) and word in str(ei.value), str(ei.value)


def test_state_machine():
    """4: the switch is refused inside an open stage-level scan, on a sharded
    (world 2) context and before a cold start has initialised; with mapping
    off the map stages are refused by name, the open scan stays usable, and
    the context still steps."""
    b = lc.base()
    s = b["seq"]
    B = lc.loaded(mapping=False)
    xyz, it, beg, end = s.scan(lc.K0)
    imu = s.imu(lc.K0)
    B.scan_load(xyz, it)
    B.propagate(imu, beg, end)
    _refused(lambda: B.set_mapping(True), "scan is open")
    _refused(lambda: B.window_push(imu), "vg_window_push")
    _refused(B.cut_voxel_multi, "vg_cut_voxel_multi")
    _refused(B.multi_recut, "vg_multi_recut")
    _refused(B.damping_iter, "vg_damping_iter")
    _refused(B.multi_margi, "vg_multi_margi")
    assert B.downsample_scan() > 0
    B.lio_state_estimation()
    B.step_end()
    assert np.array_equal(B.trajectory()[-1], b["traj"][lc.K0])  # the stage-level frozen scan is the fused one
    lc.step(B, s, lc.K0 + 1)
    assert B.stats()["iekf_matches"][0] > 0 and B.trajectory().shape[0] == lc.K0 + 2
    B.close()
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    _refused(lambda: S.set_mapping(False), "sharded")
    S.close()
    C = lc.ctx(cold_start=1)
    _refused(lambda: C.set_mapping(False), "cold-start")
    C.close()
