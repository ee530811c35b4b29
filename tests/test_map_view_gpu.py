"""Map views (vg_map_attach / vg_map_detach): a tracker with a tiny map of its
own reads an owner's frozen map and must be, bit for bit, a context that
loaded the owner's checkpoint into a private full copy and froze it (the only
way to localise a second sensor before map views). Workload: tests/loc_common.py.
M is the owner, R the private-copy reference, T the tracker."""
import math

import numpy as np
import pytest

import loc_common as lc
import vgconfig
import vgpu
from test_relocalize_gpu import WINDOW, _rz

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)


def tracker(**cfg):
    return vgpu.Context(vgconfig.to_c(vgconfig.load("mid360"), **cfg), **TINY)


def test_tracker_steps_like_a_private_copy():
    """1: T attached to M steps scans 31..40 with vg_step and equals R stepping
    the same scans: state() after every scan, trajectory rows, path rows and
    stats_log(); M's map is what it was."""
    s = lc.base()["seq"]
    M, R = lc.loaded(mapping=False), lc.loaded(mapping=False)
    snap = (lc.roots(M), lc.planes(M))
    T = tracker()
    T.attach(M)
    assert np.array_equal(T.state(), R.state())
    assert np.array_equal(T.trajectory(), R.trajectory()) and np.array_equal(T.path(), R.path())
    assert T.stats() == R.stats() and T.stats()["nodes_used"] > 0
    for k in range(lc.K0, lc.K0 + 10):
        lc.step(T, s, k)
        lc.step(R, s, k)
        assert np.array_equal(T.state(), R.state()), k
    tt, tr = T.trajectory(), R.trajectory()
    assert tt.shape == (lc.K0 + 10, 13) and tt.tobytes() == tr.tobytes()
    assert T.path().tobytes() == R.path().tobytes()
    st, sr = T.stats_log(), R.stats_log()
    assert len(st) == 10 and st == sr
    assert st[-1]["iekf_matches"][0] > 0 and st[-1]["n_ds"] > 0
    assert T.release_far()[2:] == R.release_far()[2:]  # the census reads the owner's pool
    lc.same_map(M, *snap)
    lc.same_map(T, *snap)  # vg_map_planes and the roots through the view
    T.close()
    M.close()
    R.close()


def test_scoring_and_relocalise_through_the_view():
    """2: score_poses on T equals R's for 16 poses, byte for byte; relocalize
    with test_relocalize_gpu's displaced guess returns the same pose and record."""
    b = lc.base()
    s = b["seq"]
    M, R = lc.loaded(mapping=False), lc.loaded(mapping=False)
    T = tracker()
    T.attach(M)
    xyz = s.scan(lc.K0)[0]
    ref = lc.pose_of_row(b["traj"][lc.K0])
    poses = np.tile(ref, (16, 1))
    for i in range(16):
        poses[i, :9] = (_rz(math.radians(0.5 * (i % 4))) @ ref[:9].reshape(3, 3)).reshape(9)
        poses[i, 9:] += (0.05 * (i // 4), -0.03 * (i % 4), 0.01 * i)
    a, c = T.score_poses(xyz, poses), R.score_poses(xyz, poses)
    assert a.tobytes() == c.tobytes() and a["matches"].max() > 0
    guess = ref.copy()
    guess[:9] = (_rz(math.radians(20)) @ ref[:9].reshape(3, 3)).reshape(9)
    guess[9:] += (1.5, -1.0, 0.0)
    pt, rt, okt = T.relocalize(xyz, guess, install=True, **WINDOW)
    pr, rr, okr = R.relocalize(xyz, guess, install=True, **WINDOW)
    assert okt and okr and pt.tobytes() == pr.tobytes() and rt == rr
    assert np.array_equal(T.state(), R.state())
    T.close()
    M.close()
    R.close()


def _refused(fn):
    with pytest.raises(vgpu.VgError) as ei:
        fn()
    assert "(-5)" in str(ei.value), str(ei.value)


def test_state_machine(tmp_path):
    """3: every call a view rules out returns VG_E_STATE and leaves M's map and
    T's state bit for bit; a differing vg_config is VG_E_ARG; M cannot be
    destroyed under T; after the detach T maps on its own tiny map."""
    b = lc.base()
    s = b["seq"]
    M = lc.loaded(mapping=False)
    T = tracker()
    U = tracker(cold_start=1)
    with pytest.raises(vgpu.VgError) as ei:
        U.attach(M)
    assert "(-1)" in str(ei.value) and "vg_config" in str(ei.value)
    U.close()
    Q = lc.loaded()  # an owner that is still mapping
    _refused(lambda: T.attach(Q))
    Q.close()
    T.attach(M)
    _refused(lambda: T.attach(M))  # already attached
    snap = (lc.roots(M), lc.planes(M))
    before = T.state()
    out = str(tmp_path / "x.vgck")
    for fn in (lambda: T.set_mapping(True), lambda: T.checkpoint_save(out), lambda: T.checkpoint_load(b["path"]),
               T.reset, lambda: T.set_publish(1), lambda: T.set_publish(2),
               lambda: T.shard_host(0, 2, lambda arr: None), lambda: T.profile(stages=True)):
        _refused(fn)
    for fn in (lambda: M.set_mapping(True), M.reset, lambda: M.checkpoint_load(b["path"]),
               lambda: M.checkpoint_save(out), lambda: M.release_far(compact=True),
               lambda: M.shard_host(0, 2, lambda arr: None), M.close, lambda: M.attach(T)):
        _refused(fn)
    assert M.h is not None
    lc.same_map(M, *snap)
    assert np.array_equal(T.state(), before)
    lc.step(M, s, lc.K0)  # the owner may still step frozen scans itself
    assert M.stats()["iekf_matches"][0] > 0
    lc.same_map(M, *snap)
    T.detach()
    _refused(T.detach)
    T.set_mapping(True)
    T.seed(s.gt_state(lc.K0))
    xyz, it, beg, end = s.scan(lc.K0)
    T.step(xyz[:200], it[:200], beg, end, s.imu(lc.K0))  # a scan its 1024-node pool holds
    st = T.stats()
    assert st["n_raw"] == 200 and st["nodes_used"] > 0
    lc.same_map(M, *snap)
    M.close()
    assert M.h is None
    T.close()


def test_captured_graphs_follow_the_map():
    """4: a context replays its IEKF as a captured graph, which holds the map's pointers as they were
    at the capture. (a) A tracker that stepped before attaching (graph on its own, empty map) equals
    R once attached. (c) Detached and attached to a second owner with another map, it equals that
    map's private copy. (b) Detached again, with both owners destroyed, it maps on its own tiny map
    exactly as a fresh tiny context does."""
    s = lc.base()["seq"]
    M, R = lc.loaded(mapping=False), lc.loaded(mapping=False)
    T = tracker()
    T.set_mapping(False)
    T.seed(s.gt_state(lc.K0))
    lc.step(T, s, lc.K0)  # a frozen scan in an empty map: the graph is captured, nothing matches
    assert T.stats()["iekf_matches"] == [0, 0, 0, 0]
    T.attach(M)
    for k in range(lc.K0, lc.K0 + 3):
        lc.step(T, s, k)
        lc.step(R, s, k)
        assert np.array_equal(T.state(), R.state()), k
    assert T.stats_log() == R.stats_log() and T.stats()["iekf_matches"][0] > 0
    assert T.trajectory().tobytes() == R.trajectory().tobytes()
    # (c) a second owner whose map went on for three mapping scans
    M2, R2 = lc.loaded(), lc.loaded()
    for c in (M2, R2):
        for k in range(lc.K0, lc.K0 + 3):
            lc.step(c, s, k)
        c.set_mapping(False)
    assert lc.planes(M2).tobytes() != lc.planes(M).tobytes()
    T.detach()
    T.attach(M2)
    for k in range(lc.K0 + 3, lc.K0 + 6):
        lc.step(T, s, k)
        lc.step(R2, s, k)
        assert np.array_equal(T.state(), R2.state()), k
    assert T.trajectory().tobytes() == R2.trajectory().tobytes()
    assert T.stats_log() == R2.stats_log()[-3:]
    # (b) on its own map again, the owners gone
    T.detach()
    for c in (M, M2, R, R2):
        c.close()
    F = tracker()
    T.set_mapping(True)
    for c in (T, F):
        c.seed(s.gt_state(lc.K0))
    for k in range(lc.K0, lc.K0 + 2):
        xyz, it, beg, end = s.scan(k)
        for c in (T, F):
            c.step(xyz[:200], it[:200], beg, end, s.imu(k))
        assert np.array_equal(T.state(), F.state()), k
        assert T.stats() == F.stats(), k
    assert T.stats()["nodes_used"] > 0 and T.trajectory().tobytes() == F.trajectory().tobytes()
    T.close()
    F.close()
