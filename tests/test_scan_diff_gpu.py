"""vg_scan_diff on the GPU against the numpy restatement of its rule
(tests/raycast_ref.py diff_rule) applied to vg_raycast's records of the same
beams, on the localisation tests' map (loc_common: after scan 30): scan 31 as
it is, with a panel added in front of a mapped wall, and with a mapped panel
removed."""
import copy

import numpy as np
import pytest

import loc_common as lc
import raycast_ref as rr
import vgpu

pytestmark = pytest.mark.gpu

# test 9: the class shares of scan 31's downsampled cloud from the numpy restatement, as measured
# on the MI355X ("Ray-casting the map")
STATIC_CONSISTENT = 0.8223   # (unknown 0.1246, appeared 0.0029, vanished 0.0501)

_cache = {}


def _pose31():
    return lc.pose_of_row(lc.base()["traj"][lc.K0])


def _restate(M, xyz, pose):
    """(per-point restatement (cls, leaf, r_map, gate, margin), r) from M.raycast of the points' beams."""
    ext_R, ext_t = lc.ext()
    o, dv, r = rr.beams(xyz, pose, ext_R, ext_t)
    return rr.diff_rule(M.raycast(o, dv), r), r


def _compare(pp, ref, r, summary=None):
    """GPU per-point records against the restatement; returns the share left out (|margin| <= 1e-9 m)."""
    cls, leaf, r_map, gate, margin = ref
    edge = np.abs(margin) <= 1e-9
    keep = ~edge
    assert edge.mean() <= 0.005
    assert np.array_equal(pp["cls"][keep], cls[keep]) and np.array_equal(pp["leaf"][keep], leaf[keep])
    assert np.abs(pp["r_map"] - r_map)[keep].max() <= 1e-9 and np.abs(pp["gate"] - gate)[keep].max() <= 1e-9
    assert np.abs(pp["r_meas"] - r).max() <= 1e-9
    if summary is not None:
        assert summary["n"] == np.bincount(pp["cls"], minlength=4).tolist() and sum(summary["n"]) == pp.shape[0]
    return edge.mean()


def _static():
    if not _cache:
        M = rr.workload()["M"]
        s = lc.base()["seq"]
        xyz, inten = s.scan(lc.K0)[:2]
        ds = np.ascontiguousarray(M.downsample(xyz, inten, 0.1)[:, :3])
        summ, pp = M.scan_diff(ds, _pose31(), per_point=True)
        ref, r = _restate(M, ds, _pose31())
        _cache.update(ds=ds, summ=summ, pp=pp, ref=ref, r=r)
    return _cache


def test_rule_restated():
    """6: per point, class and leaf equal the restatement's, r_map and gate within 1e-9; the summary
    equals the per-point histogram; pose=None is the context's state pose."""
    c = _static()
    M = rr.workload()["M"]
    assert c["ds"].shape[0] > 1000
    share = _compare(c["pp"], c["ref"], c["r"], c["summ"])
    print("left out (gate margin within 1e-9 m): %.4f %%" % (100.0 * share))
    ok = c["pp"]["cls"] == vgpu.DIFF_CONSISTENT
    s_abs = np.abs(c["pp"]["r_map"] - c["pp"]["r_meas"])[ok].sum()
    assert abs(c["summ"]["sum_abs_consistent"] - s_abs) <= 1e-9 * max(1.0, s_abs)
    assert c["summ"]["n_truncated"] == 0
    # without the per-point records, and again: the same summary
    assert M.scan_diff(c["ds"], _pose31()) == c["summ"]
    # position in the batch: the reversed cloud's records, reversed
    s2, p2 = M.scan_diff(c["ds"][::-1], _pose31(), per_point=True)
    assert p2[::-1].tobytes() == c["pp"].tobytes() and s2["n"] == c["summ"]["n"]
    a, pa = M.scan_diff(c["ds"], None, per_point=True)
    b, pb = M.scan_diff(c["ds"], M.state()[1:13], per_point=True)
    assert a == b and pa.tobytes() == pb.tobytes() and sum(a["n"]) == c["ds"].shape[0]
    e, pe = M.scan_diff(np.zeros((0, 3), dtype=np.float32), _pose31(), per_point=True)
    assert e["n"] == [0, 0, 0, 0] and pe.shape == (0,)
    out = vgpu.DiffSummary()
    assert vgpu.lib().vg_scan_diff(M.h, None, 5, None, None, None, out) == -1
    assert vgpu.lib().vg_scan_diff(M.h, vgpu._f(c["ds"]), lc.CAP["max_points"] + 1, None, None, None, out) == -1


def _cast31(scene):
    """Scan 31's beams (noiseless) through `scene` from the mapping run's pose: (LiDAR-frame points
    of the rays that return, their surface ids, the rays' mask)."""
    s = lc.base()["seq"]
    pose = _pose31()
    R, p = pose[:9].reshape(3, 3), pose[9:]
    ext_R, ext_t = lc.ext()
    r, sid = scene.cast(R @ ext_t + p, s.dirs @ (R @ ext_R).T)
    ok = np.isfinite(r) & (r >= s.blind)
    return (s.dirs[ok] * r[ok, None]).astype(np.float32), sid[ok], ok


def test_appeared():
    """7: a panel 1.5 m in front of the wall x = 20 (mapped: ~1,000 of scan 31's beams end on it). The
    new panel's points equal the restatement, and those whose beam reaches the map behind it are all
    APPEARED, the reference saying first that they are more than a gate short of the map's range."""
    M = rr.workload()["M"]
    scene = copy.copy(lc.base()["seq"].scene)
    scene.panels = list(scene.panels)
    n, a = np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0])
    scene.panels.append((np.array([18.5, 4.0, 2.5]), n, a, np.cross(n, a), 2.5, 1.5))   # clear of the floor
    xyz, sid, ok = _cast31(scene)
    new = sid == 6 + len(scene.panels) - 1
    assert new.sum() > 50
    xyz = xyz[new]
    # the same beams in the unmodified scene: those that hit the map there, i.e. whose point the map
    # confirms (first hit within the gate of the measured range: the wall x = 20). On the MI355X 379 of
    # 380; the one left meets a leaf plane stretched past its panel's edge 11 m before the wall, in
    # both scenes (the false VANISHED of test 9).
    xyz0, _, ok0 = _cast31(lc.base()["seq"].scene)
    beams0 = np.zeros((ok.shape[0], 3), dtype=np.float32)
    beams0[ok0] = xyz0
    ref0, _ = _restate(M, beams0[ok][new], _pose31())
    ref, r = _restate(M, xyz, _pose31())
    summ, pp = M.scan_diff(xyz, _pose31(), per_point=True)
    _compare(pp, ref, r, summ)
    cls, leaf, r_map, gate, _ = ref
    behind = (leaf >= 0) & (ref0[0] == vgpu.DIFF_CONSISTENT)
    print("new panel: %d points, %d with the map's wall behind them, classes %s"
          % (new.sum(), behind.sum(), np.bincount(cls, minlength=4).tolist()))
    print("r_map - r over them: min %.3f, gate max %.3f" % ((r_map - r)[behind].min(), gate[behind].max()))
    assert behind.sum() > 20
    assert (r_map[behind] - r[behind] > gate[behind]).all() and (r_map[behind] - r[behind] >= 1.0).all()
    assert (pp["cls"][behind] == vgpu.DIFF_APPEARED).all()


def test_vanished():
    """8: scene panel 24 (x = 0.78, ~1,400 of scan 31's beams end on it, the map holds planes on it)
    removed: the points that now reach the surface behind it equal the restatement, and some are
    VANISHED: their beam passed through the panel's mapped planes."""
    M = rr.workload()["M"]
    scene0 = lc.base()["seq"].scene
    j = 24
    c, nrm, a, b, ha, hb = scene0.panels[j]
    pc = rr.workload()["planes"]["center"] - c[None, :]
    on = (np.abs(pc @ nrm) < 0.1) & (np.abs(pc @ a) <= ha) & (np.abs(pc @ b) <= hb)
    assert on.sum() >= 5   # the map holds planes for it
    scene = copy.copy(scene0)
    scene.panels = [q for i, q in enumerate(scene0.panels) if i != j]
    _, sid0, ok0 = _cast31(scene0)
    s = lc.base()["seq"]
    pose = _pose31()
    R, p = pose[:9].reshape(3, 3), pose[9:]
    ext_R, ext_t = lc.ext()
    r1, _ = scene.cast(R @ ext_t + p, s.dirs @ (R @ ext_R).T)
    was = np.zeros(s.dirs.shape[0], dtype=bool)
    was[np.flatnonzero(ok0)[sid0 == 6 + j]] = True
    sel = was & np.isfinite(r1) & (r1 >= s.blind)
    assert sel.sum() > 100
    xyz = (s.dirs[sel] * r1[sel, None]).astype(np.float32)
    ref, r = _restate(M, xyz, pose)
    print("through the removed panel: %d points, classes %s" % (sel.sum(), np.bincount(ref[0], minlength=4).tolist()))
    assert (ref[0] == vgpu.DIFF_VANISHED).sum() >= 1
    summ, pp = M.scan_diff(xyz, pose, per_point=True)
    _compare(pp, ref, r, summ)
    assert summ["n"][vgpu.DIFF_VANISHED] == (ref[0] == vgpu.DIFF_VANISHED).sum()


def test_static_share():
    """9 (characterisation): the restatement's class shares of test 6's scan; CONSISTENT above half
    the recorded share guards against a degenerate setup. Leaf planes extend to their cube's faces
    past a real panel's edge, so some false VANISHED is expected and reported, not tuned away."""
    c = _static()
    share = np.bincount(c["ref"][0], minlength=4) / c["ds"].shape[0]
    print("shares unknown %.4f consistent %.4f appeared %.4f vanished %.4f, occupied-unknown rays %d of %d"
          % (share[0], share[1], share[2], share[3], c["summ"]["n_occupied_unknown"], c["ds"].shape[0]))
    assert share[1] > 0.5 * STATIC_CONSISTENT
