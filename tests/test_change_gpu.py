"""The change layer (vg_change_*) on the GPU: scan-vs-map evidence summed per
map leaf and per cell over scans 31..34 of the localisation tests' map
(loc_common / raycast_ref.workload(): frozen after scan 30), against a numpy
aggregation of vg_scan_diff's per-point records, which test_scan_diff_gpu pins.
M (the shared owner) always gets its layer ended and its trackers closed."""
import copy
import ctypes
import threading

import numpy as np
import pytest

import loc_common as lc
import raycast_ref as rr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

CELL = vgconfig.to_c(vgconfig.load("mid360")).voxel_size / 4   # the default cell edge
FACE = 1e-6            # a point this close to a cell face may fall in either cell by rounding
NSCAN = 4
TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
# measured on the MI355X with the default query ("The change layer"); the tests
# assert half of each as a floor
VANISHED_ON_PANEL = 45  # leaves on removed panel 24 that meet the removed rule over the four poses
APPEARED_CELLS = 124     # 0.2 m cells of the added panel that meet the added rule over the four poses

_cache = {}


def _tracker():
    return vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)


def _pose(i):
    return lc.pose_of_row(lc.base()["traj"][lc.K0 + i])


def _static():
    """The four downsampled clouds, their poses and vg_scan_diff's records of them."""
    if not _cache:
        M = rr.workload()["M"]
        s = lc.base()["seq"]
        scans = []
        for i in range(NSCAN):
            xyz, inten = s.scan(lc.K0 + i)[:2]
            ds = np.ascontiguousarray(M.downsample(xyz, inten, 0.1)[:, :3])
            summ, pp = M.scan_diff(ds, _pose(i), per_point=True)
            scans.append((ds, _pose(i), summ, pp))
        _cache["scans"] = scans
    return _cache["scans"]


def _pack(k):
    k = np.asarray(k, dtype=np.int64) + (1 << 20)
    return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]


def _restate(scans, cell=CELL):
    """numpy aggregation of (xyz, pose, per-point records) per scan, in scan order: the node counters,
    and the cells from w in double: (nodes dict of arrays, cells dict of arrays sorted by packed key,
    packed keys left out because a point of theirs lies within FACE of a cell face, APPEARED points)."""
    ext_R, ext_t = lc.ext()
    top = max([int(pp["leaf"].max()) + 1 for _, _, pp in scans if pp.shape[0]] + [1])
    cons, van, occ, nsc = (np.zeros(top, dtype=np.int64) for _ in range(4))
    keys, eps, ws, skip = [], [], [], []
    for e, (xyz, pose, pp) in enumerate(scans):
        cls, leaf = pp["cls"], pp["leaf"]
        cons += np.bincount(leaf[cls == vgpu.DIFF_CONSISTENT], minlength=top)
        van += np.bincount(leaf[cls == vgpu.DIFF_VANISHED], minlength=top)
        occ += np.bincount(leaf[cls == vgpu.DIFF_APPEARED], minlength=top)
        seen = np.unique(leaf[(cls == vgpu.DIFF_CONSISTENT) | (cls == vgpu.DIFF_VANISHED)])
        nsc[seen] += 1
        R, p = pose[:9].reshape(3, 3), pose[9:]
        w = (np.asarray(xyz, dtype=np.float64)[cls == vgpu.DIFF_APPEARED] @ ext_R.T + ext_t) @ R.T + p
        k = np.floor(w / cell)
        keys.append(_pack(k.astype(np.int64)))
        eps.append(np.full(w.shape[0], e))
        ws.append(w)
        f = w - k * cell
        near = (np.minimum(f, cell - f) <= FACE).any(axis=1)
        for dx in (-2 * FACE, 2 * FACE):
            for dy in (-2 * FACE, 2 * FACE):
                for dz in (-2 * FACE, 2 * FACE):
                    skip.append(_pack(np.floor((w[near] + (dx, dy, dz)) / cell).astype(np.int64)))
    keys, eps, ws = np.concatenate(keys), np.concatenate(eps), np.concatenate(ws)
    skip = np.unique(np.concatenate(skip)) if skip else np.zeros(0, dtype=np.int64)
    uk, inv = np.unique(keys, return_inverse=True)
    n_app = np.bincount(inv, minlength=uk.shape[0])
    pairs = np.unique(np.stack([inv, eps], 1), axis=0) if keys.shape[0] else np.zeros((0, 2), dtype=np.int64)
    n_sc = np.bincount(pairs[:, 0], minlength=uk.shape[0])
    cen = np.stack([np.bincount(inv, weights=ws[:, j], minlength=uk.shape[0]) for j in range(3)], 1) / np.maximum(n_app, 1)[:, None]
    node = np.flatnonzero((cons + van + occ) > 0)
    nodes = dict(node=node, n_consistent=cons[node], n_vanished=van[node], n_occluded=occ[node], n_scans=nsc[node])
    cells = dict(key=uk, n_appeared=n_app, n_scans=n_sc, centroid=cen)
    return nodes, cells, skip, keys.shape[0]


def _rules(nodes, cells, min_obs=5, min_scans=2, ratio=0.8):
    v, c = nodes["n_vanished"], nodes["n_consistent"]
    removed = (v >= min_obs) & (nodes["n_scans"] >= min_scans) & (v.astype(np.float64) >= ratio * (v + c).astype(np.float64))
    added = (cells["n_appeared"] >= min_obs) & (cells["n_scans"] >= min_scans)
    return removed, added


def _check(report, scans, cell=CELL, query=None):
    """A flags = 1 report against the restatement of `scans`; returns (restated nodes, cells, removed, added)."""
    leaves, gc, tot = report
    nodes, cells, skip, n_app = _restate(scans, cell)
    q = query or {}
    removed, added = _rules(nodes, cells, **q)
    assert np.array_equal(leaves["node"], nodes["node"])
    for f in ("n_consistent", "n_vanished", "n_occluded", "n_scans"):
        assert np.array_equal(leaves[f], nodes[f]), f
    assert np.array_equal(leaves["flags"] & 1, removed.astype(np.int32))
    assert tot["leaves_touched"] == leaves.shape[0] and tot["cells_used"] == gc.shape[0]
    assert tot["calls"] == len(scans) and tot["points"] == sum(s[0].shape[0] for s in scans)
    assert tot["n"] == np.sum([np.bincount(s[2]["cls"], minlength=4) for s in scans], axis=0).tolist()
    assert int(gc["n_appeared"].sum()) + tot["dropped"] + tot["out_of_range"] == tot["n"][vgpu.DIFF_APPEARED] == n_app
    gk = _pack(gc["key"])
    assert np.all(np.diff(gk) > 0)   # ascending packed key, no cell twice
    out = np.isin(cells["key"], skip)
    left = cells["n_appeared"][out].sum() / max(n_app, 1)
    print("cells: %d, left out (a point within %g m of a face) %d with %.4f %% of the APPEARED points"
          % (cells["key"].shape[0], FACE, out.sum(), 100.0 * left))
    assert left <= 0.005
    gkeep = ~np.isin(gk, skip)
    assert np.array_equal(gk[gkeep], cells["key"][~out])
    assert np.array_equal(gc["n_appeared"][gkeep], cells["n_appeared"][~out])
    assert np.array_equal(gc["n_scans"][gkeep], cells["n_scans"][~out])
    assert np.array_equal(gc["flags"][gkeep] & 1, added[~out].astype(np.int32))
    if gkeep.any():
        assert np.abs(gc["centroid"][gkeep] - cells["centroid"][~out]).max() <= 2 * cell / 65536 + 1e-9
    return nodes, cells, removed, added


def _blob(report):
    leaves, cells, tot = report
    return leaves.tobytes() + cells.tobytes() + repr(sorted(tot.items())).encode()


def _layer(M, **kw):
    """Begin a layer on M whatever an earlier, failed test left behind."""
    try:
        M.change_end()
    except vgpu.VgError:
        pass
    M.change_begin(**kw)


def test_same_bits_as_scan_diff():
    """1: per_point and the summary of change_accumulate are scan_diff's, byte for byte."""
    M = rr.workload()["M"]
    _layer(M)
    try:
        for ds, pose, summ, pp in _static():
            assert pp.shape[0] > 1000
            s2, p2 = M.change_accumulate(ds, pose, per_point=True)
            assert p2.tobytes() == pp.tobytes()
            assert s2["n"] == summ["n"] and s2["n_truncated"] == summ["n_truncated"]
            assert s2["n_occupied_unknown"] == summ["n_occupied_unknown"]
            assert np.float64(s2["sum_abs_consistent"]).tobytes() == np.float64(summ["sum_abs_consistent"]).tobytes()
            assert M.change_accumulate(ds, pose) == s2   # without the per-point records
    finally:
        M.change_end()


def test_layer_equals_the_aggregation():
    """2: after the four scans the flags = 1 report's leaf counters and n_scans equal a bincount over
    vg_scan_diff's per-point records exactly; the cells equal numpy's w in double but for cells with a
    point within 1e-6 m of a face (at most 0.5 % of the APPEARED points); the totals' identity holds;
    centroids within 2 cell / 65536 + 1e-9; the flags are the rules, for the defaults and for one other
    query; the default report is the flagged subset; the leaf geometry is vg_map_planes'."""
    M = rr.workload()["M"]
    scans = [(ds, pose, pp) for ds, pose, _, pp in _static()]
    _layer(M)
    try:
        for ds, pose, _ in scans:
            M.change_accumulate(ds, pose)
        full = M.change_report(flags=1)
        nodes, cells, removed, added = _check(full, scans)
        print("static scene, default query: %d of %d touched leaves meet the removed rule, %d of %d cells the added rule"
              % (removed.sum(), removed.shape[0], added.sum(), added.shape[0]))
        other = dict(min_obs=2, min_scans=1, ratio=0.5)
        _check(M.change_report(min_obs=2, min_scans=1, vanished_ratio=0.5, flags=1), scans, query=other)
        leaves, gc, tot = M.change_report()
        assert leaves.tobytes() == full[0][(full[0]["flags"] & 1) == 1].tobytes()
        assert gc.tobytes() == full[1][(full[1]["flags"] & 1) == 1].tobytes() and tot == full[2]
        # geometry: the snapshot's record of the same voxel
        planes = rr.workload()["planes"]
        idx = {(p["voxel_center"].tobytes(), int(p["layer"])): i for i, p in enumerate(planes)}
        at = [idx[(l["voxel_center"].tobytes(), int(l["layer"]))] for l in full[0]]
        for f in ("quater_length", "center", "normal"):
            assert full[0][f].tobytes() == planes[f][at].tobytes(), f
        # capacities below the counts: the first records, the counts still returned
        q = vgpu.ChangeQuery()
        q.flags = 1
        nl, nc = ctypes.c_int(0), ctypes.c_int(0)
        a = np.zeros(3, dtype=vgpu.CHANGE_LEAF_DTYPE)
        b = np.zeros(2, dtype=vgpu.CHANGE_CELL_DTYPE)
        assert vgpu.lib().vg_change_report(M.h, ctypes.byref(q), a.ctypes.data, 3, ctypes.byref(nl), b.ctypes.data, 2,
                                           ctypes.byref(nc), None) == 0
        assert (nl.value, nc.value) == (full[0].shape[0], full[1].shape[0])
        assert a.tobytes() == full[0][:3].tobytes() and b.tobytes() == full[1][:2].tobytes()
    finally:
        M.change_end()


def test_order_and_caller_independence():
    """3: forwards, backwards, alternating owner / tracker, two trackers on two threads, point-reversed
    clouds and the device-array entry give identical report bytes, totals included."""
    import torch
    M = rr.workload()["M"]
    scans = [(ds, pose) for ds, pose, _, _ in _static()]
    T1, T2 = _tracker(), _tracker()
    _layer(M)
    try:
        T1.attach(M)
        T2.attach(M)

        def run(fn):
            M.change_clear()
            fn()
            return _blob(M.change_report(flags=1))

        def forwards():
            for ds, pose in scans:
                M.change_accumulate(ds, pose)

        def backwards():
            for ds, pose in scans[::-1]:
                M.change_accumulate(ds, pose)

        def alternating():
            for i, (ds, pose) in enumerate(scans):
                (M if i % 2 == 0 else T1).change_accumulate(ds, pose)

        def threads():
            err = []

            def work(T, part):
                try:
                    for ds, pose in part:
                        T.change_accumulate(ds, pose)
                except Exception as e:  # noqa: BLE001 - reported below
                    err.append(e)
            th = [threading.Thread(target=work, args=(T1, scans[:2])), threading.Thread(target=work, args=(T2, scans[2:]))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert not err, err

        def reversed_points():
            for ds, pose in scans:
                M.change_accumulate(ds[::-1], pose)

        def device_arrays():
            for i, (ds, pose) in enumerate(scans):
                t = torch.from_numpy(np.ascontiguousarray(ds.T)).to(torch.device("cuda", 0))
                torch.cuda.synchronize()
                s = (M if i % 2 == 0 else T2).change_accumulate_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                                                    ds.shape[0], pose)
                assert s["n"] == _static()[i][2]["n"]

        ref = run(forwards)
        assert M.change_report(flags=1)[2]["dropped"] == 0 and len(ref) > 1000
        for fn in (backwards, alternating, threads, reversed_points, device_arrays):
            assert run(fn) == ref, fn.__name__
    finally:
        T1.close()
        T2.close()
        M.change_end()


def test_map_is_read_only():
    """4: a context that had a layer and accumulated into it has the map, the state and a frozen step of
    scan 31 of a context that never had one, bit for bit."""
    s = lc.base()["seq"]
    C, R = lc.loaded(mapping=False), lc.loaded(mapping=False)
    C.change_begin()
    for ds, pose, _, _ in _static():
        C.change_accumulate(ds, pose)
    assert C.change_report()[2]["points"] > 4000
    lc.same_map(C, lc.roots(R), lc.planes(R))
    assert C.state().tobytes() == R.state().tobytes()
    C.change_accumulate(_static()[0][0])   # pose None: the context's state
    lc.step(C, s, lc.K0)                   # a frozen step with the layer in place
    C.change_end()
    lc.step(R, s, lc.K0)
    assert C.state().tobytes() == R.state().tobytes() and C.trajectory().tobytes() == R.trajectory().tobytes()
    lc.same_map(C, lc.roots(R), lc.planes(R))
    C.close()
    R.close()


def _cast(scene, i):
    """Scan K0 + i's beams (noiseless) through `scene` from the mapping run's pose: (ranges, surface ids, pose)."""
    s = lc.base()["seq"]
    pose = _pose(i)
    R, p = pose[:9].reshape(3, 3), pose[9:]
    ext_R, ext_t = lc.ext()
    r, sid = scene.cast(R @ ext_t + p, s.dirs @ (R @ ext_R).T)
    return r, sid, pose


def _accumulate_scene(M, clouds):
    out = []
    for xyz, pose in clouds:
        _, pp = M.change_accumulate(xyz, pose, per_point=True)
        out.append((xyz, pose, pp))
    return out


def test_scene_panel_added():
    """5a: test_appeared's panel, seen from the poses of rows K0..K0+3: every cell of the default report
    has its centroid within one cell of the panel's slab, and there are cells. The panel stands at x = 18.5,
    a face of the default 0.125 m cells, where the x index of every noiseless point is a matter of the
    last bit; the layer of this test therefore has 0.2 m cells (18.5 / 0.2 = 92.5: mid-cell)."""
    cell = 0.2
    M = rr.workload()["M"]
    s = lc.base()["seq"]
    scene = copy.copy(s.scene)
    scene.panels = list(scene.panels)
    n, a = np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0])
    c, ha, hb = np.array([18.5, 4.0, 2.5]), 2.5, 1.5
    b = np.cross(n, a)
    scene.panels.append((c, n, a, b, ha, hb))
    clouds = []
    for i in range(NSCAN):
        r, sid, pose = _cast(scene, i)
        new = np.isfinite(r) & (r >= s.blind) & (sid == 6 + len(scene.panels) - 1)
        assert new.sum() > 50
        clouds.append(((s.dirs[new] * r[new, None]).astype(np.float32), pose))
    _layer(M, cell=cell)
    try:
        scans = _accumulate_scene(M, clouds)
        _, cells, _, added = _check(M.change_report(flags=1), scans, cell=cell)
        print("panel added: %d points, %d cells, %d meet the added rule"
              % (sum(x.shape[0] for x, _ in clouds), added.shape[0], added.sum()))
        assert added.sum() >= 1                      # the restatement first
        _, gc, _ = M.change_report()
        assert gc.shape[0] >= max(1, APPEARED_CELLS // 2)
        d = gc["centroid"] - c[None, :]
        dist = np.stack([np.maximum(np.abs(d @ n) - 0.0, 0), np.maximum(np.abs(d @ a) - ha, 0),
                         np.maximum(np.abs(d @ b) - hb, 0)], 1)
        assert np.linalg.norm(dist, axis=1).max() <= cell
    finally:
        M.change_end()


def test_scene_panel_removed():
    """5b: test_vanished's removed panel 24 from the four poses: the leaves of the default report include
    leaves on the panel."""
    M = rr.workload()["M"]
    s = lc.base()["seq"]
    scene0 = s.scene
    j = 24
    c, nrm, a, b, ha, hb = scene0.panels[j]
    planes = rr.workload()["planes"]
    pc = planes["center"] - c[None, :]
    on = (np.abs(pc @ nrm) < 0.1) & (np.abs(pc @ a) <= ha) & (np.abs(pc @ b) <= hb)
    assert on.sum() >= 5
    on_vox = {(p["voxel_center"].tobytes(), int(p["layer"])) for p in planes[on]}
    scene = copy.copy(scene0)
    scene.panels = [q for i, q in enumerate(scene0.panels) if i != j]
    clouds = []
    for i in range(NSCAN):
        r0, sid0, pose = _cast(scene0, i)
        r1, _, _ = _cast(scene, i)
        sel = np.isfinite(r0) & (r0 >= s.blind) & (sid0 == 6 + j) & np.isfinite(r1) & (r1 >= s.blind)
        assert sel.sum() > 100
        clouds.append(((s.dirs[sel] * r1[sel, None]).astype(np.float32), pose))
    _layer(M)
    try:
        scans = _accumulate_scene(M, clouds)
        nodes, _, removed, _ = _check(M.change_report(flags=1), scans)
        assert removed.sum() >= 1                    # the restatement first
        leaves, _, _ = M.change_report()
        assert np.array_equal(leaves["node"], nodes["node"][removed])
        hit = np.array([(l["voxel_center"].tobytes(), int(l["layer"])) in on_vox for l in leaves])
        print("panel removed: %d points, %d leaves touched, %d meet the removed rule: %d on the panel, %d off it"
              % (sum(x.shape[0] for x, _ in clouds), removed.shape[0], removed.sum(), hit.sum(), (~hit).sum()))
        assert hit.sum() >= max(1, VANISHED_ON_PANEL // 2)
    finally:
        M.change_end()


def _refused(fn):
    with pytest.raises(vgpu.VgError) as ei:
        fn()
    assert "(-5)" in str(ei.value), str(ei.value)


def test_edges(tmp_path):
    """6: n == 0; clear; end then begin; every guard returns VG_E_STATE and the context keeps working;
    a 16-slot table drops points and says so; an empty map gives an empty report."""
    b = lc.base()
    s = b["seq"]
    ds, pose, summ, pp = _static()[0]
    C = lc.loaded(mapping=False)
    _refused(lambda: C.change_accumulate(ds, pose))      # no layer yet
    _refused(C.change_clear)
    _refused(C.change_end)
    C.change_begin()
    _refused(C.change_begin)                              # a layer already
    # vg_scan_diff's argument rules: VG_E_ARG, and a refused call takes no epoch and counts nothing
    L, dsum = vgpu.lib(), vgpu.DiffSummary()
    assert L.vg_change_accumulate(C.h, None, 5, None, None, dsum) == -1                                  # NULL xyz, n > 0
    assert L.vg_change_accumulate(C.h, vgpu._f(ds), -1, None, None, dsum) == -1                          # n < 0
    assert L.vg_change_accumulate(C.h, vgpu._f(ds), lc.CAP["max_points"] + 1, None, None, dsum) == -1    # n too large
    assert L.vg_change_accumulate_dev(C.h, None, None, None, 5, None, dsum) == -1                        # NULL arrays
    assert L.vg_change_accumulate_dev(C.h, None, None, None, -1, None, dsum) == -1
    assert C.change_report(flags=1)[2]["calls"] == 0
    e = C.change_accumulate(np.zeros((0, 3), dtype=np.float32), pose)
    assert e["n"] == [0, 0, 0, 0]
    leaves, cells, tot = C.change_report(flags=1)
    assert leaves.shape == (0,) and cells.shape == (0,) and tot["calls"] == 1 and tot["points"] == 0
    C.change_accumulate(ds, pose)
    one = C.change_report(flags=1)
    assert one[2]["calls"] == 2 and one[0].shape[0] > 100 and one[0]["n_scans"].max() == 1
    C.change_clear()
    leaves, cells, tot = C.change_report(flags=1)
    assert leaves.shape == (0,) and cells.shape == (0,) and all(v in (0, [0, 0, 0, 0]) for v in tot.values())
    C.change_accumulate(ds, pose)                         # the epochs restarted: the same layer but for the calls
    again = C.change_report(flags=1)
    assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes() and again[2]["calls"] == 1
    # the guards: VG_E_STATE, nothing changed
    snap = (lc.roots(C), lc.planes(C))
    out = str(tmp_path / "x.vgck")
    for fn in (lambda: C.set_mapping(True), C.reset, lambda: C.checkpoint_load(b["path"]), lambda: C.checkpoint_save(out),
               lambda: C.release_far(compact=True), lambda: C.shard_host(0, 1, lambda arr: None), C.close):
        _refused(fn)
    assert C.h and C.release_far()[2] > 0                 # the census alone is allowed
    lc.same_map(C, *snap)
    assert _blob(C.change_report(flags=1)) == _blob(again)
    lc.step(C, s, lc.K0)                                  # the context keeps working
    assert C.scan_diff(ds, pose)["n"] == summ["n"]
    T = _tracker()
    T.attach(C)
    _refused(T.change_begin)                              # attached: the layer belongs to the owner
    _refused(T.change_clear)
    _refused(T.change_end)
    assert T.change_report(flags=1)[0].tobytes() == again[0].tobytes()   # a tracker reads the owner's layer
    T.close()
    C.change_end()
    C.change_begin(cell_hash_log2=4)                      # end then begin; 16 slots
    _, p2 = C.change_accumulate(ds, pose, per_point=True)
    leaves, cells, tot = C.change_report(flags=1)
    assert p2.tobytes() == pp.tobytes() and cells.shape[0] == 16 == tot["cells_used"] and tot["dropped"] > 0
    assert int(cells["n_appeared"].sum()) + tot["dropped"] + tot["out_of_range"] == tot["n"][vgpu.DIFF_APPEARED]
    C.change_end()
    with pytest.raises(vgpu.VgError) as ei:
        C.change_begin(cell_hash_log2=27)
    assert "(-1)" in str(ei.value)
    # begin's own guards
    B = lc.loaded(mapping=False)
    xyz, it, beg, end = s.scan(lc.K0)
    B.scan_load(xyz, it)
    B.propagate(s.imu(lc.K0), beg, end)
    _refused(B.change_begin)                              # inside a scan
    B.downsample_scan()
    B.lio_state_estimation()
    B.step_end()
    B.change_begin()
    B.change_end()
    B.close()
    Q = lc.loaded()
    _refused(Q.change_begin)                              # mapping
    Q.close()
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    _refused(S.change_begin)                              # sharded (and mapping)
    with pytest.raises(vgpu.VgError) as ei:
        S.change_accumulate(ds, pose)
    assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()
    E = lc.ctx()                                          # an empty map
    E.set_mapping(False)
    E.change_begin()
    assert E.change_accumulate(ds, pose)["n"] == [ds.shape[0], 0, 0, 0]
    leaves, cells, tot = E.change_report(flags=1)
    assert leaves.shape == (0,) and cells.shape == (0,) and tot["n"][0] == ds.shape[0] and tot["leaves_touched"] == 0
    E.change_end()
    E.close()
    C.close()


def test_replay_scan_diff_and_changes(tmp_path):
    """7: vg_node_replay --map ... --localize --scan-diff --changes on test_checkpoint_node_gpu's event log:
    one scan_diff line per localised scan whose four class columns sum to n_ds, and a CSV that parses and
    equals the API's report of the same clouds at the same poses (the tool's --changes-scans dump)."""
    import json
    import math
    import os
    import subprocess

    import synth
    from test_node_core import REPO, _events, _fmt, _write_log
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 12, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    cfg = vgconfig.to_c(p)
    log = tmp_path / "ev.bin"
    _write_log(log, cfg, _fmt(g["blind"]), seq.gt_state(0), _events(seq, 16))
    exe = os.path.join(REPO, "vina-slam_amd", "bin", "vg_node_replay")

    def run(args, rc=0):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == rc, r.stderr
        return r.stdout.strip().splitlines()

    ck, csv, dump = tmp_path / "map.vgck", tmp_path / "out.csv", tmp_path / "scans.bin"
    run([log, tmp_path / "a.tum", 0, tmp_path / "a.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    run([log, tmp_path / "x.tum", "--changes", csv], rc=2)       # only with --map ... --localize
    run([log, tmp_path / "x.tum", "--scan-diff"], rc=2)
    assert not csv.exists()
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    lines = run([log, tmp_path / "b.tum", "--map", ck, "--localize", "--guess", guess, "--scan-diff", "--changes", csv,
                 "--changes-scans", dump])
    summary = json.loads(lines[-1])
    rows = [ln.split() for ln in lines if ln.startswith("scan_diff ")]
    assert len(rows) == summary["stepped"] >= 14
    raw = dump.read_bytes()
    scans, at = [], 0
    while at < len(raw):
        n = int(np.frombuffer(raw, dtype="<i4", count=1, offset=at)[0])
        pose = np.frombuffer(raw, dtype="<f8", count=12, offset=at + 4).copy()
        xyz = np.frombuffer(raw, dtype="<f4", count=3 * n, offset=at + 100).reshape(n, 3).copy()
        scans.append((xyz, pose))
        at += 100 + 12 * n
    assert len(scans) == len(rows)
    C = vgpu.Context(cfg, max_points=400_000)
    C.checkpoint_load(str(ck))
    C.set_mapping(False)
    C.change_begin()
    for k, (row, (xyz, pose)) in enumerate(zip(rows, scans)):
        assert len(row) == 8 and int(row[1]) == k
        n_ds, cols = int(row[3]), [int(v) for v in row[4:8]]
        assert n_ds == xyz.shape[0] > 100 and sum(cols) == n_ds
        assert C.change_accumulate(xyz, pose)["n"] == cols
    leaves, cells, tot = C.change_report(flags=1)
    C.change_end()
    C.close()
    recs = [ln.split(",") for ln in csv.read_text().splitlines()]
    cl = [r for r in recs if r[0] == "leaf"]
    cc = [r for r in recs if r[0] == "cell"]
    ct = [r for r in recs if r[0] == "totals"]
    assert len(cl) + len(cc) + len(ct) == len(recs) and len(ct) == 1
    assert len(cl) == leaves.shape[0] > 100 and len(cc) == cells.shape[0]
    for r, l in zip(cl, leaves):
        assert len(r) == 18
        assert [int(v) for v in r[1:8]] == [int(l[f]) for f in ("node", "layer", "n_consistent", "n_vanished",
                                                                "n_occluded", "n_scans", "flags")]
        ref = np.concatenate([l["voxel_center"], [l["quater_length"]], l["center"], l["normal"]])
        assert np.array([float(v) for v in r[8:]]).tobytes() == ref.tobytes()
    for r, c in zip(cc, cells):
        assert len(r) == 10
        assert [int(v) for v in r[1:7]] == [int(v) for v in c["key"]] + [int(c["n_appeared"]), int(c["n_scans"]), int(c["flags"])]
        assert np.array([float(v) for v in r[7:]]).tobytes() == c["centroid"].tobytes()
    assert [int(v) for v in ct[0][1:]] == [tot["calls"], tot["points"]] + tot["n"] + [
        tot["cells_used"], tot["dropped"], tot["out_of_range"], tot["leaves_touched"]]
    assert tot["calls"] == len(rows)
