"""vg_view_gain (vina_gpu.h "View gain") against the numpy restatement of its
definition (tests/view_ref.py), bit for bit: the records, the seen plane and the
summary. Shapes are the smallest at which the kernels can still go wrong: 200
viewpoints are 200 workgroups; R = 1 is a bitmap of one word, R = 24 one of 76
words with 192 rays on 256 lanes, R = 64 and more give every lane several rays
and words; R = 255 is the largest bitmap and lies above the radius up to which
the window's classes can be staged in LDS (208), so both variants run at every
radius below it and only the unstaged one there."""
import ctypes

import numpy as np
import pytest

import clr_ref as cr
import view_ref as vr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
U, F, O = vr.UNKNOWN, vr.FREE, vr.OCCUPIED

_cache = {}


def _ctx():
    """A context with no map (shared, never closed): vg_view_gain reads none."""
    if "C" not in _cache:
        _cache["C"] = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    return _cache["C"]


def _ref(key, grid, views, R, mu=0):
    """view_ref.view_gain, computed once per key and left unchanged."""
    if key not in _cache:
        _cache[key] = vr.view_gain(grid, views, R, mu)
    return _cache[key]


def _same(got, want, seen=True):
    rec, sn, s = got
    assert rec.dtype == vr.REC and rec.shape == want[0].shape
    bad = np.flatnonzero(rec != want[0])
    assert not bad.size, (bad[:8], rec[bad[:4]], want[0][bad[:4]])
    assert rec.tobytes() == want[0].tobytes()
    if seen:
        assert sn.dtype == np.int32 and sn.shape == want[1].shape
        bad = np.argwhere(sn != want[1])
        assert not bad.size, (bad[:8], sn[tuple(bad[0])], want[1][tuple(bad[0])])
    else:
        assert sn is None
    assert s == want[2], (s, want[2])


def _both(grid, views, R, want, mu=0, C=None):
    """The call with the window's classes read from the grid and staged in LDS, with and without seen: all equal
    the restatement. Returns the last result."""
    C = C or _ctx()
    for stage in (0, 1):
        vgpu.lib().vgx_view_stage(C.h, stage)
        for want_seen in (True, False):
            got = C.view_gain(views, R, grid, max_unknown=mu, want_seen=want_seen)
            _same(got, want, want_seen)
    vgpu.lib().vgx_view_stage(C.h, 0)
    return got


@pytest.mark.parametrize("nx,ny,seed", [(61, 47, 7), (130, 67, 11), (67, 130, 11)])
def test_random_grids(nx, ny, seed):
    """1: random grids, 200 viewpoints with the corners, cells outside, occupied cells and a cell twice."""
    g = cr.random_grid(nx, ny, seed, p_unknown=0.3, p_occ=0.1)
    views = vr.mixed_views(g, 200, seed)
    assert views.shape == (200, 2) and (views[-1] == views[16]).all()
    n_diag = 0
    for R in (1, 2, 9, 24):
        for mu in (0, 3):
            want = _ref(("rand", nx, ny, R, mu), g, views, R, mu)
            rec = want[0]
            # the inputs bite, on the reference alone
            assert ((rec["status"] == vr.OK) & (rec["n_unknown"] > 0)).sum() >= 50
            assert set(rec["status"].tolist()) == {vr.OK, vr.OUTSIDE, vr.BLOCKED}
            n_diag += want[3]
            _both(g, views, R, want, mu)
    assert n_diag >= 1
    w0, w3 = _cache[("rand", nx, ny, 24, 0)], _cache[("rand", nx, ny, 24, 3)]
    assert w0[2]["unknown_seen"] > w3[2]["unknown_seen"] > 0        # max_unknown ends rays early
    assert _ctx().view_gain_ms() > 0.0


@pytest.mark.parametrize("R", [1, 7, 64, 127, 255])
def test_open_room(R):
    """2: an all-free (2R + 5)^2 grid, one viewpoint at its centre: the disc's cell count. R = 255: the largest
    bitmap."""
    side = 2 * R + 5
    g = np.zeros((side, side), dtype=np.int8)
    views = [[side // 2, side // 2]]
    want = _ref(("room", R), g, views, R)
    rec, seen, s = _both(g, views, R, want)
    assert rec[0]["n_visible"] == vr.circle_count(R) == rec[0]["n_free"] == s["cells_seen"]
    assert rec[0]["n_rays_open"] == 8 * R == s["rays"]


def test_diamond_ring():
    """3: the closed diamond from its five origins: nothing beyond it is seen."""
    g, c = vr.diamond_ring()
    views = [[c + x, c + y] for x, y in vr.RING_ORIGINS]
    want = _ref(("ring",), g, views, 30)
    rec, seen, s = _both(g, views, 30, want)
    assert s["unknown_seen"] == 0 and (rec["n_rays_open"] == 0).all() and rec[0]["n_free"] == 181
    for k, v in enumerate(views):                                    # and one at a time
        _same(_ctx().view_gain([v], 30, g, want_seen=True), _ref(("ring", k), g, [v], 30))


def test_clipping():
    """4: the window overhangs the grid on every side: the corners of 61 x 47 with R = 255; a row and a column."""
    g = cr.random_grid(61, 47, 7, p_unknown=0.3, p_occ=0.02)
    g[0, 0] = g[46, 60] = F
    views = [[0, 0], [60, 46]]
    _both(g, views, 255, _ref(("clip",), g, views, 255))
    _both(g, views, 200, _ref(("clip", 200), g, views, 200))         # the same with the staged classes
    line = np.zeros(300, dtype=np.int8)
    line[5::37] = U
    line[290] = O
    for shape, views in (((1, 300), [[0, 0], [150, 0], [299, 0], [290, 0]]), ((300, 1), [[0, 0], [0, 150], [0, 299], [0, 290]])):
        gl = line.reshape(shape)
        for R in (3, 255):
            want = _ref(("line", shape, R), gl, views, R)
            rec, _, _ = _both(gl, views, R, want)
            assert rec["status"].tolist() == [vr.OK, vr.OK, vr.OK, vr.BLOCKED]
        # from cell 150: the 150 cells before it, the 140 up to the occupied cell 290, which ends one ray
        assert rec[1]["n_visible"] == 1 + 150 + 140 and rec[1]["n_rays_open"] == 8 * 255 - 1


def test_seen_is_order_free_and_additive():
    """5: a permutation of the viewpoints permutes the records and leaves seen and the summary's set counts; two
    calls over a split add up to one; best_view's ties go to the smaller index."""
    C = _ctx()
    g = cr.random_grid(130, 67, 11, p_unknown=0.3, p_occ=0.1)
    views = vr.mixed_views(g, 200, 11)
    rec, seen, s = C.view_gain(views, 9, g, want_seen=True)
    _same((rec, seen, s), _ref(("rand", 130, 67, 9, 0), g, views, 9))
    perm = np.random.default_rng(3).permutation(200)
    rec_p, seen_p, s_p = C.view_gain(views[perm], 9, g, want_seen=True)
    assert rec_p.tobytes() == rec[perm].tobytes() and seen_p.tobytes() == seen.tobytes()
    assert {k: v for k, v in s_p.items() if k != "best_view"} == {k: v for k, v in s.items() if k != "best_view"}
    assert rec_p[s_p["best_view"]]["n_unknown"] == s["max_unknown_seen"]
    (_, sa, _), (_, sb, _) = C.view_gain(views[:77], 9, g, want_seen=True), C.view_gain(views[77:], 9, g, want_seen=True)
    assert (sa + sb).tobytes() == seen.tobytes()
    # ties: the best viewpoint named three times, the first of them behind a blocked one and another
    best = views[s["best_view"]].tolist()
    tie = [np.argwhere(g == O)[0][::-1].tolist(), views[20].tolist(), best, best, [-3, 5], best]
    rec_t, _, s_t = C.view_gain(tie, 9, g)
    first = int(np.flatnonzero((rec_t["status"] == vr.OK) & (rec_t["n_unknown"] == rec_t["n_unknown"].max()))[0])
    assert s_t["best_view"] == first <= 2 and s_t["max_unknown_seen"] == s["max_unknown_seen"]
    _same((rec_t, None, s_t), vr.view_gain(g, tie, 9), seen=False)


def test_many_viewpoints():
    """6: 65,536 viewpoints, the most a call takes, at R = 2: the reference once per distinct cell, indexed."""
    g = cr.random_grid(130, 67, 11, p_unknown=0.3, p_occ=0.1)
    rng = np.random.default_rng(17)
    views = np.stack([rng.integers(-2, 133, 65536), rng.integers(-2, 70, 65536)], axis=1).astype(np.int32)
    cells, inv = np.unique(views, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    rec_u, seen_u, s_u, _ = vr.view_gain(g, cells, 2)
    want = rec_u[inv]
    # the seen plane: every distinct cell's visible set, times the number of times the cell is named
    mult = np.bincount(inv, minlength=cells.shape[0])
    seen = np.zeros(g.shape, dtype=np.int64)
    ok = np.flatnonzero(rec_u["status"] == vr.OK)
    vis, _, _ = vr.visible(g, cells[ok], 2)
    mi, wy, wx = np.nonzero(vis)
    np.add.at(seen, (cells[ok[mi], 1] + wy - 2, cells[ok[mi], 0] + wx - 2), mult[ok[mi]])
    rec, sn, s = _ctx().view_gain(views, 2, g, want_seen=True)
    assert rec.tobytes() == want.tobytes() and np.array_equal(sn, seen)
    st = want["status"]
    gain = np.where(st == vr.OK, want["n_unknown"], -1)
    assert s == dict(n_views=65536, n_ok=int((st == vr.OK).sum()), n_outside=int((st == vr.OUTSIDE).sum()),
                     n_blocked=int((st == vr.BLOCKED).sum()), rays=16 * int((st == vr.OK).sum()),
                     max_unknown_seen=int(gain.max()), best_view=int(np.argmax(gain)), cells_seen=s_u["cells_seen"],
                     unknown_seen=s_u["unknown_seen"])
    assert s["n_outside"] > 1000 and s["n_blocked"] > 1000


def test_chain_and_state():
    """7: occupancy -> clearance -> navfn -> frontiers -> view_gain on the grid where it lies equals the call on the
    downloaded grid and the restatement; VG_E_STATE without a grid, on another nx, ny and on a sharded context;
    vg_clearance's and vg_nav_paths' outputs are what they were; view_order equals the restatement's."""
    import loc_common as lc
    import nav_ref as nr
    import test_occupancy_gpu as tog
    w = tog._work()
    M, geom = w["M"], w["geom"]
    nx, ny = geom["nx"], geom["ny"]
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)

    def refused(call, word=None):
        with pytest.raises(vgpu.VgError) as ei:
            call()
        assert "(-5)" in str(ei.value) and (word is None or word in str(ei.value)), str(ei.value)

    refused(lambda: T.view_gain([[1, 1]], 5, None, nx=nx, ny=ny), "vg_occupancy")
    M.occupancy(w["pos"], w["dirs"], **geom, **tog.BAND)
    out, _ = M.clearance(None, nx=nx, ny=ny, **cr.PARAMS["nav"])
    cost = out["cost"]
    trav = nr.trav_table()
    robot = nr.passable_cells(cost, trav, 1, 2)
    M.navfn(None, robot, nx=nx, ny=ny)
    starts = nr.passable_cells(cost, trav, 8, 3)
    paths = M.nav_paths(starts, 200)
    _, frec, fs = M.frontiers(None, nx=nx, ny=ny, use_cost=True, use_pot=True)
    assert frec.size >= 1 and (frec["best_cell"] >= 0).all()
    views = np.stack([frec["best_cell"] % nx, frec["best_cell"] // nx], axis=1)
    dev = M.view_gain(views, 12, None, nx=nx, ny=ny, want_seen=True)
    again = M.view_gain(views, 12, None, nx=nx, ny=ny, want_seen=True)
    host = M.view_gain(views, 12, w["grid"], want_seen=True)
    other = T.view_gain(views, 12, w["grid"], want_seen=True)
    for r in (again, host, other):
        assert r[0].tobytes() == dev[0].tobytes() and r[1].tobytes() == dev[1].tobytes() and r[2] == dev[2]
    want = vr.view_gain(w["grid"], views, 12)
    _same(dev, want)
    assert (dev[0]["status"] == vr.OK).all() and (dev[0]["n_unknown"] >= 1).all()   # a frontier cell touches unknown
    for pots in (None, frec["best_pot"]):
        order = vgpu.view_order(dev[0], pots)
        assert order.tolist() == vr.view_order(want[0], pots).tolist() and order.size == frec.size
    assert M.view_gain_ms() > 0.0
    refused(lambda: M.view_gain(views, 12, None, nx=nx + 1, ny=ny), "vg_occupancy")
    T.close()
    # the refused calls and the view gain left the neighbours' planes alone
    out2, _ = M.clearance(None, nx=nx, ny=ny, **cr.PARAMS["nav"])
    assert out2["cost"].tobytes() == cost.tobytes()
    for a, b in zip(M.nav_paths(starts, 200), paths):
        assert np.array_equal(a, b)
    _, frec2, fs2 = M.frontiers(None, nx=nx, ny=ny, use_cost=True, use_pot=True)
    assert frec2.tobytes() == frec.tobytes() and fs2 == fs
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    refused(lambda: S.view_gain(views, 12, w["grid"]), "sharded")
    S.close()


def test_argument_errors():
    """8: every VG_E_ARG condition returns it and writes nothing: no record, no seen cell, not the summary."""
    C = _ctx()
    L, P = vgpu.lib(), C.h
    nx, ny = 8, 5
    g = cr.random_grid(nx, ny, 3)
    g[2, 3] = F
    views = np.array([[3, 2], [0, 0], [9, 9]], dtype=np.int32)
    rec = np.full(3, 7, dtype=np.uint8).repeat(32).view(vr.REC)
    seen = np.full(nx * ny, 7, dtype=np.int32)
    sm = vgpu.ViewSummary()

    def params(**kw):
        p = vgpu.ViewParams()
        for k, v in dict(dict(nx=nx, ny=ny, radius=2), **kw).items():
            setattr(p, k, v)
        return p

    def call(ctx=P, prm=params(), v=views.ctypes.data, n=3, r=rec.ctypes.data, out=sm):
        return L.vg_view_gain(ctx, g.ctypes.data, None if prm is None else ctypes.byref(prm), v, n, r, seen.ctypes.data,
                              None if out is None else ctypes.byref(out))

    bad = [dict(ctx=None), dict(prm=None), dict(v=None), dict(r=None), dict(out=None), dict(n=0), dict(n=-1),
           dict(n=vgpu.NAV_MAX_POINTS + 1)]
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-4), dict(nx=vgpu.CLR_MAX_SIDE + 1, ny=1), dict(nx=1, ny=vgpu.CLR_MAX_SIDE + 1),
               dict(nx=4097, ny=4097), dict(radius=0), dict(radius=-1), dict(radius=vgpu.VIEW_MAX_RADIUS + 1),
               dict(max_unknown=-1), dict(flags=1), dict(flags=2), dict(flags=-1)):
        bad.append(dict(prm=params(**kw)))
    before = rec.tobytes()
    for kw in bad:
        assert call(**kw) == -1, kw
        assert (seen == 7).all() and rec.tobytes() == before and not bytes(sm).strip(b"\0"), kw
    assert call() == 0
    want = vr.view_gain(g, views, 2)
    assert rec.tobytes() == want[0].tobytes() and np.array_equal(seen.reshape(ny, nx), want[1])
    assert {k: getattr(sm, k) for k in vr.SUMMARY} == want[2]
    assert call(prm=params(radius=vgpu.VIEW_MAX_RADIUS, max_unknown=2 ** 31 - 1)) == 0
    assert L.vg_view_gain(P, g.ctypes.data, ctypes.byref(params()), views.ctypes.data, 3, rec.ctypes.data, None,
                          ctypes.byref(sm)) == 0


def test_replay_view_gain(tmp_path):
    """9: vg_node_replay ... --frontiers f.csv --view-gain g.csv --view-radius METRES writes one
    label,best_x,best_y,best_pot,n_unknown,n_free,n_occupied,n_rays_open row per frontier of Context.view_gain at the
    frontiers' best cells over the written grid, in view_order over best_pot; f.csv is byte-identical with and
    without the new options; without --plan or a radius they are refused."""
    import math
    import os
    import subprocess

    import synth
    from test_node_core import REPO, _events, _fmt, _write_log
    p = vgconfig.load("mid360")
    gc = p["General"]
    seq = synth.Sequence("16line", 12, blind=gc["blind"], ext_R=gc["extrinsic_rota"], ext_t=gc["extrinsic_tran"])
    log = tmp_path / "ev.bin"
    _write_log(log, vgconfig.to_c(p), _fmt(gc["blind"]), seq.gt_state(0), _events(seq, 16))
    exe = os.path.join(REPO, "vina-slam_amd", "bin", "vg_node_replay")

    def run(args, rc=0):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == rc, r.stderr
        return r.stdout

    ck = tmp_path / "map.vgck"
    run([log, tmp_path / "a.tum", 0, tmp_path / "a.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    pre, cpre, path = str(tmp_path / "nav"), str(tmp_path / "cost"), tmp_path / "plan.csv"
    f0, f1, gcsv = tmp_path / "fr0.csv", tmp_path / "fr1.csv", tmp_path / "gain.csv"
    prm = cr.PARAMS["replay"]
    base = [log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--occupancy", pre, "--occ-res", prm["res"],
            "--costmap", cpre, "--inscribed", prm["inscribed_radius"], "--inflation", prm["inflation_radius"],
            "--cost-scaling", prm["cost_scaling"]]
    plan = ["--plan", "%r %r" % (float(p0[0]), float(p0[1])), "--path", path]
    radius_m, mu = 3.1, 40
    run(base + ["--frontiers", f1, "--view-gain", gcsv, "--view-radius", radius_m], rc=2)      # no --plan
    run(base + plan + ["--frontiers", f1, "--view-gain", gcsv], rc=2)                            # no radius
    run(base + plan + ["--view-gain", gcsv, "--view-radius", radius_m], rc=2)                    # no --frontiers
    run(base + plan + ["--frontiers", f0])
    out = run(base + plan + ["--frontiers", f1, "--view-gain", gcsv, "--view-radius", radius_m, "--view-max-unknown", mu])
    assert f0.read_bytes() == f1.read_bytes() and f0.stat().st_size > 0
    C = _ctx()
    grid, gx0, gy0, gres = vgpu.read_occupancy(pre)
    cost, x0, y0, res = vgpu.read_costmap(cpre)
    nx = cost.shape[1]
    C.navfn(cost, [[math.floor((float(p0[0]) - x0) / res), math.floor((float(p0[1]) - y0) / res)]])
    _, frec, _ = C.frontiers(grid, cost=cost, use_pot=True)
    R = int(math.floor(radius_m / res + 0.5))
    assert R == 16 and frec.size >= 1
    views = np.stack([frec["best_cell"] % nx, frec["best_cell"] // nx], axis=1)
    rec, _, s = C.view_gain(views, R, grid, max_unknown=mu)
    order = vgpu.view_order(rec, frec["best_pot"])
    rows = np.loadtxt(gcsv, delimiter=",", ndmin=2)
    assert rows.shape == (order.size, 8) and order.size >= 1
    assert np.array_equal(rows[:, 0].astype(np.int64), frec["label"][order])
    assert np.array_equal(rows[:, 1:3], vgpu.cells_to_world(frec["best_cell"][order], nx, x0, y0, res))
    assert np.array_equal(rows[:, 3].astype(np.int64), frec["best_pot"][order].astype(np.int64))
    for col, name in enumerate(("n_unknown", "n_free", "n_occupied", "n_rays_open")):
        assert np.array_equal(rows[:, 4 + col].astype(np.int64), rec[name][order]), name
    assert ("view gain: %d of %d frontiers, radius %d cells, %d unknown cells in view"
            % (order.size, frec.size, R, s["unknown_seen"])) in out, out
