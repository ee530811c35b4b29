"""vg_frontiers (vina_gpu.h "Exploration frontiers") against the numpy restatement
of its definition (tests/frontier_ref.py), bit for bit: the labels, the records
and the summary. Grids are the smallest at which the kernels can still go wrong:
a tile is 64 x 64 cells, so 61 x 47 is one partial tile, 130 x 67 two tiles and a
remainder each way; the serpentine's one frontier changes tile 99 times; the
border cases cross a tile border by a single diagonal step."""
import ctypes

import numpy as np
import pytest

import clr_ref as cr
import frontier_ref as fr
import nav_ref as nr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
TRAV = nr.trav_table()
U, F, O = fr.UNKNOWN, fr.FREE, fr.OCCUPIED

_cache = {}


def _ctx():
    """A context with no map (shared, never closed): vg_frontiers reads none."""
    if "C" not in _cache:
        _cache["C"] = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    return _cache["C"]


def _same(got, want):
    lab, rec, s = got
    wl, wr, ws = want
    if wl is not None:
        assert lab.dtype == np.int32 and lab.shape == wl.shape
        bad = np.argwhere(lab != wl)
        assert not bad.size, (bad[:8], lab[tuple(bad[0])], wl[tuple(bad[0])])
    assert rec.dtype == fr.REC and rec.tobytes() == wr.tobytes(), (rec, wr)
    assert s == ws, (s, ws)


def _check(grid, cost=None, pot=None, C=None, **kw):
    """frontiers(grid) on the device equals the restatement. pot: the field to leave on the device first, by a navfn
    call whose result it is (cost_for_pot, goals). Returns the device's tuple."""
    C = C or _ctx()
    grid = np.ascontiguousarray(grid, dtype=np.int8)
    field = None
    if pot is not None:
        field, _ = C.navfn(pot[0], pot[1])
    got = C.frontiers(grid, cost=cost, use_pot=pot is not None, **kw)
    ref_kw = {k: v for k, v in kw.items() if k in ("cost_max", "min_size", "max_records")}
    want = fr.frontiers(grid, cost=cost, pot=field, **ref_kw)
    _same(got, want)
    print("frontiers %d x %d: %s" % (grid.shape[1], grid.shape[0], got[2]))
    return got


@pytest.mark.parametrize("nx,ny,seed", [(61, 47, 7), (130, 67, 11), (67, 130, 11)])
def test_against_the_restatement(nx, ny, seed):
    """1: random grids with 7 % unknown; plain, with the cost test on clr_ref's plane, with the reach test on a
    field from one goal, and with both."""
    g = cr.random_grid(nx, ny, seed, p_unknown=0.07)
    lab, rec, s = _check(g)
    if nx > 64:
        assert s["n_components"] >= 100 and fr.spanning(lab) >= 10
    assert s["n_kept"] == s["n_components"] == rec.size and (rec["best_cell"] == -1).all()
    cost = cr.clearance(g, **cr.PARAMS["nav"])["cost"]
    _, _, sc = _check(g, cost=cost)
    assert 0 < sc["n_rejected_cost"] and sc["n_frontier_cells"] + sc["n_rejected_cost"] == s["n_frontier_cells"]
    _check(g, cost=cost, cost_max=40)
    goal = [[int(v) for v in np.argwhere(cost == 0)[0][::-1]]]
    _, rp, sp = _check(g, pot=(cost, goal))
    assert 0 < sp["n_rejected_unreached"] and (rp["best_cell"] >= 0).all() and rp.size > 5
    _, _, sb = _check(g, cost=cost, pot=(cost, goal), min_size=2)
    assert sb["n_rejected_cost"] == sc["n_rejected_cost"] and 0 < sb["n_kept"] < sb["n_components"]
    for combine in (0, 1):           # the statistics kernel's two variants give the same bytes
        vgpu.lib().vgx_frontier_combine(_ctx().h, combine)
        _check(g, pot=(cost, goal))
    assert _ctx().frontiers_ms() > 0.0


@pytest.mark.parametrize("shape", [(1, 300), (300, 1)])     # [ny, nx]
def test_lines(shape):
    """2: a row and a column of 300 cells, five tiles in a line, with more than 64 tiny components: one-cell
    frontiers on either side of every unknown cell; free runs whose two ends are separate frontiers; two-cell
    frontiers astride the tile borders."""
    g = np.zeros(300, dtype=np.int8)
    g[2::5] = U                      # F F U F O | F F U F O: the two cells beside each U, each a frontier of its own
    g[4::5] = O
    g = g.reshape(shape)
    lab, rec, s = _check(g)
    assert s["n_components"] >= 64 and s["max_size"] <= 2
    g = np.zeros(300, dtype=np.int8)
    g[0::9] = U                      # free runs of 8 between unknowns: the runs' two end cells are separate frontiers
    _check(g.reshape(shape))
    g = np.where(np.arange(300) % 7 == 3, U, F).astype(np.int8)
    g[63] = g[64] = g[127] = g[128] = F
    g[62] = g[65] = g[126] = g[129] = U      # two-cell frontiers astride the borders 63 | 64 and 127 | 128
    lab, rec, s = _check(g.reshape(shape))
    assert lab.ravel()[64] == 63 and lab.ravel()[128] == 127


def test_serpentine():
    """3: one frontier of 6630 cells that changes tile 99 times: what a round-by-round propagation gets slowly and a
    broken merge gets wrong."""
    lab, rec, s = _check(fr.serpentine_grid())
    assert rec.size == 1 and rec[0]["label"] == 0 and rec[0]["size"] == 6630 and s["n_components"] == 1
    assert s["max_size"] == 6630 == s["n_frontier_cells"]
    # transposed: the corridor runs along the columns, and the tiles stack the other way
    lab, rec, s = _check(np.ascontiguousarray(fr.serpentine_grid().T))
    assert s["n_components"] == 1 and rec[0]["size"] == 6630


def _cells(shape, free, unknown):
    g = np.full(shape, O, dtype=np.int8)
    for x, y in free:
        g[y, x] = F
    for x, y in unknown:
        g[y, x] = U
    return g


def test_border_cases():
    """4: frontiers that cross a tile border only by a diagonal step: x = 63 | 64, y = 63 | 64, and each of the two
    diagonals of the corner where four tiles meet; a U whose arms start in different tiles and join only in the
    last tile, so that the smaller label has to travel backwards."""
    shape = (130, 130)
    # (63, 10) - (64, 11): only the diagonal joins them; each has an unknown beside it
    lab, rec, s = _check(_cells(shape, [(63, 10), (64, 11)], [(62, 10), (65, 11)]))
    assert s["n_components"] == 1 and rec[0]["size"] == 2
    lab, rec, s = _check(_cells(shape, [(63, 11), (64, 10)], [(62, 11), (65, 10)]))
    assert s["n_components"] == 1 and rec[0]["label"] == 10 * 130 + 64
    # across y = 63 | 64
    lab, rec, s = _check(_cells(shape, [(10, 63), (11, 64)], [(10, 62), (11, 65)]))
    assert s["n_components"] == 1 and rec[0]["size"] == 2
    lab, rec, s = _check(_cells(shape, [(11, 63), (10, 64)], [(11, 62), (10, 65)]))
    assert s["n_components"] == 1 and rec[0]["size"] == 2
    # the corner (63 | 64, 63 | 64): the main diagonal, then the other one
    lab, rec, s = _check(_cells(shape, [(63, 63), (64, 64)], [(63, 62), (64, 65)]))
    assert s["n_components"] == 1 and rec[0]["label"] == 63 * 130 + 63
    lab, rec, s = _check(_cells(shape, [(64, 63), (63, 64)], [(64, 62), (63, 65)]))
    assert s["n_components"] == 1 and rec[0]["label"] == 63 * 130 + 64
    # all four corner cells free with unknowns outside: one frontier of 4; and the two diagonals apart when the
    # grid has only those
    lab, rec, s = _check(_cells(shape, [(63, 63), (64, 63), (63, 64), (64, 64)], [(62, 63), (65, 63), (62, 64), (65, 64)]))
    assert s["n_components"] == 1 and rec[0]["size"] == 4
    # a U: arms down the columns x = 20 (tile 0) and x = 100 (tile 1) from y = 5, joined along y = 120 (tiles 2, 3);
    # unknown beside every cell of it. The arm at x = 100 learns the label of (20, 5) only through the last tiles
    g = np.full(shape, O, dtype=np.int8)
    g[5:121, 20] = g[5:121, 100] = F
    g[5:121, 19] = g[5:121, 101] = U
    g[120, 20:101] = F
    g[121, 20:101] = U
    lab, rec, s = _check(g)
    assert s["n_components"] == 1 and rec[0]["label"] == 5 * 130 + 20 and lab[5, 100] == 5 * 130 + 20
    assert rec[0]["size"] == 2 * 116 + 79
    # the same with the left arm starting lower: the label starts in tile 1 and travels to tile 0 through tiles 3, 2
    g[5:40, 20] = O
    lab, rec, s = _check(g)
    assert s["n_components"] == 1 and rec[0]["label"] == 5 * 130 + 100 and lab[40, 20] == 5 * 130 + 100


def test_degenerate():
    """5: grids without any frontier; 1 x 1; min_size above every size; max_records 0 and below n_kept."""
    for v in (U, F, O):
        lab, rec, s = _check(np.full((70, 67), v, dtype=np.int8))
        assert (lab == -1).all() and rec.size == 0 and (s["n_components"], s["n_kept"], s["max_size"]) == (0, 0, 0)
        assert s["cells_free"] == (70 * 67 if v == F else 0) and s["cells_unknown"] == (70 * 67 if v == U else 0)
    for v in (U, F, O):
        lab, rec, s = _check(np.array([[v]], dtype=np.int8))
        assert lab[0, 0] == -1 and s["n_frontier_cells"] == 0
    lab, rec, s = _check(np.array([[F, U]], dtype=np.int8))
    assert lab.tolist() == [[0, -1]] and rec[0].tolist()[:8] == (0, 1, 0, 0, 0, 0, 0, 0)
    g = cr.random_grid(130, 67, 11, p_unknown=0.07)
    _, _, s0 = _check(g)
    lab, rec, s = _check(g, min_size=s0["max_size"] + 1)
    assert s["n_kept"] == 0 == s["n_written"] and rec.size == 0 and s["n_components"] == s0["n_components"]
    lab, rec, s = _check(g, max_records=0)                          # recs == NULL
    assert rec.size == 0 and s["n_written"] == 0 and s["n_kept"] == s0["n_kept"]
    lab, rec, s = _check(g, max_records=7, min_size=2)
    assert rec.size == 7 == s["n_written"] < s["n_kept"] and (np.diff(rec["label"]) > 0).all()
    none, rec2, s2 = _ctx().frontiers(g, max_records=7, min_size=2, want_labels=False)
    assert none is None and rec2.tobytes() == rec.tobytes() and s2 == s


def test_best_cell_ties():
    """6: an open plane, a column of frontier cells, the goal level with the middle of two of them: both cost the
    same, and the smaller index wins."""
    g = np.zeros((9, 12), dtype=np.int8)
    g[:, 11] = U                             # the frontier: the column x = 10
    cost = np.zeros((9, 12), dtype=np.uint8)
    cost[:, 11] = 255
    for goal, best in (([4, 3], 3 * 12 + 10), ([10, 5], 5 * 12 + 10)):
        lab, rec, s = _check(g, pot=(cost, [goal]))
        assert rec.size == 1 and rec[0]["size"] == 9 and rec[0]["best_cell"] == best
    # the goal on the line between the rows 3 and 4 does not exist on a grid: take two goals, (4, 3) and (4, 5):
    # the cells (10, 3) and (10, 5) tie at 6 steps of 1200, and (10, 4) costs a diagonal more
    field, _ = _ctx().navfn(cost, [[4, 3], [4, 5]])
    assert field[3, 10] == field[5, 10] == 7200 < field[4, 10]
    lab, rec, s = _check(g, pot=(cost, [[4, 3], [4, 5]]))
    assert rec[0]["best_cell"] == 3 * 12 + 10 and rec[0]["best_pot"] == 7200


def test_chain_and_state():
    """7a: occupancy -> clearance -> navfn -> frontiers on the planes where they lie equals the same call on the
    downloaded planes; two runs and a second context give identical bytes; VG_E_STATE without a plane, on another
    nx, ny for each of the three planes and on a sharded context; vg_clearance's and vg_nav_paths' outputs are
    what they were."""
    import loc_common as lc
    import test_occupancy_gpu as tog
    w = tog._work()
    M, geom = w["M"], w["geom"]
    nx, ny = geom["nx"], geom["ny"]
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)

    def refused(call, word=None):
        with pytest.raises(vgpu.VgError) as ei:
            call()
        assert "(-5)" in str(ei.value) and (word is None or word in str(ei.value)), str(ei.value)

    refused(lambda: T.frontiers(None, nx=nx, ny=ny), "vg_occupancy")
    refused(lambda: T.frontiers(w["grid"], use_cost=True), "vg_clearance")
    refused(lambda: T.frontiers(w["grid"], use_pot=True), "vg_navfn")
    M.occupancy(w["pos"], w["dirs"], **geom, **tog.BAND)
    out, _ = M.clearance(None, nx=nx, ny=ny, **cr.PARAMS["nav"])
    cost = out["cost"]
    robot = nr.passable_cells(cost, TRAV, 1, 2)
    pot, _ = M.navfn(None, robot, nx=nx, ny=ny)
    starts = nr.passable_cells(cost, TRAV, 8, 3)
    paths = M.nav_paths(starts, 200)
    dev = M.frontiers(None, nx=nx, ny=ny, use_cost=True, use_pot=True)
    again = M.frontiers(None, nx=nx, ny=ny, use_cost=True, use_pot=True)
    host = M.frontiers(w["grid"], cost=cost, use_pot=True)
    T.navfn(cost, robot)
    other = T.frontiers(w["grid"], cost=cost, use_pot=True)
    for r in (again, host, other):
        assert r[0].tobytes() == dev[0].tobytes() and r[1].tobytes() == dev[1].tobytes() and r[2] == dev[2]
    _same(dev, fr.frontiers(w["grid"], cost=cost, pot=pot))
    assert dev[2]["n_components"] >= 1 and dev[1].size >= 1
    order = vgpu.frontier_order(dev[1])
    assert order.tolist() == fr.frontier_order(dev[1]).tolist() and dev[1][order[0]]["best_pot"] == dev[1]["best_pot"].min()
    # a shape mismatch for each of the three planes
    refused(lambda: M.frontiers(None, nx=nx + 1, ny=ny), "vg_occupancy")
    refused(lambda: M.frontiers(np.zeros((ny, nx + 1), dtype=np.int8), use_cost=True), "vg_clearance")
    refused(lambda: M.frontiers(np.zeros((ny + 1, nx), dtype=np.int8), use_pot=True), "vg_navfn")
    T.close()
    # the refused calls and the frontiers left the neighbours' planes alone
    out2, _ = M.clearance(None, nx=nx, ny=ny, **cr.PARAMS["nav"])
    assert out2["cost"].tobytes() == cost.tobytes()
    for a, b in zip(M.nav_paths(starts, 200), paths):
        assert np.array_equal(a, b)
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    refused(lambda: S.frontiers(w["grid"]), "sharded")
    S.close()


def test_argument_errors():
    """7b: every VG_E_ARG condition returns it and writes nothing, neither an output nor the summary."""
    C = _ctx()
    L, P = vgpu.lib(), C.h
    nx, ny = 8, 5
    g = cr.random_grid(nx, ny, 3)
    cost = np.zeros((ny, nx), dtype=np.uint8)
    lab = np.full(nx * ny, 7, dtype=np.int32)
    rec = np.full(4, 7, dtype=np.uint8).repeat(64).view(fr.REC)
    sm = vgpu.FrontierSummary()

    def params(**kw):
        p = vgpu.FrontierParams()
        for k, v in dict(dict(nx=nx, ny=ny), **kw).items():
            setattr(p, k, v)
        return p

    def call(ctx=P, prm=params(), c=None, r=rec.ctypes.data, n=4, out=sm):
        return L.vg_frontiers(ctx, g.ctypes.data, c, None if prm is None else ctypes.byref(prm), lab.ctypes.data, r, n,
                              None if out is None else ctypes.byref(out))

    bad = [dict(ctx=None), dict(prm=None), dict(out=None), dict(r=None), dict(n=-1), dict(n=vgpu.FRONTIER_MAX_RECORDS + 1),
           dict(c=cost.ctypes.data), dict(c=cost.ctypes.data, prm=params(flags=2))]
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-4), dict(nx=vgpu.CLR_MAX_SIDE + 1, ny=1), dict(nx=1, ny=vgpu.CLR_MAX_SIDE + 1),
               dict(nx=4097, ny=4097), dict(flags=4), dict(flags=7), dict(flags=-1), dict(flags=1, cost_max=-1),
               dict(flags=1, cost_max=256), dict(cost_max=300)):
        bad.append(dict(prm=params(**kw)))
    before = rec.tobytes()
    for kw in bad:
        assert call(**kw) == -1, kw
        assert (lab == 7).all() and rec.tobytes() == before and not bytes(sm).strip(b"\0"), kw
    assert call() == 0
    want = fr.frontiers(g, max_records=4)
    assert np.array_equal(lab.reshape(ny, nx), want[0]) and rec[:sm.n_written].tobytes() == want[1].tobytes()
    assert {k: getattr(sm, k) for k in fr.SUMMARY} == want[2]
    assert call(c=cost.ctypes.data, prm=params(flags=1, cost_max=255)) == 0
    assert L.vg_frontiers(P, g.ctypes.data, None, ctypes.byref(params()), None, None, 0, ctypes.byref(sm)) == 0


def test_replay_frontiers(tmp_path):
    """7c: vg_node_replay ... --costmap C --frontiers out.csv writes one label,size,cx,cy,best_x,best_y,best_pot row
    per kept frontier of Context.frontiers over the replay's grid and read_costmap(C)'s plane, in frontier_order, and
    prints their count; with --plan the frontiers are ranked by that field; without --costmap it is refused."""
    import math
    import os
    import re
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
    pre, cpre, csv, path = str(tmp_path / "nav"), str(tmp_path / "cost"), tmp_path / "fr.csv", tmp_path / "plan.csv"
    prm = cr.PARAMS["replay"]
    base = [log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--occupancy", pre, "--occ-res", prm["res"]]
    cm = ["--costmap", cpre, "--inscribed", prm["inscribed_radius"], "--inflation", prm["inflation_radius"],
          "--cost-scaling", prm["cost_scaling"]]
    run(base + ["--frontiers", csv], rc=2)
    C = _ctx()

    def compare(out, goal_xy):
        grid, gx0, gy0, gres = vgpu.read_occupancy(pre)
        cost, x0, y0, res = vgpu.read_costmap(cpre)
        assert grid.shape == cost.shape and (gx0, gy0, gres) == (x0, y0, res)
        nx = cost.shape[1]
        if goal_xy is not None:
            C.navfn(cost, [[math.floor((goal_xy[0] - x0) / res), math.floor((goal_xy[1] - y0) / res)]])
        lab, rec, s = C.frontiers(grid, cost=cost, use_pot=goal_xy is not None)
        rec = rec[vgpu.frontier_order(rec)]
        rows = np.loadtxt(csv, delimiter=",", ndmin=2) if os.path.getsize(csv) else np.zeros((0, 7))
        assert rows.shape == (rec.size, 7) and rec.size >= 1
        assert np.array_equal(rows[:, 0].astype(np.int64), rec["label"]) and np.array_equal(rows[:, 1].astype(np.int64), rec["size"])
        cx = x0 + (rec["sum_x"] / rec["size"] + 0.5) * res
        cy = y0 + (rec["sum_y"] / rec["size"] + 0.5) * res
        assert np.allclose(rows[:, 2], cx, rtol=0, atol=1e-9) and np.allclose(rows[:, 3], cy, rtol=0, atol=1e-9)
        if goal_xy is not None:
            assert np.array_equal(rows[:, 4:6], vgpu.cells_to_world(rec["best_cell"], nx, x0, y0, res))
            assert np.array_equal(rows[:, 6].astype(np.int64), rec["best_pot"].astype(np.int64))
        assert ("frontiers: %d kept of %d, %d cells" % (s["n_kept"], s["n_components"], s["n_frontier_cells"])) in out, out

    out = run(base + cm + ["--frontiers", csv])
    compare(out, None)
    goal = (float(p0[0]), float(p0[1]))
    out = run(base + cm + ["--plan", "%r %r" % goal, "--path", path, "--frontiers", csv])
    compare(out, goal)
