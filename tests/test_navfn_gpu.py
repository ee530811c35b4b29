"""vg_navfn and vg_nav_paths (vina_gpu.h "Navigation function") against the numpy
restatement of their definition (tests/nav_ref.py), bit for bit: the potential,
the paths, their statuses and every reproducible field of the summary. Planes
are the smallest at which the kernels can still go wrong: a tile is 64 x 64
cells, so 61 x 47 is one partial tile, 130 x 67 two tiles and a remainder each
way; the serpentine re-enters its tiles dozens of times; the saturated corridor
needs 4000 cells to pass 2^32."""
import ctypes

import numpy as np
import pytest

import nav_ref as nr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
TRAV = nr.trav_table()

_cache = {}


def _ctx():
    """A context with no map (shared, never closed): vg_navfn reads none."""
    if "C" not in _cache:
        _cache["C"] = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    return _cache["C"]


def _check(cost, goals, trav=None, C=None, **params):
    """navfn(cost, goals) on the device equals the restatement, and its summary counts it. Returns (pot, summary)."""
    cost = np.ascontiguousarray(cost, dtype=np.uint8)
    table = nr.trav_table(**params) if trav is None else trav
    ref = nr.potential(cost, table, goals)
    pot, s = (C or _ctx()).navfn(cost, goals, trav=trav, **params)
    assert pot.dtype == np.uint32 and pot.shape == cost.shape
    bad = np.argwhere(pot != ref)
    assert not bad.size, (bad[:8], pot[tuple(bad[0])], ref[tuple(bad[0])])
    want = nr.summary(cost, table, goals, ref)
    print("navfn %d x %d: %s" % (cost.shape[1], cost.shape[0], s))
    assert {k: s[k] for k in nr.REPRODUCIBLE} == want
    assert s["rounds"] >= 1 and s["tile_runs"] >= (1 if want["n_goals_used"] else 0)
    return pot, s


def _check_paths(cost, table, pot, starts, max_len, C=None):
    """nav_paths(starts) on the device equals the restatement's descent of pot. Returns the device's tuple."""
    got = (C or _ctx()).nav_paths(starts, max_len)
    want = nr.descend(cost, table, pot, starts, max_len)
    for g, w, name in zip(got, want, ("cells", "len", "status", "path_cost")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, g, w)
    nr.check_paths(cost, table, pot, *got[:3])
    return got


@pytest.mark.parametrize("flags", [0, 1])
def test_against_the_restatement(flags):
    """1: 61 x 47, costs 0 .. 252, 25 % lethal, 5 % unknown, two goals, both values of flags bit 0."""
    cost = nr.random_plane(61, 47, 7)
    assert cost.shape == (47, 61) and (cost >= 253).mean() > 0.2 and (cost == 255).sum() > 80
    prm = dict(flags=flags, unknown_as=100)
    goals = nr.passable_cells(cost, nr.trav_table(**prm), 2, 7)
    pot, s = _check(cost, goals, **prm)
    assert s["n_goals_used"] == 2 and 1000 < s["cells_reached"] <= s["cells_passable"] and s["cells_saturated"] == 0
    assert ((cost == 255) & (pot != nr.UNREACHED)).any() == bool(flags)
    assert s["cells_passable"] == int((cost < 253).sum()) + (int((cost == 255).sum()) if flags else 0)


def test_tie_breaks():
    """2: an open 7 x 7 plane, the start in the centre, two goals mirrored about it. Left and right neighbour tie
    at 2400 + 1200 (the diagonals cost 2900 + 1700): the smaller index, the left one, wins; mirrored about the row,
    the upper one."""
    cost = np.zeros((7, 7), dtype=np.uint8)
    pot, _ = _check(cost, [[0, 3], [6, 3]])
    assert pot[3].tolist() == [0, 1200, 2400, 3600, 2400, 1200, 0]
    cells, ln, status, pc = _check_paths(cost, TRAV, pot, [[3, 3]], 10)
    assert cells[0, :ln[0]].tolist() == [24, 23, 22, 21] and status[0] == vgpu.NAV_REACHED and pc[0] == 3600
    pot, _ = _check(cost, [[3, 0], [3, 6]])
    cells, ln, status, pc = _check_paths(cost, TRAV, pot, [[3, 3], [2, 3]], 10)
    assert cells[0, :ln[0]].tolist() == [24, 17, 10, 3] and status[0] == vgpu.NAV_REACHED
    # from (2, 3) the step up to (2, 2), 2900 + 1200, ties with the diagonal to (3, 2), 2400 + 1700: a tie across
    # the two kinds of step, and the smaller index wins
    assert pot[3, 2] == 4100 and cells[1, :2].tolist() == [23, 16]


def test_corner_cutting():
    """3: a wall whose only gap is two lethal cells touching diagonally leaves the far side unreached; one of the
    two cells freed, it is reached."""
    cost = np.zeros((9, 11), dtype=np.uint8)
    cost[:, 5] = 254
    cost[:, 6] = 254
    cost[4, 5] = cost[5, 6] = 0              # (5, 4) and (6, 5) free: between them only the corner of (6, 4), (5, 5)
    pot, s = _check(cost, [[0, 0]])
    assert pot[4, 5] != nr.UNREACHED and pot[5, 6] == nr.UNREACHED and (pot[:, 7:] == nr.UNREACHED).all()
    assert s["cells_reached"] == 9 * 5 + 1
    cost[4, 6] = 0
    pot, s = _check(cost, [[0, 0]])
    assert (pot[:, 7:] != nr.UNREACHED).all() and s["cells_reached"] == s["cells_passable"] == 9 * 9 + 3


def test_degenerate():
    """4: every cell lethal; a 1 x 1 plane that is its own goal; all goals ignored; a start on a goal."""
    C = _ctx()
    cost = np.full((5, 9), 254, dtype=np.uint8)
    pot, s = _check(cost, [[2, 2]])
    assert (pot == nr.UNREACHED).all() and (s["n_goals_used"], s["n_goals_ignored"], s["cells_passable"]) == (0, 1, 0)
    assert s["max_pot"] == 0
    _, _, status, pc = _check_paths(cost, TRAV, pot, [[2, 2]], 4)
    assert status[0] == vgpu.NAV_NO_PATH and pc[0] == -1
    cost = np.array([[17]], dtype=np.uint8)
    pot, s = _check(cost, [[0, 0]])
    assert pot[0, 0] == 0 and (s["cells_reached"], s["max_pot"]) == (1, 0)
    cells, ln, status, pc = _check_paths(cost, TRAV, pot, [[0, 0]], 1)
    assert (cells[0, 0], ln[0], status[0], pc[0]) == (0, 1, vgpu.NAV_REACHED, 0)
    cost = nr.random_plane(20, 13, 5)
    lethal = np.argwhere(cost == 254)[0]
    pot, s = _check(cost, [[-1, 0], [20, 3], [3, 13], [0, -2], [lethal[1], lethal[0]]])
    assert (pot == nr.UNREACHED).all() and (s["n_goals_used"], s["n_goals_ignored"], s["cells_reached"]) == (0, 5, 0)
    goals = nr.passable_cells(cost, TRAV, 3, 1)
    pot, s = _check(cost, np.concatenate([goals, goals[:1]]))       # a cell named twice counts twice
    assert s["n_goals_used"] == 4
    cells, ln, status, pc = _check_paths(cost, TRAV, pot, goals, 5, C)
    assert ln.tolist() == [1, 1, 1] and (status == vgpu.NAV_REACHED).all() and not pc.any()
    assert np.array_equal(cells[:, 0], goals[:, 1] * 20 + goals[:, 0])


@pytest.mark.parametrize("shape", [(1, 300), (300, 1), (67, 130), (130, 67)])     # [ny, nx]
def test_shapes_that_cross_tiles(shape):
    """5a: a row and a column of 300 cells (five tiles in a line); 130 x 67 and 67 x 130 (two tiles and a remainder
    by one tile and a remainder), random costs with 10 % lethal, a goal in each corner tile."""
    ny, nx = shape
    line = min(shape) == 1
    cost = nr.random_plane(nx, ny, 11, p_lethal=0.0 if line else 0.10, p_unknown=0.0 if line else 0.05)
    if line:
        cost.ravel()[[97, 201]] = 254                                # a corridor cut in three: the middle has no goal
        goals = [[0, 0], [nx - 1, ny - 1]]
    else:
        for gy, gx in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)):
            cost[gy, gx] = 0
        goals = [[0, 0], [nx - 1, 0], [0, ny - 1], [nx - 1, ny - 1]]
    pot, s = _check(cost, goals)
    assert s["n_goals_used"] == len(goals)
    if line:
        assert s["cells_reached"] == 97 + 98 and (pot.ravel()[98:201] == nr.UNREACHED).all()
        _check(cost, [[nx // 2, ny // 2]])                           # ... and from the middle, across two tile borders each way
    else:
        assert s["cells_reached"] > 0.8 * s["cells_passable"] and s["tile_runs"] >= (nx + 63) // 64 * ((ny + 63) // 64)
        _check(cost, [[nx - 1, ny - 1]])                             # one goal: the field crosses every tile border


def test_goal_on_a_tile_rim():
    """5c: a goal whose cell lies on its tile's rim is in a neighbouring tile's halo, and that tile has to run
    though no cell of the goal's tile falls on that side: a row and a column of 300 cells with the goal at 63, 64
    and 128; a one-cell corridor across a tile border, along x and along y, with the goal on the border cell on
    either side; a 3 x 3 free block around the corner where four tiles meet, the goal on each of its cells."""
    for nx, ny in ((300, 1), (1, 300)):
        cost = nr.random_plane(nx, ny, 12, p_lethal=0.0, p_unknown=0.0)
        for k in (63, 64, 128):
            pot, s = _check(cost, [[k if nx > 1 else 0, k if ny > 1 else 0]])
            assert s["cells_reached"] == 300 and pot.ravel()[k] == 0
    cost = np.full((67, 130), 254, dtype=np.uint8)
    cost[10, :] = 0                                                  # along x, across x = 63 | 64
    cost[:, 70] = 0                                                  # along y, across y = 63 | 64
    for goal in ([63, 10], [64, 10], [70, 63], [70, 64]):
        pot, s = _check(cost, [goal])
        assert s["cells_reached"] == s["cells_passable"] == 130 + 67 - 1
    cost = np.full((67, 130), 254, dtype=np.uint8)
    cost[63:66, 63:66] = 0
    for gy in (63, 64, 65):
        for gx in (63, 64, 65):
            pot, s = _check(cost, [[gx, gy]])
            assert s["cells_reached"] == 9
    cost[64, 63:66] = cost[63:66, 64] = 254                          # the four corners alone: nothing but the goal
    pot, s = _check(cost, [[63, 63], [-1, 0]])
    assert s["cells_reached"] == 1 and s["cells_passable"] == 4


def test_serpentine():
    """5b: 200 x 65 cells, walls on the odd rows with gaps at alternating ends: one corridor of 6632 cells that
    re-enters the four tiles of a row band 33 times. max_pot is 6631 steps of 12 (50 + 50)."""
    cost = nr.serpentine()
    assert cost.shape == (65, 200)
    pot, s = _check(cost, [[0, 0]])
    assert s["max_pot"] == 7_957_200 == int(pot[64, 199]) and s["cells_reached"] == s["cells_passable"] == 33 * 200 + 32
    assert s["rounds"] > 33 * 3 + 1                                  # a round carries the field across one tile border
    cells, ln, status, pc = _check_paths(cost, TRAV, pot, [[199, 64], [199, 64]], 7000)
    assert ln.tolist() == [6632, 6632] and status.tolist() == [vgpu.NAV_REACHED] * 2 and pc[0] == 7_957_200
    cells, ln, status, pc = _ctx().nav_paths([[199, 64]], 6631)
    assert (ln[0], status[0], cells[0, -1]) == (6631, vgpu.NAV_TRUNCATED, 1)


def test_saturation():
    """6: a 1 x 4000 corridor under an explicit table of 65535: step k holds 12 * 131070 k up to k = 2730, VG_NAV_SAT
    past it; a start in the plateau is STUCK, one before it REACHED."""
    trav = np.full(256, 65535, dtype=np.uint16)
    cost = np.zeros((1, 4000), dtype=np.uint8)
    pot, s = _check(cost, [[0, 0]], trav=trav)
    k = np.arange(4000, dtype=np.int64)
    assert np.array_equal(pot[0], np.where(k <= 2730, 12 * 131070 * k, vgpu.NAV_SAT))
    assert (s["cells_saturated"], s["cells_reached"], s["max_pot"]) == (4000 - 2731, 4000, vgpu.NAV_SAT)
    cells, ln, status, pc = _check_paths(cost, trav, pot, [[3999, 0], [2732, 0], [2731, 0], [2730, 0], [40, 0]], 4000)
    assert status.tolist() == [vgpu.NAV_STUCK, vgpu.NAV_STUCK, vgpu.NAV_REACHED, vgpu.NAV_REACHED, vgpu.NAV_REACHED]
    assert ln.tolist() == [1, 1, 2732, 2731, 41] and pc.tolist()[:3] == [vgpu.NAV_SAT] * 3
    assert pc[3] == 12 * 131070 * 2730 and cells[4, :41].tolist() == list(range(40, -1, -1))


def test_paths():
    """7: 64 starts in one call against the restatement's descent; TRUNCATED at max_len; NO_PATH for starts outside,
    on a lethal cell and walled off; path_cost is pot[start]; along every path consecutive cells are joined by
    an edge and pot strictly falls (nav_ref.check_paths)."""
    cost = nr.random_plane(130, 67, 3, p_lethal=0.2)
    cost[20:30, 40] = cost[20:30, 50] = cost[20, 40:51] = cost[29, 40:51] = 254       # a closed box
    cost[25, 45] = 0
    goals = nr.passable_cells(cost, TRAV, 2, 4)
    assert not ((goals[:, 0] > 40) & (goals[:, 0] < 50) & (goals[:, 1] > 20) & (goals[:, 1] < 29)).any()
    pot, s = _check(cost, goals)
    assert pot[25, 45] == nr.UNREACHED and TRAV[cost[25, 45]] > 0
    starts = nr.passable_cells(cost, TRAV, 58, 5).tolist()
    lethal = np.argwhere(cost == 254)[0]
    starts += [[-1, 5], [130, 0], [4, 67], [int(lethal[1]), int(lethal[0])], [45, 25], goals[0].tolist()]
    assert len(starts) == 64
    cells, ln, status, pc = _check_paths(cost, TRAV, pot, starts, 400)
    assert status[58:63].tolist() == [vgpu.NAV_NO_PATH] * 5 and not ln[58:63].any() and (pc[58:63] == -1).all()
    assert (status[:58] == vgpu.NAV_REACHED).sum() > 40 and status[63] == vgpu.NAV_REACHED and ln[63] == 1
    st = np.asarray(starts)
    ok = status == vgpu.NAV_REACHED
    assert np.array_equal(pc[ok], pot[st[ok, 1], st[ok, 0]].astype(np.int64)) and ln[ok].max() > 40
    far = int(np.argmax(ln))
    short = int(ln[far]) - 3
    c2, l2, s2, p2 = _check_paths(cost, TRAV, pot, [starts[far], goals[0].tolist()], short)
    assert (l2.tolist(), s2.tolist()) == ([short, 1], [vgpu.NAV_TRUNCATED, vgpu.NAV_REACHED]) and p2[0] == pc[far]
    assert np.array_equal(c2[0], cells[far, :short])
    assert _ctx().navfn_ms() > 0.0


def test_chain_and_determinism():
    """8a: occupancy -> clearance -> navfn(cost=None) equals navfn of the downloaded cost; two runs and a second
    context give identical bytes; want_pot=False still gives the summary and leaves the field for nav_paths;
    VG_E_STATE before any clearance, on another nx, ny, for nav_paths before navfn, and on a sharded context."""
    import clr_ref as cr
    import loc_common as lc
    import test_occupancy_gpu as tog
    w = tog._work()
    M, geom = w["M"], w["geom"]
    nx, ny = geom["nx"], geom["ny"]
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    for call in (lambda: T.navfn(None, [[1, 1]], nx=nx, ny=ny), lambda: T.nav_paths([[1, 1]], 4)):
        with pytest.raises(vgpu.VgError) as ei:
            call()
        assert "(-5)" in str(ei.value)
    M.occupancy(w["pos"], w["dirs"], **geom, **tog.BAND)
    out, _ = M.clearance(None, nx=nx, ny=ny, **cr.PARAMS["nav"])
    cost = out["cost"]
    goals = nr.passable_cells(cost, TRAV, 2, 2)
    dev, sd = M.navfn(None, goals, nx=nx, ny=ny)
    host, sh = M.navfn(cost, goals)
    T.clearance(w["grid"], want=("dist2",), **cr.PARAMS["nav"])     # a call that leaves no cost plane
    with pytest.raises(vgpu.VgError) as ei:
        T.navfn(None, goals, nx=nx, ny=ny)
    assert "(-5)" in str(ei.value)
    other, so = T.navfn(cost, goals)
    T.close()
    drop = lambda s: {k: s[k] for k in nr.REPRODUCIBLE}
    assert dev.tobytes() == host.tobytes() == other.tobytes() and drop(sd) == drop(sh) == drop(so)
    assert np.array_equal(dev, nr.potential(cost, TRAV, goals)) and sd["cells_reached"] > 100
    for bad in (dict(nx=nx + 1, ny=ny), dict(nx=ny, ny=nx - 1)):
        with pytest.raises(vgpu.VgError) as ei:
            M.navfn(None, goals, **bad)
        assert "(-5)" in str(ei.value)
    _check_paths(cost, TRAV, dev, goals, 4, M)                       # the refused calls left the field as it was
    none, sn = M.navfn(None, goals, nx=nx, ny=ny, want_pot=False)
    assert none is None and drop(sn) == drop(sd)
    starts = nr.passable_cells(cost, TRAV, 16, 3)
    _check_paths(cost, TRAV, dev, starts, 200, M)
    again, sa = M.clearance(None, nx=nx, ny=ny, **cr.PARAMS["nav"])  # vg_clearance's bytes are what they were
    assert again["cost"].tobytes() == cost.tobytes()
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    with pytest.raises(vgpu.VgError) as ei:
        S.navfn(cost, goals)
    assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()


def test_argument_errors():
    """8b: every VG_E_ARG condition returns it and writes nothing, neither an output nor the summary."""
    C = _ctx()
    L, P = vgpu.lib(), C.h
    nx, ny = 8, 5
    cost = nr.random_plane(nx, ny, 3)
    goals = np.array([[1, 1], [6, 3]], dtype=np.int32)
    pot = np.full(nx * ny, 7, dtype=np.uint32)
    sm = vgpu.NavSummary()

    def params(**kw):
        p = vgpu.NavParams()
        for k, v in dict(dict(nx=nx, ny=ny), **kw).items():
            setattr(p, k, v)
        return p

    def call(ctx=P, prm=params(), g=goals.ctypes.data, n=2, out=sm):
        return L.vg_navfn(ctx, cost.ctypes.data, None if prm is None else ctypes.byref(prm), None, g, n, pot.ctypes.data,
                          None if out is None else ctypes.byref(out))

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(prm=None), dict(out=None), dict(g=None), dict(n=0), dict(n=-1), dict(n=vgpu.NAV_MAX_POINTS + 1)]
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-4), dict(nx=vgpu.CLR_MAX_SIDE + 1, ny=1), dict(nx=1, ny=vgpu.CLR_MAX_SIDE + 1),
               dict(nx=4097, ny=4097), dict(flags=2), dict(flags=-1), dict(neutral=-1), dict(lethal_from=-1),
               dict(lethal_from=256), dict(unknown_as=-1), dict(unknown_as=255), dict(factor=-0.1), dict(factor=nan),
               dict(factor=inf), dict(factor=300.0), dict(neutral=65500, factor=1.0)):
        bad.append(dict(prm=params(**kw)))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert (pot == 7).all() and not bytes(sm).strip(b"\0"), kw
    assert call() == 0 and sm.n_goals_used + sm.n_goals_ignored == 2
    ref = nr.potential(cost, TRAV, goals)
    assert np.array_equal(pot.reshape(ny, nx), ref)
    cells, ln, st = np.full(8, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32), np.full(2, 7, dtype=np.int32)
    pc = np.full(2, 7, dtype=np.int64)

    def paths(ctx=P, s=goals.ctypes.data, n=2, m=4, c=cells.ctypes.data, l=ln.ctypes.data, t=st.ctypes.data):
        return L.vg_nav_paths(ctx, s, n, m, c, l, t, pc.ctypes.data)

    for kw in (dict(ctx=None), dict(s=None), dict(c=None), dict(l=None), dict(t=None), dict(n=0), dict(n=vgpu.NAV_MAX_POINTS + 1),
               dict(m=0), dict(m=-3), dict(m=vgpu.NAV_MAX_PATH_CELLS // 2 + 1)):
        assert paths(**kw) == -1, kw
        assert (cells == 7).all() and (ln == 7).all() and (st == 7).all() and (pc == 7).all(), kw
    assert paths() == 0 and L.vg_nav_paths(P, goals.ctypes.data, 2, 4, cells.ctypes.data, ln.ctypes.data, st.ctypes.data, None) == 0
    want = nr.descend(cost, TRAV, ref, goals, 4)
    assert np.array_equal(cells.reshape(2, 4), want[0]) and np.array_equal(st, want[2]) and np.array_equal(pc, want[3])


def test_replay_plan(tmp_path):
    """8c: vg_node_replay ... --costmap C --plan "gx gy" [--from "sx sy"] --path out.csv writes one x,y,pot row per
    cell of the path that Context.nav_paths gives over read_costmap(C)'s plane, and prints its status; without
    --costmap it is refused."""
    import math
    import os
    import re
    import subprocess

    import clr_ref as cr
    import synth
    from test_node_core import REPO, _events, _fmt, _write_log
    p = vgconfig.load("mid360")
    g = p["General"]
    seq = synth.Sequence("16line", 12, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    log = tmp_path / "ev.bin"
    _write_log(log, vgconfig.to_c(p), _fmt(g["blind"]), seq.gt_state(0), _events(seq, 16))
    exe = os.path.join(REPO, "vina-slam_amd", "bin", "vg_node_replay")

    def run(args, rc=0):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == rc, r.stderr
        return r.stdout

    ck = tmp_path / "map.vgck"
    run([log, tmp_path / "a.tum", 0, tmp_path / "a.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    pre, cpre, csv = str(tmp_path / "nav"), str(tmp_path / "cost"), tmp_path / "plan.csv"
    prm = cr.PARAMS["replay"]
    base = [log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--occupancy", pre, "--occ-res", prm["res"]]
    cm = ["--costmap", cpre, "--inscribed", prm["inscribed_radius"], "--inflation", prm["inflation_radius"],
          "--cost-scaling", prm["cost_scaling"]]
    run(base + ["--plan", "0 0", "--path", csv], rc=2)
    C = _ctx()

    def compare(out, goal_xy, start_xy):
        cost, x0, y0, res = vgpu.read_costmap(cpre)
        cell = lambda xy: [math.floor((xy[0] - x0) / res), math.floor((xy[1] - y0) / res)]
        pot, s = C.navfn(cost, [cell(goal_xy)])
        cells, ln, status, pc = C.nav_paths([cell(start_xy)], min(cost.size, 65536))
        rows = np.loadtxt(csv, delimiter=",", ndmin=2) if os.path.getsize(csv) else np.zeros((0, 3))
        path = cells[0, :ln[0]]
        assert rows.shape == (ln[0], 3)
        assert np.array_equal(rows[:, :2], vgpu.cells_to_world(path, cost.shape[1], x0, y0, res))
        assert np.array_equal(rows[:, 2].astype(np.int64), pot.ravel()[path].astype(np.int64))
        name = ["REACHED", "NO_PATH", "TRUNCATED", "STUCK"][status[0]]
        assert ("plan: %s, %d cells, cost %d," % (name, ln[0], pc[0])) in out, out
        return cost, x0, y0, res, pot, status[0]

    # the default start: the last pose of the run
    out = run(base + cm + ["--plan", "%r %r" % (float(p0[0]), float(p0[1])), "--path", csv])
    last = [float(v) for v in re.search(r"from (\S+) (\S+) to ", out).groups()]
    assert np.allclose(last, [float(v) for v in open(tmp_path / "g.tum").read().split("\n")[-2].split()[1:3]], atol=1e-8)
    cost, x0, y0, res, pot, _ = compare(out, p0, last)
    # a goal and a start chosen on the plane: the farthest reached cell from the first passable one
    iy, ix = [int(v[0]) for v in np.nonzero(TRAV[cost] > 0)]
    field, s = C.navfn(cost, [[ix, iy]])
    far = int(np.argmax(np.where(field == nr.UNREACHED, 0, field)))
    world = lambda c: vgpu.cells_to_world([c], cost.shape[1], x0, y0, res)[0].tolist()
    goal_xy, start_xy = world(iy * cost.shape[1] + ix), world(far)
    out = run(base + cm + ["--plan", "%r %r" % tuple(goal_xy), "--from", "%r %r" % tuple(start_xy), "--path", csv])
    *_, status = compare(out, goal_xy, start_xy)
    assert status == vgpu.NAV_REACHED and field.ravel()[far] > 0
