"""The parts the 2-D query layers share (csrc/vg_reduce.h, csrc/query_host.cpp), where the layers' own tests reach
them only indirectly: the tails of the wave and workgroup reductions behind every summary count, and the state and
shape errors of the entry points with their texts.

Shapes: 1 x 1 is a single lane, 63 x 1 a wave one lane short, 65 x 3 a wave one lane over (and a second tile of 64),
257 x 2 one lane past a 256-thread workgroup. The expected counts are numpy's on the planes the call returned and the
restatements' (clr_ref, nav_ref, frontier_ref, view_ref), never a second run of the device code."""
import numpy as np
import pytest

import clr_ref as cr
import frontier_ref as fr
import nav_ref as nr
import view_ref as vr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
U, F, O = cr.UNKNOWN, cr.FREE, cr.OCCUPIED
SHAPES = [(1, 1), (63, 1), (65, 3), (257, 2)]
RES = dict(res=0.25)

_cache = {}


def _ctx():
    """A context with no map (shared, never closed): none of these calls reads one."""
    if "C" not in _cache:
        _cache["C"] = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    return _cache["C"]


def _grid(nx, ny):
    """A seeded grid with all three classes (1 x 1 holds one cell: free) and its viewpoints, free cells inside it."""
    g = cr.random_grid(nx, ny, 100 * nx + ny, p_occ=0.15, p_unknown=0.35, n_other=1)
    views = [[0, 0]] if nx * ny == 1 else [[0, 0], [nx - 1, ny - 1]]
    if nx * ny >= 5:
        g.ravel()[[1, 2]] = U, O
    for x, y in views:
        g[y, x] = F
    assert nx * ny == 1 or {U, F, O} <= set(g.ravel().tolist())
    return g, np.array(views, dtype=np.int32)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_clearance_counts(nx, ny):
    g, _ = _grid(nx, ny)
    for flags in (0, 1):
        out, s = _ctx().clearance(g, flags=flags, **cr.PARAMS["nav"])
        want = cr.summary(g, flags, out["dist2"], out["cost"])
        print(nx, ny, flags, s)
        assert s == want, (s, want)
        ref = cr.clearance(g, flags, **cr.PARAMS["nav"])
        assert all(np.array_equal(out[k], ref[k]) for k in ("dist2", "nearest", "cost"))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_frontier_counts(nx, ny):
    g, _ = _grid(nx, ny)
    lab, rec, s = _ctx().frontiers(g)
    roots = lab.ravel() == np.arange(nx * ny)
    sizes = np.bincount(lab.ravel()[lab.ravel() >= 0], minlength=nx * ny)[roots]
    want = dict(n_frontier_cells=int((lab >= 0).sum()), n_components=int(roots.sum()), n_kept=int(roots.sum()),
                n_written=int(rec.size), max_size=int(sizes.max()) if sizes.size else 0, cells_free=int((g == F).sum()),
                cells_unknown=int((g == U).sum()), n_rejected_cost=0, n_rejected_unreached=0)
    print(nx, ny, s)
    assert s == want, (s, want)
    lab_r, rec_r, s_r = fr.frontiers(g)
    assert np.array_equal(lab, lab_r) and rec.tobytes() == rec_r.tobytes() and s == s_r
    # the rejections' counts: every cell too costly, then every cell unreached
    cost = np.full((ny, nx), 254, dtype=np.uint8)
    _, _, sc = _ctx().frontiers(g, cost=cost)
    assert sc == fr.frontiers(g, cost=cost)[2] and sc["n_rejected_cost"] == s["n_frontier_cells"]


@pytest.mark.parametrize("nx,ny", SHAPES)
@pytest.mark.parametrize("R", [1, 2])
def test_view_counts(nx, ny, R):
    g, views = _grid(nx, ny)
    rec, seen, s = _ctx().view_gain(views, R, g, want_seen=True)
    ok = rec["status"] == vr.OK
    gain = np.where(ok, rec["n_unknown"], -1)
    want = dict(n_views=int(views.shape[0]), n_ok=int(ok.sum()), n_outside=int((rec["status"] == vr.OUTSIDE).sum()),
                n_blocked=int((rec["status"] == vr.BLOCKED).sum()), rays=8 * R * int(ok.sum()),
                max_unknown_seen=int(gain.max()), best_view=int(np.argmax(gain)), cells_seen=int((seen > 0).sum()),
                unknown_seen=int(((seen > 0) & (g == U)).sum()))
    print(nx, ny, R, s)
    assert s == want and ok.all(), (s, want)
    rec_r, seen_r, s_r, _ = vr.view_gain(g, views, R)
    assert rec.tobytes() == rec_r.tobytes() and np.array_equal(seen, seen_r) and s == s_r
    assert (rec["n_visible"] == rec["n_unknown"] + rec["n_free"] + rec["n_occupied"]).all()


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_navfn_counts(nx, ny):
    cost = nr.random_plane(nx, ny, 100 * nx + ny, p_lethal=0.03)   # (few walls: the field spans the waves' tails)
    cost[0, 0] = 0
    trav = nr.trav_table()
    goal = nr.passable_cells(cost, trav, 1, 5)
    pot, s = _ctx().navfn(cost, goal)
    want = nr.summary(cost, trav, goal, pot)
    print(nx, ny, s)
    assert {k: s[k] for k in nr.REPRODUCIBLE} == want and want["n_goals_used"] == 1, (s, want)
    tiles = ((nx + 63) // 64) * ((ny + 63) // 64)
    assert 1 <= s["rounds"] and 1 <= s["tile_runs"] <= s["rounds"] * tiles   # (these two depend on the schedule)
    assert np.array_equal(pot, nr.potential(cost, trav, goal))
    # a goal outside the grid and one on a lethal cell: both ignored, nothing reached
    cost[0, 0] = 254
    pot, s = _ctx().navfn(cost, [[-1, 0], [0, 0]])
    assert {k: s[k] for k in nr.REPRODUCIBLE} == nr.summary(cost, trav, [[-1, 0], [0, 0]], pot)
    assert s["n_goals_ignored"] == 2 and s["cells_reached"] == 0


NO_GRID = "%s: grid == NULL, and no vg_occupancy call left a grid on this context"
NO_COST = "%s: cost == NULL, and no vg_clearance call left a cost plane on this context"
COST_DIFFERS = "%s: cost == NULL, and the last vg_clearance call's nx, ny differ from prm's"
NO_FIELD = "vg_frontiers: flags bit 1, and no vg_navfn call left a field on this context"
FIELD_DIFFERS = "vg_frontiers: flags bit 1, and the last vg_navfn call's nx, ny differ from prm's"
NO_FIELD_PATHS = "vg_nav_paths: no vg_navfn call left a field on this context"


def _refused(call, code, text=None):
    with pytest.raises(vgpu.VgError) as ei:
        call()
    msg = str(ei.value)
    assert "(%d): " % code in msg, msg
    if text is not None:
        assert msg.split("): ", 1)[1] == text, msg


def test_state_and_shape_errors():
    """VG_E_STATE (-5) and its text where a call names a device plane that is not there or has another shape, and
    VG_E_ARG (-1) for the shapes outside the limits, on a fresh context and an 8 x 8 shape."""
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    g, _ = _grid(8, 8)
    g9 = np.zeros((8, 9), dtype=np.int8)
    table = [
        (lambda: T.clearance(None, nx=8, ny=8, **RES), NO_GRID % "vg_clearance"),
        (lambda: T.frontiers(None, nx=8, ny=8), NO_GRID % "vg_frontiers"),
        (lambda: T.view_gain([[1, 1]], 2, None, nx=8, ny=8), NO_GRID % "vg_view_gain"),
        (lambda: T.navfn(None, [[1, 1]], nx=8, ny=8), NO_COST % "vg_navfn"),
        (lambda: T.frontiers(g, use_cost=True), NO_COST % "vg_frontiers"),
        (lambda: T.frontiers(g, use_pot=True), NO_FIELD),
        (lambda: T.nav_paths([[1, 1]], 4), NO_FIELD_PATHS),
    ]
    for call, text in table:
        _refused(call, -5, text)
    # an occupancy-free chain on a caller grid leaves a cost plane and a field of 8 x 8
    out, _ = T.clearance(g, want=("cost",), **cr.PARAMS["nav"])
    assert set(out) == {"cost"}
    T.navfn(None, [[0, 0]], nx=8, ny=8)
    T.frontiers(g, use_cost=True, use_pot=True)
    T.nav_paths([[0, 0]], 4)
    for call, text in [
        (lambda: T.navfn(None, [[1, 1]], nx=9, ny=8), COST_DIFFERS % "vg_navfn"),
        (lambda: T.frontiers(g9, use_cost=True), COST_DIFFERS % "vg_frontiers"),
        (lambda: T.frontiers(g9, use_pot=True), FIELD_DIFFERS),
        (lambda: T.frontiers(g9, use_cost=True, use_pot=True), COST_DIFFERS % "vg_frontiers"),   # the cost check wins
        (lambda: T.clearance(None, nx=8, ny=8, **RES), NO_GRID % "vg_clearance"),                # still no grid
        (lambda: T.frontiers(None, nx=8, ny=8, use_cost=True, use_pot=True), NO_GRID % "vg_frontiers"),
        (lambda: T.view_gain([[1, 1]], 2, None, nx=8, ny=8), NO_GRID % "vg_view_gain"),
    ]:
        _refused(call, -5, text)
    # the shape check comes before any state check
    for nx in (0, vgpu.CLR_MAX_SIDE + 1):
        for call in (lambda: T.clearance(None, nx=nx, ny=8, **RES), lambda: T.navfn(None, [[0, 0]], nx=nx, ny=8),
                     lambda: T.frontiers(None, nx=nx, ny=8), lambda: T.view_gain([[0, 0]], 1, None, nx=nx, ny=8)):
            _refused(call, -1)
    # vgx_ter_cells: the cell limit alone, no side limit (a row of CLR_MAX_SIDE + 1 cells is a legal grid there)
    n = vgpu.CLR_MAX_SIDE + 1
    g_n, g_min, g_max = (np.zeros(n, dtype=np.int32) for _ in range(3))
    g_sum, out3 = np.zeros(n, dtype=np.int64), np.zeros(3, dtype=np.int64)
    L = vgpu.lib()

    def ter_cells(nx, ny):
        return L.vgx_ter_cells(T.h, nx, ny, 1, g_n.ctypes.data, g_sum.ctypes.data, g_min.ctypes.data, g_max.ctypes.data,
                               None, None, out3.ctypes.data)

    assert ter_cells(0, 1) == -1 and ter_cells(1, 0) == -1 and ter_cells(4097, 4097) == -1
    assert ter_cells(n, 1) == 0 and out3.tolist() == [0, 0, 0]
    T.close()
