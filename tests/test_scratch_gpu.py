"""The query-side scratch (csrc/vg_scratch.h: DevBuf, KernelTimer) through the
calls that own it: every buffer is grown, shrunk back and regrown on one
context, and every result is compared bit for bit with the CPU restatements
(clr_ref, nav_ref) or with the same call's first run on a fresh context. No
tolerances."""
import numpy as np
import pytest

import clr_ref as cr
import loc_common as lc
import nav_ref as nr
import test_occupancy_gpu as tog
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
NAV = cr.PARAMS["nav"]
TRAV = nr.trav_table()
STATE = "(-5)"  # VG_E_STATE in a VgError's text


def _tiny():
    return vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)


def _fresh(call):
    """call(c)'s result on a context that has made no other query: the frozen loaded map, closed afterwards."""
    c = lc.loaded(mapping=False)
    try:
        return call(c)
    finally:
        c.close()


def _same(a, b):
    """Bit for bit: arrays by their bytes, dicts and tuples member by member."""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return a == b


def _clearance_equals(out, summ, g, want):
    ref = cr.clearance(g, 0, **NAV)
    cr.boundary_free(ref["dist2"], NAV)
    assert set(out) == set(want)
    for k in want:
        assert out[k].dtype == ref[k].dtype and out[k].tobytes() == ref[k].tobytes(), k
    if "dist2" in want and "cost" in want:
        assert summ == cr.summary(g, 0, out["dist2"], out["cost"])


def test_clearance_planes_grow_and_hand_over():
    """The optional planes come into being one by one and are dropped when the grid regrows: 8 x 8 dist2 only,
    40 x 24 all three, 8 x 8 cost only, 41 x 24 nearest only (regrows, no cost plane: vg_navfn(cost=NULL) of that
    shape is VG_E_STATE), 41 x 24 cost, then vg_navfn(cost=NULL) equals nav_ref on that plane."""
    C = _tiny()
    g8, g40, g41 = cr.random_grid(8, 8, 1, p_occ=0.1), cr.random_grid(40, 24, 2), cr.random_grid(41, 24, 3)
    for g, want in ((g8, ("dist2",)), (g40, ("dist2", "nearest", "cost")), (g8, ("cost",)), (g41, ("nearest",))):
        out, s = C.clearance(g, want=want, **NAV)
        _clearance_equals(out, s, g, want)
    with pytest.raises(vgpu.VgError) as ei:
        C.navfn(None, [[3, 3]], nx=41, ny=24)
    assert STATE in str(ei.value)
    out, s = C.clearance(g41, want=("cost",), **NAV)
    _clearance_equals(out, s, g41, ("cost",))
    goals = nr.passable_cells(out["cost"], TRAV, 2, 3)
    pot, _ = C.navfn(None, goals, nx=41, ny=24)
    assert pot.dtype == np.uint32 and np.array_equal(pot, nr.potential(out["cost"], TRAV, goals))
    C.close()


def _cost_plane(nx, ny, seed):
    return cr.clearance(cr.random_grid(nx, ny, seed), 0, **NAV)["cost"]


def test_navfn_planes_and_path_staging_grow():
    """8 x 8, 70 x 66 (four 64 x 64 tiles: the planes and the activity planes grow), 8 x 8 again: each field equals
    nav_ref; then vg_nav_paths of 2 x 4, 5 x 200 and 2 x 4 cells equals nav_ref's descent in cells, len, status
    and cost."""
    C = _tiny()
    for nx, ny, seed in ((8, 8, 4), (70, 66, 5), (8, 8, 4)):
        cost = _cost_plane(nx, ny, seed)
        goals = nr.passable_cells(cost, TRAV, 2, seed)
        pot, s = C.navfn(cost, goals)
        ref = nr.potential(cost, TRAV, goals)
        assert pot.dtype == np.uint32 and np.array_equal(pot, ref)
        assert {k: s[k] for k in nr.REPRODUCIBLE} == nr.summary(cost, TRAV, goals, ref)
    cost = _cost_plane(70, 66, 5)
    goals = nr.passable_cells(cost, TRAV, 2, 5)
    pot, _ = C.navfn(cost, goals)
    for n_starts, max_len in ((2, 4), (5, 200), (2, 4)):
        starts = nr.passable_cells(cost, TRAV, n_starts, 7)
        got = C.nav_paths(starts, max_len)
        want = nr.descend(cost, TRAV, pot, starts, max_len)
        for g, w, name in zip(got, want, ("cells", "len", "status", "path_cost")):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, n_starts, max_len)
    C.close()


def test_occupancy_planes_grow_and_hand_over():
    """8 x 8, 48 x 40, 8 x 8 over the small map fixture, with and without counts: each equals the first call of a
    fresh context. Then vg_clearance(grid=NULL) of another nx is VG_E_STATE, and of the right shape equals clr_ref
    on the grid vg_occupancy returned."""
    w = tog._work()
    g0 = w["geom"]
    cx, cy = g0["x0"] + 0.5 * g0["nx"] * g0["res"], g0["y0"] + 0.5 * g0["ny"] * g0["res"]
    geom = lambda nx, ny: dict(x0=cx - 0.5 * nx * g0["res"], y0=cy - 0.5 * ny * g0["res"], res=g0["res"], nx=nx, ny=ny)
    assert NAV["res"] == g0["res"]
    occ = lambda c, nx, ny, counts: c.occupancy(w["pos"], w["dirs"], counts=counts, **geom(nx, ny), **tog.BAND)
    C = lc.loaded(mapping=False)
    ref = {}
    for counts in (True, False):
        for nx, ny in ((8, 8), (48, 40), (8, 8)):
            if (nx, ny, counts) not in ref:
                ref[nx, ny, counts] = _fresh(lambda c: occ(c, nx, ny, counts))
            got = occ(C, nx, ny, counts)
            assert (got[1] is None) == (not counts) and (nx == 8 or got[2]["cells_occupied"] > 0)
            assert _same(got, ref[nx, ny, counts]), (nx, ny, counts)
    grid = got[0]
    with pytest.raises(vgpu.VgError) as ei:
        C.clearance(None, nx=9, ny=8, **NAV)
    assert STATE in str(ei.value)
    out, s = C.clearance(None, nx=8, ny=8, **NAV)
    _clearance_equals(out, s, grid, ("dist2", "nearest", "cost"))
    C.close()


def _scan():
    """(the downsampled scan K0, A's pose of that row): the cloud the scan_diff tests use."""
    import test_scan_diff_gpu as tsd
    return tsd._static()["ds"], tsd._pose31()


def test_score_buffers_grow():
    """K = 3, then K = 200 (the pose buffer passes 1,024 doubles and doubles), then K = 3; per_point on, off, on:
    scores and per-point records equal a fresh context's."""
    xyz = lc.base()["seq"].scan(lc.K0)[0]
    pose = lc.pose_of_row(lc.base()["traj"][lc.K0])
    rng = np.random.default_rng(11)
    P = np.tile(pose, (200, 1))
    P[:, 9:12] += rng.uniform(-0.2, 0.2, (200, 3))
    C = lc.loaded(mapping=False)
    ref = {K: _fresh(lambda c: c.score_poses(xyz, P[:K])) for K in (3, 200)}
    for K in (3, 200, 3):
        assert _same(C.score_poses(xyz, P[:K]), ref[K]), K
    assert ref[200]["matches"].max() > 0
    ref_pp = _fresh(lambda c: c.score_poses(xyz, pose, per_point=True))
    ref_one = _fresh(lambda c: c.score_poses(xyz, pose))
    for per_point in (True, False, True):
        got = C.score_poses(xyz, pose, per_point=per_point)
        assert _same(got, ref_pp if per_point else ref_one), per_point
    C.close()


def test_ray_staging_shared_by_three_calls():
    """vg_scan_diff, vg_raycast of as many rays, vg_scan_info, vg_scan_diff on one context: they use one staging
    for different things. The first and last results are identical and each equals a fresh context's."""
    ds, pose = _scan()
    w = tog._work()
    n = ds.shape[0]
    O, D = np.resize(w["O"], (n, 3)), np.resize(w["Dd"], (n, 3))
    diff = lambda c: c.scan_diff(ds, pose, per_point=True)
    C = lc.loaded(mapping=False)
    first = diff(C)
    hits = C.raycast(O, D)
    info = C.scan_info(ds, pose)
    last = diff(C)
    C.close()
    assert first[0]["n"][vgpu.DIFF_CONSISTENT] > 0 and _same(first, last)
    assert _same(first, _fresh(diff))
    assert _same(hits, _fresh(lambda c: c.raycast(O, D)))
    assert _same(info, _fresh(lambda c: c.scan_info(ds, pose)))


def test_lifecycle_three_rounds():
    """A context that has used every query above, a place index and a change layer is destroyed and created again
    three times: every call succeeds and the last round's results equal the first's."""
    ds, pose = _scan()
    w = tog._work()
    xyz = lc.base()["seq"].scan(lc.K0)[0]
    g = cr.random_grid(40, 24, 2)
    lattice = vgpu.place_lattice((-18.0, -8.0), (18.0, 8.0), 3.0, 1.5)
    R = pose[:9].reshape(3, 3)

    def round_():
        c = lc.loaded(mapping=False)
        out = [c.score_poses(xyz, pose, per_point=True), c.scan_diff(ds, pose, per_point=True),
               c.raycast(w["O"], w["Dd"]), c.scan_info(ds, pose), c.localizability(w["pos"], w["dirs"]),
               c.occupancy(w["pos"], w["dirs"], counts=True, **w["geom"], **tog.BAND)]
        clr = c.clearance(None, nx=w["geom"]["nx"], ny=w["geom"]["ny"], **NAV)
        goals = nr.passable_cells(clr[0]["cost"], TRAV, 2, 2)
        nav = c.navfn(None, goals, nx=w["geom"]["nx"], ny=w["geom"]["ny"])
        out += [clr, nav[0], {k: nav[1][k] for k in nr.REPRODUCIBLE}, c.nav_paths(goals, 16), c.clearance(g, **NAV)]
        c.places_build(lattice)
        out.append(c.places_query(xyz, R, top_k=4, scores=True))
        c.places_end()
        c.change_begin()
        out.append(c.change_accumulate(ds, pose, per_point=True))
        out.append(c.change_report(flags=1))
        c.change_end()
        c.close()
        return out

    rounds = [round_() for _ in range(3)]
    assert _same(rounds[0], rounds[2]) and _same(rounds[0], rounds[1])
