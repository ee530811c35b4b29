"""The live obstacle layer (vg_live_*) on the GPU against tests/live_ref.py, on the
localisation tests' map (loc_common: the 16-line sequence 3 after scan 30,
frozen): a 64 x 64 grid of 0.25 m cells round the sensor of scan 31, obstacles as
synthetic panels cast the way test_change_gpu casts its scenes. The tests share
one context of their own (C): vg_live_compose replaces the grid a context holds,
and the other query tests' shared context keeps its own."""
import copy
import ctypes

import numpy as np
import pytest

import live_ref as lr
import loc_common as lc
import raycast_ref as rr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
RES, N = 0.25, 64
NSCAN = 4
PRM = dict(z_lo=-0.5, z_hi=0.5, r_min=0.5, mark_max=8.0, clear_max=10.0)   # nav2-like ranges: marks to 8 m, clears to 10 m
# vg_scan_diff casts a point's ray to just behind the point: a thing that stands in free space, metres from any
# mapped surface, is UNKNOWN, not APPEARED, and marks with params flags bit 0 (mark_max keeps far UNKNOWN points out)
FREE_SPACE = dict(flags=1)
NAV = dict(res=RES, inscribed_radius=0.3, inflation_radius=0.8, cost_scaling=3.0)

_cache = {}


def _pose(i):
    return lc.pose_of_row(lc.base()["traj"][lc.K0 + i])


def _origin(i):
    pose = _pose(i)
    return pose[:9].reshape(3, 3) @ lc.ext()[1] + pose[9:]


def _work():
    """{C: a frozen loaded context of this module's own, geom, base: vg_occupancy's grid in geom, scans: the four
    downsampled clouds of scans 31..34 with their poses and vg_scan_diff's results}."""
    if not _cache:
        C = lc.loaded(mapping=False)
        s = lc.base()["seq"]
        o = _origin(0)
        # (the sensor of scan 31 stands inside its cell, not on a lattice line, where every beam's a would be a matter
        # of the last bit)
        geom = dict(x0=float(o[0] - 0.5 * N * RES - 0.11), y0=float(o[1] - 0.5 * N * RES - 0.07), res=RES, nx=N, ny=N)
        g = lc.gt_traj(s, 5, 31)
        rows = g[np.linspace(0, g.shape[0] - 1, 4).astype(int)]
        pos = np.array([row[10:13] + row[1:10].reshape(3, 3) @ lc.ext()[1] for row in rows])
        _, dirs = rr.fan(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), np.zeros(3), n_az=64, n_el=4, el_deg=15.0)
        base, _, _ = C.occupancy(pos, dirs, **geom, z_lo=-0.3, z_hi=1.0)
        scans = []
        for i in range(NSCAN):
            xyz, inten = s.scan(lc.K0 + i)[:2]
            ds = np.ascontiguousarray(C.downsample(xyz, inten, 0.1)[:, :3])
            summ, pp = C.scan_diff(ds, _pose(i), per_point=True)
            scans.append((ds, _pose(i), summ, pp))
        _cache.update(C=C, geom=geom, base=base, scans=scans)
    return _cache


def _layer(C, base, **kw):
    """Begin a layer on C whatever an earlier, failed test left behind."""
    try:
        C.live_end()
    except vgpu.VgError:
        pass
    prm = dict(PRM)
    prm.update(kw)
    C.live_begin(base, **_work()["geom"], **prm)


def _rec(flags, a=(0, 0), b=(0, 0), m=(0, 0)):
    return (2, flags, a[0], a[1], b[0], b[1], m[0], m[1])


def _blob(C):
    hit, clear, _ = C.live_info()
    return hit.tobytes() + clear.tobytes()


def _panel_scene(c, ha, hb):
    """The sequence's scene with one more panel, normal x, centred on c, half-sizes ha (along y) and hb (along z)."""
    s = lc.base()["seq"]
    scene = copy.copy(s.scene)
    scene.panels = list(scene.panels)
    n, a = np.array([1.0, 0.0, 0.0]), np.array([0.0, -1.0, 0.0])
    scene.panels.append((np.asarray(c, dtype=np.float64), n, a, np.cross(n, a), ha, hb))
    return scene


def _cast(scene, i):
    """Scan K0 + i's beams (noiseless) through `scene` from the mapping run's pose: (ranges, surface ids)."""
    s = lc.base()["seq"]
    pose = _pose(i)
    R, p = pose[:9].reshape(3, 3), pose[9:]
    ext_R, ext_t = lc.ext()
    return scene.cast(R @ ext_t + p, s.dirs @ (R @ ext_R).T)


def _panel_clouds(c, ha, hb, poses=(0, 3)):
    """Per pose: (the rays that hit the panel as a cloud, the same rays' cloud in the scene without it, pose)."""
    s = lc.base()["seq"]
    scene = _panel_scene(c, ha, hb)
    out = []
    for i in poses:
        r1, sid = _cast(scene, i)
        r0, _ = _cast(s.scene, i)
        new = np.isfinite(r1) & (r1 >= s.blind) & (sid == 6 + len(scene.panels) - 1) & np.isfinite(r0)
        # (without the panel: those of its rays that end beyond mark_max, so that the clearing scan itself marks nothing
        # whatever class the static scene's points get)
        far = new & (r0 > PRM["mark_max"])
        out.append(((s.dirs[new] * r1[new, None]).astype(np.float32), (s.dirs[far] * r0[far, None]).astype(np.float32),
                    _pose(i)))
    return out


def _panel_at(dx, dy, dz):
    """A panel centre dx, dy, dz from scan 31's sensor, its x moved to the middle of a cell."""
    g, o = _work()["geom"], _origin(0)
    x = g["x0"] + (np.floor((o[0] + dx - g["x0"]) / RES) + 0.5) * RES
    return np.array([x, o[1] + dy, o[2] + dz])


def _slab_cells(c, ha):
    """The cells within one cell of the panel's slab (bool [ny, nx])."""
    g = _work()["geom"]
    cx = (g["x0"] + (np.arange(N) + 0.5) * RES)[None, :]
    cy = (g["y0"] + (np.arange(N) + 0.5) * RES)[:, None]
    return (np.abs(cx - c[0]) <= 1.5 * RES) & (np.abs(cy - c[1]) <= ha + 1.5 * RES)


# ---- 2: the rasteriser alone

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_walk_wave_and_workgroup_edges(n):
    """vgx_live_walk on n random records equals live_ref.planes byte for byte, on 64 x 64."""
    w = _work()
    C = w["C"]
    _layer(C, w["base"])
    rng = np.random.default_rng(100 + n)
    recs = np.zeros(n, dtype=vgpu.LIVE_POINT_DTYPE)
    recs["flags"] = rng.integers(0, 4, n)                  # marks, clears, both, neither
    for f in ("ax", "ay", "bx", "by", "mx", "my"):
        recs[f] = rng.integers(-20, N + 20, n)
    recs["cls"] = 2
    C.live_walk(recs, 3)
    hit, clear, _ = C.live_info()
    rh, rc, _ = lr.planes(recs, 3, N, N)
    assert hit.tobytes() == rh.tobytes() and clear.tobytes() == rc.tobytes()
    assert n < 63 or (rh.any() and rc.any())
    C.live_end()


@pytest.mark.parametrize("nx,ny", [(1, 1), (5, 3), (64, 64)])
def test_walk_grids_and_edge_beams(nx, ny):
    """Origin outside the grid, beams that cross the whole grid from outside, a == b, the longest beam, marks on the
    rim and outside, an over-long beam of a given record; two stamps in both orders: the bytes of live_ref.planes.
    "Beams that leave the grid and re-enter it" do not exist: both coordinates of a beam's cells are monotonic in k,
    so a beam that has left a rectangle on one axis never comes back, which is what lets k_live_walk end a beam past
    the grid's far side. What can happen is covered: beams that start outside, enter and leave again (the first three
    rows and the anti-diagonal), on every side, and beams whose first 4,000 cells lie outside."""
    C = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    C.set_mapping(False)
    try:
        C.live_begin(np.zeros((ny, nx), dtype=np.int8), x0=0.0, y0=0.0, res=RES, nx=nx, ny=ny)
        both = lr.MARKS | lr.CLEARS
        rows = [_rec(lr.CLEARS, a=(-9, -4), b=(nx + 7, ny + 3)), _rec(lr.CLEARS, a=(nx + 5, ny // 2), b=(-6, ny // 2)),
                _rec(lr.CLEARS, a=(nx // 2, -7), b=(nx // 2, ny + 7)), _rec(both, a=(0, 0), b=(0, 0), m=(0, 0)),
                _rec(both, a=(nx - 1, ny - 1), b=(0, 0), m=(nx - 1, ny - 1)), _rec(lr.MARKS, m=(nx, 0)),
                _rec(lr.MARKS, m=(-1, ny - 1)), _rec(lr.CLEARS, a=(-3, ny + 2), b=(nx + 2, -3)),
                _rec(lr.CLEARS, a=(0, 0), b=(4097, 1)), _rec(lr.CLEARS, a=(-4000, 0), b=(97, ny - 1)),
                _rec(lr.CLEARS, a=(0, 0), b=(5000, 0)), _rec(lr.CLEARS, a=(-(1 << 30), 0), b=(1 << 30, 0)),
                _rec(0, a=(0, 0), b=(nx, ny), m=(0, 0))]
        recs = np.array(rows, dtype=vgpu.LIVE_POINT_DTYPE)
        first, second = recs[: len(rows) // 2], recs[len(rows) // 2:]
        blobs = []
        for order in (((first, 7), (second, 4)), ((second, 4), (first, 7))):
            C.live_clear()
            h = c = None
            for part, stamp in order:
                C.live_walk(part, stamp)
                h, c, _ = lr.planes(part, stamp, nx, ny, h, c)
            hit, clear, tot = C.live_info()
            assert hit.tobytes() == h.tobytes() and clear.tobytes() == c.tobytes()
            assert tot["stamp"] == 7
            blobs.append(hit.tobytes() + clear.tobytes())
        assert blobs[0] == blobs[1]
        assert h.max() == 7 and c.max() == 7
    finally:
        C.close()


def test_walk_two_thousand_beams_through_one_cell():
    """The read-before-atomic path: 2,000 beams leave one origin cell round the compass, twice at one stamp and
    once at an older one; the planes are live_ref's."""
    w = _work()
    C = w["C"]
    _layer(C, w["base"])
    ang = np.linspace(0.0, 2.0 * np.pi, 2000, endpoint=False)
    recs = np.zeros(2000, dtype=vgpu.LIVE_POINT_DTYPE)
    recs["cls"], recs["flags"] = 2, lr.MARKS | lr.CLEARS
    recs["ax"], recs["ay"] = 31, 33
    recs["bx"] = recs["mx"] = 31 + np.round(29 * np.cos(ang)).astype(np.int32)
    recs["by"] = recs["my"] = 33 + np.round(29 * np.sin(ang)).astype(np.int32)
    h, c, _ = lr.planes(recs, 9, N, N)
    for stamp in (9, 9, 2):
        C.live_walk(recs, stamp)
        hit, clear, _ = C.live_info()
        assert hit.tobytes() == h.tobytes() and clear.tobytes() == c.tobytes()
    assert c[33, 31] == 9 and (c == 9).sum() > 2000 and (h == 9).sum() > 100
    C.live_end()


# ---- 3, 4: the records

def test_same_bits_as_scan_diff():
    """3: per_point.cls and the class counts of vg_live_mark are vg_scan_diff's for the same input."""
    w = _work()
    C = w["C"]
    _layer(C, w["base"])
    for ds, pose, summ, pp in w["scans"]:
        assert pp.shape[0] > 1000
        s, rec = C.live_mark(ds, pose, per_point=True)
        assert np.array_equal(rec["cls"], pp["cls"]) and s["n"] == summ["n"]
        assert C.live_mark(ds, pose, stamp=s["stamp"])["n"] == summ["n"]      # without the per-point records
    C.live_end()


def test_records_against_numpy():
    """4: cells and flags equal live_ref.points (double, from the device's classes) outside the uncertain set,
    which holds at most 0.5 % of the points; hit / clear equal live_ref.planes over the device's records byte for
    byte; the summary's counts are the records'; the workload marks and clears something."""
    w = _work()
    C, g = w["C"], w["geom"]
    ext_R, ext_t = lc.ext()
    _layer(C, w["base"], flags=1)       # UNKNOWN marks too: the static scene has few APPEARED points
    h = c = None
    n_unc = n_pts = n_obs = n_beams = 0
    for k, (ds, pose, _, pp) in enumerate(w["scans"]):
        s, rec = C.live_mark(ds, pose, per_point=True)
        assert s["stamp"] == k + 1
        ref, unc = lr.points(ds, pose, ext_R, ext_t, rec["cls"], g["x0"], g["y0"], RES, flags=1, **PRM)
        ok = ~unc
        for f in vgpu.LIVE_POINT_DTYPE.names:
            bad = np.flatnonzero(ok & (rec[f] != ref[f]))
            assert bad.size == 0, (f, bad[:8], rec[bad[:8]], ref[bad[:8]])
        h0, c0 = (np.zeros((N, N), dtype=np.int32),) * 2 if h is None else (h, c)
        h, c, cnt = lr.planes(rec, k + 1, N, N, h, c)
        assert (s["n_obstacle"], s["marks_dropped"], s["n_beams"]) == cnt
        assert s["cells_live"] == ((h == k + 1) & (h0 != k + 1)).sum()
        assert s["cells_cleared"] == ((c == k + 1) & (c0 != k + 1)).sum()
        n_unc, n_pts, n_obs, n_beams = n_unc + int(unc.sum()), n_pts + ds.shape[0], n_obs + cnt[0], n_beams + cnt[2]
    hit, clear, tot = C.live_info()
    print("points %d, uncertain %d, obstacle points %d, beams %d, cells hit %d, cells cleared %d"
          % (n_pts, n_unc, n_obs, n_beams, (hit > 0).sum(), (clear > 0).sum()))
    assert n_unc <= 0.005 * n_pts
    assert hit.tobytes() == h.tobytes() and clear.tobytes() == c.tobytes()
    assert tot["calls"] == NSCAN and tot["stamp"] == NSCAN and tot["n_beams"] == n_beams == n_pts
    assert n_obs >= 20 and (hit > 0).sum() >= 5 and (clear > 0).sum() >= 500
    C.live_end()


# ---- 5: order independence

def test_order_independence():
    """Scans forwards and backwards with explicit stamps, point-reversed clouds, the device-array entry, a fleet's
    way of sharing obstacles (two trackers attached to C, each localised elsewhere, whose scans are marked with their
    poses into C's one layer, alternating with C's own), and a layer begun on an attached tracker and marked by pose:
    identical plane bytes."""
    import torch
    w = _work()
    C = w["C"]
    scans = [(ds, pose) for ds, pose, _, _ in w["scans"]]
    _layer(C, w["base"], flags=1)

    def run(fn, ctx=C):
        ctx.live_clear()
        fn(ctx)
        return _blob(ctx)

    def forwards(ctx):
        for k, (ds, pose) in enumerate(scans):
            ctx.live_mark(ds, pose, stamp=k + 1)

    def auto_stamps(ctx):
        for ds, pose in scans:
            ctx.live_mark(ds, pose)

    def backwards(ctx):
        for k, (ds, pose) in list(enumerate(scans))[::-1]:
            ctx.live_mark(ds, pose, stamp=k + 1)

    def reversed_points(ctx):
        for k, (ds, pose) in enumerate(scans):
            ctx.live_mark(ds[::-1], pose, stamp=k + 1)

    def device_arrays(ctx):
        for k, (ds, pose) in enumerate(scans):
            t = torch.from_numpy(np.ascontiguousarray(ds.T)).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            s = ctx.live_mark_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), ds.shape[0], pose, stamp=k + 1)
            assert s["n"] == w["scans"][k][2]["n"]

    ref = run(forwards)
    assert len(set(ref)) > 2
    for fn in (auto_stamps, backwards, reversed_points, device_arrays):
        assert run(fn) == ref, fn.__name__
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    T2 = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    try:
        T.attach(C)
        T2.attach(C)

        def trackers_into_one_layer(ctx):
            # (the layer is C's: a tracker's scan reaches it with the tracker's pose, through C; the trackers' own
            # states are not read)
            for k, (ds, pose) in enumerate(scans):
                assert (T, T2)[k % 2].scan_diff(ds, pose)["n"] == w["scans"][k][2]["n"]   # the tracker sees that scan
                ctx.live_mark(ds, pose, stamp=k + 1)

        assert run(trackers_into_one_layer) == ref
        T2.close()
        T.live_begin(w["base"], **w["geom"], **dict(PRM, flags=1))
        assert run(backwards, T) == ref
        T.live_end()
    finally:
        T2.close()
        T.close()
    C.live_end()


# ---- 6: a panel appears and goes

def test_panel_appears_and_goes():
    """A panel 4.3 m ahead in free space, in band, marked from two poses: occupied within one cell of its slab, the
    base elsewhere; the same beams without the panel at later stamps clear it: the base bytes again."""
    w = _work()
    C, base = w["C"], w["base"]
    c, ha = _panel_at(4.3, 1.0, 0.0), 0.6
    clouds = _panel_clouds(c, ha, 0.4)
    slab = _slab_cells(c, ha)
    _layer(C, base, **FREE_SPACE)
    n_obs = 0
    for with_panel, _, pose in clouds:
        assert with_panel.shape[0] > 50
        n_obs += C.live_mark(with_panel, pose)["n_obstacle"]
    grid, s = C.live_compose()
    raised = grid != base
    print("panel: %d obstacle points, %d cells raised, %d slab cells, base occupied in the slab %d"
          % (n_obs, raised.sum(), slab.sum(), (base[slab] == 100).sum()))
    assert n_obs > 50 and raised.sum() >= 4 and s["cells_raised"] == raised.sum()
    assert not (raised & ~slab).any() and np.all(grid[raised] == 100)
    hit, _, _ = C.live_info()
    assert s["cells_live"] == (hit > 0).sum() and not ((hit > 0) & ~slab).any()
    assert C.live_compose()[0].tobytes() == grid.tobytes()          # a second compose does not compound
    for _, without, pose in clouds:
        assert without.shape[0] > 50 and C.live_mark(without, pose)["n_obstacle"] == 0
    grid2, s2 = C.live_compose()
    assert grid2.tobytes() == base.tobytes() and s2["cells_live"] == 0 and s2["cells_raised"] == 0
    C.live_end()


def test_panel_expires():
    """With persist = 3 the panel marked at stamp 5 is there at now = 5, 6, 7 and gone at now = 8, with no
    clearing scan at all."""
    w = _work()
    C, base = w["C"], w["base"]
    clouds = _panel_clouds(_panel_at(4.3, 1.0, 0.0), 0.6, 0.4)
    _layer(C, base, persist=3, **FREE_SPACE)
    for with_panel, _, pose in clouds:
        C.live_mark(with_panel, pose, stamp=5)
    hit, clear, _ = C.live_info()
    want = C.live_compose(5)[0]
    assert (want != base).sum() >= 4 and want.tobytes() == lr.compose(base, hit, clear, 5, 3).tobytes()
    for now in (6, 7):
        assert C.live_compose(now)[0].tobytes() == want.tobytes()
    grid, s = C.live_compose(8)
    assert grid.tobytes() == base.tobytes() and s["cells_live"] == 0 and s["stamp"] == 8
    assert C.live_compose()[0].tobytes() == want.tobytes()           # now = 0: the largest stamp, 5
    C.live_end()


def test_band():
    """A panel entirely above z_hi never marks, and its beams, which rise out of the band on the way, do not clear
    the marked cells of a low panel beneath them."""
    w = _work()
    C, base = w["C"], w["base"]
    low, high = _panel_at(4.3, 1.0, 0.0), _panel_at(6.3, 1.0, 1.0)
    _layer(C, base, z_lo=-0.3, z_hi=0.3, **FREE_SPACE)
    for with_panel, _, pose in _panel_clouds(low, 0.6, 0.2):
        C.live_mark(with_panel, pose, stamp=1)
    want, s = C.live_compose()
    assert s["cells_raised"] >= 4
    n_beams = 0
    for with_panel, _, pose in _panel_clouds(high, 0.6, 0.2):
        s, rec = C.live_mark(with_panel, pose, stamp=2, per_point=True)
        assert with_panel.shape[0] > 20 and s["n_obstacle"] == 0 and s["n_beams"] == with_panel.shape[0]
        assert np.all((rec["flags"] & lr.LEFT_BAND) != 0) and not np.any(rec["flags"] & (lr.MARKS | lr.IN_BAND))
        n_beams += s["n_beams"]
    got, s = C.live_compose()
    hit, clear, _ = C.live_info()
    assert (clear == 2).sum() > 0 and got.tobytes() == want.tobytes() and hit.max() == 1
    C.live_end()


# ---- 7: the chain

def test_chain():
    """After compose vg_clearance(grid == NULL) and vg_navfn give the bytes of the same calls on the downloaded
    grid; a path that crossed the panel's cells avoids them after the mark; vg_occupancy afterwards leaves the
    layer's base intact; compose with flags bit 0 is live_ref's."""
    w = _work()
    C, g = w["C"], w["geom"]
    base = np.zeros((N, N), dtype=np.int8)        # an open floor: the path is the straight line
    base[0, :] = base[-1, :] = -1
    c, ha = _panel_at(4.3, 0.0, 0.0), 1.0
    clouds = _panel_clouds(c, ha, 0.4)
    _layer(C, base, **FREE_SPACE)
    iy = int((_origin(0)[1] - g["y0"]) / RES)
    start, goal = np.array([[2, iy]]), np.array([[N - 3, iy]])

    def plan(grid):
        clr, _ = C.clearance(grid, nx=N, ny=N, **NAV)
        pot, _ = C.navfn(None, goal, nx=N, ny=N)
        cells, ln, status, _ = C.nav_paths(start, 4 * N)
        assert status[0] == vgpu.NAV_REACHED
        return clr, pot, cells[0, : ln[0]]

    grid0, _ = C.live_compose()
    assert grid0.tobytes() == base.tobytes()
    _, _, path0 = plan(None)
    for with_panel, _, pose in clouds:
        C.live_mark(with_panel, pose)
    grid, s = C.live_compose()
    occupied = np.flatnonzero(grid.reshape(-1) == 100)
    assert s["cells_raised"] == occupied.size >= 6 and np.intersect1d(path0, occupied).size > 0
    clr_d, pot_d, path = plan(None)                 # from the device's composed grid
    clr_h, pot_h, path_h = plan(grid)               # from the downloaded one
    for k in clr_d:
        assert clr_d[k].tobytes() == clr_h[k].tobytes(), k
    assert pot_d.tobytes() == pot_h.tobytes() and np.array_equal(path, path_h)
    assert np.intersect1d(path, occupied).size == 0
    C.live_compose(want_grid=False)                 # stays on the device only
    assert C.clearance(None, nx=N, ny=N, **NAV)[0]["cost"].tobytes() == clr_h["cost"].tobytes()
    # a later vg_occupancy replaces the held grid, not the base
    C.occupancy(np.zeros((0, 3)), **g)
    assert C.live_compose()[0].tobytes() == grid.tobytes()
    # flags bit 0: base-unknown cells a beam crossed become free
    hit, clear, _ = C.live_info()
    unk = np.full((N, N), -1, dtype=np.int8)
    C.live_end()
    C.live_begin(unk, **g, **PRM, **FREE_SPACE)
    for with_panel, _, pose in clouds:
        C.live_mark(with_panel, pose)
    h2, c2, _ = C.live_info()
    assert h2.tobytes() == hit.tobytes() and c2.tobytes() == clear.tobytes()
    g1, s1 = C.live_compose(flags=1)
    assert g1.tobytes() == lr.compose(unk, hit, clear, 2, 0, 1).tobytes()
    assert s1["cells_free"] == (g1 == 0).sum() == s1["cells_cleared"] > 10 and s1["cells_occupied"] == (g1 == 100).sum()
    assert s1["cells_free"] + s1["cells_occupied"] + s1["cells_unknown"] == N * N
    assert C.live_compose()[0].tobytes() == lr.compose(unk, hit, clear, 2).tobytes()
    C.live_end()


# ---- 8: read-only and lifecycle

def test_map_is_read_only():
    """A context that had a layer, marked into it and composed has the map, the state and a frozen step of scan 31
    of a context that never had one, bit for bit."""
    w = _work()
    s = lc.base()["seq"]
    A, R = lc.loaded(mapping=False), lc.loaded(mapping=False)
    A.live_begin(w["base"], **w["geom"], **PRM)
    for ds, pose, _, _ in w["scans"]:
        A.live_mark(ds, pose)
    A.live_compose()
    lc.same_map(A, lc.roots(R), lc.planes(R))
    assert A.state().tobytes() == R.state().tobytes()
    A.live_mark(w["scans"][0][0])          # pose None: the context's state
    lc.step(A, s, lc.K0)                   # a frozen step with the layer in place
    lc.step(R, s, lc.K0)
    assert A.state().tobytes() == R.state().tobytes() and A.trajectory().tobytes() == R.trajectory().tobytes()
    lc.same_map(A, lc.roots(R), lc.planes(R))
    A.close()                              # vg_destroy with a live layer
    R.close()


def _code(fn):
    with pytest.raises(vgpu.VgError) as ei:
        fn()
    return int(str(ei.value).split("(")[1].split(")")[0])


def test_errors_write_nothing():
    """Every VG_E_ARG / VG_E_STATE case of the header, and the layer's bytes after them."""
    w = _work()
    g, base = w["geom"], w["base"]
    ds, pose = w["scans"][0][:2]
    L = vgpu.lib()
    C = lc.loaded(mapping=False)
    for fn in (lambda: C.live_mark(ds, pose), C.live_clear, C.live_end, lambda: C.live_walk(np.zeros(1, lr.REC), 1),
               C.live_compose, C.live_info, C.live_ms):
        assert _code(fn) == -5                                   # no layer
    assert L.vg_live_compose(C.h, 0, 0, None, None) == -5 and L.vg_live_info(C.h, None, None, None) == -5
    assert _code(lambda: C.live_begin(None, **g)) == -5          # no held grid
    C.occupancy(np.zeros((0, 3)), x0=0.0, y0=0.0, res=RES, nx=8, ny=8)
    assert _code(lambda: C.live_begin(None, **g)) == -5          # a held grid of another shape
    bad = [dict(res=0.0), dict(res=np.nan), dict(x0=np.inf), dict(nx=0), dict(ny=vgpu.CLR_MAX_SIDE + 1),
           dict(nx=8192, ny=8192), dict(z_lo=0.2, z_hi=1.0), dict(z_lo=-1.0, z_hi=-0.2), dict(z_lo=0.0, z_hi=np.nan),
           dict(clear_max=4096.5 * RES), dict(flags=2)]
    for kw in bad:
        assert _code(lambda: C.live_begin(None, **dict(g, **kw))) == -1, kw
    assert _code(C.live_end) == -5                               # none of them created a layer
    C.live_begin(base, **g, **PRM)
    assert _code(lambda: C.live_begin(base, **g)) == -5          # a layer already
    C.live_mark(ds, pose)
    snap, tot = _blob(C), C.live_info()[2]
    summ, rec = vgpu.LiveSummary(), np.full(4, 77, dtype=vgpu.LIVE_POINT_DTYPE)
    before = (bytes(summ), rec.tobytes())
    assert L.vg_live_mark(C.h, None, 5, None, 0, rec.ctypes.data, summ) == -1                        # NULL xyz, n > 0
    assert L.vg_live_mark(C.h, vgpu._f(ds), -1, None, 0, rec.ctypes.data, summ) == -1                # n < 0
    assert L.vg_live_mark(C.h, vgpu._f(ds), lc.CAP["max_points"] + 1, None, 0, None, summ) == -1    # n too large
    assert L.vg_live_mark(C.h, vgpu._f(ds), 4, None, -3, rec.ctypes.data, summ) == -1                # stamp < 0
    assert L.vg_live_mark_dev(C.h, None, None, None, 5, None, 0, summ) == -1
    assert L.vg_live_compose(C.h, -1, 0, None, summ) == -1 and L.vg_live_compose(C.h, 0, 2, None, summ) == -1
    assert L.vg_live_begin(C.h, None, None) == -1 and L.vg_live_mark(None, None, 0, None, 0, None, None) == -1
    assert (bytes(summ), rec.tobytes()) == before
    assert _blob(C) == snap and C.live_info()[2] == tot          # no stamp taken, nothing counted
    e = C.live_mark(np.zeros((0, 3), dtype=np.float32), pose)    # n == 0 takes its stamp
    assert e["stamp"] == 2 and e["n"] == [0, 0, 0, 0] and _blob(C) == snap and C.live_info()[2]["calls"] == 2
    assert C.live_mark(ds, pose, stamp=2 ** 31 - 1)["stamp"] == 2 ** 31 - 1
    assert _code(lambda: C.live_mark(ds, pose)) == -4            # no stamp after INT32_MAX
    # vg_live_clear restarts the stamps and keeps the base
    C.live_clear()
    hit, clear, tot = C.live_info()
    assert not hit.any() and not clear.any() and all(v in (0, [0, 0, 0, 0]) for v in tot.values())
    assert C.live_mark(ds, pose)["stamp"] == 1 and _blob(C) == snap
    assert C.live_compose()[0].tobytes() == lr.compose(base, *C.live_info()[:2], 1).tobytes()
    # vg_reset frees the layer; a sharded context has none
    C.set_mapping(True)
    C.reset()
    assert _code(C.live_end) == -5
    C.close()
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    assert _code(lambda: S.live_begin(base, **g)) == -5
    S.close()


def test_destroy_with_a_layer_three_rounds():
    """A context with a live layer is destroyed and created again three times: every call succeeds and the last
    round's planes and grid equal the first's. This does not detect a leak: the tree has no allocation hook, and the
    device's free memory is shared with other processes, so it cannot be asserted. That vg_destroy frees the layer
    is by construction: it calls vg_live_end, which deletes the LiveLayer, whose buffers are DevBuf members."""
    w = _work()

    def round_():
        c = lc.loaded(mapping=False)
        c.live_begin(w["base"], **w["geom"], **PRM)
        for ds, pose, _, _ in w["scans"][:2]:
            c.live_mark(ds, pose)
        out = _blob(c) + c.live_compose()[0].tobytes()
        c.close()
        assert not c.h
        return out

    rounds = [round_() for _ in range(3)]
    assert rounds[0] == rounds[1] == rounds[2]


# ---- 9: the replay tool

def test_replay_live(tmp_path):
    """vg_node_replay --map ... --localize --occupancy P --costmap C --live --live-persist N (NodeCore::live_begin,
    LioCore::live_mark, NodeCore::live_costmap) writes C.live.grid.pgm and C.live.pgm: the composed grid and its cost
    equal the Python calls on the same scans (the tool's --live-scans dump) over read_occupancy(P)'s grid; without
    --costmap it is refused."""
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

    ck, dump = tmp_path / "map.vgck", tmp_path / "scans.bin"
    run([log, tmp_path / "a.tum", 0, tmp_path / "a.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    pre, cpre = str(tmp_path / "nav"), str(tmp_path / "cost")
    nav = dict(res=0.1, inscribed_radius=0.3, inflation_radius=0.8, cost_scaling=3.0)
    loc = [log, tmp_path / "b.tum", "--map", ck, "--localize", "--guess", guess]
    run(loc + ["--occupancy", pre, "--live"], rc=2)                  # only with --costmap
    run(loc + ["--occupancy", pre, "--costmap", cpre, "--live-persist", 3], rc=2)
    persist = 2
    lines = run(loc + ["--occupancy", pre, "--occ-res", nav["res"], "--costmap", cpre, "--inscribed", nav["inscribed_radius"],
                       "--inflation", nav["inflation_radius"], "--cost-scaling", nav["cost_scaling"], "--live",
                       "--live-persist", persist, "--live-scans", dump])
    said = [ln.split() for ln in lines if ln.startswith("live: ")]
    assert len(said) == 1
    raw = dump.read_bytes()
    scans, at = [], 0
    while at < len(raw):
        n = int(np.frombuffer(raw, dtype="<i4", count=1, offset=at)[0])
        pose = np.frombuffer(raw, dtype="<f8", count=12, offset=at + 4).copy()
        scans.append((np.frombuffer(raw, dtype="<f4", count=3 * n, offset=at + 100).reshape(n, 3).copy(), pose))
        at += 100 + 12 * n
    assert len(scans) == int(said[0][1]) >= 3
    base, x0, y0, res = vgpu.read_occupancy(pre)
    got, gx0, gy0, gres = vgpu.read_occupancy(cpre + ".live.grid")
    cost, cx0, cy0, cres = vgpu.read_costmap(cpre + ".live")
    assert (gx0, gy0, gres) == (cx0, cy0, cres) == (x0, y0, res) and got.shape == cost.shape == base.shape
    C = vgpu.Context(cfg, max_points=400_000)
    C.checkpoint_load(str(ck))
    C.set_mapping(False)
    ny, nx = base.shape
    C.live_begin(base, x0=x0, y0=y0, res=res, nx=nx, ny=ny, persist=persist, **PRM, **FREE_SPACE)
    for xyz, pose in scans:
        C.live_mark(xyz, pose)
    want, s = C.live_compose()
    hit, clear, tot = C.live_info()
    print("replay live: %d scans, %d x %d, %d cells live, %d raised; hit at the last %d stamps only: %s"
          % (len(scans), nx, ny, s["cells_live"], s["cells_raised"], persist, (hit[want != base] > len(scans) - persist).all()))
    assert tot["stamp"] == len(scans) and tot["n_beams"] > 1000 and (clear > 0).sum() > 100
    assert got.tobytes() == want.tobytes() == lr.compose(base, hit, clear, len(scans), persist).tobytes()
    assert int(said[0][3]) == s["cells_live"] and int(said[0][6]) == s["cells_raised"]
    want_cost = C.clearance(None, nx=nx, ny=ny, want=("cost",), **nav)[0]["cost"]
    assert cost.tobytes() == want_cost.tobytes()
    C.close()
