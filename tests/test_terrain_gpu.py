"""vg_terrain (vina_gpu.h "Terrain layer") against the numpy restatement of its
definition (tests/terrain_ref.py) on the occupancy tests' map (loc_common: the
16-line sequence 3 after scan 30, frozen) with directions steep enough to reach
the floor: the ground planes, the per-cell stage, the marks over the device's own
elevation, the classification, the whole definition over brute-force hits, what
the origin band gets wrong, order and batch independence, the chaining into
vg_clearance, the per-cell stage on crafted planes, the edges and the errors."""
import ctypes
import math

import numpy as np
import pytest

import loc_common as lc
import occ_ref as oc
import raycast_ref as rr
import terrain_ref as tr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
RES, N = 0.25, 64
EL_DEG = (-24.0, -18.0, -12.0, 2.0)   # the floor 3.4, 4.6 and 7 m out from 1.5 m up; one row for the walls
PRM = dict(sensor_height=1.5)         # the trajectory's mean height over the scene's floor
ENDED = vgpu.RAY_TRUNCATED | vgpu.RAY_LEFT_RANGE | vgpu.RAY_INVALID
STEP_MAX = (0.01, 0.6)     # a step of the order of the range noise, and one no floor has

_cache = {}


def _work():
    """{M: the frozen loaded context (shared, never closed), planes, pos: the occupancy test's 4 origins, dirs: 64
    azimuths (0.37 degrees off the axes) x EL_DEG, geom: 64 x 64 cells of 0.25 m centred on the origins, O / Dd: the
    1024 rays, hits: vg_raycast of them, P: terrain_ref.defaults, grid / elev / step / counts / summ: vg_terrain of
    them, ground: its four ground planes}: computed once, read-only afterwards."""
    if not _cache:
        w = rr.workload()
        M = w["M"]
        g = lc.gt_traj(lc.base()["seq"], 5, 31)
        ext_t = lc.ext()[1]
        rows = g[np.linspace(0, g.shape[0] - 1, 4).astype(int)]
        pos = np.array([row[10:13] + row[1:10].reshape(3, 3) @ ext_t for row in rows])
        az = np.deg2rad(0.37) + np.linspace(0.0, 2.0 * np.pi, 64, endpoint=False)
        E, A = np.meshgrid(np.deg2rad(EL_DEG), az, indexing="xy")
        dirs = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
        c = pos[:, :2].mean(axis=0)
        geom = dict(x0=float(c[0] - 0.5 * N * RES), y0=float(c[1] - 0.5 * N * RES), res=RES, nx=N, ny=N)
        O, Dd = np.repeat(pos, dirs.shape[0], axis=0), np.tile(dirs, (pos.shape[0], 1))
        grid, elev, step, counts, summ = M.terrain(pos, dirs, **geom, **PRM)
        ground = M.terrain_ground(N, N)
        _cache.update(M=M, planes=w["planes"], pos=pos, dirs=dirs, geom=geom, O=O, Dd=Dd, hits=M.raycast(O, Dd),
                      P=tr.defaults(**geom, **PRM), grid=grid, elev=elev, step=step, counts=counts, summ=summ,
                      ground=ground)
    return _cache


def _records(hits):
    """(r, nz, ended, occupied) of vg_raycast records."""
    f = hits["flags"]
    return (np.where((f & vgpu.RAY_HIT) != 0, hits["range"], np.inf), hits["normal"][:, 2], (f & ENDED) != 0,
            (f & vgpu.RAY_OCCUPIED) != 0)


def _ref_on_records(w, elev=None, **kw):
    r, nz, ended, _ = _records(w["hits"])
    return tr.terrain(w["O"], w["Dd"], r, nz, dict(w["P"], **kw), elev=elev, ended=ended)


def test_ground_planes():
    """1: the four ground planes equal the definition over the device's own vg_raycast records in every cell that
    no uncertain ray's hit can fall in (its cell +- 1)."""
    w = _work()
    ref = _ref_on_records(w)
    unc = ref["uncertain"]
    reach = tr.hit_reach(ref["hit_cell"], unc, N, N)
    print("ground hits %d (ref %d) of %d rays, uncertain %d, cells in their hits' reach %d, cells with ground %d"
          % (w["summ"]["n_ground_hits"], ref["ground"].sum(), unc.size, unc.sum(), reach.sum(), (w["ground"][0] > 0).sum()))
    assert ref["ground"].sum() > 100
    for name, got, want in zip(("g_n", "g_sum", "g_min", "g_max"), w["ground"], ref["planes"]):
        assert got.dtype == want.dtype and np.array_equal(got[~reach], want[~reach]), name
    assert abs(int(w["ground"][0].sum()) - int(ref["ground"].sum())) <= int(unc.sum())
    assert w["summ"]["n_ground_hits"] == int(w["ground"][0].sum()) and w["summ"]["n_out_of_range"] == 0


def test_cells_of_the_devices_planes():
    """2: elev, step and the summary's cells_ground, max_step and max_spread are a pure integer function of the
    device's own ground planes, bit for bit."""
    w = _work()
    elev, step, (n, ms, sp) = tr.cells(*w["ground"], min_ground=1)
    assert w["elev"].dtype == np.int32 and w["elev"].tobytes() == elev.tobytes() and w["step"].tobytes() == step.tobytes()
    s = w["summ"]
    print("cells with an elevation %d, max step %d mm, max spread %d mm" % (n, ms, sp))
    assert (s["cells_ground"], s["max_step"], s["max_spread"]) == (n, ms, sp) and n > 0
    g2 = w["M"].terrain(w["pos"], w["dirs"], **w["geom"], **PRM, min_ground=3)
    e3, s3, st3 = tr.cells(*w["ground"], min_ground=3)
    assert g2[1].tobytes() == e3.tobytes() and g2[2].tobytes() == s3.tobytes() and 0 < st3[0] < n
    assert (g2[4]["cells_ground"], g2[4]["max_step"], g2[4]["max_spread"]) == st3


def test_count_planes():
    """3: both count planes equal the definition over the device's records and the device's own elev outside the
    cells the uncertain rays can touch, and within the number of uncertain rays elsewhere; uncertain rays <= 2 %;
    flags bit 0 silences exactly the rays with VG_RAY_OCCUPIED."""
    w = _work()
    occupied = _records(w["hits"])[3]
    g1 = w["M"].terrain(w["pos"], w["dirs"], **w["geom"], **PRM, flags=1)
    assert g1[1].tobytes() == w["elev"].tobytes() and g1[3][1].tobytes() == w["counts"][1].tobytes()
    for silent, c, s in ((None, w["counts"], w["summ"]), (occupied, g1[3], g1[4])):
        r, nz, ended, _ = _records(w["hits"])
        ref = tr.terrain(w["O"], w["Dd"], r, nz, w["P"], elev=w["elev"], ended=ended, silent=silent)
        unc = ref["uncertain"]
        n_unc = int(unc.sum())
        print("uncertain rays: %d of %d; free marks %d (ref %d), occ marks %d (ref %d), in band %d (ref %d)"
              % (n_unc, unc.size, c[0].sum(), ref["counts"][0].sum(), c[1].sum(), ref["counts"][1].sum(),
                 s["n_hits_in_band"], ref["in_band"].sum()))
        assert n_unc <= 0.02 * unc.size
        assert ref["counts"][0].sum() > 5 * unc.size and ref["counts"][1].sum() > 10     # the workload marks something
        touch = oc.touched(w["O"], w["Dd"], unc, rr.T_MAX, **w["geom"])
        diff = np.abs(c.astype(np.int64) - ref["counts"])
        assert not diff[:, ~touch].any(), np.argwhere(diff[:, ~touch])[:8]
        assert diff.max() <= n_unc
        assert abs(s["n_hits_in_band"] - int(ref["in_band"].sum())) <= n_unc
        assert s["free_marks"] == int(c[0].sum()) and s["occ_marks"] == int(c[1].sum())
    f = w["hits"]["flags"]
    s = w["summ"]
    assert s["n_rays"] == f.size and s["n_hits"] == int(((f & vgpu.RAY_HIT) != 0).sum()) > 0
    assert s["n_truncated"] == int(((f & vgpu.RAY_TRUNCATED) != 0).sum()) and s["n_invalid"] == 0
    assert s["n_occupied_unknown"] == int(occupied.sum())


def test_grid_is_the_classification():
    """4: the grid is the classification of the device's counts and step, without flags bit 1 and with it at two
    step_max values, and with thresholds and the ratio; the summary's class counts follow."""
    w = _work()
    M, P = w["M"], w["P"]
    assert w["grid"].dtype == np.int8 and set(np.unique(w["grid"])) <= {-1, 0, 100}
    assert np.array_equal(w["grid"], tr.classify(w["counts"], w["elev"], w["step"]))
    assert w["summ"]["cells_step_lethal"] == 0
    lethal = []
    for sm in STEP_MAX:
        g, e, st, c, s = M.terrain(w["pos"], w["dirs"], **w["geom"], **PRM, flags=2, step_max=sm)
        smax = tr.defaults(**w["geom"], flags=2, step_max=sm)["smax"]
        assert c.tobytes() == w["counts"].tobytes() and st.tobytes() == w["step"].tobytes()
        assert np.array_equal(g, tr.classify(c, e, st, flags=2, smax=smax))
        assert s["cells_step_lethal"] == int(((e != tr.NONE) & (st > smax)).sum())
        assert (s["cells_free"], s["cells_occupied"], s["cells_unknown"]) == tuple(int((g == v).sum()) for v in (0, 100, -1))
        lethal.append(s["cells_step_lethal"])
    print("cells over step_max %r: %r" % (STEP_MAX, lethal))
    assert lethal[0] > lethal[1] >= 0 and lethal[0] > 0
    for kw in (dict(min_occ=3, min_free=5), dict(occ_ratio=0.3), dict(min_occ=2, occ_ratio=0.6, min_free=2)):
        g, e, st, c, s = M.terrain(w["pos"], w["dirs"], **w["geom"], **PRM, **kw)
        assert c.tobytes() == w["counts"].tobytes() and np.array_equal(g, tr.classify(c, e, st, **kw)), kw


def test_against_brute_force_hits():
    """5: the whole definition over raycast_ref's brute-force hits and the snapshot's normals, once: the ground
    planes outside the uncertain rays' hits' reach; the counts outside what the uncertain rays can touch, a ray that
    crosses a cell whose elevation differs counting as uncertain too. The workload exercises the feature."""
    w = _work()
    _, _, ended, _ = _records(w["hits"])
    r, idx, near = rr.cast(w["planes"], w["O"], w["Dd"])
    nz = np.where(idx >= 0, np.asarray(w["planes"]["normal"], dtype=np.float64).reshape(-1, 3)[np.maximum(idx, 0), 2], 0.0)
    ref = tr.terrain(w["O"], w["Dd"], r, nz, w["P"], near=near, ended=ended)
    unc = ref["uncertain"]
    reach = tr.hit_reach(ref["hit_cell"], unc, N, N)
    for name, got, want in zip(("g_n", "g_sum", "g_min", "g_max"), w["ground"], ref["planes"]):
        assert np.array_equal(got[~reach], want[~reach]), name
    dirty = ref["elev"] != w["elev"]
    assert not dirty[~reach].any()
    ri, ix, iy, _ = oc._pieces(w["O"], oc._unit(w["Dd"]), np.zeros(unc.size), np.full(unc.size, rr.T_MAX),
                               np.ones(unc.size, bool), **w["geom"])
    unc2 = unc.copy()
    unc2[ri[dirty[iy, ix]]] = True
    n_unc = int(unc2.sum())
    print("uncertain rays: %d of %d (+ %d over %d cells whose elevation differs); ground cells %d, carried hits %d, "
          "tilted ground hits %d" % (unc.sum(), unc.size, n_unc - unc.sum(), dirty.sum(), w["summ"]["cells_ground"],
                                     ref["carried"].sum(), (ref["ground"] & (np.abs(nz) < 0.99)).sum()))
    assert unc.sum() <= 0.02 * unc.size
    touch = oc.touched(w["O"], w["Dd"], unc2, rr.T_MAX, **w["geom"])
    diff = np.abs(w["counts"].astype(np.int64) - ref["counts"])
    assert not diff[:, ~touch].any(), np.argwhere(diff[:, ~touch])[:8]
    assert diff.max() <= n_unc
    # the workload exercises the feature
    smax = tr.defaults(**w["geom"], flags=2, step_max=STEP_MAX[0])["smax"]
    has = w["elev"] != tr.NONE
    assert w["summ"]["cells_ground"] > 0
    assert (has & (w["step"] > smax)).any() and (has & (w["step"] <= smax)).any()
    assert (ref["carried"] & ~unc).any()
    assert (ref["ground"] & (np.abs(nz) < 0.99) & ~unc).any()


def test_what_the_origin_band_gets_wrong():
    """6: cells that vg_occupancy calls occupied once its band reaches down to the floor, although they have an
    elevation, no in-band hit and are free under vg_terrain."""
    w = _work()
    g_occ, _, _ = w["M"].occupancy(w["pos"], w["dirs"], **w["geom"], z_lo=-5.0, z_hi=1.0)
    wrong = (g_occ == 100) & (w["elev"] != tr.NONE) & (w["counts"][1] == 0) & (w["grid"] == 0)
    print("cells occupied under the floor-inclusive origin band, free floor under vg_terrain: %d" % wrong.sum())
    assert wrong.sum() >= 1
    w["M"].terrain(w["pos"], w["dirs"], **w["geom"], **PRM)   # (leave the shared context's grid slot as _work did)


def test_order_and_batch_independence():
    """7: the same bytes with the positions reversed, from an attached tracker and with mapping on. M split over two
    calls: the four ground planes combine to those of one call by add, min and max. The count planes do NOT: pass 2
    of a call reads the elevation of that call's own ground hits, so the halves carry other references, free other
    pieces and judge hits otherwise than the whole call does. The issue's "counts ... combine" cannot hold for a call
    that builds its own elevation; the header promises it for the ground planes only. What holds and is checked: each
    half is a complete vg_terrain of its origins (elev and step of its own planes, counts of its own records over
    its own elev), and the whole call's counts are the sum of the halves' marks over the whole call's elevation
    (the reference, per half, given that elev). The number of cells in which the plain sum differs is printed."""
    w = _work()
    M, pos, dirs, geom = w["M"], w["pos"], w["dirs"], w["geom"]
    want = tuple(w[k].tobytes() for k in ("grid", "elev", "step", "counts")) + tuple(a.tobytes() for a in w["ground"])

    def got(c, p):
        g, e, st, n, s = c.terrain(p, dirs, **geom, **PRM)
        assert s == w["summ"] or p.shape[0] != pos.shape[0]
        return (g, e, st, n) + c.terrain_ground(N, N)

    assert tuple(a.tobytes() for a in got(M, pos[::-1])) == want
    a, b = got(M, pos[:1]), got(M, pos[1:])
    planes = (a[4] + b[4], a[5] + b[5], np.minimum(a[6], b[6]), np.maximum(a[7], b[7]))
    assert tuple(p.tobytes() for p in planes) == want[4:]
    r, nz, ended, _ = _records(w["hits"])
    D = dirs.shape[0]
    over_whole, reach = np.zeros_like(w["counts"], dtype=np.int64), np.zeros((N, N), bool)
    for half, sl in ((a, slice(0, D)), (b, slice(D, None))):
        e, st, _ = tr.cells(*half[4:], min_ground=1)
        assert half[1].tobytes() == e.tobytes() and half[2].tobytes() == st.tobytes()
        own = tr.terrain(w["O"][sl], w["Dd"][sl], r[sl], nz[sl], w["P"], elev=half[1], ended=ended[sl])
        touch = oc.touched(w["O"][sl], w["Dd"][sl], own["uncertain"], rr.T_MAX, **geom)
        assert own["uncertain"].sum() <= 0.02 * own["uncertain"].size
        assert np.array_equal(half[3][:, ~touch], own["counts"][:, ~touch])
        ref = tr.terrain(w["O"][sl], w["Dd"][sl], r[sl], nz[sl], w["P"], elev=w["elev"], ended=ended[sl])
        reach |= oc.touched(w["O"][sl], w["Dd"][sl], ref["uncertain"], rr.T_MAX, **geom)
        over_whole += ref["counts"]
    assert np.array_equal(over_whole[:, ~reach], w["counts"][:, ~reach]) and reach.sum() < N * N // 2
    plain = a[3].astype(np.int64) + b[3]
    print("cells in which the counts of the two separate calls do not add up to the whole call's: %d of %d"
          % ((plain != w["counts"]).any(axis=0).sum(), N * N))
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    T.attach(M)
    assert tuple(x.tobytes() for x in got(T, pos)) == want
    T.close()
    A = lc.loaded(mapping=True)
    assert tuple(x.tobytes() for x in got(A, pos)) == want
    A.close()
    assert tuple(x.tobytes() for x in got(M, pos)) == want


def test_chains_into_clearance():
    """8: vg_clearance(grid = NULL) after vg_terrain equals vg_clearance on the returned grid, byte for byte; with
    another nx it is VG_E_STATE."""
    w = _work()
    M = w["M"]
    grid = M.terrain(w["pos"], w["dirs"], **w["geom"], **PRM)[0]
    assert grid.tobytes() == w["grid"].tobytes()
    kw = dict(res=RES, inscribed_radius=0.3, inflation_radius=1.0, cost_scaling=3.0)
    dev, sd = M.clearance(None, nx=N, ny=N, **kw)
    host, sh = M.clearance(grid, **kw)
    assert set(dev) == {"dist2", "nearest", "cost"}
    for k in dev:
        assert dev[k].tobytes() == host[k].tobytes(), k
    assert sd == sh and sd["n_obstacles"] == int((grid == 100).sum()) > 0
    with pytest.raises(vgpu.VgError) as ei:
        M.clearance(None, nx=N + 1, ny=N, **kw)
    assert "(-5)" in str(ei.value)


def _crafted(ny, nx, seed, min_ground):
    """Ground planes with a ramp, a single step, holes and borders without ground, values at +-(2^30 - 1), g_n below
    and at min_ground, and negative sums."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    e = (7 * xx - 13 * yy - 40).astype(np.int64)                  # a ramp through negative heights
    e[:, nx // 2:] += 300                                         # a single step
    e[rng.random((ny, nx)) < 0.03] = 2 ** 30 - 1
    e[rng.random((ny, nx)) < 0.03] = -(2 ** 30 - 1)
    g_n = rng.choice([0, min_ground - 1, min_ground, min_ground + 4], size=(ny, nx), p=[0.15, 0.15, 0.4, 0.3]).astype(np.int32)
    if seed % 2 and ny > 2:                                       # borders without ground (every other case)
        g_n[[0, -1], :] = 0
    if seed % 2 and nx > 2:
        g_n[:, [0, -1]] = 0
    if ny > 8 and nx > 8:
        g_n[ny // 3:ny // 3 + 3, nx // 3:nx // 3 + 5] = 0         # a hole
    rem = (rng.integers(0, 1 << 30, size=(ny, nx)) % np.maximum(g_n, 1)).astype(np.int64)
    g_sum = np.where(g_n > 0, e * g_n + rem, 0)                   # floor(g_sum / g_n) = e
    lim = 2 ** 30 - 1
    g_min = np.where(g_n > 0, np.maximum(e - rng.integers(0, 50, size=(ny, nx)), -lim), 2 ** 31 - 1).astype(np.int32)
    g_max = np.where(g_n > 0, np.minimum(e + rng.integers(0, 50, size=(ny, nx)) + (rem > 0), lim), -2 ** 31).astype(np.int32)
    return g_n, g_sum, g_min, g_max


@pytest.mark.parametrize("shape", [(1, 1), (1, 130), (65, 67), (130, 70), (70, 130)])
def test_cells_on_crafted_planes(shape):
    """9: the per-cell stage alone (vgx_ter_cells) on crafted integer planes, bit for bit with terrain_ref.cells,
    cells on both sides of every 32- and 8-cell tile boundary (and of 64), and a last tile that is not full."""
    M = _work()["M"]
    ny, nx = shape
    for seed, min_ground in ((ny + nx, 1), (ny + nx + 1, 3)):
        planes = _crafted(ny, nx, seed, min_ground)
        want = tr.cells(*planes, min_ground=min_ground)
        elev, step, stats = M.terrain_cells(*planes, min_ground=min_ground)
        assert elev.tobytes() == want[0].tobytes() and step.tobytes() == want[1].tobytes(), seed
        assert stats == want[2], seed
        if nx > 1:
            assert want[2][0] > 0 and (want[0] == tr.NONE).any()
            assert want[2][1] > 2 ** 29 and want[2][2] > 0         # a step up to an extreme value fits an int32
    with pytest.raises(vgpu.VgError) as ei:
        M.terrain_ground(nx, ny)                                   # the hook forgot the last call's planes
    assert "(-5)" in str(ei.value)
    M.terrain(_work()["pos"], _work()["dirs"], **_work()["geom"], **PRM)
    with pytest.raises(vgpu.VgError) as ei:
        M.terrain_ground(N + 1, N)                                 # not the last call's shape: nothing is written
    assert "(-1)" in str(ei.value)


def test_edges_and_errors():
    """10: M = 0; an empty map with and without free_on_miss; vertical rays; a grid off the map; NULL outputs; the
    argument errors of the new parameters and vg_occupancy's; a sharded context."""
    w = _work()
    M, pos, dirs, geom = w["M"], w["pos"], w["dirs"], w["geom"]
    g, e, st, c, s = M.terrain(np.zeros((0, 3)), dirs, **geom, **PRM)
    assert (g == -1).all() and (e == tr.NONE).all() and not st.any() and not c.any()
    assert s["cells_unknown"] == N * N and s["n_rays"] == 0 and s["cells_ground"] == 0 and s["max_spread"] == 0
    gp = M.terrain_ground(N, N)
    assert not gp[0].any() and not gp[1].any() and (gp[2] == 2 ** 31 - 1).all() and (gp[3] == -2 ** 31).all()
    off = dict(geom, x0=geom["x0"] + 5000.0)
    g, e, st, c, s = M.terrain(pos, dirs, **off, **PRM)
    assert (g == -1).all() and (e == tr.NONE).all() and not c.any() and s["n_hits"] == w["summ"]["n_hits"]
    assert s["n_ground_hits"] == 0
    # straight down / up: the cell the ray stands in and no other, as the definition over the records has it
    vert = np.array([(0.0, 0.0, -1.0), (0.0, 0.0, 2.0)])
    g, e, st, c, s = M.terrain(pos[:1], vert, **geom, **PRM, free_on_miss=3.0)
    h = M.raycast(np.repeat(pos[:1], 2, axis=0), vert)
    r, nz, ended, _ = _records(h)
    ref = tr.terrain(np.repeat(pos[:1], 2, axis=0), vert, r, nz, tr.defaults(**geom, **PRM, free_on_miss=3.0), ended=ended)
    iy, ix = int((pos[0, 1] - geom["y0"]) // RES), int((pos[0, 0] - geom["x0"]) // RES)
    other = c.copy()
    other[:, iy, ix] = 0
    assert not other.any() and s["n_rays"] == 2 and np.array_equal(c, ref["counts"]) and np.array_equal(e, ref["elev"])
    # an empty map: nothing to hit; a miss marks only with free_on_miss, and only in the band over q(o_z - sensor_height)
    E = lc.ctx()
    g, e, st, c, s = E.terrain(pos, dirs, **geom, **PRM)
    assert (g == -1).all() and (e == tr.NONE).all() and s["n_hits"] == 0 and s["free_marks"] == 0
    g, e, st, c, s = E.terrain(pos, dirs, **geom, **PRM, free_on_miss=2.0)
    ref = tr.terrain(w["O"], w["Dd"], np.full(w["O"].shape[0], np.inf), np.zeros(w["O"].shape[0]),
                     tr.defaults(**geom, **PRM, free_on_miss=2.0))
    touch = oc.touched(w["O"], w["Dd"], ref["uncertain"], 2.0, **geom)
    assert ref["uncertain"].sum() <= 0.02 * ref["uncertain"].size
    assert np.array_equal(c[:, ~touch], ref["counts"][:, ~touch]) and not c[1].any() and c[0].sum() > 1000
    assert s["cells_free"] == int((c[0] > 0).sum()) and (e == tr.NONE).all()
    E.close()
    # NULL outputs and the argument errors
    L, P = vgpu.lib(), M.h
    pp, dd = vgpu._d(np.ascontiguousarray(pos)), vgpu._d(np.ascontiguousarray(dirs))
    grid, sm = np.zeros(N * N, dtype=np.int8), vgpu.TerrainSummary()
    ok = vgpu.terrain_params(**geom, **PRM)

    def call(ctx=P, p=pp, m=4, d=dd, nd=256, prm=ok, g=grid.ctypes.data, out=sm):
        return L.vg_terrain(ctx, p, m, d, nd, None if prm is None else ctypes.byref(prm), g, None, None, None,
                            None if out is None else ctypes.byref(out))

    assert call() == 0 and grid.tobytes() == w["grid"].tobytes() and call(p=None, m=0) == 0
    assert sm.n_rays == 0 and call() == 0 and sm.n_ground_hits == w["summ"]["n_ground_hits"]
    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(p=None), dict(m=-1), dict(d=None), dict(nd=0), dict(nd=4097), dict(prm=None),
           dict(g=None), dict(out=None)]
    for kw in (dict(res=0.0), dict(res=-1.0), dict(res=nan), dict(res=inf), dict(x0=nan), dict(y0=inf), dict(nx=0),
               dict(ny=-3), dict(nx=4097, ny=4097), dict(flags=4), dict(flags=7), dict(z_res=nan), dict(z_res=inf),
               dict(up_min=nan), dict(g_lo=-0.1, g_hi=-0.1), dict(g_lo=-0.1, g_hi=-3.0), dict(g_lo=nan, g_hi=-0.1),
               dict(clear_lo=1.5, clear_hi=1.5), dict(clear_lo=1.5, clear_hi=0.15), dict(clear_lo=0.1, clear_hi=nan),
               dict(sensor_height=-0.1), dict(sensor_height=nan), dict(sensor_height=inf),
               dict(flags=2, step_max=-0.1), dict(flags=2, step_max=nan)):
        bad.append(dict(prm=vgpu.terrain_params(**dict(dict(geom, **PRM), **kw))))
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(prm=vgpu.terrain_params(**dict(geom, nx=4096, ny=1), **PRM)) == 0
    assert call(prm=vgpu.terrain_params(**geom, **PRM, step_max=nan)) == 0      # (read only with flags bit 1)
    assert call() == 0
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    with pytest.raises(vgpu.VgError) as ei:
        S.terrain(pos, dirs, **geom, **PRM)
    assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()


def test_replay_terrain(tmp_path):
    """11: vg_node_replay --map ... --localize --terrain writes a grid and an elevation that are Context.terrain's of
    the same origins, directions and parameters (--terrain-rays) in the same map; with --costmap the cost is that of
    the terrain grid, with --occupancy beside it or without; without --localize it is refused."""
    import os
    import subprocess

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
        return r.stderr

    ck = tmp_path / "map.vgck"
    run([log, tmp_path / "a.tum", 0, tmp_path / "a.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    pre, occ, cm = str(tmp_path / "ter"), str(tmp_path / "nav"), str(tmp_path / "cost")
    run([log, tmp_path / "x.tum", "--terrain", pre], rc=2)
    run([log, tmp_path / "x.tum", "--sensor-height", 1.5], rc=2)
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    err = run([log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--occupancy", occ, "--occ-res", 0.2,
               "--terrain", pre, "--sensor-height", 1.5, "--step-max", 0.25, "--terrain-rays", tmp_path / "rays.bin",
               "--costmap", cm])
    assert "terrain: " in err and "occupancy: " in err
    cm2 = str(tmp_path / "cost2")                                  # --costmap goes with --terrain alone
    err2 = run([log, tmp_path / "h.tum", "--map", ck, "--localize", "--guess", guess, "--occ-res", 0.2, "--terrain",
                str(tmp_path / "ter2"), "--sensor-height", 1.5, "--step-max", 0.25, "--costmap", cm2])
    assert "terrain: " in err2 and "costmap: " in err2 and "occupancy: " not in err2
    run([log, tmp_path / "x.tum", "--map", ck, "--localize", "--guess", guess, "--costmap", cm2], rc=2)
    raw = open(tmp_path / "rays.bin", "rb").read()
    m, d = np.frombuffer(raw, dtype=np.int32, count=2)
    prm = vgpu.TerrainParams.from_buffer_copy(raw, 8)
    at = 8 + ctypes.sizeof(vgpu.TerrainParams)
    pos = np.frombuffer(raw, dtype=np.float64, count=3 * m, offset=at).reshape(m, 3)
    dirs = np.frombuffer(raw, dtype=np.float64, count=3 * d, offset=at + 24 * m).reshape(d, 3)
    assert m >= 1 and d == 5 * 360 and len(raw) == at + 24 * (m + d)
    assert (prm.res, prm.sensor_height, prm.step_max, prm.flags) == (0.2, 1.5, 0.25, 2)
    grid, x0, y0, res = vgpu.read_occupancy(pre)
    elev, ex0, ey0, eres, z_res = vgpu.read_terrain(pre)
    assert (x0, y0, res) == (ex0, ey0, eres) == (prm.x0, prm.y0, prm.res) and z_res == 0.001
    assert grid.shape == elev.shape == (prm.ny, prm.nx)
    occ_grid = vgpu.read_occupancy(occ)[0]
    cost = vgpu.read_costmap(cm)[0]
    C = vgpu.Context(vgconfig.to_c(p), max_points=400_000)
    C.checkpoint_load(str(ck))
    C.set_mapping(False)
    want, welev, wstep, _, s = C.terrain(pos, dirs, prm=prm)
    wcost = C.clearance(None, nx=prm.nx, ny=prm.ny, res=prm.res, inscribed_radius=0.3, inflation_radius=1.0,
                        cost_scaling=3.0, want=("cost",))[0]["cost"]
    C.close()
    print("replay terrain %d x %d: %d ground cells, %d occupied (%d by their step), %d free; differs from --occupancy's "
          "grid in %d cells" % (prm.nx, prm.ny, s["cells_ground"], s["cells_occupied"], s["cells_step_lethal"],
                                s["cells_free"], (occ_grid != want).sum()))
    assert s["cells_ground"] > 0 and s["cells_free"] > s["cells_occupied"] > 0
    assert np.array_equal(grid, want) and np.array_equal(elev, welev)
    assert np.array_equal(cost, wcost) and (occ_grid != want).any()
    assert np.array_equal(vgpu.read_costmap(cm2)[0], wcost) and np.array_equal(vgpu.read_occupancy(str(tmp_path / "ter2"))[0], want)
