"""vg_occupancy (vina_gpu.h "Occupancy grid") against the numpy restatement of its
definition (tests/occ_ref.py) on the localisation tests' map (loc_common: the
16-line sequence 3 after scan 30, frozen; the ray-cast tests' workload): the
definition, order and batch independence, the band, flags bit 0, the edges, the
summary's arithmetic and the replay tool's --occupancy."""
import ctypes
import math

import numpy as np
import pytest

import loc_common as lc
import occ_ref as oc
import raycast_ref as rr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
RES, N = 0.25, 64
BAND = dict(z_lo=-0.3, z_hi=1.0)
ENDED = vgpu.RAY_TRUNCATED | vgpu.RAY_LEFT_RANGE | vgpu.RAY_INVALID

_cache = {}


def _work():
    """{M: the frozen loaded context (shared, never closed), planes, pos: 4 LiDAR origins of the
    ground-truth trajectory, dirs: 64 azimuths (0.37 degrees off the axes) x 4 elevations, geom: 64 x 64 cells
    of 0.25 m centred on the origins, O / Dd: the 1024 rays, hits: vg_raycast of them, grid / counts /
    summ: vg_occupancy of them in BAND}: computed once, read-only afterwards."""
    if not _cache:
        w = rr.workload()
        M = w["M"]
        g = lc.gt_traj(lc.base()["seq"], 5, 31)
        ext_t = lc.ext()[1]
        rows = g[np.linspace(0, g.shape[0] - 1, 4).astype(int)]
        pos = np.array([row[10:13] + row[1:10].reshape(3, 3) @ ext_t for row in rows])
        _, dirs = rr.fan(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]), np.zeros(3), n_az=64, n_el=4, el_deg=15.0)
        c = pos[:, :2].mean(axis=0)
        geom = dict(x0=float(c[0] - 0.5 * N * RES), y0=float(c[1] - 0.5 * N * RES), res=RES, nx=N, ny=N)
        O, Dd = np.repeat(pos, dirs.shape[0], axis=0), np.tile(dirs, (pos.shape[0], 1))
        grid, counts, summ = M.occupancy(pos, dirs, counts=True, **geom, **BAND)
        _cache.update(M=M, planes=w["planes"], pos=pos, dirs=dirs, geom=geom, O=O, Dd=Dd, hits=M.raycast(O, Dd),
                      grid=grid, counts=counts, summ=summ)
    return _cache


def _ranges(hits):
    return np.where((hits["flags"] & vgpu.RAY_HIT) != 0, hits["range"], np.inf)


def test_against_the_reference():
    """1: both count planes equal the numpy definition over raycast_ref's brute-force hits in every cell no
    uncertain ray could touch, elsewhere within the number of uncertain rays; the grid is the
    classification of the device's own counts; uncertain rays <= 1 % of the 1024."""
    w = _work()
    ended = (w["hits"]["flags"] & ENDED) != 0
    r, _, near = rr.cast(w["planes"], w["O"], w["Dd"])
    ref, unc, in_band = oc.marks(w["O"], w["Dd"], r, near=near, ended=ended, **w["geom"], **BAND)
    n_unc = int(unc.sum())
    print("uncertain rays: %d of %d; free marks %d (ref %d), occ marks %d (ref %d), ended %d"
          % (n_unc, unc.size, w["counts"][0].sum(), ref[0].sum(), w["counts"][1].sum(), ref[1].sum(), ended.sum()))
    assert n_unc <= 0.01 * unc.size
    assert ref[0].sum() > 10 * unc.size and ref[1].sum() > unc.size // 8      # the workload marks something
    touch = oc.touched(w["O"], w["Dd"], unc, rr.T_MAX, **w["geom"])
    diff = np.abs(w["counts"].astype(np.int64) - ref)
    assert not diff[:, ~touch].any(), np.argwhere(diff[:, ~touch])[:8]
    assert diff.max() <= n_unc
    assert np.array_equal(w["grid"], oc.classify(w["counts"]))
    assert w["grid"].dtype == np.int8 and set(np.unique(w["grid"])) <= {-1, 0, 100}
    # thresholds and the ratio, on the same counts
    for kw in (dict(min_occ=3, min_free=5), dict(occ_ratio=0.3), dict(min_occ=2, occ_ratio=0.6, min_free=2)):
        g2, c2, _ = w["M"].occupancy(w["pos"], w["dirs"], counts=True, **w["geom"], **BAND, **kw)
        assert c2.tobytes() == w["counts"].tobytes() and np.array_equal(g2, oc.classify(c2, **kw)), kw


def test_order_and_batch_independence():
    """2: the same bytes with the positions reversed, with M split over two calls whose counts are added,
    from an attached tracker, and with mapping on."""
    w = _work()
    M, pos, dirs, geom = w["M"], w["pos"], w["dirs"], w["geom"]
    want = (w["grid"].tobytes(), w["counts"].tobytes())

    def got(c, p):
        g, n, s = c.occupancy(p, dirs, counts=True, **geom, **BAND)
        assert s == w["summ"] or p.shape[0] != pos.shape[0]
        return g, n

    g, n = got(M, pos[::-1])
    assert (g.tobytes(), n.tobytes()) == want
    (ga, na), (gb, nb) = got(M, pos[:1]), got(M, pos[1:])
    assert (na + nb).tobytes() == want[1] and oc.classify(na + nb).tobytes() == want[0]
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    T.attach(M)
    g, n = got(T, pos)
    assert (g.tobytes(), n.tobytes()) == want
    T.close()
    A = lc.loaded(mapping=True)
    g, n = got(A, pos)
    assert (g.tobytes(), n.tobytes()) == want
    A.close()


def test_band():
    """3: a band above every horizontal ray gives no mark at all; the cells occupied with the floor kept
    out of the band are a subset of those with it in."""
    w = _work()
    M, pos, geom = w["M"], w["pos"], w["geom"]
    flat = vgpu.occupancy_dirs(n_az=90, elevations_deg=(0,)) @ np.array([[math.cos(0.0065), math.sin(0.0065), 0.0],
                                                                            [-math.sin(0.0065), math.cos(0.0065), 0.0],
                                                                            [0.0, 0.0, 1.0]])
    g, c, s = M.occupancy(pos, flat, counts=True, **geom, z_lo=5.0, z_hi=6.0)
    assert not c.any() and (g == -1).all() and s["free_marks"] == 0 and s["occ_marks"] == 0
    assert s["n_hits_in_band"] == 0 and s["n_hits"] > 0 and s["cells_unknown"] == N * N
    down = vgpu.occupancy_dirs(n_az=180, elevations_deg=(-30, -12, 0))
    g_no, _, s_no = M.occupancy(pos, down, **geom, **BAND)
    g_fl, _, s_fl = M.occupancy(pos, down, **geom, z_lo=-5.0, z_hi=1.0)
    assert not ((g_no == 100) & (g_fl != 100)).any()
    assert s_no["n_hits"] == s_fl["n_hits"] and s_no["n_hits_in_band"] < s_fl["n_hits_in_band"]
    assert s_no["cells_occupied"] < s_fl["cells_occupied"]


def test_flags_bit0():
    """4: with flags bit 0 free_marks does not grow, the occupied plane keeps its bytes, and the rays
    silenced are exactly those whose vg_raycast record has VG_RAY_OCCUPIED: both free planes equal the
    definition over the device's own records, with and without those rays, outside the uncertain rays'
    reach."""
    w = _work()
    M, pos, dirs, geom, hits = w["M"], w["pos"], w["dirs"], w["geom"], w["hits"]
    g1, c1, s1 = M.occupancy(pos, dirs, counts=True, flags=1, **geom, **BAND)
    occupied = (hits["flags"] & vgpu.RAY_OCCUPIED) != 0
    print("rays with VG_RAY_OCCUPIED: %d of %d; free marks %d -> %d" % (occupied.sum(), occupied.size,
                                                                        w["summ"]["free_marks"], s1["free_marks"]))
    assert s1["free_marks"] <= w["summ"]["free_marks"] and c1[1].tobytes() == w["counts"][1].tobytes()
    assert s1["n_occupied_unknown"] == w["summ"]["n_occupied_unknown"] == int(occupied.sum())
    assert (s1["free_marks"] == w["summ"]["free_marks"]) == (not (w["counts"][0] != c1[0]).any())
    ended = (hits["flags"] & ENDED) != 0
    for silent, c in ((None, w["counts"]), (occupied, c1)):
        ref, unc, _ = oc.marks(w["O"], w["Dd"], _ranges(hits), ended=ended, silent=silent, **geom, **BAND)
        touch = oc.touched(w["O"], w["Dd"], unc, rr.T_MAX, **geom)
        assert unc.sum() <= 0.01 * unc.size
        assert not (c.astype(np.int64) - ref)[:, ~touch].any()


def test_edges():
    """5: M = 0; a 1 x 1 grid; a grid off the map; vertical rays; a ray with d_y = 0 from a point exactly on
    an x-lattice line; an empty map; the argument errors; a sharded context."""
    w = _work()
    M, pos, dirs, geom = w["M"], w["pos"], w["dirs"], w["geom"]
    g, c, s = M.occupancy(np.zeros((0, 3)), dirs, counts=True, **geom, **BAND)
    assert (g == -1).all() and not c.any() and s["cells_unknown"] == N * N and s["n_rays"] == 0 and s["n_hits"] == 0
    one = dict(x0=float(pos[0, 0] - 0.1), y0=float(pos[0, 1] - 0.1), res=0.25, nx=1, ny=1)
    g, c, s = M.occupancy(pos[:1], dirs, counts=True, **one, **BAND)
    n_hit = int(((M.raycast(pos[0], dirs)["flags"] & vgpu.RAY_HIT) != 0).sum())   # (a miss marks nothing here)
    assert g.shape == (1, 1) and g[0, 0] == 0 and c[0, 0, 0] == n_hit > 0 and c[1, 0, 0] == 0   # every ray starts in it
    off = dict(geom, x0=geom["x0"] + 5000.0)
    g, c, s = M.occupancy(pos, dirs, counts=True, **off, **BAND)
    assert (g == -1).all() and not c.any() and s["n_hits"] == w["summ"]["n_hits"]
    # straight down / up: the cell the ray stands in and no other
    g, c, s = M.occupancy(pos[:1], [(0.0, 0.0, -1.0), (0.0, 0.0, 2.0)], counts=True, **geom, z_lo=-50.0, z_hi=50.0,
                          free_on_miss=3.0)
    iy, ix = int((pos[0, 1] - geom["y0"]) // RES), int((pos[0, 0] - geom["x0"]) // RES)
    other = c.copy()
    other[:, iy, ix] = 0
    assert not other.any() and c[:, iy, ix].sum() == 2 and s["n_rays"] == 2
    # d_y = 0 from a point exactly on an x-lattice line: ends, marks what the definition allows
    lat = dict(geom, x0=float(math.floor(pos[0, 0]) - 8.0))
    on = np.array([[math.floor(pos[0, 0]) + 0.0, pos[0, 1], pos[0, 2]]])
    ax = np.array([(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)])
    g, c, s = M.occupancy(on, ax, counts=True, **lat, **BAND, free_on_miss=4.0)
    h = M.raycast(np.repeat(on, 2, axis=0), ax)
    ref, unc, _ = oc.marks(np.repeat(on, 2, axis=0), ax, _ranges(h), free_on_miss=4.0, **lat, **BAND)
    assert unc.all() and np.abs(c.astype(np.int64) - ref).max() <= 2 and s["n_rays"] == 2
    # an empty map: nothing to hit; a miss marks only with free_on_miss
    E = lc.ctx()
    g, c, s = E.occupancy(pos, dirs, counts=True, **geom, **BAND)
    assert (g == -1).all() and s["n_hits"] == 0 and s["free_marks"] == 0
    g, c, s = E.occupancy(pos, dirs, counts=True, **geom, **BAND, free_on_miss=2.0)
    ref, unc, _ = oc.marks(w["O"], w["Dd"], np.full(w["O"].shape[0], np.inf), free_on_miss=2.0, **geom, **BAND)
    assert not unc.any() and np.array_equal(c, ref) and not c[1].any() and s["cells_free"] == int((ref[0] > 0).sum())
    E.close()
    # argument errors
    L, P = vgpu.lib(), M.h
    pp, dd = vgpu._d(np.ascontiguousarray(pos)), vgpu._d(np.ascontiguousarray(dirs))
    grid, cnt, sm = np.zeros(N * N, dtype=np.int8), np.zeros(2 * N * N, dtype=np.int32), vgpu.OccSummary()
    ok = vgpu.occ_params(**geom, **BAND)

    def call(ctx=P, p=pp, m=4, d=dd, nd=256, prm=ok, g=grid.ctypes.data, out=sm):
        return L.vg_occupancy(ctx, p, m, d, nd, None if prm is None else ctypes.byref(prm), g, cnt.ctypes.data,
                              None if out is None else ctypes.byref(out))

    assert call() == 0 and call(p=None, m=0) == 0
    bad = [dict(ctx=None), dict(p=None), dict(m=-1), dict(d=None), dict(nd=0), dict(nd=4097), dict(prm=None),
           dict(g=None), dict(out=None)]
    for kw in (dict(res=0.0), dict(res=-1.0), dict(res=float("nan")), dict(res=float("inf")), dict(x0=float("nan")),
               dict(y0=float("inf")), dict(nx=0), dict(ny=-3), dict(nx=4097, ny=4097), dict(z_lo=1.0, z_hi=1.0),
               dict(z_lo=2.0, z_hi=1.0), dict(z_lo=float("nan")), dict(flags=2)):
        bad.append(dict(prm=vgpu.occ_params(**dict(dict(geom, **BAND), **kw))))
    for kw in bad:
        assert call(**kw) == -1, kw
    assert call(prm=vgpu.occ_params(**dict(geom, nx=4096, ny=1), **BAND)) == 0
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    with pytest.raises(vgpu.VgError) as ei:
        S.occupancy(pos, dirs, **geom, **BAND)
    assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()


def test_summary_arithmetic():
    """6: the marks are the planes' sums, the classes add up to the cells, and the ray counts are vg_raycast's
    on the same rays."""
    w = _work()
    s, c, f = w["summ"], w["counts"], w["hits"]["flags"]
    assert s["free_marks"] == int(c[0].sum()) and s["occ_marks"] == int(c[1].sum())
    assert s["cells_free"] + s["cells_occupied"] + s["cells_unknown"] == N * N
    assert (s["cells_free"], s["cells_occupied"], s["cells_unknown"]) == tuple(int((w["grid"] == v).sum()) for v in (0, 100, -1))
    assert s["n_rays"] == f.size and s["n_hits"] == int(((f & vgpu.RAY_HIT) != 0).sum()) and s["n_hits"] > 0
    assert s["n_truncated"] == int(((f & vgpu.RAY_TRUNCATED) != 0).sum())
    assert s["n_occupied_unknown"] == int(((f & vgpu.RAY_OCCUPIED) != 0).sum()) and s["n_invalid"] == 0
    rz = w["hits"]["range"] * (w["Dd"][:, 2] / np.linalg.norm(w["Dd"], axis=1))
    inb = ((f & vgpu.RAY_HIT) != 0) & ((f & ENDED) == 0) & (rz >= BAND["z_lo"]) & (rz <= BAND["z_hi"])
    assert s["n_hits_in_band"] == int(inb.sum()) and s["occ_marks"] <= s["n_hits_in_band"]
    d = w["dirs"].copy()
    d[7] = np.nan
    assert w["M"].occupancy(w["pos"], d, **w["geom"], **BAND)[2]["n_invalid"] == w["pos"].shape[0]


def test_replay_occupancy(tmp_path):
    """7: vg_node_replay --map ... --localize --occupancy writes a pgm whose pixels are Context.occupancy's
    grid of the same origins, directions and parameters (--occ-rays) in the same map, and a yaml with the
    grid's origin and resolution; without --localize it is refused."""
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
    pre = str(tmp_path / "nav")
    run([log, tmp_path / "x.tum", "--occupancy", pre], rc=2)
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    err = run([log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--occupancy", pre, "--occ-res", 0.2,
               "--occ-rays", tmp_path / "rays.bin"])
    assert "occupancy: " in err
    raw = open(tmp_path / "rays.bin", "rb").read()
    m, d = np.frombuffer(raw, dtype=np.int32, count=2)
    prm = vgpu.OccParams.from_buffer_copy(raw, 8)
    at = 8 + ctypes.sizeof(vgpu.OccParams)
    pos = np.frombuffer(raw, dtype=np.float64, count=3 * m, offset=at).reshape(m, 3)
    dirs = np.frombuffer(raw, dtype=np.float64, count=3 * d, offset=at + 24 * m).reshape(d, 3)
    assert m >= 1 and d == 1080 and len(raw) == at + 24 * (m + d) and prm.res == 0.2
    assert np.all(np.linalg.norm(np.diff(pos, axis=0), axis=1) >= 0.2)          # one origin per cell edge
    grid, x0, y0, res = vgpu.read_occupancy(pre)
    assert (x0, y0, res) == (prm.x0, prm.y0, prm.res) and grid.shape == (prm.ny, prm.nx)
    C = vgpu.Context(vgconfig.to_c(p), max_points=400_000)
    C.checkpoint_load(str(ck))
    C.set_mapping(False)
    want, _, s = C.occupancy(pos, dirs, prm=prm)
    C.close()
    print("replay grid %d x %d: %d occupied, %d free" % (prm.nx, prm.ny, s["cells_occupied"], s["cells_free"]))
    assert s["cells_occupied"] > 0 and s["cells_free"] > s["cells_occupied"]
    assert np.array_equal(grid, want)
