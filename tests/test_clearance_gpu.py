"""vg_clearance (vina_gpu.h "Clearance field and costmap") against the numpy
restatement of its definition (tests/clr_ref.py), byte for byte: the definition
on a random grid, the tie-break, the degenerate obstacle sets, shapes that cross
the kernels' tiles, the nullable outputs and determinism, the chain behind
vg_occupancy (grid == NULL), the replay tool's --costmap and the argument
errors. Grids are the smallest at which the kernels can still go wrong; every
parameter set is one test_clr_ref.py holds boundary_free for."""
import ctypes
import math

import numpy as np
import pytest

import clr_ref as cr
import loc_common as lc
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
NAV, FINE = cr.PARAMS["nav"], cr.PARAMS["fine"]

_cache = {}


def _ctx():
    """A context with no map (shared, never closed): vg_clearance reads none."""
    if "C" not in _cache:
        _cache["C"] = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    return _cache["C"]


def _check(g, flags=0, prm=NAV, C=None):
    """clearance(g) on the device equals the restatement in all three outputs and its summary counts them."""
    ref = cr.clearance(g, flags, **prm)
    cr.boundary_free(ref["dist2"], prm)
    out, s = (C or _ctx()).clearance(g, flags=flags, **prm)
    for k in ("dist2", "nearest", "cost"):
        assert out[k].dtype == ref[k].dtype and out[k].shape == g.shape
        bad = np.argwhere(out[k] != ref[k])
        assert not bad.size, (k, bad[:8], out[k][tuple(bad[0])], ref[k][tuple(bad[0])])
    assert s == cr.summary(g, flags, out["dist2"], out["cost"])
    assert s["cells_lethal"] + s["cells_inscribed"] + s["cells_inflated"] + s["cells_free"] + s["cells_no_info"] == g.size
    return out, s


@pytest.mark.parametrize("flags", [0, 1])
def test_against_the_restatement(flags):
    """1: 61 x 47, about 3 % occupied, 20 % unknown, the byte 50 in a few cells, with both values of flags bit 0."""
    g = cr.random_grid(61, 47, 7)
    assert g.shape == (47, 61) and (g == 100).sum() > 40 and (g == -1).sum() > 400 and (g == 50).sum() >= 4
    out, s = _check(g, flags)
    assert s["n_obstacles"] == int((g == 100).sum()) + (int((g == -1).sum()) if flags else 0)
    assert s["cells_inflated"] > 0 and s["cells_inscribed"] > 0 and (flags == 1 or s["cells_no_info"] > 0)
    assert (s["cells_free"] > 0) == (flags == 0) and len(np.unique(out["cost"])) > (6 if flags else 12)


def test_tie_break():
    """2: among equally near obstacles `nearest` is the smallest linear index: two obstacles mirrored about a
    column, about a row, and four on a square's corners seen from its centre."""
    g = np.zeros((7, 9), dtype=np.int8)
    g[3, 1] = g[3, 7] = 100                                          # mirrored about column 4
    out, _ = _check(g)
    assert (out["nearest"][:, 4] == 3 * 9 + 1).all() and out["nearest"][3, 5] == 3 * 9 + 7
    g = np.zeros((9, 7), dtype=np.int8)
    g[1, 3] = g[7, 3] = 100                                          # mirrored about row 4
    out, _ = _check(g)
    assert (out["nearest"][4, :] == 1 * 7 + 3).all() and out["nearest"][5, 3] == 7 * 7 + 3
    g = np.zeros((11, 11), dtype=np.int8)
    g[2, 2] = g[2, 8] = g[8, 2] = g[8, 8] = 100
    out, _ = _check(g)
    assert out["nearest"][5, 5] == 2 * 11 + 2 and out["dist2"][5, 5] == 18
    assert out["nearest"][5, 2] == 2 * 11 + 2 and out["nearest"][2, 5] == 2 * 11 + 2 and out["nearest"][8, 5] == 8 * 11 + 2
    g[5, 1] = g[5, 9] = g[1, 5] = g[9, 5] = 100                      # four more, nearer (16 < 18): the topmost wins
    out, _ = _check(g)
    assert out["nearest"][5, 5] == 1 * 11 + 5 and out["dist2"][5, 5] == 16


def test_degenerate_sets():
    """3: no obstacle; every cell an obstacle; one obstacle at a corner of 130 x 3; a 1 x 1 grid."""
    g = np.zeros((6, 70), dtype=np.int8)
    g[2, 5:9] = -1
    out, s = _check(g)
    assert (out["dist2"] == vgpu.CLR_NONE).all() and (out["nearest"] == -1).all()
    assert np.array_equal(out["cost"], np.where(g == -1, 255, 0)) and s["max_dist2"] == 0 and s["n_obstacles"] == 0
    assert (s["n_unknown"], s["cells_no_info"], s["cells_free"]) == (4, 4, 6 * 70 - 4)
    out, s = _check(g, flags=1)                                      # ... and the four unknown cells as the only obstacles
    assert s["n_obstacles"] == 4 and s["cells_lethal"] == 4 and s["cells_no_info"] == 0 and s["max_dist2"] == 61 ** 2 + 9
    g = np.full((13, 20), 100, dtype=np.int8)
    out, s = _check(g)
    assert not out["dist2"].any() and np.array_equal(out["nearest"].ravel(), np.arange(260)) and s["cells_lethal"] == 260
    for corner in ((0, 0), (0, 129), (2, 0), (2, 129)):
        g = np.zeros((3, 130), dtype=np.int8)
        g[corner] = 100
        out, s = _check(g)
        assert (out["nearest"] == corner[0] * 130 + corner[1]).all() and s["max_dist2"] == 129 ** 2 + 4
    for v, c in ((0, 0), (-1, 255), (100, 254)):
        out, s = _check(np.array([[v]], dtype=np.int8))
        assert out["cost"][0, 0] == c and out["dist2"][0, 0] == (0 if v == 100 else vgpu.CLR_NONE)


def test_shapes_that_cross_tiles():
    """4: 1 x 300 and 300 x 1 (more than one workgroup of columns, more than one cell per thread of a row); 9000
    x 2 with obstacles only at its two ends, the longest search; the widest and the tallest legal grid; 257 x
    257 with a single centre obstacle against dx^2 + dy^2."""
    rng = np.random.default_rng(11)
    for shape in ((300, 1), (1, 300)):                               # [ny, nx]
        g = np.zeros(shape, dtype=np.int8)
        g.ravel()[rng.choice(300, size=5, replace=False)] = 100
        g.ravel()[rng.choice(300, size=40, replace=False)] -= 1      # unknown cells, and 99 (free) on an obstacle
        _check(g)
        _check(g, flags=1)
    g = np.zeros((2, 9000), dtype=np.int8)
    g[0, 0] = g[1, 8999] = 100
    out, s = _check(g)
    assert s["max_dist2"] == 4499 ** 2 + 1 and out["nearest"][1, 4499] == 0 and out["nearest"][0, 4500] == 9000 + 8999
    for shape in ((1, vgpu.CLR_MAX_SIDE), (vgpu.CLR_MAX_SIDE, 1)):
        g = np.zeros(shape, dtype=np.int8)
        g.ravel()[[0, 20000, 20003]] = 100
        out, s = _check(g)
        assert s["max_dist2"] == (vgpu.CLR_MAX_SIDE - 1 - 20003) ** 2
    g = np.zeros((257, 257), dtype=np.int8)
    g[128, 128] = 100
    out, s = _check(g, prm=FINE)
    iy, ix = np.mgrid[0:257, 0:257]
    assert np.array_equal(out["dist2"], (ix - 128) ** 2 + (iy - 128) ** 2) and (out["nearest"] == 128 * 257 + 128).all()
    assert s["max_dist2"] == 2 * 128 ** 2 and s["cells_inflated"] > 4000 and s["cells_free"] > 0


def test_nullable_outputs_and_determinism():
    """5: each output alone equals its plane of the full call; two identical calls and a call from a second
    context give identical bytes; want=() still gives the summary."""
    g = cr.random_grid(61, 47, 7)
    C = _ctx()
    full, s = C.clearance(g, flags=0, **NAV)
    for k in ("dist2", "nearest", "cost"):
        out, s1 = C.clearance(g, flags=0, want=(k,), **NAV)
        assert list(out) == [k] and out[k].tobytes() == full[k].tobytes() and s1 == s
    out, s1 = C.clearance(g, flags=0, want=(), **NAV)
    assert out == {} and s1 == s
    again, s2 = C.clearance(g, flags=0, **NAV)
    D = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    other, s3 = D.clearance(g, flags=0, **NAV)
    D.close()
    for k in full:
        assert again[k].tobytes() == full[k].tobytes() and other[k].tobytes() == full[k].tobytes()
    assert s2 == s and s3 == s
    assert C.clearance_ms() > 0.0


def test_chained_to_occupancy():
    """6: clearance(grid=None) after occupancy() equals clearance(grid=the returned grid); another nx, or a
    context without an occupancy call, is VG_E_STATE; a following occupancy() returns the bytes it returned
    before; the same from an attached tracker."""
    import test_occupancy_gpu as tog
    w = tog._work()
    M, geom = w["M"], w["geom"]
    prm = dict(cr.PARAMS["nav"])
    assert prm["res"] == geom["res"]

    def chain(c):
        grid, counts, summ = c.occupancy(w["pos"], w["dirs"], counts=True, **geom, **tog.BAND)
        assert grid.tobytes() == w["grid"].tobytes() and counts.tobytes() == w["counts"].tobytes() and summ == w["summ"]
        for flags in (0, 1):
            dev, sd = c.clearance(None, nx=geom["nx"], ny=geom["ny"], flags=flags, **prm)
            host, sh = c.clearance(grid, flags=flags, **prm)
            for k in dev:
                assert dev[k].tobytes() == host[k].tobytes(), k
            assert sd == sh and sd["n_obstacles"] == summ["cells_occupied"] + (summ["cells_unknown"] if flags else 0)
            assert sd["n_obstacles"] > 0 and sd["n_unknown"] == summ["cells_unknown"]
        ref = cr.clearance(grid, 1, **prm)
        assert all(dev[k].tobytes() == ref[k].tobytes() for k in ("dist2", "nearest"))
        with pytest.raises(vgpu.VgError) as ei:
            c.clearance(None, nx=geom["nx"] + 1, ny=geom["ny"], **prm)
        assert "(-5)" in str(ei.value)
        with pytest.raises(vgpu.VgError) as ei:
            c.clearance(None, nx=geom["ny"], ny=geom["nx"] - 1, **prm)
        assert "(-5)" in str(ei.value)
        grid2, counts2, summ2 = c.occupancy(w["pos"], w["dirs"], counts=True, **geom, **tog.BAND)
        assert grid2.tobytes() == w["grid"].tobytes() and counts2.tobytes() == w["counts"].tobytes() and summ2 == w["summ"]

    chain(M)
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    with pytest.raises(vgpu.VgError) as ei:                          # no occupancy call yet, a host grid or not before it
        T.clearance(None, nx=geom["nx"], ny=geom["ny"], **prm)
    assert "(-5)" in str(ei.value)
    T.clearance(w["grid"], **prm)
    with pytest.raises(vgpu.VgError) as ei:
        T.clearance(None, nx=geom["nx"], ny=geom["ny"], **prm)
    assert "(-5)" in str(ei.value)
    T.attach(M)
    chain(T)
    T.close()
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    with pytest.raises(vgpu.VgError) as ei:
        S.clearance(w["grid"], **prm)
    assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()


def test_replay_costmap(tmp_path):
    """7: vg_node_replay --occupancy P --costmap C writes C.pgm and C.yaml; the pgm's bytes are
    Context.clearance's cost of read_occupancy(P)'s grid with the same radii; without --occupancy it is refused."""
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
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    pre, cpre = str(tmp_path / "nav"), str(tmp_path / "cost")
    prm = cr.PARAMS["replay"]
    radii = ["--inscribed", prm["inscribed_radius"], "--inflation", prm["inflation_radius"], "--cost-scaling",
             prm["cost_scaling"]]
    run([log, tmp_path / "x.tum", "--map", ck, "--localize", "--guess", guess, "--costmap", cpre], rc=2)
    err = run([log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--occupancy", pre, "--occ-res",
               prm["res"], "--costmap", cpre] + radii)
    assert "costmap: " in err
    grid, x0, y0, res = vgpu.read_occupancy(pre)
    cost, cx0, cy0, cres = vgpu.read_costmap(cpre)
    assert (cx0, cy0, cres) == (x0, y0, res) and res == prm["res"] and cost.shape == grid.shape
    assert "image: cost.pgm" in open(cpre + ".yaml").read()
    want, s = _ctx().clearance(grid, **prm)
    cr.boundary_free(want["dist2"], prm)
    print("replay costmap %d x %d: %s" % (grid.shape[1], grid.shape[0], s))
    assert s["cells_lethal"] > 0 and s["cells_inflated"] > 0 and s["cells_no_info"] > 0
    assert ("%d obstacles, %d lethal, %d inscribed, %d inflated" % (s["n_obstacles"], s["cells_lethal"], s["cells_inscribed"],
                                                                    s["cells_inflated"])) in err
    assert cost.tobytes() == want["cost"].tobytes()
    assert np.array_equal(cost, cr.cost(grid, want["dist2"], **prm))


def test_argument_errors():
    """8: every VG_E_ARG condition returns it and writes nothing, neither an output nor the summary."""
    C = _ctx()
    L, P = vgpu.lib(), C.h
    nx, ny = 8, 5
    g = cr.random_grid(nx, ny, 3)
    d2, nr = np.full(nx * ny, -7, dtype=np.int32), np.full(nx * ny, -7, dtype=np.int32)
    co = np.full(nx * ny, 7, dtype=np.uint8)
    sm = vgpu.ClrSummary()

    def params(**kw):
        p = vgpu.ClrParams()
        for k, v in dict(dict(nx=nx, ny=ny, flags=0, **NAV), **kw).items():
            setattr(p, k, v)
        return p

    def call(ctx=P, grid=g.ctypes.data, prm=params(), out=sm):
        return L.vg_clearance(ctx, grid, None if prm is None else ctypes.byref(prm), d2.ctypes.data, nr.ctypes.data,
                              co.ctypes.data, None if out is None else ctypes.byref(out))

    nan, inf = float("nan"), float("inf")
    bad = [dict(ctx=None), dict(prm=None), dict(out=None)]
    for kw in (dict(nx=0), dict(ny=0), dict(nx=-4), dict(nx=vgpu.CLR_MAX_SIDE + 1, ny=1), dict(nx=1, ny=vgpu.CLR_MAX_SIDE + 1),
               dict(nx=4097, ny=4097), dict(res=0.0), dict(res=-0.25), dict(res=nan), dict(res=inf),
               dict(inscribed_radius=-0.1), dict(inscribed_radius=nan), dict(inflation_radius=inf), dict(inflation_radius=nan),
               dict(inscribed_radius=2.0), dict(inflation_radius=0.32), dict(cost_scaling=-1.0), dict(cost_scaling=nan),
               dict(cost_scaling=inf), dict(flags=2), dict(flags=3), dict(flags=-1),
               dict(res=0.001, inflation_radius=4.1)):               # a table of 4100^2 > 2^24 entries
        bad.append(dict(prm=params(**kw)))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert (d2 == -7).all() and (nr == -7).all() and (co == 7).all() and not bytes(sm).strip(b"\0"), kw
    assert call(prm=params(res=0.001, inflation_radius=4.0)) == 0    # 4000^2 < 2^24: legal, the table cut to the grid's reach
    assert call() == 0 and sm.n_obstacles == int((g == 100).sum()) and (d2 >= 0).all() and (nr >= 0).all()
    ref = cr.clearance(g, **NAV)
    assert np.array_equal(d2.reshape(ny, nx), ref["dist2"]) and np.array_equal(co.reshape(ny, nx), ref["cost"])
