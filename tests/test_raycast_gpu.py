"""vg_raycast on the GPU against the brute-force restatement of its hit
definition (tests/raycast_ref.py) on the localisation tests' map (loc_common:
the 16-line sequence 3 after scan 30): equality on a 2,048-ray fan, degenerate
rays, determinism and placement, where it runs, and the fan against the scene."""
import numpy as np
import pytest

import loc_common as lc
import raycast_ref as rr
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
VS = 0.5   # Odometry.voxel_size of the mid360 parameters
# test 5: |range - true| of the numpy reference over the fan's rays that hit both the map and the
# scene, as measured on the MI355X ("Ray-casting the map")
SCENE_MEDIAN, SCENE_P95 = 0.0112, 4.07   # (the tail: leaf planes reach past the panels' edges)


def _hit(h):
    return (h["flags"] & vgpu.RAY_HIT) != 0


def test_equals_brute_force():
    """1: every ray's hit / miss equals the reference's, |range - range_ref| <= 1e-9 m, and node ids
    and snapshot leaves correspond one to one (the snapshot carries no node id: the hit point must
    lie in the reference leaf's cube). Left out: rays with a candidate within 1e-7 m of a cube
    face (reference side), at most 0.5 %."""
    w = rr.workload()
    g, (t, idx, near) = w["hits"], w["ref"]
    planes = w["planes"]
    n = g.shape[0]
    assert n == 2048 and planes.shape[0] > 1000
    print("excluded share %.4f %% (%d rays), hits %d of %d" % (100.0 * near.mean(), near.sum(), _hit(g).sum(), n))
    assert near.mean() <= 0.005
    keep = ~near
    assert np.array_equal(_hit(g)[keep], np.isfinite(t)[keep])
    both = keep & _hit(g)
    assert both.sum() > 500   # the fan sees the map
    assert np.abs(g["range"][both] - t[both]).max() <= 1e-9
    assert not (g["flags"] & (vgpu.RAY_TRUNCATED | vgpu.RAY_INVALID | vgpu.RAY_LEFT_RANGE)).any()
    node_of, leaf_of = {}, {}
    d = w["d"]
    for i in np.flatnonzero(both):
        q, leaf = int(idx[i]), int(g["leaf"][i])
        assert node_of.setdefault(leaf, q) == q and leaf_of.setdefault(q, leaf) == leaf, i
        h = w["o"] + g["range"][i] * d[i]
        assert np.all(np.abs(h - planes["voxel_center"][q]) <= 2.0 * planes["quater_length"][q] + 1e-9), i
        nn = g["normal"][i] / np.linalg.norm(g["normal"][i])
        assert np.abs(nn - planes["normal"][q]).max() < 1e-12 and abs(g["ndotd"][i] - g["normal"][i] @ d[i]) < 1e-12
        assert g["var"][i] >= 0.0
    miss = ~_hit(g)
    assert not g["range"][miss].any() and (g["leaf"][miss] == -1).all()


def _check_valid(w, o, d, rec, **prm):
    """The lattice cases' properties: a returned hit lies on its leaf's plane and in its cube, and
    the reference has no valid candidate nearer by more than 1e-7 m; a miss: the reference has none
    that is clear of every cube face."""
    planes = w["planes"]
    t, idx, near = rr.cast(planes, o, d, **prm)
    dn = d / np.linalg.norm(d)
    if _hit(rec):
        h = o + rec["range"] * dn
        on = np.abs(np.einsum("ij,ij->i", planes["normal"], h[None, :] - planes["center"])) < 1e-9
        inside = np.all(np.abs(h[None, :] - planes["voxel_center"]) <= 2.0 * planes["quater_length"][:, None] + 1e-9, axis=1)
        assert (on & inside).any()
        assert not (t[0] < rec["range"] - 1e-7)
    else:
        assert np.isinf(t[0]) or near[0]


def test_degenerate_rays():
    """2: none may truncate or hang."""
    w = rr.workload()
    M, o0 = w["M"], w["o"]
    assert M.raycast(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)
    flags_bad = vgpu.RAY_TRUNCATED | vgpu.RAY_INVALID
    # axis-parallel directions, n = 1 each
    for d in np.vstack([np.eye(3), -np.eye(3), [[1.0, 1.0, 0.0], [0.0, -1.0, 2.0]]]):
        rec = M.raycast(o0, d[None, :])[0]
        assert not (rec["flags"] & flags_bad), d
        _check_valid(w, o0, d, rec)
    # an origin exactly on a root-cell corner
    corner = np.round(o0 / VS) * VS
    for d in ([1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0], [1.0, -1.0, 0.0]):
        d = np.array(d)
        rec = M.raycast(corner, d[None, :])[0]
        assert not (rec["flags"] & flags_bad), d
        _check_valid(w, corner, d, rec)
    # an origin inside a plane leaf past its plane: the plane behind is not returned
    i = int(np.flatnonzero(_hit(w["hits"]) & ~w["ref"][2])[0])
    d = d_i = w["d"][i]
    o_past = o0 + (w["hits"]["range"][i] + 1e-3) * d
    rec = M.raycast(o_past, d[None, :])[0]
    assert not (rec["flags"] & flags_bad)
    assert not _hit(rec) or rec["leaf"] != w["hits"]["leaf"][i]
    _check_valid(w, o_past, d, rec)
    # t_max shorter than the first cell; t_min past the first hit
    rec = M.raycast(o0, d[None, :], t_max=1e-3)[0]
    assert rec["flags"] == 0 and rec["leaf"] == -1
    rec = M.raycast(o0, d[None, :], t_min=w["hits"]["range"][i])[0]
    assert not (rec["flags"] & flags_bad) and (not _hit(rec) or rec["range"] > w["hits"]["range"][i])
    # an origin outside the key range; a ray that leaves it
    rec = M.raycast(np.array([VS * 2.0 ** 20 + 1.0, 0.0, 0.0]), np.array([[1.0, 0.0, 0.0]]))[0]
    assert rec["flags"] == vgpu.RAY_LEFT_RANGE and rec["leaf"] == -1
    rec = M.raycast(np.array([VS * 2.0 ** 20 - 1.0, 0.3, 0.3]), np.array([[1.0, 0.0, 0.0]]))[0]
    assert rec["flags"] == vgpu.RAY_LEFT_RANGE and rec["leaf"] == -1
    # a zero direction, a NaN origin, a NaN and an infinite direction
    for o, d in ((o0, [0.0, 0.0, 0.0]), ([np.nan, 0.0, 0.0], [1.0, 0.0, 0.0]), (o0, [np.nan, 1.0, 0.0]),
                 (o0, [np.inf, 0.0, 0.0]), ([np.inf, 0.0, 0.0], [1.0, 0.0, 0.0])):
        rec = M.raycast(np.array(o), np.array([d]))[0]
        assert rec["flags"] == vgpu.RAY_INVALID and rec["leaf"] == -1 and rec["range"] == 0.0
    # max_steps = 3 on a long ray
    rec = M.raycast(o0, d_i[None, :], max_steps=3)[0]
    assert rec["flags"] & vgpu.RAY_TRUNCATED and not _hit(rec) and rec["leaf"] == -1 and rec["range"] == 0.0
    # n = 257 (a block's tail): the fan's first 257 rays
    part = M.raycast(o0, w["d"][:257])
    assert part.tobytes() == w["hits"][:257].tobytes()


def test_determinism_and_placement():
    """3: a ray's record has the same bytes alone, in the batch, in the reversed batch, with a
    shared or a per-ray origin, and in a batch of more than one slab."""
    w = rr.workload()
    M, o, d, g = w["M"], w["o"], w["d"], w["hits"]
    assert M.raycast(o, d).tobytes() == g.tobytes()
    assert M.raycast(o, d[100:101])[0].tobytes() == g[100].tobytes()
    assert M.raycast(o, d[::-1])[::-1].tobytes() == g.tobytes()
    assert M.raycast(np.tile(o, (d.shape[0], 1)), d).tobytes() == g.tobytes()
    reps = 2 * lc.CAP["max_points"] // d.shape[0] + 1   # 200,704 rays over a 100,000-ray slab
    big = M.raycast(o, np.tile(d, (reps, 1)))
    assert big.shape[0] > 2 * lc.CAP["max_points"] and big.tobytes() == np.tile(g, reps).tobytes()
    per = np.tile(o, (d.shape[0], 1)) + np.arange(d.shape[0])[:, None] * 1e-3   # per-ray origins across slabs
    a = M.raycast(np.tile(per, (reps, 1)), np.tile(d, (reps, 1)))
    assert a.tobytes() == np.tile(M.raycast(per, d), reps).tobytes()


def test_where_it_runs():
    """4: the frozen loaded context, the mapping context at the same map state, an attached
    tiny-capacity tracker and that tracker in a fleet return the same bytes; the map is untouched;
    an empty context misses everywhere; argument errors."""
    w = rr.workload()
    M, o, d, g = w["M"], w["o"], w["d"], w["hits"]
    snap = (lc.roots(M), lc.planes(M))
    A = lc.loaded(mapping=True)
    assert A.raycast(o, d).tobytes() == g.tobytes()
    lc.same_map(A, *snap)
    A.close()
    E = lc.ctx()
    e = E.raycast(o, d)
    assert not e["flags"].any() and (e["leaf"] == -1).all() and not e["range"].any()
    E.close()
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    T.attach(M)
    assert T.raycast(o, d).tobytes() == g.tobytes()
    F = vgpu.Fleet(M, [T])
    assert T.raycast(o, d).tobytes() == g.tobytes()
    F.close()
    L, P = vgpu.lib(), M.h
    out = np.zeros(4, dtype=vgpu.RAY_HIT_DTYPE)
    oo, dd = np.zeros((4, 3)), np.ones((4, 3))
    for args in ((None, 1, vgpu._d(dd), 4, None, out.ctypes.data), (vgpu._d(oo), 1, None, 4, None, out.ctypes.data),
                 (vgpu._d(oo), 1, vgpu._d(dd), 4, None, None), (vgpu._d(oo), 1, vgpu._d(dd), -1, None, out.ctypes.data),
                 (vgpu._d(oo), 2, vgpu._d(dd), 4, None, out.ctypes.data), (vgpu._d(oo), 0, vgpu._d(dd), 4, None, out.ctypes.data)):
        assert L.vg_raycast(P, *args) == -1, args
    assert L.vg_raycast(None, vgpu._d(oo), 1, vgpu._d(dd), 4, None, out.ctypes.data) == -1
    assert L.vg_raycast(P, vgpu._d(oo), 4, vgpu._d(dd), 4, None, out.ctypes.data) == 0
    lc.same_map(M, *snap)
    lc.same_map(T, *snap)
    T.close()


def test_against_the_scene():
    """5 (characterisation): the numpy reference's ranges against the scene's true ranges over the
    fan's rays that hit both. Centimetres, from range_sigma = 0.02 and the leaves' extents; the
    factor 2 is there because the value depends on the map's noise, not on the kernel (test 1 pins
    the GPU to the reference)."""
    w = rr.workload()
    t = w["ref"][0]
    true, _ = lc.base()["seq"].scene.cast(w["o"], w["d"])
    both = np.isfinite(t) & np.isfinite(true)
    err = np.abs(t[both] - true[both])
    print("reference vs scene over %d rays: median %.4f m, p95 %.4f m" % (both.sum(), np.median(err), np.percentile(err, 95)))
    assert both.sum() > 500
    assert np.median(err) < 2.0 * SCENE_MEDIAN
