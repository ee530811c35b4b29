"""vg_score_poses (csrc/score.hip): OctoTree::match for one scan under many
poses. Checked against the IEKF's own first-iteration match count, against
the map snapshot per point in numpy float64, for batch independence, at the
edges, and for discrimination around the true pose. Workload:
tests/loc_common.py (the map after scan 30, scan 31's cloud)."""
import math

import numpy as np
import pytest

import loc_common as lc
import vgpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def w():
    """A loaded context, scan 31's cloud, A's pose of scan 31, the map before any scoring."""
    b = lc.base()
    c = lc.loaded()
    xyz = b["seq"].scan(lc.K0)[0]
    out = dict(ctx=c, xyz=xyz, pose=lc.pose_of_row(b["traj"][lc.K0]), roots=lc.roots(c), planes=lc.planes(c), base=b)
    yield out
    c.close()


def _perturbed(pose, rng, k, dp=0.3, da=0.05):
    """k poses around `pose`: position +- dp m, a rotation of up to da rad about a random axis."""
    out = np.tile(pose, (k, 1))
    for i in range(k):
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        a = rng.uniform(-da, da)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rd = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * K @ K
        out[i, :9] = (Rd @ pose[:9].reshape(3, 3)).reshape(9)
        out[i, 9:] += rng.uniform(-dp, dp, size=3)
    return out


def test_matches_equal_the_iekf(w):
    """5: on a stage-level twin the propagated state (vg_get_state inside the
    open scan reads the device's x_curr after the opening: host_mirror.cpp
    host_state) and its covariance blocks go into score_poses with K = 1;
    matches == iekf_matches[0] of that scan, exactly. The cloud is the one the
    IEKF reads: VNC_lio runs on the full scan (local_mapping.cpp:408-413), not
    on the downsampled one, so scan 31 itself is scored."""
    b = w["base"]
    s = b["seq"]
    T = lc.loaded()
    xyz, it, beg, end = s.scan(lc.K0)
    T.scan_load(xyz, it)
    T.propagate(s.imu(lc.K0), beg, end)
    T.downsample_scan()
    st = T.state()
    cov = st[25:250].reshape(15, 15)
    pv = np.concatenate([cov[0:3, 0:3].reshape(9), cov[3:6, 3:6].reshape(9)])
    rec = T.score_poses(xyz, st[1:13], pose_var=pv)  # inside the open scan
    T.lio_state_estimation()
    T.step_end()
    m0 = T.stats()["iekf_matches"][0]
    T.close()
    assert m0 > 0 and m0 == b["stats"][lc.K0]["iekf_matches"][0]
    assert int(rec["matches"][0]) == m0, (int(rec["matches"][0]), m0)


def test_per_point_against_snapshot(w):
    """6: every matched record's leaf is looked up in map_planes(all_nodes);
    r = n.(w - c) recomputed in float64 agrees to 1e-12 m (one dot product of
    O(10 m) operands: ~1e-15 x 10 m, with headroom), the point lies inside the
    leaf's cube, and the record's sums equal math.fsum over the per-point
    records to 1e-12 relative (summation order only, n <= ~1e4 terms)."""
    c, xyz, pose = w["ctx"], w["xyz"], w["pose"]
    rec, pp = c.score_poses(xyz, pose, per_point=True)
    rec = rec[0]
    lv = c.map_planes()  # the plane leaves: disjoint cubes, found through voxel_center / quater_length
    vc, hl = lv["voxel_center"], 2 * lv["quater_length"]
    eR, et = lc.ext()
    R, p = pose[:9].reshape(3, 3), pose[9:]
    wld = (R @ (eR @ xyz.astype(np.float64).T + et[:, None])).T + p
    m = np.nonzero(pp["flag"])[0]
    assert m.size > 100 and m.size == int(rec["matches"])
    assert int(rec["in_map"]) == int((pp["leaf"] >= 0).sum()) >= m.size
    nn = np.zeros((m.size, 3))
    node_of = {}
    for j, i in enumerate(m):
        inside = np.nonzero(np.all(np.abs(wld[i] - vc) <= hl[:, None], axis=1))[0]
        assert inside.size >= 1, i  # the point lies inside a plane leaf's cube
        rs = np.einsum("ij,ij->i", lv["normal"][inside], wld[i] - lv["center"][inside])
        k = int(np.argmin(np.abs(rs - pp["r"][i])))  # (a point on a shared face lies in two cubes)
        assert abs(rs[k] - pp["r"][i]) <= 1e-12, (i, rs[k], pp["r"][i])
        q = int(inside[k])
        assert node_of.setdefault(int(pp["leaf"][i]), q) == q  # one node id, one snapshot leaf
        assert pp["sigma_d"][i] > 0
        nn[j] = lv["normal"][q]
    assert len(set(node_of.values())) == len(node_of)
    rel = lambda a, ref: abs(a - ref) <= 1e-12 * max(abs(ref), 1e-300)
    assert rel(rec["cost"], math.fsum(pp["r"][m] ** 2 / (0.0005 + pp["sigma_d"][m])))
    assert rel(rec["sum_abs"], math.fsum(np.abs(pp["r"][m])))
    for k, (a, bb) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        ref = math.fsum(nn[:, a] * nn[:, bb])
        assert abs(rec["nn"][k] - ref) <= 1e-12 * m.size, (k, rec["nn"][k], ref)
    assert np.all(pp["r"][pp["flag"] == 0] == 0)


def test_batch_independence_and_determinism(w):
    """7: K = 130 poses, the true pose among random perturbations: a pose's
    record is bit-identical scored alone, at positions 0, 63, 64 and 129 of a
    batch, and in a second identical call."""
    c, xyz, pose = w["ctx"], w["xyz"], w["pose"]
    rng = np.random.default_rng(7)
    P = _perturbed(pose, rng, 130)
    P[17] = pose
    full = c.score_poses(xyz, P)
    assert full.tobytes() == c.score_poses(xyz, P).tobytes()
    assert int(full["matches"][17]) == int(full["matches"].max())
    for i in (0, 17, 63, 64, 129):
        alone = c.score_poses(xyz, P[i])
        assert alone[0].tobytes() == full[i].tobytes(), i
        for pos in (0, 63, 64, 129):
            Q = P.copy()
            Q[pos] = P[i]
            assert c.score_poses(xyz, Q)[pos].tobytes() == full[i].tobytes(), (i, pos)


def test_edges(w):
    """8: prefixes n in {0, 1, 63, 64, 65, 257} agree with the full cloud's
    per-point records; K in {1, 2, 65, 4096}; an empty map and a cloud 5,000 km
    away give zeros with VG_OK; bad arguments give VG_E_ARG; the map is
    untouched by all of it (and by every test above)."""
    c, xyz, pose = w["ctx"], w["xyz"], w["pose"]
    _, pp = c.score_poses(xyz, pose, per_point=True)
    for n in (0, 1, 63, 64, 65, 257):
        r = c.score_poses(xyz[:n], pose)[0]
        f = pp["flag"][:n] != 0
        assert int(r["matches"]) == int(f.sum()) and int(r["in_map"]) == int((pp["leaf"][:n] >= 0).sum()), n
        ref = math.fsum(np.abs(pp["r"][:n][f]))
        assert abs(r["sum_abs"] - ref) <= 1e-12 * max(ref, 1e-300), n
        if n:
            _, q = c.score_poses(xyz[:n], pose, per_point=True)
            assert q.tobytes() == pp[:n].tobytes(), n
    one = c.score_poses(xyz, pose)[0]
    for K in (1, 2, 65, 4096):
        r = c.score_poses(xyz, np.tile(pose, (K, 1)))
        assert r.shape == (K,) and all(r[i].tobytes() == one.tobytes() for i in (0, K // 2, K - 1)), K
    zero = np.zeros(1, dtype=vgpu.POSE_SCORE_DTYPE)[0].tobytes()
    E = lc.ctx()
    assert E.score_poses(xyz, pose)[0].tobytes() == zero  # an empty map
    E.close()
    far = xyz + np.float32(5.0e6)
    assert c.score_poses(far, pose)[0].tobytes() == zero  # |key| >= 2^20: not in the map, no VG_E_RANGE
    L = vgpu.lib()
    rec = np.zeros(2, dtype=vgpu.POSE_SCORE_DTYPE)
    x32 = np.ascontiguousarray(xyz, dtype=np.float32)
    args = lambda n, K, xp=vgpu._f(x32), pp_=None: L.vg_score_poses(c.h, xp, n, vgpu._d(np.tile(pose, (2, 1))), K, None,
                                                                   rec.ctypes.data, pp_)
    assert args(10, 0) == -1 and args(10, -3) == -1 and args(-1, 1) == -1 and args(10, 1, xp=None) == -1
    assert args(10, 2, pp_=rec.ctypes.data) == -1  # per_point with K != 1
    assert L.vg_score_poses(c.h, vgpu._f(x32), 10, None, 1, None, rec.ctypes.data, None) == -1
    assert L.vg_score_poses(c.h, vgpu._f(x32), 10, vgpu._d(pose.copy()), 1, None, None, None) == -1
    assert L.vg_score_poses(c.h, vgpu._f(x32), 10, vgpu._d(pose.copy()), 65537, None, rec.ctypes.data, None) == -1
    lc.same_map(c, w["roots"], w["planes"])


def test_discrimination(w):
    """9: a 2-D grid of +-2 m x +-2 m at 0.25 m around scan 31's pose
    (sequence id 3): the arg-max of matches is the centre cell or one of its
    8 neighbours."""
    c, xyz, pose = w["ctx"], w["xyz"], w["pose"]
    g = np.arange(-8, 9) * 0.25
    P = np.tile(pose, (g.size * g.size, 1))
    P[:, 9] += np.repeat(g, g.size)
    P[:, 10] += np.tile(g, g.size)
    r = c.score_poses(xyz, P)
    k = int(np.argmax(r["matches"]))
    ix, iy = k // g.size - 8, k % g.size - 8
    print("discrimination: arg-max cell (%d, %d), matches %d, centre %d" % (ix, iy, r["matches"][k],
                                                                        r["matches"][8 * g.size + 8]))
    assert abs(ix) <= 1 and abs(iy) <= 1, (ix, iy)
