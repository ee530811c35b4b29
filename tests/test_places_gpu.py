"""The place index on the device (vina_gpu.h "Place index"): place rows against
vg_raycast, the scan descriptor and the match against the numpy restatement
(tests/place_ref.py), global recovery without a position, failure and
lifetime. Workload: tests/loc_common.py; the lattice is 1 m over x in [-18, 18],
y in [-8, 8] at z = 1.5 (629 places)."""
import math

import numpy as np
import pytest

import loc_common as lc
import place_ref as pr
import synth
import vgconfig
import vgpu
from test_localize_gpu import ATE_BAR, ATE_MARGIN
from test_relocalize_gpu import ANG_BOUND, POS_BOUND, _errors

pytestmark = pytest.mark.gpu

YAW = math.radians(137.0)
TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
LATTICE = vgpu.place_lattice((-18.0, -8.0), (18.0, 8.0), 1.0, 1.5)
EIGHT = [0, 36, 300, 314, 328, 466, 592, 628]   # corners, centre row, the two true nodes' neighbourhood

_cache = {}


def _work():
    """{M: the frozen map with the full lattice's index, desc, hit}: built once, read-only afterwards."""
    if not _cache:
        M = lc.loaded(mapping=False)
        M.places_build(LATTICE)
        info = M.places_info(desc=True)
        _cache.update(M=M, desc=info["desc"].copy(), hit=info["hit_bins"].copy(), n_valid=info["n_valid"])
    return _cache


def _level(k):
    R, _ = lc.base()["seq"].gt_pose(k)
    return pr.rot_up(YAW) @ R


def _a_level(k):
    """A's attitude of row k re-yawed by +137 degrees."""
    return pr.rot_up(YAW) @ lc.pose_of_row(lc.base()["traj"][k])[:9].reshape(3, 3)


def test_place_rows_equal_the_raycaster():
    """1: rows = rint(512 range) of vg_raycast on the same origins and vg_places_dirs' directions, misses 0;
    hit_bins and validity; the same bytes alone, reversed and inside the full lattice."""
    w = _work()
    M = w["M"]
    p = pr.params()
    D = vgpu.places_dirs()
    pos = LATTICE[EIGHT]
    hits = M.raycast(np.repeat(pos, D.shape[0], axis=0), np.tile(D, (len(EIGHT), 1)), t_max=p["t_max"])
    rng = np.where(hits["flags"] & vgpu.RAY_HIT, hits["range"], 0.0)
    want = pr.quantise(rng).reshape(len(EIGHT), p["n_el"], p["n_az"])
    assert (want > 0).sum() > 0.3 * want.size
    assert np.array_equal(w["desc"][EIGHT], want)
    assert np.array_equal(w["hit"], pr.hit_bins(w["desc"]))
    assert w["n_valid"] == int((w["hit"] >= p["min_bins"]).sum()) and w["n_valid"] > 600
    B = lc.loaded(mapping=False)
    B.places_build(pos)
    a = B.places_info(desc=True)
    B.places_build(pos[::-1])              # replaces the index
    b = B.places_info(desc=True)
    B.close()                              # vg_destroy ends the index
    assert a["M"] == 8 and a["desc"].tobytes() == want.tobytes() and b["desc"][::-1].tobytes() == want.tobytes()
    assert np.array_equal(a["hit_bins"], w["hit"][EIGHT]) and np.array_equal(b["hit_bins"][::-1], w["hit"][EIGHT])


def test_scan_descriptor_equals_numpy():
    """2: vg_places_scan on scan 31 against place_ref, the points within 1e-9 rad of a bin edge or 1e-9 m
    of t_max left out of both sides; order independence; the edge shapes."""
    M = _work()["M"]
    s = lc.base()["seq"]
    eR, _ = lc.ext()
    p = pr.params()
    xyz = s.scan(31)[0]
    Rl = _level(31)
    skip = pr.edge_mask(xyz, Rl, eR, p)
    share = skip.mean()
    print("points left out near a bin edge: %d of %d (%.4f %%)" % (skip.sum(), xyz.shape[0], 100 * share))
    assert share <= 0.001
    d, n = M.places_scan(xyz, Rl)
    rd, rn = pr.scan_descriptor(xyz, Rl, eR, p)
    b_all = pr.scan_bins(xyz, Rl, eR, p)[0]
    touched = np.zeros(p["n_az"] * p["n_el"], dtype=bool)
    touched[b_all[skip & (b_all >= 0)]] = True
    if skip.any():   # a left-out point may sit in the neighbouring bin on the device
        A = p["n_az"]
        for b in b_all[skip & (b_all >= 0)]:
            e, a = divmod(int(b), A)
            for ee in (e - 1, e, e + 1):
                for aa in (a - 1, a, a + 1):
                    if 0 <= ee < p["n_el"]:
                        touched[ee * A + aa % A] = True
    ok = ~touched.reshape(p["n_el"], p["n_az"])
    assert ok.sum() >= 0.99 * ok.size and (rn > 0).sum() > 500
    assert np.array_equal(n[ok], rn[ok]) and np.array_equal(d[ok], rd[ok])
    d2, n2 = M.places_scan(xyz[::-1], Rl)
    assert d2.tobytes() == d.tobytes() and n2.tobytes() == n.tobytes()
    # n = 0
    d0, n0 = M.places_scan(np.zeros((0, 3), np.float32), Rl)
    assert not d0.any() and not n0.any()
    assert M.places_query(np.zeros((0, 3), np.float32), Rl).shape[0] == 0
    # n = 1; all points in one bin; 257 points (one full workgroup and one lane)
    for cloud in (xyz[:1], np.repeat(xyz[100:101], 1000, axis=0), xyz[:257]):
        dd, nn = M.places_scan(cloud, Rl)
        r1, r2 = pr.scan_descriptor(cloud, Rl, eR, p)
        assert np.array_equal(dd, r1) and np.array_equal(nn, r2) and nn.sum() > 0
    assert M.places_scan(np.repeat(xyz[100:101], 1000, axis=0), Rl)[1].max() == 1000


def test_scan_descriptor_at_the_bin_limit():
    """2, A E = 4096: 32 KB of LDS per workgroup in k_place_scan."""
    s = lc.base()["seq"]
    eR, _ = lc.ext()
    B = lc.loaded(mapping=False)
    kw = dict(n_az=128, n_el=32)
    B.places_build(LATTICE[EIGHT[:2]], **kw)
    p = pr.params(**kw)
    xyz = s.scan(31)[0][:5000]
    Rl = _level(31)
    skip = pr.edge_mask(xyz, Rl, eR, p)
    d, n = B.places_scan(xyz[~skip], Rl)
    rd, rn = pr.scan_descriptor(xyz[~skip], Rl, eR, p)
    B.close()
    assert d.shape == (32, 128) and np.array_equal(n, rn) and np.array_equal(d, rd) and rn.sum() > 2000


def _check_match(C, desc, hit, xyz, Rl, p, top_k=16):
    eR, _ = lc.ext()
    cand, scores = C.places_query(xyz, Rl, top_k=top_k, scores=True)
    sd, _ = C.places_scan(xyz, Rl)          # the device's own scan descriptor
    want = pr.match_scores(desc, sd, int(round(p["clip"] * pr.Q)))
    valid = hit >= p["min_bins"]
    assert np.array_equal(scores[valid], want[valid].astype(np.int32))
    assert np.all(scores[~valid] == vgpu.PLACE_NONE)
    top = pr.top_k(want, valid, top_k)       # best and second-best per place by the tie rules, then the order
    got = [(int(c["score"]), int(c["place"]), int(c["shift"])) for c in cand]
    assert got == top, (got[:4], top[:4])
    assert all(valid[c["place"]] for c in cand)
    nv = int((sd > 0).sum())
    for c in cand:
        assert c["n_valid"] == nv and np.array_equal(c["pos"], C_pos(C, c["place"]))
        assert c["yaw"] == 2.0 * math.pi * c["shift"] / p["n_az"]
    return cand


_positions = {}


def C_pos(C, i):
    return _positions[id(C)][i]


def test_match_equals_numpy():
    """3: scores_all (629 x 120) = place_ref's integer scores of the device's own descriptors; the per-place
    best / second-best shifts and the top-k order; invalid places never returned."""
    w = _work()
    M = w["M"]
    _positions[id(M)] = LATTICE
    p = pr.params()
    xyz = lc.base()["seq"].scan(31)[0]
    cand = _check_match(M, w["desc"], w["hit"], xyz, _level(31), p, top_k=40)
    assert cand.shape[0] == 40
    # an index with invalid places: four of the eight lie 200 m outside the map
    pos = LATTICE[EIGHT].copy()
    pos[::2, 0] += 200.0
    B = lc.loaded(mapping=False)
    B.places_build(pos)
    _positions[id(B)] = pos
    info = B.places_info(desc=True)
    assert info["n_valid"] == 4 and np.all(info["hit_bins"][::2] < p["min_bins"])
    cand = _check_match(B, info["desc"], info["hit_bins"], xyz, _level(31), p, top_k=64)
    assert cand.shape[0] == 8 and set(cand["place"]) == {1, 3, 5, 7}
    B.close()


@pytest.mark.parametrize("kw", [dict(n_az=64), dict(n_az=65), dict(n_az=256), dict(n_el=1)])
def test_match_edge_shapes(kw):
    """3: A = 64 (one wave exactly), 65, 256; E = 1."""
    p = pr.params(**kw)
    B = lc.loaded(mapping=False)
    pos = LATTICE[EIGHT]
    B.places_build(pos, **kw)
    _positions[id(B)] = pos
    info = B.places_info(desc=True)
    assert info["desc"].shape == (8, p["n_el"], p["n_az"])
    _check_match(B, info["desc"], info["hit_bins"], lc.base()["seq"].scan(31)[0][::3], _level(31), p)
    B.close()


def _rank_of_true_node(C, xyz, Rl, k):
    s = lc.base()["seq"]
    _, et = lc.ext()
    R, t = s.gt_pose(k)
    org = t + R @ et
    near = int(np.argmin(np.linalg.norm(LATTICE[:, :2] - org[:2], axis=1)))
    cand = C.places_query(xyz, Rl, top_k=64)
    ranks = [i for i, c in enumerate(cand) if c["place"] == near]
    rank = ranks[0] + 1 if ranks else None
    print("scan %d: true lattice node %d at rank %s of vg_places_query (best: place %d shift %d score %d)" %
          (k, near, rank, cand[0]["place"], cand[0]["shift"], cand[0]["score"]))
    return rank


def test_global_recovery_and_install():
    """4: scan 31 with A's attitude re-yawed by +137 degrees and no position: ok, the pose within
    test_relocalize_gpu's bounds of A's row 31, and the next 10 frozen scans keep test_localize_gpu's ATE
    bound. Scan 45 in the at-30 map: ok and within one coarse step (0.25 m, 2.5 degrees) of A's row 45."""
    b = lc.base()
    s = b["seq"]
    B = lc.loaded(mapping=False)
    B.places_build(LATTICE)
    xyz = s.scan(lc.K0)[0]
    ref = lc.pose_of_row(b["traj"][lc.K0])
    rank = _rank_of_true_node(B, xyz, _a_level(lc.K0), lc.K0)
    pose, rec, cand, ok = B.relocalize_global(xyz, _a_level(lc.K0), top_k=16, install=True)
    dp, da = _errors(pose, ref)
    print("global relocalise, scan 31: position error %.6f m, angle error %.6f deg, matches %d of %d, place %d yaw %.1f deg"
          % (dp, math.degrees(da), rec["matches"], xyz.shape[0], cand["place"], math.degrees(cand["yaw"])))
    assert rank is not None and rank <= 16
    assert ok and rec["matches"] >= 0.5 * xyz.shape[0]
    assert dp <= POS_BOUND and da <= ANG_BOUND, (dp, math.degrees(da))
    st = B.state()
    assert np.array_equal(st[1:13], pose)
    assert np.array_equal(st[25:250].reshape(15, 15), np.diag([1e-4] * 9 + [1e-5] * 6))
    for k in range(lc.K0 + 1, lc.K0 + 11):
        lc.step(B, s, k)
    tb = B.trajectory()[-10:]
    ta = b["traj"][lc.K0 + 1:lc.K0 + 11]
    gt = lc.gt_traj(s, lc.K0 + 1, lc.K0 + 11)
    ate_a, ate_b = synth.ate(ta, gt), synth.ate(tb, gt)
    print("after install: ATE mapping %.6f m, ATE frozen %.6f m" % (ate_a, ate_b))
    assert ate_b <= ate_a * ATE_MARGIN and ate_b <= ATE_BAR, (ate_a, ate_b)
    B.close()
    C = lc.loaded(mapping=False)
    C.places_build(LATTICE)
    xyz = s.scan(45)[0]
    ref = lc.pose_of_row(b["traj"][45])
    rank = _rank_of_true_node(C, xyz, _a_level(45), 45)
    pose, rec, cand, ok = C.relocalize_global(xyz, _a_level(45), top_k=16)
    dp, da = _errors(pose, ref)
    print("global relocalise, scan 45 in the at-30 map: position error %.6f m, angle error %.6f deg, matches %d of %d"
          % (dp, math.degrees(da), rec["matches"], xyz.shape[0]))
    C.close()
    assert rank is not None and rank <= 16
    assert ok and dp <= 0.25 and da <= math.radians(2.5), (dp, math.degrees(da))


def _refused(fn, *a, **kw):
    with pytest.raises(vgpu.VgError) as ei:
        fn(*a, **kw)
    assert "(-5)" in str(ei.value), str(ei.value)


def test_failure_and_lifetime(tmp_path):
    """5: no valid place: ok = 0 with VG_OK and the state bit for bit; what the index rules out on its owner;
    an attached tracker gets the owner's result bit for bit; VG_E_STATE after the end."""
    b = lc.base()
    s = b["seq"]
    xyz = s.scan(lc.K0)[0]
    Rl = _a_level(lc.K0)
    C = lc.loaded()
    _refused(C.places_build, LATTICE[:4])                 # mapping is on
    C.set_mapping(False)
    far = LATTICE[EIGHT].copy()
    far[:, 0] += 200.0
    C.places_build(far)
    assert C.places_info()["n_valid"] == 0
    before = C.state()
    pose, rec, cand, ok = C.relocalize_global(xyz, Rl, install=True)
    assert not ok and cand["place"] == -1 and np.array_equal(C.state(), before)
    assert C.places_query(xyz, Rl).shape[0] == 0
    _refused(C.set_mapping, True)
    _refused(C.checkpoint_load, b["path"])
    _refused(C.reset)
    with pytest.raises(vgpu.VgError) as ei:
        C.places_query(xyz, Rl, top_k=0)
    assert "(-1)" in str(ei.value)
    C.places_end()
    _refused(C.places_query, xyz, Rl)
    _refused(C.places_end)
    C.set_mapping(True)
    C.reset()
    C.checkpoint_load(b["path"])
    C.set_mapping(False)
    # the map's own path as the places: LiDAR origins at least 1 m apart
    pos = C.places_from_path(1.0)
    assert pos.shape[0] >= 3 and C.places_info()["M"] == pos.shape[0]
    assert np.all(np.linalg.norm(np.diff(pos, axis=0), axis=1) >= 1.0)
    assert C.places_query(xyz, Rl, top_k=4).shape[0] == 4
    # an attached tracker with tiny capacities reads the owner's index
    C.places_build(LATTICE)
    before = C.state()
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    T.attach(C)
    _refused(T.places_build, LATTICE[:4])
    _refused(T.places_end)
    own = C.relocalize_global(xyz, Rl, top_k=8)
    got = T.relocalize_global(xyz, Rl, top_k=8, install=True)
    assert own[3] and got[3]
    assert np.array_equal(own[0], got[0]) and own[1] == got[1] and own[2].tobytes() == got[2].tobytes()
    assert np.array_equal(T.state()[1:13], got[0]) and np.array_equal(C.state(), before)
    assert T.places_info()["M"] == LATTICE.shape[0]
    C.places_end()
    _refused(T.places_query, xyz, Rl)
    T.close()
    C.close()


def test_replay_global(tmp_path):
    """6: vg_node_replay --map ... --localize --global on test_node_core's event log (the log format the
    tool reads) reaches the same first pose as --guess with the true pose, within test 4's bounds;
    --global --guess is refused."""
    import os
    import subprocess

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
    run([log, tmp_path / "x.tum", "--map", ck, "--localize", "--global", "--guess", guess], rc=2)
    run([log, tmp_path / "x.tum", "--global"], rc=2)
    err_g = run([log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess])
    err_p = run([log, tmp_path / "p.tum", "--map", ck, "--localize", "--global"])
    print(err_p.strip())
    assert "relocalise: ok" in err_g and "relocalise: ok" in err_p
    line = [ln for ln in err_p.splitlines() if ln.startswith("relocalise: global place ")]
    assert len(line) == 1 and len(line[0].split()) == 8
    a, b = synth.read_tum(str(tmp_path / "g.tum")), synth.read_tum(str(tmp_path / "p.tum"))
    back = np.flatnonzero(np.diff(a[:, 0]) <= 0)              # the map's own rows come first; then time restarts
    assert a.shape == b.shape and back.shape[0] == 1
    n0 = int(back[0]) + 1
    assert np.array_equal(a[:n0], b[:n0])
    ra, rb = a[n0], b[n0]                                     # the first localised scan
    dp = float(np.linalg.norm(ra[1:4] - rb[1:4]))
    da = 2.0 * math.acos(min(1.0, abs(float(np.dot(ra[4:8], rb[4:8])))))
    print("replay: first pose --global vs --guess: %.6f m, %.6f deg" % (dp, math.degrees(da)))
    assert dp <= POS_BOUND and da <= ANG_BOUND, (dp, math.degrees(da))
