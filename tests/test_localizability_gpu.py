"""vg_localizability and vg_scan_info (vina_gpu.h "Localisability") against the
numpy restatement of their sums over vg_raycast's records (tests/info_ref.py),
on the localisation tests' map (loc_common: the 16-line sequence 3 after scan
30, frozen) with the mid360 parameters: the definition, the eigen outputs,
degenerate shapes, determinism and placement, the scan form, where it runs, and
the replay tool's --scan-info. The layout checks at the top need no device."""
import ctypes
import math

import numpy as np
import pytest

import info_ref as ir
import loc_common as lc
import raycast_ref as rr
import vgconfig
import vgpu

gpu = pytest.mark.gpu

TINY = dict(max_points=100_000, max_nodes=1024, max_fix_points=1024, hash_log2=10)
DIRS = {96: dict(n_az=24, n_el=4), 777: dict(n_az=111, n_el=7)}   # 777: no multiple of the wave or the block

_cache = {}


# ---- host only

def test_record_layout(tmp_path):
    """vg_info_rec is 416 bytes and vg_info_params 112, field for field the header's, in the ctypes
    structures and the numpy record type alike; the flag constants are the header's."""
    from test_abi import _c_layout
    assert ctypes.sizeof(vgpu.InfoRec) == 416 and vgpu.INFO_REC_DTYPE.itemsize == 416
    assert ctypes.sizeof(vgpu.InfoParams) == 112
    for struct, cls in (("vg_info_rec", vgpu.InfoRec), ("vg_info_params", vgpu.InfoParams)):
        names = [f for f, _ in cls._fields_]
        size, offs = _c_layout(tmp_path, struct, names)
        assert ctypes.sizeof(cls) == size and [getattr(cls, f).offset for f in names] == offs
    names = [f for f, _ in vgpu.InfoRec._fields_]
    assert list(vgpu.INFO_REC_DTYPE.names) == names
    assert [vgpu.INFO_REC_DTYPE.fields[f][1] for f in names] == [getattr(vgpu.InfoRec, f).offset for f in names]
    hdr = open(vgpu.HEADER).read()
    for name, v in (("VALID", vgpu.INFO_VALID), ("ROT_DEGENERATE", vgpu.INFO_ROT_DEGENERATE),
                    ("TRANS_DEGENERATE", vgpu.INFO_TRANS_DEGENERATE), ("RAY_ENDED", vgpu.INFO_RAY_ENDED)):
        assert "#define VG_INFO_%s %d\n" % (name, v) in hdr


def test_params_and_null_context():
    """info_params leaves every field the caller does not name at zero (the library's defaults), and
    both calls refuse a NULL context without touching a device."""
    p = vgpu.info_params()
    assert bytes(p) == bytes(112)
    p = vgpu.info_params(floor_var=1e-4, min_hits=7, t_max=40.0)
    assert (p.floor_var, p.min_hits, p.ray.t_max, p.ray.min_cos, p.pad) == (1e-4, 7, 40.0, 0.0, 0)
    L = vgpu.lib()
    out = np.zeros(1, dtype=vgpu.INFO_REC_DTYPE)
    d = np.ones((4, 3))
    assert L.vg_localizability(None, vgpu._d(d), 1, vgpu._d(d), 4, None, out.ctypes.data) == -1
    assert L.vg_scan_info(None, None, 0, None, None, None, out.ctypes.data) == -1


# ---- the GPU tests' shared workload

def _origins():
    """8 LiDAR origins p + R ext_t of the ground-truth trajectory, scans 5..30."""
    g = lc.gt_traj(lc.base()["seq"], 5, 31)
    ext_t = lc.ext()[1]
    rows = g[np.linspace(0, g.shape[0] - 1, 8).astype(int)]
    return np.array([row[10:13] + row[1:10].reshape(3, 3) @ ext_t for row in rows])


def _work():
    """{M: the frozen loaded context (never closed: shared), pos: the 8 origins, dirs / rec / ref per D}:
    computed once, read-only afterwards."""
    if not _cache:
        M = lc.loaded(mapping=False)
        pos = _origins()
        dirs, rec, ref = {}, {}, {}
        for D, bins in DIRS.items():
            dirs[D] = vgpu.places_dirs(**bins)
            assert dirs[D].shape == (D, 3)
            rec[D] = M.localizability(pos, dirs[D])
            ref[D] = [ir.place_ref(M, o, dirs[D]) for o in pos]
        _cache.update(M=M, pos=pos, dirs=dirs, rec=rec, ref=ref)
    return _cache


def _check_H(H, H_ref, n_terms, what):
    err, lim = np.abs(H - H_ref), ir.bound(H_ref, n_terms)
    print("%s: max |H - ref| / bound = %.4f" % (what, (err / np.maximum(lim, 1e-300)).max()))
    assert np.all(err <= lim), (what, err, lim)


@gpu
def test_equals_the_definition():
    """1: H, n_hits and sum_w of 8 places at D = 96 and D = 777 against the fsum of the terms recomputed
    from the device's own vg_raycast records of the same M D rays: counts exact, |H_ij - ref_ij| <= (D + 32)
    2^-52 sqrt(H_ii H_jj), H equal to its transpose bitwise."""
    w = _work()
    for D in DIRS:
        for k, (r, (H, n_hits, sum_w, hits)) in enumerate(zip(w["rec"][D], w["ref"][D])):
            assert r["n_rays"] == D and r["n_hits"] == n_hits and n_hits > D // 8, (D, k, r["n_hits"], n_hits)
            assert r["H"].tobytes() == np.ascontiguousarray(r["H"].T).tobytes()
            _check_H(r["H"], H, D, "D %d place %d" % (D, k))
            assert abs(r["sum_w"] - sum_w) <= (D + 32) * ir.EPS * sum_w
            ended = (hits["flags"] & (vgpu.RAY_TRUNCATED | vgpu.RAY_LEFT_RANGE)).any()
            assert bool(r["flags"] & vgpu.INFO_RAY_ENDED) == bool(ended)
            assert r["flags"] & vgpu.INFO_VALID and r["reserved"] == 0.0 and r["pad"] == 0


def _sign_rule(v):
    k = int(np.argmax(np.abs(v)))
    return v[k] > 0.0


@gpu
def test_eigen_outputs():
    """2: eig_t / eig_r against numpy.linalg.eigvalsh of the Schur complements of the device's H, |d lambda|
    <= 1e-9 lambda_max, over the valid, non-degenerate records whose H_tt and H_pp numpy conditions
    below 1e6 (at least half of them); dir_t is unit, follows the sign rule and is S_t's eigenvector."""
    w = _work()
    used = total = 0
    for D in DIRS:
        for r in w["rec"][D]:
            total += 1
            if r["flags"] & (vgpu.INFO_ROT_DEGENERATE | vgpu.INFO_TRANS_DEGENERATE) or not r["flags"] & vgpu.INFO_VALID:
                continue
            H = r["H"]
            ct, cp = np.linalg.cond(H[3:, 3:]), np.linalg.cond(H[:3, :3])
            if not (ct < 1e6 and cp < 1e6):
                continue
            used += 1
            S_t, S_r = ir.schur(H)
            for S, eig, dr in ((S_t, r["eig_t"], r["dir_t"]), (S_r, r["eig_r"], r["dir_r"])):
                ev = np.linalg.eigvalsh(0.5 * (S + S.T))
                assert np.abs(eig - ev).max() <= 1e-9 * ev[2], (eig, ev)
                assert eig[0] <= eig[1] <= eig[2]
                assert abs(np.linalg.norm(dr) - 1.0) <= 1e-12 and _sign_rule(dr)
                assert np.abs(S @ dr - eig[0] * dr).max() <= 1e-9 * ev[2]
    print("eigen outputs checked on %d of %d records" % (used, total))
    assert 2 * used >= total


def _one_plane_fan(M, o):
    """64 directions within 0.5 degrees of one that all hit one leaf from o (None: no such direction)."""
    _, cand = rr.fan(np.concatenate([np.eye(3).reshape(9), o]), np.zeros(3), n_az=64, n_el=16)
    h = M.raycast(o, cand)
    order = [i for i in np.argsort(h["range"]) if h["flags"][i] & vgpu.RAY_HIT][:256]
    a = np.deg2rad(np.linspace(-0.35, 0.35, 8))   # an 8 x 8 grid: at most 0.35 sqrt(2) = 0.495 degrees off
    fans = []
    for i in order:
        d = cand[i]
        u = np.cross(d, [0.0, 0.0, 1.0])
        u /= np.linalg.norm(u)
        v = np.cross(d, u)
        A, B = np.meshgrid(a, a)
        fans.append(d[None, :] + np.tan(A).reshape(-1, 1) * u[None, :] + np.tan(B).reshape(-1, 1) * v[None, :])
    rec = M.raycast(o, np.concatenate(fans)).reshape(len(order), 64)
    for f, r in zip(fans, rec):
        if (r["flags"] & vgpu.RAY_HIT).all() and (r["leaf"] == r["leaf"][0]).all():
            return f
    return None


@gpu
def test_degenerate_and_edge_shapes():
    """3: an origin far from the map; a fan on one plane; D = 1 and D = 4096; a NaN direction; M = 0;
    argument errors."""
    w = _work()
    M, pos = w["M"], w["pos"]
    d96 = w["dirs"][96]
    far = M.localizability(pos[:1] + [500.0, 0.0, 0.0], d96)[0]
    assert far["n_hits"] == 0 and far["n_rays"] == 96 and not far["flags"] & vgpu.INFO_VALID
    assert not far["H"].any() and not far["eig_t"].any() and not far["eig_r"].any() and far["sum_w"] == 0.0
    # the default min_hits is 16; a bar above the hits clears the valid bit and the eigen outputs, not H
    r0 = w["rec"][96][0]
    assert M.localizability(pos[:1], d96, min_hits=16)[0].tobytes() == r0.tobytes()
    low = M.localizability(pos[:1], d96, min_hits=int(r0["n_hits"]) + 1)[0]
    assert not low["flags"] & vgpu.INFO_VALID and low["H"].tobytes() == r0["H"].tobytes()
    assert low["n_hits"] == r0["n_hits"] and not low["eig_t"].any() and not low["dir_r"].any()
    # one plane: neither block has full rank. Both bits are set, eig_t is H_pp's (one direction), eig_r zero
    fan = _one_plane_fan(M, pos[3])
    assert fan is not None
    r = M.localizability(pos[3:4], fan)[0]
    assert r["n_hits"] == 64 and r["flags"] & vgpu.INFO_VALID and r["flags"] & vgpu.INFO_ROT_DEGENERATE
    assert r["flags"] & vgpu.INFO_TRANS_DEGENERATE
    assert r["eig_t"][2] > 0.0 and r["eig_t"][0] <= 1e-9 * r["eig_t"][2] and r["eig_t"][1] <= 1e-9 * r["eig_t"][2]
    assert not r["eig_r"].any() and not r["dir_r"].any()
    # D = 1, and D = 4096 with M = 1
    one = M.localizability(pos[:1], d96[40:41])[0]
    h1 = M.raycast(pos[0], d96[40:41])[0]
    assert one["n_rays"] == 1 and one["n_hits"] == int(bool(h1["flags"] & vgpu.RAY_HIT)) and not one["flags"] & vgpu.INFO_VALID
    d4096 = vgpu.places_dirs(n_az=256, n_el=16)
    big = M.localizability(pos[:1], d4096)[0]
    H, n_hits, sum_w, _ = ir.place_ref(M, pos[0], d4096)
    assert big["n_rays"] == 4096 and big["n_hits"] == n_hits
    _check_H(big["H"], H, 4096, "D 4096")
    # a NaN direction is an invalid ray. Last of 96: the others keep their lanes, H has the bytes of the
    # first 95 alone. In the middle: the others' sums, against the reference
    d = d96.copy()
    d[95] = np.nan
    a, b = M.localizability(pos[:1], d)[0], M.localizability(pos[:1], d96[:95])[0]
    assert a["H"].tobytes() == b["H"].tobytes() and a["n_hits"] == b["n_hits"] and a["n_rays"] == 96
    d = d96.copy()
    d[40] = [np.nan, 1.0, 0.0]
    a = M.localizability(pos[:1], d)[0]
    H, n_hits, sum_w, _ = ir.place_ref(M, pos[0], np.delete(d96, 40, axis=0))
    assert a["n_hits"] == n_hits
    _check_H(a["H"], H, 96, "NaN direction")
    nan_o = M.localizability([[np.nan, 0.0, 0.0]], d96)[0]
    assert nan_o["n_hits"] == 0 and not nan_o["H"].any()
    # M = 0; argument errors
    assert M.localizability(np.zeros((0, 3)), d96).shape == (0,)
    L, P = vgpu.lib(), M.h
    out = np.zeros(8, dtype=vgpu.INFO_REC_DTYPE)
    pp, dd = vgpu._d(pos), vgpu._d(d4096)
    assert L.vg_localizability(P, None, 0, dd, 96, None, None) == 0
    for args in ((pp, 8, dd, 0, None, out.ctypes.data), (pp, 8, dd, 4097, None, out.ctypes.data),
                 (None, 8, dd, 96, None, out.ctypes.data), (pp, 8, None, 96, None, out.ctypes.data),
                 (pp, 8, dd, 96, None, None), (pp, -1, dd, 96, None, out.ctypes.data)):
        assert L.vg_localizability(P, *args) == -1, args
    assert L.vg_localizability(P, pp, 8, dd, 96, None, out.ctypes.data) == 0


@gpu
def test_determinism_and_placement():
    """4: a place's record has the same bytes in a second call, in the reversed batch, among 1000 places
    and on either side of a slab boundary (the slab set to 5 places through the test hook)."""
    w = _work()
    M, pos, d, g = w["M"], w["pos"], w["dirs"][96], w["rec"][96]
    assert M.localizability(pos, d).tobytes() == g.tobytes()
    assert M.localizability(pos[::-1], d)[::-1].tobytes() == g.tobytes()
    big = M.localizability(np.tile(pos, (125, 1)), d)
    assert big.shape == (1000,) and big.tobytes() == np.tile(g, 125).tobytes()
    M.info_slab(5)
    try:
        assert M.localizability(pos, d).tobytes() == g.tobytes()
        assert M.localizability(pos, w["dirs"][777]).tobytes() == w["rec"][777].tobytes()
    finally:
        M.info_slab(0)
    assert M.localizability(pos, d).tobytes() == g.tobytes()


@gpu
def test_scan_info():
    """5: scan 35's downsampled cloud at A's trajectory pose: n_hits is vg_scan_diff's CONSISTENT count, H
    within test 1's bound (the scan's n for D) of the fsum over vg_scan_diff's per-point records and
    vg_raycast of the same beams; two calls give the same bytes; n = 0 gives a zero record."""
    M = _work()["M"]
    s = lc.base()["seq"]
    pose = lc.pose_of_row(lc.base()["traj"][35])
    xyz, inten = s.scan(35)[:2]
    ds = np.ascontiguousarray(M.downsample(xyz, inten, 0.1)[:, :3])
    n = ds.shape[0]
    assert n > 1000
    summ, pp = M.scan_diff(ds, pose, per_point=True)
    rec = M.scan_info(ds, pose)
    assert rec["n_rays"] == n and rec["n_hits"] == summ["n"][vgpu.DIFF_CONSISTENT] and rec["n_hits"] > n // 2
    ext_R, ext_t = lc.ext()
    o, dv, _ = rr.beams(ds, pose, ext_R, ext_t)
    hits = M.raycast(o, dv)
    use = pp["cls"] == vgpu.DIFF_CONSISTENT
    assert np.array_equal(hits["leaf"][use], pp["leaf"][use])   # the beam's hit is the one the class came from
    H, n_hits, sum_w = ir.info_sum(*ir.terms(hits, dv, pp["r_meas"], use=use))
    assert n_hits == rec["n_hits"]
    _check_H(rec["H"], H, n, "scan 35")
    assert abs(rec["sum_w"] - sum_w) <= (n + 32) * ir.EPS * sum_w
    assert rec["H"].tobytes() == np.ascontiguousarray(rec["H"].T).tobytes() and rec["flags"] & vgpu.INFO_VALID
    assert M.scan_info(ds, pose).tobytes() == rec.tobytes()
    # the eigen outputs follow the same finish as the places'
    assert not rec["flags"] & (vgpu.INFO_ROT_DEGENERATE | vgpu.INFO_TRANS_DEGENERATE)
    if np.linalg.cond(rec["H"][3:, 3:]) < 1e6 and np.linalg.cond(rec["H"][:3, :3]) < 1e6:
        S_t, S_r = ir.schur(rec["H"])
        for S, eig in ((S_t, rec["eig_t"]), (S_r, rec["eig_r"])):
            ev = np.linalg.eigvalsh(0.5 * (S + S.T))
            assert np.abs(eig - ev).max() <= 1e-9 * ev[2]
    zero = M.scan_info(np.zeros((0, 3), dtype=np.float32), pose)
    assert zero.tobytes() == bytes(416)
    out = np.zeros(1, dtype=vgpu.INFO_REC_DTYPE)
    L = vgpu.lib()
    assert L.vg_scan_info(M.h, None, 5, None, None, None, out.ctypes.data) == -1
    assert L.vg_scan_info(M.h, vgpu._f(ds), n, None, None, None, None) == -1
    assert L.vg_scan_info(M.h, vgpu._f(ds), lc.CAP["max_points"] + 1, None, None, None, out.ctypes.data) == -1


@gpu
def test_where_it_runs():
    """6: an attached tracker with tiny capacities and a mapping-on context at the same map state give the
    owner's bytes for the same places and the same scan; the map is bit-identical before and after; a
    sharded context is refused with VG_E_STATE."""
    w = _work()
    M, pos, d, g = w["M"], w["pos"], w["dirs"][96], w["rec"][96]
    snap = (lc.roots(M), lc.planes(M))
    s = lc.base()["seq"]
    pose = lc.pose_of_row(lc.base()["traj"][35])
    xyz, inten = s.scan(35)[:2]
    ds = np.ascontiguousarray(M.downsample(xyz, inten, 0.1)[:, :3])
    scan = M.scan_info(ds, pose)
    A = lc.loaded(mapping=True)
    assert A.localizability(pos, d).tobytes() == g.tobytes() and A.scan_info(ds, pose).tobytes() == scan.tobytes()
    lc.same_map(A, *snap)
    A.close()
    T = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), **TINY)
    T.attach(M)
    assert T.localizability(pos, d).tobytes() == g.tobytes() and T.scan_info(ds, pose).tobytes() == scan.tobytes()
    lc.same_map(M, *snap)
    lc.same_map(T, *snap)
    T.close()
    S = lc.ctx()
    S.shard_host(0, 2, lambda arr: None)
    for fn in (lambda: S.localizability(pos, d), lambda: S.scan_info(ds, pose)):
        with pytest.raises(vgpu.VgError) as ei:
            fn()
        assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()


@gpu
def test_replay_scan_info(tmp_path):
    """7: vg_node_replay --map ... --localize --scan-info on test_node_core's event log prints one
    parsable scan_info line per localised scan (as many as --scan-diff prints), each with n_hits > 0."""
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
        return r.stdout

    ck = tmp_path / "map.vgck"
    run([log, tmp_path / "a.tum", 0, tmp_path / "a.path", "--checkpoint-out", ck, "--checkpoint-at", 12])
    run([log, tmp_path / "x.tum", "--scan-info"], rc=2)
    R0, p0 = seq.gt_pose(0)
    guess = "%r %r %r %r" % (float(p0[0]), float(p0[1]), float(p0[2]), math.atan2(R0[1, 0], R0[0, 0]))
    out = run([log, tmp_path / "g.tum", "--map", ck, "--localize", "--guess", guess, "--scan-diff", "--scan-info"])
    info = [ln.split() for ln in out.splitlines() if ln.startswith("scan_info ")]
    diff = [ln.split() for ln in out.splitlines() if ln.startswith("scan_diff ")]
    print("\n".join(" ".join(f) for f in info[:3]))
    assert len(info) >= 1 and len(info) == len(diff)
    for k, (f, dfl) in enumerate(zip(info, diff)):
        assert len(f) == 9 and int(f[1]) == k and f[2] == dfl[2]
        n_hits, v = int(f[3]), [float(x) for x in f[4:]]
        assert n_hits > 0 and n_hits == int(dfl[5])              # the CONSISTENT count of the same cloud and pose
        assert all(math.isfinite(x) for x in v)
        assert v[0] > 0.0 and v[4] > 0.0 and abs(math.sqrt(v[1] ** 2 + v[2] ** 2 + v[3] ** 2) - 1.0) < 1e-6
