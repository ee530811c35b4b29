"""Checkpoint and resume (vg_checkpoint_save / vg_checkpoint_load): a run that
is saved, destroyed, re-created and resumed produces the same bits as a run
that never stopped. No oracle: the uninterrupted device run is the reference.

Every test steps the 16-line synthetic sequence with the mid360 parameters at
max_points 100,000, max_nodes 400,000, max_fix_points 2,000,000, hash_log2 18:
the smallest workload with a full window, BA, margi, subdividing leaves and
abandoned point_fix blocks.

max_points (vg_capacity::max_points_per_scan) is the window arrays' slot
stride and part of the file's layout: a loader must use the saver's (else
VG_E_ARG). max_nodes, max_fix_points and hash_log2 are free (test 4).
"""
import os

import numpy as np
import pytest

import synth
import vgckpt
import vgconfig
import vgpu
from test_pipeline_gpu import COUNTERS

pytestmark = pytest.mark.gpu

CAP = dict(max_points=100_000, max_nodes=400_000, max_fix_points=2_000_000, hash_log2=18)
CAP_BIG = dict(max_points=100_000, max_nodes=800_000, max_fix_points=4_000_000, hash_log2=19)
N = 40


def _seq(seq_id=3):
    g = vgconfig.load("mid360")["General"]
    return synth.Sequence("16line", seq_id, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])


def _ctx(cap=CAP, **cfg):
    return vgpu.Context(vgconfig.to_c(vgconfig.load("mid360"), **cfg), **cap)


def _roots(ctx):
    """The root map, hash layout aside: sorted (key, jour stamp bit for bit, flags, subtree counts)."""
    return sorted((key, np.float64(v[0]).tobytes(), tuple(v[1:])) for key, v in ctx.roots().items())


def _step(ctx, seq, k):
    xyz, it, b, e = seq.scan(k)
    ctx.step(xyz, it, b, e, seq.imu(k))


def _run(ctx, seq, k0, k1, rec):
    """Scans [k0, k1): per scan the counters and the root map."""
    for k in range(k0, k1):
        _step(ctx, seq, k)
        s = ctx.stats()
        rec[k] = ({key: s[key] for key in COUNTERS}, _roots(ctx))


def _final(ctx):
    return ctx.trajectory(), ctx.path(), ctx.window_states(), ctx.state()


def _same_final(fa, fb):
    for x, y in zip(fa, fb):
        assert x.shape == y.shape and np.array_equal(x, y)


def _same_scans(ra, rb, k0, k1):
    for k in range(k0, k1):
        for key in COUNTERS:
            assert ra[k][0][key] == rb[k][0][key], (k, key, ra[k][0][key], rb[k][0][key])
        assert ra[k][1] == rb[k][1], (k, "root map")


@pytest.fixture(scope="module")
def ref():
    """The uninterrupted run A over scans 0..39 (shared, read-only)."""
    seq = _seq()
    A = _ctx()
    A.seed(seq.gt_state(0))
    rec = {}
    _run(A, seq, 0, N, rec)
    out = (seq, rec, _final(A))
    A.close()
    return out


@pytest.fixture(scope="module")
def file25(ref, tmp_path_factory):
    """B steps 0..24, saves, keeps stepping to 39 (test 2 reads its record); the file serves tests 1, 4, 5, 6."""
    seq = ref[0]
    path = str(tmp_path_factory.mktemp("ckpt") / "at25.vgck")
    B = _ctx()
    B.seed(seq.gt_state(0))
    rec = {}
    _run(B, seq, 0, 25, rec)
    nbytes = B.checkpoint_save(path)
    again = path + ".again"
    B.checkpoint_save(again)
    _run(B, seq, 25, N, rec)
    out = (path, nbytes, again, rec, _final(B))
    B.close()
    return out


def _resume(seq, path, k0, cap=CAP, used_scans=0):
    """A fresh (or used) context loads `path`, without seed, and steps k0..39."""
    C = _ctx(cap)
    for k in range(used_scans):
        if k == 0:
            C.seed(seq.gt_state(0))
        _step(C, seq, k)
    C.checkpoint_load(path)
    rec = {}
    fin0 = _final(C)
    _run(C, seq, k0, N, rec)
    out = (rec, _final(C), fin0)
    C.close()
    return out


def test_resume_is_invisible(ref, file25):
    """1: B' = load(file at 25) steps 25..39 as A did: counters, root map (jour
    stamps bit for bit) after every scan, trajectory (rows 0..24 included),
    path, window states and state."""
    seq, ra, fa = ref
    rb, fb, fin0 = _resume(seq, file25[0], 25)
    assert fin0[0].shape[0] == 25 and np.array_equal(fin0[0], fa[0][:25])  # the saved rows are there at once
    _same_scans(ra, rb, 25, N)
    _same_final(fa, fb)


@pytest.mark.parametrize("at", [11, 19, 20])
def test_resume_at_ring_and_jour_edges(ref, tmp_path, at):
    """1, repeated: the save right after the window first filled (11), and
    around the scans whose win_base + win_count reaches a multiple of 10 (the
    jour update runs in the margi of scan index 19 and 29: saves at 19 and 20
    put it right after and right before the resume). The loader is a context
    that has already stepped 3 scans (load has vg_reset semantics)."""
    seq, ra, fa = ref
    path = str(tmp_path / "edge.vgck")
    B = _ctx()
    B.seed(seq.gt_state(0))
    _run(B, seq, 0, at, {})
    B.checkpoint_save(path)
    B.close()
    rb, fb, _ = _resume(seq, path, at, used_scans=3)
    _same_scans(ra, rb, at, N)
    _same_final(fa, fb)


def test_saving_does_not_disturb_the_saver(ref, file25):
    """2: B went on stepping after its save at 25 and stays bit-identical to A."""
    seq, ra, fa = ref
    _same_scans(ra, file25[3], 0, N)
    _same_final(fa, file25[4])


def _release_run(seq, n, save_at=None, path=None, load=None, k0=0):
    """test_lifetime_gpu._det_run's shape: vg_release_far after every scan."""
    gpu = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360"), release_dis=3), max_points=100_000, max_nodes=400_000,
                       max_fix_points=8_000_000, hash_log2=18)
    if load:
        gpu.checkpoint_load(load)
    else:
        gpu.seed(seq.gt_state(0))
    rec = {}
    for k in range(k0, n):
        _step(gpu, seq, k)
        s = gpu.stats()
        roots = _roots(gpu)
        rec[k] = ({key: s[key] for key in COUNTERS}, gpu.release_far(), hash(tuple(roots)))
        if save_at == k:
            gpu.checkpoint_save(path)
    out = (rec, _final(gpu))
    gpu.close()
    return out


def test_resume_after_releases(tmp_path):
    """3: release_dis 3 m, sequence 5, 120 scans, vg_release_far after every
    scan on both sides; the save comes after the first release that erased
    roots, and a release erases roots after the load on both sides."""
    seq = _seq(5)
    path = str(tmp_path / "rel.vgck")
    ra, fa = _release_run(seq, 120)
    erased = [k for k in range(120) if ra[k][1][0] > 0]
    assert len(erased) >= 3, erased
    # the save follows the second erasing release in the same idle slot: that release has just
    # compacted, so the save's own compaction moves nothing and the census that vg_release_far
    # reports afterwards (arena used, out[5]) is the uninterrupted run's as well
    at = erased[1]
    rs, fs = _release_run(seq, at + 1, save_at=at, path=path)
    assert any(rs[k][1][0] > 0 for k in range(at + 1))  # a release erased roots before the save
    rb, fb = _release_run(seq, 120, load=path, k0=at + 1)
    for k in range(at + 1, 120):
        assert ra[k] == rb[k], (k, ra[k][:2], rb[k][:2])
    assert any(rb[k][1][0] > 0 for k in range(at + 1, 120))  # ... and one after the load
    _same_final(fa, fb)


def test_other_capacities(ref, file25, tmp_path):
    """4: the file loads into a context with twice the nodes / point_fix /
    hash and continues bit-identically; such a context run on the same scans
    writes a byte-identical file; saving twice in a row gives identical bytes."""
    seq, ra, fa = ref
    path, nbytes, again = file25[0], file25[1], file25[2]
    assert os.path.getsize(path) == nbytes
    data = open(path, "rb").read()
    assert data == open(again, "rb").read()
    rb, fb, _ = _resume(seq, path, 25, cap=CAP_BIG)
    _same_scans(ra, rb, 25, N)
    _same_final(fa, fb)
    big = _ctx(CAP_BIG)
    big.seed(seq.gt_state(0))
    _run(big, seq, 0, 25, {})
    p2 = str(tmp_path / "big.vgck")
    big.checkpoint_save(p2)
    big.close()
    assert open(p2, "rb").read() == data


def _mutations(data, tmp_path):
    h, cfg, tab, img = vgckpt.read(data)
    hb = int(h["head_bytes"])
    pl = [s for s in tab if vgckpt.NAMES[int(s["id"])] == "plane"][0]
    flip = bytearray(data)
    flip[hb + int(pl["off"]) + int(pl["bytes"]) // 2] ^= 0x40
    magic = bytearray(data)
    magic[0] ^= 0xFF
    out = {"flipped": bytes(flip), "truncated": data[: len(data) - 4096], "magic": bytes(magic)}
    paths = {}
    for name, b in out.items():
        paths[name] = str(tmp_path / (name + ".vgck"))
        open(paths[name], "wb").write(b)
    return paths


def test_rejections_leave_the_context_intact(ref, file25, tmp_path):
    """5: a flipped payload byte, a truncated file, a bad magic and a context
    with another voxel_size return VG_E_ARG, max_nodes below the file's node
    count VG_E_CAPACITY; vg_last_error names the check; the context, 15 scans
    in, then steps 15..24 as if it had never seen a load attempt."""
    seq, ra, fa = ref
    data = open(file25[0], "rb").read()
    bad = _mutations(data, tmp_path)
    names = {"flipped": "checksum", "truncated": "file length", "magic": "magic"}
    C = _ctx()
    C.seed(seq.gt_state(0))
    rec = {}
    _run(C, seq, 0, 15, rec)
    for name, word in names.items():
        with pytest.raises(vgpu.VgError) as ei:
            C.checkpoint_load(bad[name])
        assert "(-1)" in str(ei.value) and word in str(ei.value), (name, str(ei.value))
    _run(C, seq, 15, 25, rec)
    _same_scans(ra, rec, 0, 25)
    assert np.array_equal(C.trajectory(), fa[0][:25])
    C.close()
    # another configuration: VG_E_ARG (its own context: a different voxel_size steps differently anyway)
    p = vgconfig.load("mid360")
    p["Odometry"]["voxel_size"] = p["Odometry"]["voxel_size"] * 2
    D = vgpu.Context(vgconfig.to_c(p), **CAP)
    D.seed(seq.gt_state(0))
    d0, d1 = {}, {}
    _run(D, seq, 0, 15, d0)
    with pytest.raises(vgpu.VgError) as ei:
        D.checkpoint_load(file25[0])
    assert "(-1)" in str(ei.value) and "config" in str(ei.value), str(ei.value)
    _run(D, seq, 15, 25, d0)
    fd = _final(D)
    D.close()
    D2 = vgpu.Context(vgconfig.to_c(p), **CAP)
    D2.seed(seq.gt_state(0))
    _run(D2, seq, 0, 25, d1)
    _same_scans(d0, d1, 0, 25)
    _same_final(fd, _final(D2))
    D2.close()
    # too small: VG_E_CAPACITY
    h, _ = vgckpt.verify(data)
    small = dict(CAP, max_nodes=int(h["n_nodes"]) - 1)
    rec = {}
    try:
        E = _ctx(small)
        E.seed(seq.gt_state(0))
        _run(E, seq, 0, 15, rec)
    except vgpu.VgError:
        pytest.fail("max_nodes %d cannot hold the first 15 scans" % small["max_nodes"])
    with pytest.raises(vgpu.VgError) as ei:
        E.checkpoint_load(file25[0])
    assert "(-3)" in str(ei.value) and "capacity" in str(ei.value), str(ei.value)
    _run(E, seq, 15, 20, rec)
    _same_scans(ra, rec, 0, 20)
    E.close()


def test_checksum_pinned(file25):
    """6: every section's checksum recomputed with numpy matches the device's,
    and the section table adds up."""
    h, secs = vgckpt.verify(file25[0])
    n_nodes, n_fix = int(h["n_nodes"]), int(h["n_fix"])
    assert n_nodes > 0 and n_fix > 0
    for name in vgckpt.NODE_SECTIONS:
        assert secs[name][1] == n_nodes, name
    assert secs["fix_pnt"][1] == n_fix and secs["fix_var"][1] == n_fix
    wp = int(np.sum(h["wpn"]))
    assert wp > 0
    for name in vgckpt.WINDOW_SECTIONS:
        assert secs[name][1] == wp, name
    assert secs["root_id"][1] == int(h["n_roots"]) == secs["root_key"][1]
    assert secs["slide"][1] == int(h["n_slide"])
    ids = np.frombuffer(vgckpt.sections(file25[0])["root_id"][2], dtype="<i4")
    assert np.all(np.diff(ids) > 0)  # ordered by id: a function of the data, not of the append order


def test_outputs_survive(tmp_path):
    """7: /map_cmap and the marker events after a resume equal the
    uninterrupted run's (vg_set_publish(3) on A, set again on B' after the
    load); no deferral at the default marker capacity. A scan's events are
    compared as a sorted list of records, as tests/test_markers_gpu.py does:
    the collection appends them a wave at a time, in no defined order."""
    seq = _seq()
    path = str(tmp_path / "pub.vgck")

    def run(ctx, k0, k1, out):
        for k in range(k0, k1):
            _step(ctx, seq, k)
            mk, deferred = ctx.markers()
            assert deferred == 0
            out[k] = (ctx.local_map().copy(), sorted(r.tobytes() for r in mk))

    A = _ctx()
    A.seed(seq.gt_state(0))
    A.set_publish(3)
    oa = {}
    run(A, 0, 32, oa)
    A.close()
    B = _ctx()
    B.seed(seq.gt_state(0))
    B.set_publish(3)
    run(B, 0, 22, {})
    B.checkpoint_save(path)
    B.close()
    C = _ctx()
    C.checkpoint_load(path)
    C.set_publish(3)
    oc = {}
    run(C, 22, 32, oc)
    C.close()
    assert any(oa[k][0].shape[0] > 0 for k in range(22, 32))
    for k in range(22, 32):
        assert np.array_equal(oa[k][0], oc[k][0]), (k, "local map")
        assert oa[k][1] == oc[k][1], (k, "markers")


def test_state_errors(tmp_path):
    """8: VG_E_STATE on a sharded (world 2) context, inside an open
    stage-level scan and during a cold start's window phase; a cold-start
    context saved after init_phase 3 resumes bit-identically."""
    seq = _seq()
    path = str(tmp_path / "state.vgck")
    S = _ctx()
    S.shard_host(0, 2, lambda arr: None)
    with pytest.raises(vgpu.VgError) as ei:
        S.checkpoint_save(path)
    assert "(-5)" in str(ei.value) and "sharded" in str(ei.value)
    S.close()
    T = _ctx()
    T.seed(seq.gt_state(0))
    _step(T, seq, 0)
    xyz, it, b, e = seq.scan(1)
    T.scan_load(xyz, it)
    T.propagate(seq.imu(1), b, e)
    with pytest.raises(vgpu.VgError) as ei:
        T.checkpoint_save(path)
    assert "(-5)" in str(ei.value) and "scan is open" in str(ei.value)
    T.close()
    assert not os.path.exists(path)
    # cold start (tests/test_cold_start.py's first case): phase 2 refuses, phase 3 + 5 scans resume
    g = vgconfig.load("mid360")["General"]
    cs = synth.Sequence("16line", 0, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    cap = dict(max_points=200_000, max_nodes=1_000_000, max_fix_points=3_000_000, hash_log2=20)

    def cstep(ctx, k):
        xyz, it, tm, b, e = cs.scan_raw(k)
        ctx.step_deskew(xyz, it, tm, b, e, cs.imu(k))
        return ctx.stats()

    A = _ctx(cap, cold_start=1)
    B = _ctx(cap, cold_start=1)
    k, refused, k3 = 1, False, None
    while k3 is None and k <= 20:
        sa, sb = cstep(A, k), cstep(B, k)
        assert sa["init_phase"] == sb["init_phase"]
        if sb["init_phase"] == 2 and not refused:
            with pytest.raises(vgpu.VgError) as ei:
                B.checkpoint_save(path)
            assert "(-5)" in str(ei.value) and "cold-start" in str(ei.value)
            refused = True
        if sb["init_phase"] == 3:
            k3 = k
        k += 1
    assert refused and k3 is not None
    B.checkpoint_save(path)
    B.close()
    C = _ctx(cap, cold_start=1)
    C.checkpoint_load(path)
    for k in range(k3 + 1, k3 + 6):
        sa, sc = cstep(A, k), cstep(C, k)
        assert sc["init_phase"] == 0
        for key in COUNTERS:
            assert sa[key] == sc[key], (k, key)
    _same_final(_final(A), _final(C))
    A.close()
    C.close()
