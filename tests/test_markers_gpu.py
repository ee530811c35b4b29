"""The map's /voxel_plane + /voxel_normal markers (vg_set_publish bit 1,
vg_markers, vg_map_planes; csrc/markers.hip) on the 16-line synthetic sequence
with the mid360 parameters: the device's marker math at its branch points
against tests/marker_ref.py, the per-scan event stream against a replay of map
snapshots under the reference's rule (octree.cpp:761-850), the whole-scan path
against the stage path, publication off against never enabled, the pool
compaction and vg_reset, the bounded event buffer, and the ABI."""
import ctypes

import numpy as np
import pytest

import marker_ref as mr
import synth
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu
CAP = dict(max_points=100_000, max_nodes=400_000, max_fix_points=2_000_000, hash_log2=18)
SEQ_ID = 3
NSCAN = 40
RAW = ("voxel_center", "quater_length", "center", "normal", "eig", "trace", "layer")


def _params():
    return vgconfig.load("mid360")


def _seq(p):
    g = p["General"]
    return synth.Sequence("16line", SEQ_ID, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])


def _ctx(p, seq, publish=2, capacity=None, release_dis=1_000_000):
    c = vgpu.Context(vgconfig.to_c(p, release_dis=release_dis), **CAP)
    if capacity:
        c.marker_capacity(capacity)
    if publish:
        c.set_publish(publish)
    c.seed(seq.gt_state(0))
    return c


def _key(r):
    return (r["voxel_center"].tobytes(), int(r["layer"]))


def _bytes_set(rec):
    return sorted(r.tobytes() for r in rec)


def _stage_scan(c, seq, k, W):
    """One scan through the stage API; the map snapshot at the reference's collection point."""
    xyz, it, beg, end = seq.scan(k)
    imu = seq.imu(k)
    c.scan_load(xyz, it)
    c.propagate(imu, beg, end)
    c.downsample_scan()
    c.lio_state_estimation()
    c.window_push(imu)
    c.cut_voxel_multi()
    c.multi_recut()
    snap = c.map_planes(all_nodes=True)
    if c.win_count() >= W:
        c.damping_iter()
        c.multi_margi()
    c.step_end()
    return snap


def _run_stage(capacity=None, n=NSCAN):
    p = _params()
    seq = _seq(p)
    c = _ctx(p, seq, capacity=capacity)
    W = p["LocalBA"]["win_size"]
    snaps, events, deferred = [], [], []
    for k in range(n):
        snaps.append(_stage_scan(c, seq, k, W))
        ev, d = c.markers()
        events.append(ev.copy())
        deferred.append(d)
    out = dict(snaps=snaps, events=events, deferred=deferred, stats=c.stats_log(), traj=c.trajectory())
    c.close()
    return out


def _run_step(publish=2, n=NSCAN, toggle_at=None, compact_every=0, read=True, then=None, release_dis=1_000_000,
              compact=True):
    p = _params()
    seq = _seq(p)
    c = _ctx(p, seq, publish=publish, release_dis=release_dis)
    events, rel = [], []
    for k in range(n):
        if toggle_at is not None and k == toggle_at:
            c.set_publish(2)
        xyz, it, beg, end = seq.scan(k)
        c.step(xyz, it, beg, end, seq.imu(k))
        if read:
            events.append(c.markers()[0].copy())
        if compact_every and k % compact_every == compact_every - 1:
            r = c.release_far(compact=compact)
            assert release_dis < 1_000_000 or r[0] in (-1, 0)
            rel.append(r)
    out = dict(rel=rel, events=events, stats=c.stats_log(), traj=c.trajectory(), win=c.window_states(), path=c.path())
    if then:
        out["then"] = then(c, seq)
    c.close()
    return out


@pytest.fixture(scope="module")
def stage_run():
    return _run_stage()


@pytest.fixture(scope="module")
def step_run():
    return _run_step()


def _plane_bits(r):
    return r["center"].tobytes() + r["normal"].tobytes()


def _model(snaps, max_layer):
    """The reference's flags replayed over the snapshots: per scan the expected
    {key: action}, the published set after it, and the nodes whose plane
    changed since the previous snapshot."""
    prev, flags, out = {}, {}, []
    for snap in snaps:
        cur = {_key(r): r for r in snap}
        assert len(cur) == snap.shape[0], "a (voxel_center, layer) key twice in one snapshot"
        changed = 0
        for key, r in cur.items():
            if key in prev:
                dirty = _plane_bits(prev[key]) != _plane_bits(r)
            else:
                dirty = bool(np.any(r["center"] != 0) or np.any(r["normal"] != 0))
            if dirty:
                changed += 1
                f = flags.setdefault(key, [False, False])
                f[0] = True
        expect = {}
        for key, r in cur.items():
            fl = int(r["flags"])
            if not (fl & 4) or int(r["layer"]) > max_layer:
                continue
            f = flags.setdefault(key, [False, False])
            is_plane, octo = bool(fl & 1), bool(fl & 2)
            if not octo:
                if not is_plane and f[1]:
                    expect[key] = 2
                    f[0] = f[1] = False
                elif is_plane and f[0]:
                    expect[key] = 0
                    f[0], f[1] = False, True
            elif f[1]:
                expect[key] = 2
                f[0] = f[1] = False
        out.append(dict(expect=expect, published={k for k, f in flags.items() if f[1]}, changed=changed, cur=cur))
        prev = cur
    return out


def _check_adds_against_snapshot(ev, cur, k):
    adds = ev[ev["action"] == 0]
    for r in adds:
        s = cur[_key(r)]
        for f in RAW:
            assert r[f].tobytes() == s[f].tobytes(), (k, f)
        assert (int(r["flags"]) & 7) == (int(s["flags"]) & 7) == 5, (k, int(r["flags"]), int(s["flags"]))
    if adds.shape[0]:
        mr.check_derived(adds, mr.evaluate(mr.inputs_of_records(adds)), "scan %d" % k)
    return adds.shape[0]


def test_marker_math_at_branch_points():
    """Test 1: vgx_marker_eval on the hand-built inputs against the numpy restatement."""
    p = _params()
    c = vgpu.Context(vgconfig.to_c(p), max_points=10_000, max_nodes=10_000, max_fix_points=10_000, hash_log2=12)
    a = mr.branch_inputs()
    rec = c.marker_eval(a)
    c.close()
    ref = mr.evaluate(a)
    assert ref["rgba_unsafe"].mean() <= 0.01
    assert (rec["action"] == 0).all() and (rec["flags"] == 0).all()
    for f, col in (("voxel_center", slice(0, 3)), ("center", slice(5, 8)), ("eig", slice(12, 15))):
        assert np.array_equal(rec[f], a[:, col])
    assert np.array_equal(rec["trace"], a[:, 11]) and np.array_equal(rec["quater_length"], a[:, 4])
    mr.check_derived(rec, ref, "branch points")


def test_event_stream_equals_snapshot_replay(stage_run):
    """Test 2: per scan the emitted events equal the reference's rule applied to
    the snapshots; the replayed stream leaves exactly the model's published set."""
    max_layer = _params()["LocalBA"]["max_layer"]
    model = _model(stage_run["snaps"], max_layer)
    shown, n_add, n_del = {}, 0, 0
    for k, (ev, m) in enumerate(zip(stage_run["events"], model)):
        got = {}
        for r in ev:
            assert _key(r) not in got, (k, "a node emitted twice")
            got[_key(r)] = int(r["action"])
        print("scan %d: %d ADD %d DELETE, %d nodes, plane_updates %d" % (
            k, sum(1 for a in got.values() if a == 0), sum(1 for a in got.values() if a == 2), len(m["cur"]),
            stage_run["stats"][k]["plane_updates"]))
        assert got == m["expect"], (k, len(got), len(m["expect"]))
        n_add += _check_adds_against_snapshot(ev, m["cur"], k)
        for r in ev:
            if r["action"] == 0:
                shown[_key(r)] = r
            else:
                n_del += 1
                assert _key(r) in shown, (k, "DELETE of a marker never shown")
                del shown[_key(r)]
                assert int(r["id"]) == int(mr.voxel_id(r["voxel_center"][None], [r["layer"]])[0])
        assert set(shown) == m["published"], k
        assert stage_run["deferred"][k] == 0
    # the model's validity: the planes that changed between the snapshots of k and k + 1 are scan k's plane_updates
    for k in range(len(model) - 1):
        assert model[k + 1]["changed"] == stage_run["stats"][k]["plane_updates"], k
    assert model[0]["changed"] == 0
    assert n_add >= 200 and n_del >= 1, (n_add, n_del)


def test_step_path_equals_stage_path(stage_run, step_run):
    """Test 3: vg_step's per-scan events are the stage API's, record for record."""
    assert np.array_equal(stage_run["traj"], step_run["traj"])
    for k in range(NSCAN):
        assert _bytes_set(stage_run["events"][k]) == _bytes_set(step_run["events"][k]), k


def test_off_means_off(step_run):
    """Test 4: a context that never touches the feature and one that publishes
    and reads every scan agree bit for bit; enabling at scan 20 starts blank."""
    a = _run_step(publish=0, read=False)
    b = step_run
    assert np.array_equal(a["traj"], b["traj"])
    assert np.array_equal(a["win"], b["win"])
    assert np.array_equal(a["path"], b["path"])
    assert a["stats"] == b["stats"]
    c = _run_step(publish=0, toggle_at=20)
    assert np.array_equal(a["traj"], c["traj"]) and a["stats"] == c["stats"]
    for k in range(21):  # off, then enabled on a blank slate: nothing before the margi of scan 20 has run
        assert c["events"][k].shape[0] == 0, k
    total = 0
    for k in range(21, NSCAN):
        ck = {_key(r) for r in c["events"][k] if r["action"] == 0}
        bk = {_key(r) for r in b["events"][k] if r["action"] == 0}
        assert ck <= bk, k
        total += len(ck)
    assert total > 0


def test_compaction_and_reset(step_run):
    """Test 5: compacting the pool every 7 scans leaves the event stream as it
    was; after vg_reset and a re-seed the stream is a fresh context's."""
    def again(c, seq):
        c.reset()
        c.seed(seq.gt_state(0))
        ev = []
        for k in range(15):
            xyz, it, beg, end = seq.scan(k)
            c.step(xyz, it, beg, end, seq.imu(k))
            ev.append(c.markers()[0].copy())
        return ev
    b = _run_step(compact_every=7, then=again)
    for k in range(NSCAN):
        assert _bytes_set(b["events"][k]) == _bytes_set(step_run["events"][k]), k
    for k in range(15):
        assert _bytes_set(b["then"][k]) == _bytes_set(step_run["events"][k]), k
    assert sum(e.shape[0] for e in b["then"]) > 0
    # with nothing released no node moves in the pool, so the same pair again with a release distance of
    # 1 m: both release the same roots, only the second compacts, and its survivors change their ids
    a2 = _run_step(compact_every=7, release_dis=1, compact=False)
    b2 = _run_step(compact_every=7, release_dis=1, compact=True)
    print("release without / with compaction:", a2["rel"], b2["rel"])
    assert [r[:3] for r in a2["rel"]] == [r[:3] for r in b2["rel"]]
    assert sum(r[1] for r in b2["rel"]) > 0, "no node erased: the compaction moved nothing"
    assert np.array_equal(a2["traj"], b2["traj"])
    for k in range(NSCAN):
        assert _bytes_set(a2["events"][k]) == _bytes_set(b2["events"][k]), k
    assert sum(int((e["action"] == 0).sum()) for e in b2["events"][-7:]) > 0  # planes still appear after the last one


def test_bounded_buffer(stage_run):
    """Test 6: 64 records of device buffer; what does not fit is deferred, whole."""
    r = _run_stage(capacity=64)
    assert np.array_equal(r["traj"], stage_run["traj"])
    first = None
    for k in range(NSCAN):
        ev, d = r["events"][k], r["deferred"][k]
        assert ev.shape[0] <= 64, k
        cur = {_key(x): x for x in r["snaps"][k]}
        _check_adds_against_snapshot(ev, cur, k)
        if d > 0 and first is None:
            first = k
            assert ev.shape[0] + d == stage_run["events"][k].shape[0], k
    assert first is not None


def test_sharded_refusal_and_abi():
    """Test 7."""
    p = _params()
    c = vgpu.Context(vgconfig.to_c(p), max_points=10_000, max_nodes=10_000, max_fix_points=10_000, hash_log2=12)
    c.shard_host(0, 2, lambda arr: None)
    assert vgpu.lib().vg_set_publish(c.h, 2) == -5  # VG_E_STATE
    assert vgpu.lib().vg_set_publish(c.h, 1) == 0
    c.close()
    d = vgpu.Context(vgconfig.to_c(p), max_points=10_000, max_nodes=10_000, max_fix_points=10_000, hash_log2=12)
    d.set_publish(2)
    assert vgpu.lib().vg_marker_capacity(d.h, 128) == -5  # while enabled
    d.set_publish(0)
    d.marker_capacity(128)
    ev, deferred = d.markers()
    assert ev.shape[0] == 0 and deferred == 0
    assert d.map_planes().shape[0] == 0
    d.close()
    assert ctypes.sizeof(vgpu.VgPlaneMarker) == vgpu.lib().vgx_marker_sizeof() == vgpu.MARKER_DTYPE.itemsize == 248
    syms = vgpu.header_symbols()
    for s in ("vg_markers", "vg_marker_capacity", "vg_map_planes", "vg_set_publish"):
        assert s in syms


def test_node_replay_marker_file(tmp_path):
    """Test 8 (its reduced form): vg_node_replay on a 30-scan event log with the
    marker argument. The file parses; no scan's array holds an id twice (the
    used_ids rule); the stream is consistent — a DELETE only of an id that an
    earlier array (or an earlier record) added, every ADD a plane leaf under
    surf_map_slide with the record's derived fields right. The stream is
    followed by id, as RViz follows it: the reference's id hash is symmetric
    under a sign flip of any coordinate, so voxels mirrored about the origin
    share an id and hide each other within an array (there as here), and the
    model of the snapshot test, which tells nodes apart, does not apply."""
    import json
    import os
    import subprocess
    from test_node_core import REPO, _events, _fmt, _write_log
    p = _params()
    g = p["General"]
    seq = synth.Sequence("16line", 12, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])
    events = _events(seq, 30)
    log, tum, pth, cmap, mk = (tmp_path / n for n in ("ev.bin", "out.tum", "path.txt", "cmap.bin", "markers.bin"))
    _write_log(log, vgconfig.to_c(p), _fmt(g["blind"]), seq.gt_state(0), events)
    exe = os.path.join(REPO, "vina-slam_amd", "bin", "vg_node_replay")
    r = subprocess.run([exe, str(log), str(tum), "0", str(pth), str(cmap), str(mk)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    raw = mk.read_bytes()
    at, scans = 0, []
    while at < len(raw):
        n = int(np.frombuffer(raw, dtype="<i4", count=1, offset=at)[0])
        at += 4
        scans.append(np.frombuffer(raw, dtype=vgpu.MARKER_DTYPE, count=n, offset=at))
        at += n * vgpu.MARKER_DTYPE.itemsize
    assert at == len(raw) and len(scans) == summary["stepped"]
    assert sum(s.shape[0] for s in scans) == summary["marker_records"]
    added, n_add = set(), 0
    for k, ev in enumerate(scans):
        assert len(set(ev["id"].tolist())) == ev.shape[0], (k, "an id twice in one array")
        adds = ev[ev["action"] == 0]
        assert ((adds["flags"] & 7) == 5).all(), k
        if adds.shape[0]:
            mr.check_derived(adds, mr.evaluate(mr.inputs_of_records(adds)), "scan %d" % k)
        for r_ in ev:
            assert int(r_["action"]) in (0, 2), k
            if r_["action"] == 0:
                added.add(int(r_["id"]))
                n_add += 1
            else:
                assert int(r_["id"]) in added, (k, "DELETE of an id never added")
    assert n_add >= 200
