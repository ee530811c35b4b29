"""The device voxel map against the oracle's, node for node (vgx_map_nodes /
orc_map_nodes through tests/map_dump.py): every field of every node of every
tree — clusters, cov_add, plane record, eigen-decomposition, last_num,
opt_state, point_fix and the window lists — after every scan of the smallest
sequences that reach every branch of insert.hip, recut.hip and margi.hip, after
a release with compaction and after a checkpoint round trip. What holds on
every comparison is stated in map_dump.py; a failure names the first
divergence (scan, collection point, root key, path, field, both values).

Self-consistency of the device record, independent of the oracle, on every
dump that is compared (Checker.check: every scan and collection point of every
case below):
* every plane leaf below max_points, with or without a window: eig_value /
  eig_vector are the decomposition of the covariance of the leaf's own pcr_add,
  recomputed with hp_ref.clu_cov (a cluster already decomposed in an earlier
  dump of this module's tests is not recomputed: the covariance is remembered
  by the cluster's bytes). pcr_add already holds pcr_fix (margi starts it from
  pcr_fix, octree.cpp:419). Leaves at or past max_points are left out because
  margi's full-leaf branch takes the oldest scan out of pcr_add after the
  decomposition (octree.cpp:461-469), so there the stored eig is by definition
  not that of the stored cluster; those leaves are held by the oracle alone;
* the plane itself is refreshed only when the cluster grew by five points
  (octree.cpp:441-446), so between refreshes centre, normal and radius lag the
  cluster by definition. They are held to the cluster where margi just
  refreshed them: in every such leaf whose last_num moved since the context's
  previous dump (dumps follow one another with at most one margi between),
  last_num is pcr_add.N, the centre is the cluster's mean, the normal is
  eig_vector's first column and the radius eig_value[2]. A context's first
  dump has no previous one and checks the decomposition only.
"""
import os

import numpy as np
import pytest

import hp_ref
import map_dump as MD
import oracle
import synth
import vgconfig
import vgpu

import insert_edge_input as E

pytestmark = pytest.mark.gpu
CAP = dict(max_points=120_000, max_nodes=600_000, max_fix_points=2_000_000, hash_log2=20)
# margi's pcr_fix.N >= max_points branch fires from scan 10 of the 16 with this value (chosen from
# the oracle alone: tests/test_map_dump_ref.py asserts it there too)
SMALL_MAX_POINTS = 30
# name -> (config, lidar, seq_id, scans, to_c keywords)
CASES = {
    "mid360": ("mid360", "16line", 4, 16, {}),
    "HILTI": ("HILTI", "16line", 4, 12, {}),
    "velodyne": ("velodyne", "16line", 3, 16, {}),
    "small-max-points": ("mid360", "16line", 4, 16, {"max_points": SMALL_MAX_POINTS}),
}


def sequence(p, lidar, seq_id):
    g = p["General"]
    return synth.Sequence(lidar, seq_id, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])


def open_case(name, gpus=1, **extra):
    cfgname, lidar, seq_id, nscan, kw = CASES[name]
    p = vgconfig.load(cfgname)
    seq = sequence(p, lidar, seq_id)
    kw = {**kw, **extra}
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0, **kw))
    orc.seed(seq.gt_state(0))
    ctxs = []
    for _ in range(gpus):
        c = vgpu.Context(vgconfig.to_c(p, **kw), **CAP)
        c.seed(seq.gt_state(0))
        ctxs.append(c)
    return p, seq, nscan, orc, ctxs


_COV = {}  # pcr_add's bytes -> its covariance (hp_ref.clu_cov); the cases share sequences, and equal clusters recur


class Checker:
    """One device context's dumps in order: compare() with the oracle and the self-consistency
    above, on every dump; the observed maxima accumulate in `total`."""

    def __init__(self, max_points=100):
        self.max_points, self.total, self.prev = max_points, {}, None

    def _cov(self, c):
        key = c[35:45].tobytes()
        if key not in _COV:
            _COV[key] = hp_ref.to_np(hp_ref.clu_cov(np.concatenate([c[39:45], c[36:39], c[35:36]])))
        return _COV[key]

    def self_check(self, dev, where):
        r, total = dev["rec"], self.total
        rows = r[(r[:, 13] == 0) & (r[:, 15] == 1) & (r[:, 25] < self.max_points) & (r[:, 35] > 0)]
        total["self-checked leaves"] = total.get("self-checked leaves", 0) + rows.shape[0]
        if not rows.shape[0]:
            return
        A = np.array([self._cov(c) for c in rows])
        r1, r2 = MD.decomposition_residual(A, rows[:, 118:121], rows[:, 121:130])
        r1 = r1 / np.maximum(1.0, np.abs(A).reshape(-1, 9).max(1))
        MD.merge_obs(total, {"self |A v - l v|": float(r1.max()), "self |V^T V - I|": float(r2.max())})
        for name, v, b in (("|A v - l v|", r1, MD.ILL["eig_value"]), ("|V^T V - I|", r2, MD.ILL["eig_vector"])):
            if not (v <= b).all():
                i = int(np.argmax(v))
                raise MD.Divergence("%s: %s: the device's eig is not the decomposition of its own pcr_add: %s %.3e"
                                    % (where, MD.key_of(rows[i]), name, v[i]))
        if self.prev is None:
            return
        before = {MD.key_of(x): x[17] for x in self.prev["rec"]}
        upd = rows[[before.get(MD.key_of(x), 0.0) != x[17] for x in rows]]  # (a new node starts at last_num 0)
        total["self-checked refreshed planes"] = total.get("self-checked refreshed planes", 0) + upd.shape[0]
        if upd.shape[0]:
            mean = upd[:, 36:39] / upd[:, 35:36]
            dc = np.abs(upd[:, 90:93] - mean).max(1) / np.maximum(1.0, np.abs(mean).max(1))
            MD.merge_obs(total, {"self centre": float(dc.max())})
            bad = np.flatnonzero((upd[:, 17] != upd[:, 35]) | ~(dc <= MD.TIGHT) |
                                 np.any(upd[:, 93:96] != upd[:, [121, 124, 127]], axis=1) |
                                 (upd[:, 117] != upd[:, 120].astype(np.float32)))
            if bad.size:
                i = int(bad[0])
                raise MD.Divergence("%s: %s: plane not refreshed from its cluster: last_num %d N %d centre %s mean "
                                    "%s normal %s eig_vector[:, 0] %s radius %r eig_value[2] %r" %
                                    (where, MD.key_of(upd[i]), upd[i, 17], upd[i, 35], upd[i, 90:93], mean[i],
                                     upd[i, 93:96], upd[i, [121, 124, 127]], upd[i, 117], upd[i, 120]))

    def check(self, orc_dump, dev, where):
        MD.merge_obs(self.total, MD.compare(orc_dump, dev, where))
        self.self_check(dev, where)
        self.prev = dev
        return dev


def report(name, total):
    print("%s: observed maxima (relative to max(1, |oracle field|)):" % name)
    for k in sorted(total):
        print("  %-24s %.3e" % (k, total[k]))


def step_both(orc, ctxs, seq, k):
    xyz, it, b, e = seq.scan(k)
    imu = seq.imu(k)
    orc.step(xyz, it, b, e, imu)
    for c in ctxs:
        c.step(xyz, it, b, e, imu)


def same_steps(a, b):
    assert np.array_equal(a.trajectory(), b.trajectory())
    assert np.array_equal(a.window_states(), b.window_states())
    assert a.stats_log() == b.stats_log()


def test_stage_path_after_recut_and_after_margi(oracle_lib):
    """mid360 / 16line / 16 scans through the stage API: the maps agree after
    multi_recut and again after multi_margi on every scan (the window fills at
    scan 9), which separates an insert or recut error from a margi error; the
    context dumped at both points of every scan steps bit for bit like one
    that is stepped by vg_step and never dumped, and ends with the same map,
    bit for bit (the undumped one's only dump)."""
    p, seq, nscan, orc, (a, b) = open_case("mid360", gpus=2)
    orc.map_dump_after_recut()
    W = p["LocalBA"]["win_size"]
    ck = Checker()
    for k in range(nscan):
        xyz, it, beg, end = seq.scan(k)
        imu = seq.imu(k)
        orc.step(xyz, it, beg, end, imu)
        b.step(xyz, it, beg, end, imu)
        a.scan_load(xyz, it)
        a.propagate(imu, beg, end)
        a.downsample_scan()
        a.lio_state_estimation()
        a.window_push(imu)
        a.cut_voxel_multi()
        a.multi_recut()
        ck.check(orc.map_nodes(after_recut=True), a.map_nodes(), "scan %d after multi_recut" % k)
        if a.win_count() >= W:
            a.damping_iter()
            a.multi_margi()
            ck.check(orc.map_nodes(), a.map_nodes(), "scan %d after multi_margi" % k)
        a.step_end()
    report("stage path", ck.total)
    assert ck.total["self-checked leaves"] > 10000 and ck.total["self-checked refreshed planes"] > 1000, ck.total
    same_steps(a, b)
    MD.same_dump(a.map_nodes(), b.map_nodes(), "dumped against never dumped")
    a.close()
    b.close()
    orc.close()


@pytest.mark.parametrize("name", ["HILTI", "velodyne", "small-max-points"])
def test_step_matches_oracle_node_for_node(oracle_lib, name):
    """vg_step, the maps compared after every scan: HILTI (voxel 1.0, max_layer
    2, BA off), velodyne (max_layer 3, rotated extrinsic) and mid360 with a
    small max_points, where margi's pcr_fix.N >= max_points branch fires. The
    dumped context steps bit for bit like one never dumped and ends with the
    same map."""
    p, seq, nscan, orc, (a, b) = open_case(name, gpus=2)
    mpts = CASES[name][4].get("max_points", 100)
    ck, full = Checker(mpts), 0
    for k in range(nscan):
        step_both(orc, (a, b), seq, k)
        ck.check(orc.map_nodes(), a.map_nodes(), "scan %d" % k)
        full += orc.stats()["fix_full"]
        assert orc.stats()["fix_full"] == a.stats()["fix_full"]
    report(name, ck.total)
    assert ck.total["self-checked refreshed planes"] > 100, ck.total
    if name == "small-max-points":
        assert full > 0
    same_steps(a, b)
    MD.same_dump(a.map_nodes(), b.map_nodes(), "dumped against never dumped")
    a.close()
    b.close()
    orc.close()


@pytest.mark.parametrize("pipe", [0, 1], ids=["loads-in-series", "loads-pipelined"])
def test_insert_edge_shapes_node_for_node(oracle_lib, pipe):
    """insert_edge_input.py's sequence (leaves receiving 1, 64, 65, 256, 257 and
    320 points in one scan, several octants created under one parent at once;
    test_insert_chain_gpu.py asserts those shapes), with k_push_window's loads
    in series and pipelined (vgx_debug 39)."""
    p = E.config(vgconfig)
    seq, scans, keys = E.make(p)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0))
    gpu = vgpu.Context(vgconfig.to_c(p), **CAP)
    gpu.debug(38, 1)
    gpu.debug(39, pipe)
    orc.seed(seq.gt_state(0))
    gpu.seed(seq.gt_state(0))
    ck = Checker()
    for k, (xyz, it, beg, end, imu) in enumerate(scans):
        orc.step(xyz, it, beg, end, imu)
        gpu.step(xyz, it, beg, end, imu)
        do = orc.map_nodes()
        ck.check(do, gpu.map_nodes(), "scan %d" % k)
    have = {MD.key_of(r)[0] for r in do["rec"]}
    assert all(tuple(key) in have for key in keys), keys
    report("insert edge shapes, knob 39 = %d" % pipe, ck.total)
    assert MD.excluded(do)[2] >= 8  # the exact-grid leaves: their eigenvector pair was compared as a projector
    gpu.close()
    orc.close()


def test_after_release_with_compaction(oracle_lib):
    """release_dis = 4 m on test_lifetime_gpu's sequence, up to the first
    release that erases roots: the compacted pool (release_far(compact=True)
    renumbers every node and repacks the point_fix arena after every scan)
    holds the oracle's map after every scan from 15 up to that release (scan
    19) and two scans past it."""
    p = vgconfig.load("mid360")
    seq = sequence(p, "16line", 7)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0, release_dis=4))
    gpu = vgpu.Context(vgconfig.to_c(p, release_dis=4), max_points=100_000, max_nodes=400_000,
                       max_fix_points=2_000_000, hash_log2=18)
    orc.seed(seq.gt_state(0))
    gpu.seed(seq.gt_state(0))
    ck, erased_at = Checker(), None
    for k in range(80):
        step_both(orc, (gpu,), seq, k)
        ro, rg = orc.release_far(), gpu.release_far(compact=True)
        assert ro[:5] == rg[:5], (k, ro, rg)
        if erased_at is None and ro[0] > 0:
            erased_at = k
            print("scan %d: the release erased %d roots, %d nodes" % (k, ro[0], ro[1]))
        if k >= 15:  # the release is due every tenth scan from the full window on: none can erase before scan 19
            ck.check(orc.map_nodes(), gpu.map_nodes(), "scan %d after release + compaction" % k)
        if erased_at is not None and k == erased_at + 2:
            break
    assert erased_at is not None and erased_at >= 15
    report("release + compaction", ck.total)
    gpu.close()
    orc.close()


def test_checkpoint_round_trip_node_for_node(oracle_lib, tmp_path):
    """checkpoint_save then checkpoint_load into a fresh context: the loader's
    dump equals the saver's field for field, bit for bit (device against
    device), the saver's matches the oracle, and both still hold two scans on.
    Last, the hook refuses a shared map: VG_E_STATE on an attached tracker and
    on the owner of its map."""
    p, seq, nscan, orc, (a, c) = open_case("mid360", gpus=2)
    ck = Checker()
    for k in range(12):
        step_both(orc, (a,), seq, k)
        ck.check(orc.map_nodes(), a.map_nodes(), "scan %d, the saver" % k)
    path = os.path.join(str(tmp_path), "map.vgck")
    a.checkpoint_save(path)
    c.checkpoint_load(path)
    da = a.map_nodes()
    MD.same_dump(da, c.map_nodes(), "after the load")
    ck.check(orc.map_nodes(), da, "scan 11, the saver after the save")
    for k in range(12, 14):
        step_both(orc, (a, c), seq, k)
        da = a.map_nodes()
        MD.same_dump(da, c.map_nodes(), "scan %d after the load" % k)
        ck.check(orc.map_nodes(), da, "scan %d, the saver" % k)
    report("checkpoint", ck.total)
    c.set_mapping(False)
    t = vgpu.Context(vgconfig.to_c(p), max_points=CAP["max_points"], max_nodes=1024, max_fix_points=1024,
                     hash_log2=10)
    t.attach(c)
    for x in (t, c):
        with pytest.raises(vgpu.VgError) as ei:
            x.map_nodes()
        assert "(-5)" in str(ei.value), str(ei.value)
    t.close()
    a.close()
    c.close()
    orc.close()


@pytest.mark.parametrize("knob", [1, 3, 4], ids=["recut-level-replay", "insert-replay", "host-factor-sort"])
def test_host_sized_fallbacks_node_for_node(oracle_lib, knob):
    """The three host-sized fallbacks at capacity 0 (vgx_debug 1, 3, 4: every
    occurrence takes the fallback) on the first sequence, against the oracle
    after every scan."""
    p, seq, nscan, orc, (a,) = open_case("mid360")
    a.debug(knob, 0)
    ck = Checker()
    for k in range(nscan):
        step_both(orc, (a,), seq, k)
        ck.check(orc.map_nodes(), a.map_nodes(), "scan %d" % k)
    report("fallback knob %d" % knob, ck.total)
    a.close()
    orc.close()
