"""The fleet (vg_fleet_*): B trackers attached to one owner's map, one frozen
scan each per step in ten launches. Identity only, not accuracy: every tracker
must equal a lone context (a private full copy of the map, the parent commit's
way) given the identical inputs and seed calls, bit for bit, whatever the batch.
Workload: tests/loc_common.py; trackers as in test_map_view_gpu.

Inputs per tracker (scans 31..40, one per fleet step):
  0  the scans as they are
  1  every second point (another n)
  2  the first 200 points (fewer than one workgroup's 256: most of the grid
     exits empty and the update sums (n + 255) / 256 = 1 partial row)
  3  the scans as they are, seeded with the map's state displaced by DISPLACE
     metres in x; sits out fleet step 4 (its reference is not stepped there)."""
import numpy as np
import pytest

import loc_common as lc
import vgpu
from test_map_view_gpu import tracker

pytestmark = pytest.mark.gpu

NSTEP = 10
SIT_OUT = (3, 4)  # (tracker, fleet step)
DISPLACE = 0.03   # the issue's value; the B = 4 run asserts that it makes the trackers' IEKFs differ
STAT_KEYS_SKIPPED = ("n_ds",)  # a fleet step runs no downsample (vina_gpu.h): 0 there, the voxel count on a lone context

_runs = {}


def _inputs(s, torch, dev):
    """[tracker][step] -> (tensor (4, n) x y z intensity, n, beg, end, imu)."""
    out = [[], [], [], []]
    for k in range(lc.K0, lc.K0 + NSTEP):
        xyz, it, b, e = s.scan(k)
        imu = s.imu(k)
        full = np.concatenate([xyz.T, it[None]], 0).astype(np.float32)
        for t, a in enumerate((full, full[:, ::2], full[:, :200], full)):
            out[t].append((torch.from_numpy(np.ascontiguousarray(a)).to(dev), a.shape[1], b, e, imu))
    return out


def _stats(c):
    return {k: v for k, v in c.stats().items() if k not in STAT_KEYS_SKIPPED}


def _run(B):
    """A B-tracker fleet against B lone references, compared after every step (4);
    returns what test 5 compares across batches and what 6 looks at."""
    if B in _runs:
        return _runs[B]
    import torch
    dev = torch.device("cuda", 0)
    s = lc.base()["seq"]
    data = _inputs(s, torch, dev)
    M = lc.loaded(mapping=False)
    snap = (lc.roots(M), lc.planes(M))
    trk = [tracker() for _ in range(B)]
    ref = [lc.loaded(mapping=False) for _ in range(B)]
    for t in trk:
        t.attach(M)
    if B > 3:
        st = M.state()
        st[10] += DISPLACE
        trk[3].seed(st)
        ref[3].seed(st)
    fl = vgpu.Fleet(M, trk)
    rows = [[] for _ in range(B)]
    iekf = []
    for k in range(NSTEP):
        scans = []
        for b in range(B):
            if (b, k) == SIT_OUT:
                scans.append(None)
                continue
            t, n, beg, end, imu = data[b][k]
            scans.append((t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 0, n, beg, end, imu))
            ref[b].step_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, beg, end, imu)
        fl.step_dev(scans)
        per = {}
        for b in range(B):
            tt, tr = trk[b].trajectory(), ref[b].trajectory()
            assert tt.shape == tr.shape and tt[-1].tobytes() == tr[-1].tobytes(), (b, k)
            assert trk[b].state().tobytes() == ref[b].state().tobytes(), (b, k)
            sa, sb = _stats(trk[b]), _stats(ref[b])
            assert sa == sb, (b, k, sa, sb)
            if scans[b] is not None:
                assert trk[b].stats()["n_ds"] == 0 and sa["n_raw"] == data[b][k][1]
                per[b] = (sa["iekf_iters"], tuple(sa["iekf_matches"]))
            rows[b].append((tt[-1].copy(), trk[b].state(), sa))
        iekf.append(per)
    fl.sync()
    for b in range(B):
        nsteps = NSTEP - (1 if b == SIT_OUT[0] else 0)
        assert trk[b].trajectory().shape[0] == lc.K0 + nsteps
        assert trk[b].path().tobytes() == ref[b].path().tobytes()
        assert len(trk[b].stats_log()) == nsteps
    # 6: the map did not move; a fleet's tracker is stepped only through the fleet; a bad record queues nothing
    lc.same_map(M, *snap)
    t, n, beg, end, imu = data[0][0]
    with pytest.raises(vgpu.VgError) as ei:
        trk[0].step_dev(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n, beg, end, imu)
    assert "(-5)" in str(ei.value)
    before = [c.state() for c in trk]
    ntraj = [c.trajectory().shape[0] for c in trk]
    bad = [(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 0, n, beg, end, imu)] * B
    bad[B - 1] = (0, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), 0, n, beg, end, imu)  # NULL d_x, n > 0
    with pytest.raises(vgpu.VgError) as ei:
        fl.step_dev(bad)
    assert "(-1)" in str(ei.value)
    fl.sync()
    for c, st0, nt in zip(trk, before, ntraj):
        assert np.array_equal(c.state(), st0) and c.trajectory().shape[0] == nt
    fl.close()
    for c in trk + ref:
        c.close()
    M.close()
    _runs[B] = dict(rows=rows, iekf=iekf)
    return _runs[B]


@pytest.mark.parametrize("B", [1, 4])
def test_fleet_trackers_equal_lone_contexts(B):
    """4 and 6 (asserted inside _run, after every step). B = 4: one batch holds
    IEKFs that converge differently. Trackers 0 and 3 read the same scans and
    differ only by tracker 3's displacement, so on some step their iekf_iters
    must differ (the other trackers' match counts differ anyway, by their n)."""
    r = _run(B)
    assert len(r["rows"]) == B and all(len(x) == NSTEP for x in r["rows"])
    if B == 4:
        for step in r["iekf"]:
            print("iekf (iters, matches) per tracker:", step)
        assert any(3 in step and step[0][0] != step[3][0] for step in r["iekf"]), r["iekf"]
        assert any(len({v[0] for v in step.values()}) > 1 for step in r["iekf"])


def test_result_is_independent_of_the_batch():
    """5: tracker 0 of the B = 1 fleet equals tracker 0 of the B = 4 fleet, bit for bit."""
    a, c = _run(1)["rows"][0], _run(4)["rows"][0]
    for k, ((ta, sa, qa), (tc, sc, qc)) in enumerate(zip(a, c)):
        assert ta.tobytes() == tc.tobytes() and sa.tobytes() == sc.tobytes() and qa == qc, k


def test_deskewed_scans_in_a_fleet():
    """4, the deskew case: tracker 0 takes raw scans with per-point times (the per-tracker k_deskew
    launch on the fleet stream), tracker 1 compensated scans, against lone step_deskew_dev / step_dev."""
    import torch
    dev = torch.device("cuda", 0)
    s = lc.base()["seq"]
    M = lc.loaded(mapping=False)
    trk = [tracker(), tracker()]
    ref = [lc.loaded(mapping=False), lc.loaded(mapping=False)]
    for t in trk:
        t.attach(M)
    fl = vgpu.Fleet(M, trk)
    keep = []
    for k in range(lc.K0, lc.K0 + 4):
        xyz, it, tm, b, e = s.scan_raw(k)
        raw = torch.from_numpy(np.ascontiguousarray(np.concatenate([xyz.T, it[None], tm[None]], 0).astype(np.float32))).to(dev)
        cxyz, cit, cb, ce = s.scan(k)
        cmp_ = torch.from_numpy(np.ascontiguousarray(np.concatenate([cxyz.T, cit[None]], 0).astype(np.float32))).to(dev)
        keep += [raw, cmp_]
        imu = s.imu(k)
        p, q = [raw[i].data_ptr() for i in range(5)], [cmp_[i].data_ptr() for i in range(4)]
        ref[0].step_deskew_dev(p[0], p[1], p[2], p[3], p[4], xyz.shape[0], b, e, imu)
        ref[1].step_dev(q[0], q[1], q[2], q[3], cxyz.shape[0], cb, ce, imu)
        fl.step_dev([(p[0], p[1], p[2], p[3], p[4], xyz.shape[0], b, e, imu),
                     (q[0], q[1], q[2], q[3], 0, cxyz.shape[0], cb, ce, imu)])
        for c, r in zip(trk, ref):
            assert c.trajectory()[-1].tobytes() == r.trajectory()[-1].tobytes(), k
            assert c.state().tobytes() == r.state().tobytes(), k
            assert _stats(c) == _stats(r), k
    assert trk[0].stats()["iekf_matches"][0] > 0
    fl.close()
    for c in trk + ref:
        c.close()
    M.close()


def test_empty_scan_and_no_downsample():
    """A fleet step runs no downsample: n_ds is 0 and vg_scan_points is empty afterwards, even when the
    tracker's last lone scan left a cloud behind; and an empty scan (n = 0) in a fleet equals a lone
    context's empty scan, with the scan's planes given and (fleet only) with NULL planes."""
    import torch
    dev = torch.device("cuda", 0)
    s = lc.base()["seq"]
    M = lc.loaded(mapping=False)
    trk = [tracker(), tracker()]
    ref = [lc.loaded(mapping=False), lc.loaded(mapping=False)]
    for t in trk:
        t.attach(M)
    for c in trk + ref:
        lc.step(c, s, lc.K0)  # lone frozen scans: a downsampled cloud each
    assert trk[0].scan_points().shape[0] == trk[0].stats()["n_ds"] > 0
    fl = vgpu.Fleet(M, trk)
    keep = []
    for i, k in enumerate(range(lc.K0 + 1, lc.K0 + 4)):
        xyz, it, b, e = s.scan(k)
        t = torch.from_numpy(np.ascontiguousarray(np.concatenate([xyz.T, it[None]], 0).astype(np.float32))).to(dev)
        keep.append(t)
        imu = s.imu(k)
        q = [t[j].data_ptr() for j in range(4)]
        n = xyz.shape[0]
        n0 = 0 if i >= 1 else n                 # tracker 0: steps 1 and 2 are empty scans
        p0 = [0, 0, 0, 0] if i == 2 else q      # ... step 2 with NULL planes (lone: the planes given, n = 0)
        ref[0].step_dev(q[0], q[1], q[2], q[3], n0, b, e, imu)
        ref[1].step_dev(q[0], q[1], q[2], q[3], n, b, e, imu)
        fl.step_dev([(p0[0], p0[1], p0[2], p0[3], 0, n0, b, e, imu), (q[0], q[1], q[2], q[3], 0, n, b, e, imu)])
        for c, r in zip(trk, ref):
            assert c.trajectory()[-1].tobytes() == r.trajectory()[-1].tobytes(), k
            assert c.state().tobytes() == r.state().tobytes(), k
            assert _stats(c) == _stats(r), k
            assert c.stats()["n_ds"] == 0 and c.scan_points().shape[0] == 0
    assert trk[0].stats()["n_raw"] == 0 and trk[0].stats()["iekf_matches"] == [0, 0, 0, 0]
    assert trk[1].stats()["iekf_matches"][0] > 0
    fl.close()
    for c in trk + ref:
        c.close()
    M.close()
