"""Shared workload of the localisation tests (test_localize_gpu, test_score_gpu,
test_relocalize_gpu): tests/test_checkpoint_gpu.py's — the 16-line synthetic
sequence with the mid360 parameters at max_points 100,000, max_nodes 400,000,
max_fix_points 2,000,000, hash_log2 18. Mapping context A runs scans 0..30,
saves a checkpoint, and goes on to scan 50; everything is computed once per
process and read-only afterwards."""
import os
import tempfile

import numpy as np

import synth
import vgconfig
import vgpu

CAP = dict(max_points=100_000, max_nodes=400_000, max_fix_points=2_000_000, hash_log2=18)
K0 = 31   # the first scan after the checkpoint
K1 = 51   # A's last scan + 1

_cache = {}


def seq():
    g = vgconfig.load("mid360")["General"]
    return synth.Sequence("16line", 3, blind=g["blind"], ext_R=g["extrinsic_rota"], ext_t=g["extrinsic_tran"])


def ctx(**cfg):
    return vgpu.Context(vgconfig.to_c(vgconfig.load("mid360"), **cfg), **CAP)


def ext():
    g = vgconfig.load("mid360")["General"]
    return np.array(g["extrinsic_rota"], dtype=np.float64).reshape(3, 3), np.array(g["extrinsic_tran"], dtype=np.float64)


def step(c, s, k):
    xyz, it, b, e = s.scan(k)
    c.step(xyz, it, b, e, s.imu(k))


def base():
    """{seq, path (checkpoint after scan 30), traj (A's rows 0..50), stats (A's per-scan stats), dir}."""
    if not _cache:
        s = seq()
        A = ctx()
        A.seed(s.gt_state(0))
        for k in range(K0):
            step(A, s, k)
        d = tempfile.mkdtemp(prefix="vgloc")
        path = os.path.join(d, "at30.vgck")
        A.checkpoint_save(path)
        for k in range(K0, K1):
            step(A, s, k)
        _cache.update(seq=s, path=path, traj=A.trajectory(), stats=A.stats_log(), dir=d)
        A.close()
    return _cache


def loaded(mapping=True):
    c = ctx()
    c.checkpoint_load(base()["path"])
    if not mapping:
        c.set_mapping(False)
    return c


def roots(c):
    return sorted((key, np.float64(v[0]).tobytes(), tuple(v[1:])) for key, v in c.roots().items())


def planes(c):
    """Every node's snapshot record sorted by (id, layer); the id is a hash of the voxel centre and layer
    and the snapshot's emission order is not fixed, so the centre breaks the ties."""
    p = c.map_planes(all_nodes=True)
    vc = p["voxel_center"]
    return p[np.lexsort((vc[:, 2], vc[:, 1], vc[:, 0], p["layer"], p["id"]))]


def same_map(c, ref_roots, ref_planes):
    assert roots(c) == ref_roots
    p = planes(c)
    assert p.shape == ref_planes.shape and p.tobytes() == ref_planes.tobytes()


def pose_of_row(row):
    """(12,) [R row-major, p] of a trajectory row (t, R 9, p 3)."""
    return np.asarray(row[1:13], dtype=np.float64).copy()


def gt_traj(s, k0, k1):
    out = np.zeros((k1 - k0, 13))
    for i, k in enumerate(range(k0, k1)):
        R, p = s.gt_pose(k)
        out[i, 0] = s.t_end(k)
        out[i, 1:10] = R.reshape(9)
        out[i, 10:13] = p
    return out
