"""Pins tests/marker_ref.py, the numpy restatement the GPU marker tests compare
with (no GPU): the id hash on hand-computed centres, map_jet inside each of its
five segments, the quaternion against scipy's align_vectors, and the share of
the branch-point inputs whose colour bytes are too close to a truncation edge
to compare."""
import numpy as np

import marker_ref as mr


def test_voxel_id_hand_computed():
    # (1, 2, 3) mm, layer 0: 73856093 ^ (2 * 19349663) ^ (3 * 83492791)
    assert mr.voxel_id([[0.001, 0.002, 0.003]], [0])[0] == (73856093 ^ 38699326 ^ 250478373) & 0x7FFFFFFF
    # the layer term, and a negative hash: h < 0 -> -h
    h = (-1000 * 73856093) ^ (0 * 19349663) ^ (2000 * 83492791) ^ (2 * 2654435761)
    assert h < 0
    assert mr.voxel_id([[-1.0, 0.0, 2.0]], [2])[0] == (-h) & 0x7FFFFFFF
    # ties round away from zero (llround): 0.5 mm -> 1, -0.5 mm -> -1, 1.5 mm -> 2
    assert 0.0005 * 1000.0 == 0.5 and 0.0015 * 1000.0 == 1.5
    h = (1 * 73856093) ^ (-1 * 19349663) ^ (2 * 83492791) ^ (3 * 2654435761)
    assert mr.voxel_id([[0.0005, -0.0005, 0.0015]], [3])[0] == (-h if h < 0 else h) & 0x7FFFFFFF
    # products past 2^31 (|c| = 1e5 m) stay exact in int64
    h = (100000000 * 73856093) ^ (-100000000 * 19349663) ^ (99999999 * 83492791)
    assert mr.voxel_id([[1e5, -1e5, 99999.999]], [0])[0] == (-h if h < 0 else h) & 0x7FFFFFFF


def test_map_jet_segment_interiors():
    got = mr.jet_d(np.array([0.05, 0.25, 0.5, 0.75, 0.95]))
    want = np.array([
        [0.0, 0.0, 0.504 + (0.496 / 0.1242) * 0.05],
        [0.0, (0.25 - 0.1242) / (0.3747 - 0.1242), 1.0],
        [(0.5 - 0.3747) / (0.6253 - 0.3747), 1.0, (0.6253 - 0.5) / (0.6253 - 0.3747)],
        [1.0, (0.8758 - 0.75) / (0.8758 - 0.6253), 0.0],
        [1.0 - (0.95 - 0.8758) * (0.496 / (1.0 - 0.8758)), 0.0, 0.0]])
    assert np.abs(got - want).max() < 1e-15
    col, near = mr.rgba(np.array([0.0, 0.25, 1.0]))
    assert not near.any()
    assert np.array_equal(col[0], np.array([0, 0, int(255 * 0.504), 0], dtype=np.float32) / np.float32(255)
                          + np.array([0, 0, 0, 0.8], dtype=np.float32))
    assert np.array_equal(col[1], col[2])  # the trace clamps at 0.25


def test_quaternion_against_scipy():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(5)
    n = mr.normalized(np.concatenate([rng.normal(size=(50, 3)), [[0, 0, 1], [1, 0, 0], [0, -1, 0], [0.3, 0.4, -1]]]))
    n = n[n[:, 2] > -0.999]
    assert n.shape[0] >= 50
    q, fb = mr.quat_from_z(n)
    assert not fb.any()
    # a unit n's rounding (1e-16) reaches q amplified by 1 / (1 + c), below 1e3 for these vectors
    assert (n[:, 2] > -0.999).all()
    assert np.abs(mr.rotate_z(q) - n).max() < 1e-12
    assert np.abs((q * q).sum(axis=1) - 1.0).max() < 1e-12
    for i in range(n.shape[0]):
        # the shortest-arc rotation has no component about z x n's normal plane: align_vectors gives the same one
        r, _ = Rotation.align_vectors(n[i][None], np.array([[0.0, 0.0, 1.0]]))
        assert np.abs(r.apply([0.0, 0.0, 1.0]) - n[i]).max() < 1e-12
        assert np.abs(Rotation.from_quat(q[i]).as_matrix() - r.as_matrix()).max() < 1e-7
    # the antipodal branch: a unit quaternion that still takes z to n
    na = mr.normalized(np.array([[0, 0, -1.0], [1e-7, 0, -1], [-1e-13, 1e-13, -1]]))
    qa, fa = mr.quat_from_z(na)
    assert fa.all()
    assert np.abs(np.sqrt((qa * qa).sum(axis=1)) - 1.0).max() <= 1e-15
    assert np.abs(mr.rotate_z(qa) - na).max() <= 1e-15


def test_branch_inputs_cover_the_cases_and_keep_their_colours():
    a = mr.branch_inputs()
    assert 200 <= a.shape[0] <= 1000
    ref = mr.evaluate(a)
    assert ref["rgba_unsafe"].mean() <= 0.01  # at most 1 % dropped from the exact-byte comparison
    assert ref["fallback"].sum() >= 20 and (~ref["fallback"]).sum() >= 200
    near = ~ref["fallback"] & (ref["one_plus_c"] < mr.NEAR_BRANCH)
    assert near.sum() >= 40 and ref["one_plus_c"][near].min() < 1e-11  # the first decades above the branch
    assert mr.quat_tol(ref["one_plus_c"])[~ref["fallback"] & ~near].max() == 1e-14
    # the numpy statement holds its own near-branch bound against itself
    qn = ref["quat"][near]
    tn = mr.quat_tol(ref["one_plus_c"])[near]
    assert (np.abs(np.sqrt((qn * qn).sum(axis=1)) - 1.0) <= tn).all()
    assert (np.abs(mr.rotate_z(qn) - ref["normal"][near]).max(axis=1) <= tn).all()
    t = mr.colour_t(a[:, 11])
    for lo, hi in zip((0.0,) + mr.BREAKS, mr.BREAKS + (1.0000001,)):
        assert ((t >= lo) & (t < hi)).sum() >= 4, (lo, hi)  # every map_jet segment
    assert (a[:, 12:15] < 0).any() and (a[:, 12:15] == 0).any()
    assert set(a[:, 3].astype(int)) == {0, 1, 2, 3}
    assert np.abs(a[:, 0:3]).max() >= 9e4 and (a[:, 0:3] < 0).any()
    assert np.isfinite(ref["quat"]).all() and np.isfinite(ref["tip"]).all()
