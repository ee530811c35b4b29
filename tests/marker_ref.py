"""numpy fp64 restatement of the marker math (OctoTree::collect_plane_markers /
collect_normal_markers, octree.cpp:11-63, 787-824, 900-917) for the marker
tests, plus the hand-built inputs of the branch-point test.

Inputs follow vgx_marker_eval: rows of 15 doubles, voxel_center 3, layer,
quater_length, center 3, normal 3, trace, eig 3."""
import numpy as np

BREAKS = (0.1242, 0.3747, 0.6253, 0.8758)  # map_jet's segment ends
MAX_TRACE, POW_NUM, ALPHA = 0.25, 0.2, 0.8
FALLBACK_C = -1.0 + 1e-12  # FromTwoVectors' near-antipodal branch


def llround(x):
    """C llround: nearest, ties away from zero (exact: trunc and the fraction are)."""
    x = np.asarray(x, dtype=np.float64)
    t = np.trunc(x)
    f = x - t
    return (t + np.where(f >= 0.5, 1.0, 0.0) - np.where(f <= -0.5, 1.0, 0.0)).astype(np.int64)


def voxel_id(center, layer):
    """voxel_id_from_center (octree.cpp:11-21), int64 wrap-around arithmetic."""
    c = np.asarray(center, dtype=np.float64).reshape(-1, 3)
    layer = np.asarray(layer, dtype=np.int64).reshape(-1)
    with np.errstate(over="ignore"):
        i = llround(c * 1000.0)
        h = (i[:, 0] * np.int64(73856093)) ^ (i[:, 1] * np.int64(19349663)) ^ (i[:, 2] * np.int64(83492791)) \
            ^ (layer * np.int64(2654435761))
        h = np.where(h < 0, -h, h)
    return (h & np.int64(0x7FFFFFFF)).astype(np.int32)


def jet_d(v):
    """map_jet's (dr, dg, db) before the byte truncation (octree.cpp:23-57)."""
    v = np.clip(np.asarray(v, dtype=np.float64), 0.0, 1.0)
    b0, b1, b2, b3 = BREAKS
    dr = np.select([v < b0, v < b1, v < b2, v < b3],
                   [0.0 * v, 0.0 * v, (v - b1) * (1.0 / (b2 - b1)), 1.0 + 0.0 * v],
                   1.0 - (v - b3) * ((1.0 - 0.504) / (1.0 - b3)))
    dg = np.select([v < b0, v < b1, v < b2, v < b3],
                   [0.0 * v, (v - b0) * (1.0 / (b1 - b0)), 1.0 + 0.0 * v, (b3 - v) * (1.0 / (b3 - b2))], 0.0 * v)
    db = np.select([v < b0, v < b1, v < b2, v < b3],
                   [0.504 + ((1.0 - 0.504) / b0) * v, 1.0 + 0.0 * v, (b2 - v) * (1.0 / (b2 - b1)), 0.0 * v], 0.0 * v)
    return np.stack([dr, dg, db], axis=-1)


def colour_t(trace):
    t = np.minimum(np.asarray(trace, dtype=np.float64), MAX_TRACE) * (1.0 / MAX_TRACE)
    return np.power(t, POW_NUM)


def rgba(trace):
    """(n, 4) float32 colour and, per row, whether any 255 d lies within 1e-9 of
    an integer (a last-ulp difference of pow could flip the truncated byte)."""
    d = 255 * jet_d(colour_t(trace))
    # (a channel a segment sets to the constant 0 or 1 is exact on both sides: it cannot flip)
    near = ((np.abs(d - np.rint(d)) < 1e-9) & (d != 0.0) & (d != 255.0)).any(axis=-1)
    byte = np.floor(d).astype(np.uint8)
    out = np.empty(d.shape[:-1] + (4,), dtype=np.float32)
    out[..., :3] = byte.astype(np.float32) / np.float32(255.0)
    out[..., 3] = np.float32(ALPHA)
    return out, near


def normalized(n):
    n = np.asarray(n, dtype=np.float64).reshape(-1, 3)
    nn = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    return n / nn[:, None]


def quat_from_z(n):
    """Quaterniond::FromTwoVectors(UnitZ, n) for unit n, x y z w; rows with
    c < -1 + 1e-12 (fallback[i]) hold one valid choice, not Eigen's."""
    n = np.asarray(n, dtype=np.float64).reshape(-1, 3)
    c = n[:, 2]
    fb = c < FALLBACK_C
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.sqrt(2.0 * (1.0 + c))
        q = np.stack([-n[:, 1] / s, n[:, 0] / s, 0.0 * s, s / 2.0], axis=-1)
        s2 = np.sqrt(2.0 * (1.0 - c))
        q2 = np.stack([s2 / 2.0, 0.0 * s2, n[:, 0] / s2, -n[:, 1] / s2], axis=-1)
    q[fb] = q2[fb]
    return q, fb


def rotate_z(q):
    """R(q) z for x y z w quaternions."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], axis=-1)


def evaluate(inp):
    """Every derived field for (n, 15) inputs, as a dict of arrays."""
    a = np.asarray(inp, dtype=np.float64).reshape(-1, 15)
    vc, layer, qlen, center, normal, trace, eig = a[:, 0:3], a[:, 3].astype(np.int64), a[:, 4], a[:, 5:8], \
        a[:, 8:11], a[:, 11], a[:, 12:15]
    n = normalized(normal)
    q, fb = quat_from_z(n)
    col, near = rgba(trace)
    ev = np.maximum(0.0, eig)
    length = 2.0 * qlen
    return {
        "id": voxel_id(vc, layer), "layer": layer.astype(np.int32), "normal": n, "quat": q, "fallback": fb,
        "rgba": col, "rgba_unsafe": near,
        "plane_scale": np.stack([3.0 * np.sqrt(ev[:, 2]), 3.0 * np.sqrt(ev[:, 1]), 2.0 * np.sqrt(ev[:, 0])], axis=-1),
        "tip": center + n * length[:, None],
        "tip_terms": np.abs(center) + np.abs(n * length[:, None]),
        "one_plus_c": 1.0 + n[:, 2],
        "normal_scale": np.stack([0.1 * length, 0.2 * length, 0.0 * length], axis=-1),
    }


def inputs_of_records(rec):
    """The vgx_marker_eval inputs a record's raw fields amount to (its normal is normalised already)."""
    a = np.zeros((rec.shape[0], 15))
    a[:, 0:3] = rec["voxel_center"]
    a[:, 3] = rec["layer"]
    a[:, 4] = rec["quater_length"]
    a[:, 5:8] = rec["center"]
    a[:, 8:11] = rec["normal"]
    a[:, 11] = rec["trace"]
    a[:, 12:15] = rec["eig"]
    return a


NEAR_BRANCH = 1e-5  # 1 + c below this (a normal within 4.5e-3 rad of -z), still in the regular branch


def quat_tol(one_plus_c):
    """The regular branch's quaternion bound. 1e-14 absolute (under 20 fp64
    roundings on O(1) values, FMA contraction allowed, times 5) wherever it can
    hold. Just above the branch it cannot: s = sqrt(2 (1 + c)) carries the
    rounding of the unit normal's z (up to 2 ulp of 1 between two correctly
    rounded normalisations, 2.2e-16) divided by 2 (1 + c), and so does every
    component of q; for 1 + c < NEAR_BRANCH the bound is 8e-16 / (1 + c), seven
    times that. A wrong branch (the other formula turns about another axis) or
    a wrong sign is off by O(1) and still seen."""
    return np.where(one_plus_c < NEAR_BRANCH, 8e-16 / np.maximum(one_plus_c, 1e-300), 1e-14)


def check_derived(rec, ref, what=""):
    """Test 1's tolerances on records against evaluate()'s output. normal:
    absolute 1e-14; quat: quat_tol, and for the rows just above the branch also
    |q| = 1 and R(q) z = n at that bound; plane_scale, normal_scale: relative
    1e-14 per component (normal_scale's third exactly 0); tip: per component
    1e-14 (|center_j| + |n_j length|), relative to the terms it adds, since the
    sum itself may cancel to ~0 where no relative bound on it can hold; fallback
    rows: |q| = 1 to 1e-14 and R(q) z = n to 1e-12 only; rgba exact where the
    truncation is safe."""
    assert np.array_equal(rec["id"], ref["id"]), what
    assert np.array_equal(rec["layer"], ref["layer"]), what
    ok = ~ref["rgba_unsafe"]
    assert np.array_equal(rec["rgba"][ok], ref["rgba"][ok]), what
    assert np.abs(rec["normal"] - ref["normal"]).max(initial=0.0) <= 1e-14, what
    reg = ~ref["fallback"]
    tol = quat_tol(ref["one_plus_c"])[reg]
    dq = np.abs(rec["quat"][reg] - ref["quat"][reg]).max(axis=1)
    assert (dq <= tol).all(), (what, "quat", dq.max(initial=0.0))
    near = reg & (ref["one_plus_c"] < NEAR_BRANCH)
    qn = rec["quat"][near]
    if qn.shape[0]:
        tn = quat_tol(ref["one_plus_c"])[near]
        assert (np.abs(np.sqrt((qn * qn).sum(axis=1)) - 1.0) <= tn).all(), what
        assert (np.abs(rotate_z(qn) - ref["normal"][near]).max(axis=1) <= tn).all(), what
    qf = rec["quat"][~reg]
    if qf.shape[0]:
        assert np.abs(np.sqrt((qf * qf).sum(axis=1)) - 1.0).max() <= 1e-14, what
        assert np.abs(rotate_z(qf) - ref["normal"][~reg]).max() <= 1e-12, what
    for f in ("plane_scale", "normal_scale"):
        d = np.abs(rec[f] - ref[f])
        assert (d <= 1e-14 * np.abs(ref[f])).all(), (what, f, d.max(initial=0.0))
    assert (rec["normal_scale"][:, 2] == 0.0).all(), what
    d = np.abs(rec["tip"] - ref["tip"])
    assert (d <= 1e-14 * ref["tip_terms"]).all(), (what, "tip", d.max(initial=0.0))


def branch_inputs():
    """The hand-built inputs of the branch-point test (a few hundred rows)."""
    rng = np.random.default_rng(20240607)
    normals = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]
    for d in (1e-7, 1e-13):  # both in the antipodal branch (c ~ -1 + d^2 / 2 < -1 + 1e-12)
        normals += [[d, 0, -1], [0, -d, -1], [-d, d, -1]]
    normals += [[0.5, 0, -1], [0, -0.5, -1], [0.3, 0.4, -1]]  # the regular branch's side, c ~ -0.9
    for d in (2e-6, 5e-6, 1e-5, 1e-4, 1e-3):  # just above the branch (1 + c ~ d^2 / 2 >= 2e-12): quat_tol
        normals += [[d, 0, -1], [0, -d, -1], [-0.6 * d, 0.8 * d, -1]]
    r = rng.normal(size=(40, 3))
    normals += list(r / np.sqrt((r * r).sum(axis=1))[:, None])
    normals += list(rng.normal(size=(20, 3)) * rng.uniform(1e-3, 50.0, size=(20, 1)))  # unnormalised
    normals = np.array(normals, dtype=np.float64)
    # traces: 0, both sides of each map_jet breakpoint (t = pow(trace / 0.25, 0.2)), >= 0.25
    traces = [0.0, 1e-12, 1e-6, 0.25, 0.26, 3.0]
    for b in BREAKS:
        for e in (-1e-3, -1e-9, 1e-9, 1e-3):
            traces.append(MAX_TRACE * (b + e) ** 5)
    traces += list(rng.uniform(0.0, 0.3, size=30) ** 2)
    eigs = [[-1e-3, 0.01, 0.2], [0, 0, 0], [-1.0, -2.0, -3.0], [1e-4, 2e-2, 0.3], [0, 1e-6, 4.0], [2.5e-3, 0.04, 0.09]]
    centres = [[-12.375, 3.125, -0.875], [0.0005, -0.0005, 0.0015], [-0.0005, 0.0025, -0.0035],
               [1e5, -1e5, 99999.9995], [-99999.0005, 12345.6785, -0.0004999], [0.125, 0.125, 0.125]]
    rows = []
    k = 0
    for i in range(len(normals)):
        for j in range(4):
            vc = np.array(centres[k % len(centres)]) + (0.0 if k % 3 else rng.integers(-400, 400, 3) * 0.125)
            layer = (k // 2) % 4
            qlen = float(np.float32(0.125 / (1 << layer)))
            centre = vc + rng.uniform(-0.1, 0.1, 3)
            rows.append(np.concatenate([vc, [layer, qlen], centre, normals[i], [traces[k % len(traces)]],
                                        eigs[k % len(eigs)]]))
            k += 1
    return np.array(rows)
