"""Node-for-node comparison of two voxel-map dumps (oracle.Pipeline.map_nodes,
vgpu.Context.map_nodes; record layout in oracle/vina_oracle.h).

Both dumps are keyed by (root key, octant path), the window slots are put in
ring order (position i is physical slot mp[i], so a rotation of the physical
slots is no difference), and the point lists are paired one to one after a
sort on the coordinates rounded to 1e-6.

compare() checks, in every node:
* exactly: the key set, layer, octo_state, isexist, is_plane, child mask,
  last_num, has-sw, every cluster's N, the point_fix count, every per-slot
  list length, voxel_center and quater_length;
* opt_state, with its one documented departure asserted: the device numbers
  the LM's factors in node-id order, the oracle in slide-map iteration order
  ("output ORDER ... of factors"), so between recut and
  margi a factor leaf's index differs. The same leaves carry a factor
  (opt_state >= 0 on the same keys, -1 everywhere else) and each side's
  indices are 0 .. n_factors - 1, each once. This does not pin the device's
  numbering to node-id order (the dump carries no node ids): a leaf that took
  another leaf's factor would show only after the margi that follows, in its
  pcr_add and eig, which come from that factor's slot;
* the well-conditioned reals (clusters, cov_add, plane.center, jour, points
  and their variances) within TIGHT = 1e-9 relative to max(1, max |oracle
  field|) of that node;
* the ill-conditioned reals (eig_value, eig_vector, plane.normal, plane_var,
  radius) with sign, within ILL[field] in the same relative form. A node is
  left out of these only when the oracle's own eigenvalues have a relative
  gap (l1 - l0) / l2 below GAP_MIN (the normal, plane_var's 1 / (l0 - lk) and
  every eigenvector lose their value). Where only (l2 - l1) / l2 is below
  GAP_MIN, eig_vector's columns 1 and 2 alone have no stable value (any
  rotation of the pair within their plane is as good; plane_var's sum over
  the pair is invariant under it): column 0 and all other fields are still
  compared, and of the pair what has a value is: the projector V1 V1^T +
  V2 V2^T, against the oracle's within the eig_vector bound. For every node
  whose columns are not all compared one by one, the device's decomposition
  must also hold against the device's own cluster: |A v - l v| and
  |V^T V - I| within the bounds.

The ILL bounds are 100 x the maxima measured on the first case of
tests/test_map_nodes_gpu.py (profiles/map_nodes/observed.json), rounded up to
a power of ten and never looser than 1e-6; tests/test_map_dump_ref.py pins
that file to these constants.
"""
import math

import numpy as np

NODE_REC, NODE_SLOT = 131, 11
TIGHT = 1e-9
# relative eigenvalue gap of the oracle below which a node's eigenvectors have no stable value.
# The fp64 eigenvector error is ~ eps / gap: at 1e-4 that is ~1e-12, far inside the bounds below.
GAP_MIN = 1e-4
ILL_CAP = 1e-6
# radius is a float: its rounding step, 2^-23 relative, is the floor of its bound (the measured maximum is 0)
ILL_FLOOR = {"radius": 2.0 ** -23}
ILL = {"eig_value": 1e-10, "eig_vector": 1e-6, "normal": 1e-7, "plane_var": 1e-6, "radius": 2.0 ** -23}

EXACT = {"layer": 12, "octo_state": 13, "isexist": 14, "is_plane": 15, "child_mask": 16, "last_num": 17,
         "has_sw": 19, "voxel_center": slice(20, 23), "quater_length": 23, "pcr_fix.N": 25,
         "pcr_add.N": 35, "point_fix.size": 130}
WELL = {"jour": slice(24, 25), "pcr_fix": slice(26, 35), "pcr_add": slice(36, 45), "cov_add": slice(45, 90),
        "plane.center": slice(90, 93)}
ILL_COLS = {"eig_value": slice(118, 121), "eig_vector": slice(121, 130), "normal": slice(93, 96),
            "plane_var": slice(96, 117), "radius": slice(117, 118)}


def ill_bound(observed, field=None):
    """100 x the observed maximum, rounded up to a power of ten, never looser than ILL_CAP
    (and never tighter than the field's number format, ILL_FLOOR)."""
    b = 0.0 if observed <= 0 else 10.0 ** math.ceil(math.log10(100.0 * observed) - 1e-12)
    return min(ILL_CAP, max(b, ILL_FLOOR.get(field, 0.0)))


class Divergence(AssertionError):
    pass


def _order(rec):
    """Row order by (root key, path length, path) and the key columns in that order."""
    keys = rec[:, 0:12]
    idx = np.lexsort(keys[:, ::-1].T)
    return idx, keys[idx]


def key_of(row):
    d = int(row[3])
    return tuple(int(v) for v in row[0:3]), tuple(int(v) for v in row[4:4 + d])


def ring_slots(dump):
    """rec's slot blocks reordered to ring position: (n, W, NODE_SLOT)."""
    W = dump["W"]
    s = dump["rec"][:, NODE_REC:].reshape(-1, W, NODE_SLOT)
    return s[:, dump["mp"], :]


def _points(dump, order):
    """All points as rows [node rank in `order`, list id (0 point_fix, 1 + ring position), 12 values],
    sorted for the pairing: by node, list, then the coordinates rounded to 1e-6."""
    n, W = dump["rec"].shape[0], dump["W"]
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    ring = np.empty(W, dtype=np.int64)
    ring[dump["mp"]] = np.arange(W)
    fc = np.diff(dump["fix_off"])
    wc = np.diff(dump["win_off"])
    rows = [np.column_stack([np.repeat(rank, fc), np.zeros(int(fc.sum())), dump["fixp"]]) if fc.sum() else
            np.zeros((0, 14))]
    if wc.sum():
        node = np.repeat(np.repeat(rank, W), wc)
        lst = np.repeat(np.tile(1 + ring, n), wc)
        rows.append(np.column_stack([node, lst, dump["winp"]]))
    a = np.concatenate(rows, 0)
    q = np.round(a[:, 2:5] * 1e6)
    idx = np.lexsort((q[:, 2], q[:, 1], q[:, 0], a[:, 1], a[:, 0]))
    return a[idx]


def eig_gap(ev):
    """(l1 - l0) / l2 and (l2 - l1) / l2 per row (inf where no decomposition was ever stored: all zeros)."""
    ev = np.asarray(ev)
    with np.errstate(divide="ignore", invalid="ignore"):
        g01, g12 = (ev[:, 1] - ev[:, 0]) / ev[:, 2], (ev[:, 2] - ev[:, 1]) / ev[:, 2]
    never = ~np.any(ev != 0, axis=1)
    g01[never], g12[never] = np.inf, np.inf
    return g01, g12


def excluded(orc_dump):
    """From the oracle alone: plane leaves, those left out of the ill-conditioned fields
    ((l1 - l0) / l2 < GAP_MIN), those whose eig_vector columns 1 and 2 are compared as a
    projector instead of one by one ((l2 - l1) / l2 < GAP_MIN), and the latter's root keys."""
    r = orc_dump["rec"]
    pl = (r[:, 13] == 0) & (r[:, 15] == 1)
    g01, g12 = eig_gap(r[:, 118:121])
    out = pl & ~(g01 >= GAP_MIN)
    pair = pl & ~out & ~(g12 >= GAP_MIN)
    return int(pl.sum()), int(out.sum()), int(pair.sum()), {key_of(x)[0] for x in r[pair]}


def clu_cov_np(c):
    """PointCluster::cov of rows [N, v3, P6] in long double (the self-checks' quick form)."""
    c = np.asarray(c, dtype=np.longdouble)
    N = c[:, 0:1]
    ce = c[:, 1:4] / N
    P = c[:, [4, 5, 6, 5, 7, 8, 6, 8, 9]] / N
    return (P - (ce[:, :, None] * ce[:, None, :]).reshape(-1, 9)).reshape(-1, 3, 3)


def decomposition_residual(A, ev, evec):
    """max |A v - l v| and |V^T V - I| per row (A: (n, 3, 3), ev: (n, 3), evec: (n, 9) row-major, vectors in columns)."""
    V = np.asarray(evec, dtype=np.longdouble).reshape(-1, 3, 3)
    A = np.asarray(A, dtype=np.longdouble)
    r1 = np.abs(A @ V - V * np.asarray(ev, dtype=np.longdouble)[:, None, :]).reshape(-1, 9).max(1)
    r2 = np.abs(np.transpose(V, (0, 2, 1)) @ V - np.eye(3)).reshape(-1, 9).max(1)
    return r1.astype(np.float64), r2.astype(np.float64)


def pair_projector(evec):
    """V1 V1^T + V2 V2^T of rows of eig_vector (row-major, vectors in columns): (n, 9)."""
    V = np.asarray(evec).reshape(-1, 3, 3)[:, :, 1:]
    return (V @ np.transpose(V, (0, 2, 1))).reshape(-1, 9)


def compare(orc_dump, dev_dump, where, bounds=None):
    """Raise Divergence naming the first difference (where, root key, path, field, both values);
    return the observed maximum of every real field, relative to its bound's scale."""
    bounds = dict(ILL if bounds is None else bounds)
    ro, rd = orc_dump["rec"], dev_dump["rec"]
    oo, ko = _order(ro)
    od, kd = _order(rd)

    def fail(i, field, a, b, note=""):
        key, path = key_of(ko[i]) if i is not None else (None, None)
        raise Divergence("%s: root %s path %s field %s: oracle %s device %s %s" %
                         (where, key, path, field, np.array2string(np.asarray(a), precision=17),
                          np.array2string(np.asarray(b), precision=17), note))

    if ko.shape != kd.shape or not np.array_equal(ko, kd):
        so, sd = {key_of(r) for r in ko}, {key_of(r) for r in kd}
        raise Divergence("%s: key sets differ: %d oracle nodes, %d device nodes; only oracle %s; only device %s" %
                         (where, len(so), len(sd), sorted(so - sd)[:4], sorted(sd - so)[:4]))
    assert orc_dump["W"] == dev_dump["W"] and orc_dump["win_count"] == dev_dump["win_count"], \
        (where, "window", orc_dump["win_count"], dev_dump["win_count"])
    ro, rd = ro[oo], rd[od]
    obs = {}

    def exact(field, a, b):
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        bad = np.any(a != b, axis=1)
        if bad.any():
            i = int(np.argmax(bad))
            fail(i, field, a[i], b[i], "(exact; %d nodes differ)" % int(bad.sum()))

    def real(field, a, b, bound, keep=None):
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        scale = np.maximum(1.0, np.abs(a).max(1))
        dev = np.abs(a - b).max(1) / scale
        dev[np.isnan(dev)] = np.inf
        k = np.ones(a.shape[0], dtype=bool) if keep is None else keep
        obs[field] = max(obs.get(field, 0.0), float(dev[k].max()) if k.any() else 0.0)
        bad = k & ~(dev <= bound)
        if bad.any():
            i = int(np.argmax(bad))
            fail(i, field, a[i], b[i], "(|a - b| / max(1, |oracle|) = %.3e > %.1e; %d nodes over)" %
                 (dev[i], bound, int(bad.sum())))

    for f, c in EXACT.items():
        exact(f, ro[:, c], rd[:, c])
    fo, fd = ro[:, 18], rd[:, 18]
    exact("opt_state >= 0", (fo >= 0).astype(float), (fd >= 0).astype(float))
    exact("opt_state (no factor)", np.where(fo >= 0, -1.0, fo), np.where(fd >= 0, -1.0, fd))
    nf = int((fo >= 0).sum())
    for side, f in (("oracle", fo), ("device", fd)):
        if not np.array_equal(np.sort(f[f >= 0]), np.arange(nf)):
            fail(int(np.argmax(f >= 0)), "opt_state", fo[fo >= 0][:8], fd[fd >= 0][:8],
                 "(the %s's factor indices are not 0 .. %d, each once)" % (side, nf - 1))
    so, sd = ring_slots(orc_dump)[oo], ring_slots(dev_dump)[od]
    exact("sw.points[].size", so[:, :, 0], sd[:, :, 0])
    exact("sw.pcrs_local[].N", so[:, :, 1], sd[:, :, 1])
    for f, c in WELL.items():
        real(f, ro[:, c], rd[:, c], TIGHT)
    W = orc_dump["W"]
    for i in range(W):  # ring position i
        real("sw.pcrs_local", so[:, i, 2:], sd[:, i, 2:], TIGHT)
    # the ill-conditioned fields, with sign; left out below the oracle's gap threshold
    g01, g12 = eig_gap(ro[:, 118:121])
    stable = g01 >= GAP_MIN
    pair = stable & (g12 >= GAP_MIN)
    for f, c in ILL_COLS.items():
        if f == "eig_vector":
            real(f, ro[:, [121, 124, 127]], rd[:, [121, 124, 127]], bounds[f], keep=stable)
            real(f, ro[:, [122, 125, 128, 123, 126, 129]], rd[:, [122, 125, 128, 123, 126, 129]], bounds[f], keep=pair)
            # l1 == l2 to rounding: the pair has no stable value, the plane it spans has
            real("eig_vector (in-plane pair's projector)", pair_projector(ro[:, 121:130]),
                 pair_projector(rd[:, 121:130]), bounds[f], keep=stable & ~pair)
        else:
            real(f, ro[:, c], rd[:, c], bounds[f], keep=stable if f != "eig_value" else None)
    out = ~pair & (rd[:, 35] > 0) & np.any(rd[:, 118:121] != 0, axis=1) & (ro[:, 13] == 0) \
        & (ro[:, 15] == 1)
    if out.any():  # a left-out plane leaf: the device's decomposition of its own cluster still holds
        A = clu_cov_np(rd[out][:, 35:45])
        r1, r2 = decomposition_residual(A, rd[out][:, 118:121], rd[out][:, 121:130])
        sc = np.maximum(1.0, np.abs(A).reshape(-1, 9).max(1).astype(np.float64))
        obs["left-out |A v - l v|"], obs["left-out |V^T V - I|"] = float((r1 / sc).max()), float(r2.max())
        idx = np.flatnonzero(out)
        if not (r1 / sc <= bounds["eig_value"]).all():
            i = int(np.argmax(r1 / sc))
            fail(int(idx[i]), "eig (left-out leaf) |A v - l v|", r1[i], bounds["eig_value"])
        if not (r2 <= bounds["eig_vector"]).all():
            i = int(np.argmax(r2))
            fail(int(idx[i]), "eig (left-out leaf) |V^T V - I|", r2[i], bounds["eig_vector"])
    # the point lists, paired one to one
    po, pd = _points(orc_dump, oo), _points(dev_dump, od)
    if po.shape != pd.shape or not np.array_equal(po[:, :2], pd[:, :2]):
        n = min(po.shape[0], pd.shape[0])
        d = np.flatnonzero(np.any(po[:n, :2] != pd[:n, :2], axis=1))
        i = int(d[0]) if d.size else n - 1
        fail(int(po[i, 0]), "point lists (list 0 point_fix, 1 + ring position)", po[i, :5], pd[i, :5],
             "(%d oracle points, %d device points)" % (po.shape[0], pd.shape[0]))
    for f, c in (("points.pnt", slice(2, 5)), ("points.var", slice(5, 14))):
        a, b = po[:, c], pd[:, c]
        scale = np.maximum(1.0, np.abs(a).max(1)) if a.size else np.ones(0)
        dev = np.abs(a - b).max(1) / scale if a.size else np.zeros(0)
        obs[f] = float(dev.max()) if dev.size else 0.0
        bad = ~(dev <= TIGHT)
        if bad.any():
            i = int(np.argmax(bad))
            fail(int(po[i, 0]), "%s of list %d" % (f, int(po[i, 1])), a[i], b[i],
                 "(unpaired or apart; %d points)" % int(bad.sum()))
    return obs


def same_dump(a, b, where):
    """Two dumps of device maps equal field for field, bit for bit (records in key order, slots in
    ring order, points in list order)."""
    oa, ka = _order(a["rec"])
    ob, kb = _order(b["rec"])
    assert np.array_equal(ka, kb), (where, "keys")
    ra, rb = a["rec"][oa][:, :NODE_REC], b["rec"][ob][:, :NODE_REC]
    bad = np.flatnonzero(np.any(ra.view(np.int64) != rb.view(np.int64), axis=1))
    if bad.size:
        i = int(bad[0])
        c = int(np.flatnonzero(ra[i].view(np.int64) != rb[i].view(np.int64))[0])
        raise Divergence("%s: %s record column %d: %r != %r" % (where, key_of(ka[i]), c, ra[i, c], rb[i, c]))
    sa, sb = ring_slots(a)[oa], ring_slots(b)[ob]
    assert np.array_equal(sa.view(np.int64), sb.view(np.int64)), (where, "window slots")
    pa, pb = _points(a, oa), _points(b, ob)
    assert pa.shape == pb.shape and np.array_equal(pa.view(np.int64), pb.view(np.int64)), (where, "points")


def merge_obs(total, obs):
    for k, v in obs.items():
        total[k] = max(total.get(k, 0.0), v)
    return total
