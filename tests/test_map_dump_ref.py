"""The oracle's node-for-node map dump (orc_map_nodes, tests/map_dump.py) on
the 16-line sequence, oracle alone (no GPU): it agrees with orc_roots, its
tree links are closed, its window lists account for every downsampled point
and pcrs_local is the cluster of the listed points. Also from the oracle
alone: the share of plane leaves that tests/test_map_nodes_gpu.py leaves out
of the ill-conditioned fields (at most 0.5 % in every case), the small
max_points case reaches margi's full-leaf branch, and
profiles/map_nodes/observed.json carries the bounds map_dump.py applies."""
import json
import os

import numpy as np

import map_dump as MD
import oracle
import vgconfig
from test_map_nodes_gpu import CASES, SMALL_MAX_POINTS, sequence

import insert_edge_input as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(name, **extra):
    cfgname, lidar, seq_id, nscan, kw = CASES[name]
    p = vgconfig.load(cfgname)
    seq = sequence(p, lidar, seq_id)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0, **{**kw, **extra}))
    orc.seed(seq.gt_state(0))
    return p, seq, nscan, orc


def _step(orc, seq, k):
    xyz, it, b, e = seq.scan(k)
    orc.step(xyz, it, b, e, seq.imu(k))


def test_dump_is_consistent(oracle_lib):
    p, seq, nscan, orc = _oracle("mid360")
    W, max_layer = p["LocalBA"]["win_size"], p["LocalBA"]["max_layer"]
    n_ds = []
    for k in range(nscan):
        _step(orc, seq, k)
        n_ds.append(orc.stats()["n_ds"])
        d = orc.map_nodes()
        r = d["rec"]
        assert d["W"] == W and sorted(d["mp"]) == list(range(W))
        keys = [MD.key_of(x) for x in r]
        index = {key: i for i, key in enumerate(keys)}
        assert len(index) == len(keys)
        # against orc_roots: nodes and point_fix per root, isexist, jour
        roots = orc.roots()
        nodes, nfix = {}, {}
        for i, (root, path) in enumerate(keys):
            nodes[root] = nodes.get(root, 0) + 1
            nfix[root] = nfix.get(root, 0) + int(r[i, 130])
        assert nodes.keys() == roots.keys()
        for root, (jour, flags, nn, nf) in roots.items():
            i = index[(root, ())]
            assert (nodes[root], nfix[root]) == (nn, nf), (k, root)
            assert int(r[i, 14]) == (flags >> 1) & 1 and r[i, 24] == jour, (k, root)
        assert np.array_equal(np.diff(d["fix_off"]), r[:, 130].astype(np.int64))
        # every child mask matches the records present, and only internal nodes have children
        for i, (root, path) in enumerate(keys):
            mask = sum(1 << o for o in range(8) if (root, path + (o,)) in index)
            assert int(r[i, 16]) == mask, (k, root, path)
            assert mask == 0 or int(r[i, 13]) == 1, (k, root, path)
            assert int(r[i, 12]) == len(path) and (not path or (root, path[:-1]) in index)
        # the window lists: per scan of the window, n_ds less the points the deepest layer keeps unlisted
        s = MD.ring_slots(d)
        assert np.array_equal(np.diff(d["win_off"]).reshape(-1, W)[:, d["mp"]], s[:, :, 0].astype(np.int64))
        assert not s[r[:, 19] == 0].any()
        deepest = r[:, 12] >= max_layer
        for i in range(d["win_count"]):
            scan = k - d["win_count"] + 1 + i
            listed, unlisted = int(s[:, i, 0].sum()), int(s[deepest, i, 1].sum())
            assert listed == n_ds[scan] - unlisted, (k, i, scan, listed, unlisted, n_ds[scan])
            assert not s[deepest, i, 0].any()
        assert not s[:, d["win_count"]:, :].any()
        # pcrs_local of a listed slot is the cluster of its points
        wo = d["win_off"]
        lst = np.flatnonzero(np.diff(wo) > 0)
        for j in lst[:: max(1, lst.size // 400)]:
            node, slot = divmod(int(j), W)
            pts = d["winp"][wo[j]:wo[j + 1], 0:3]
            c = r[node, MD.NODE_REC + MD.NODE_SLOT * slot:][:MD.NODE_SLOT]
            assert int(c[0]) == pts.shape[0] == int(c[1])
            P = pts.T @ pts
            ref = np.concatenate([pts.sum(0), P[np.triu_indices(3)]])
            assert np.abs(c[2:] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    assert d["win_count"] == W - 1
    orc.close()


def _shares(orc, stepper, n, grid_roots=()):
    """Worst dump of the case: (plane leaves, left out, eig_vector columns 1-2 compared as a projector)."""
    worst = (0, 0, 0)
    for k in range(n):
        stepper(k)
        planes, out, pair, roots = MD.excluded(orc.map_nodes())
        if planes and (out + pair) * max(worst[0], 1) >= (worst[1] + worst[2]) * planes:
            worst = (planes, out, pair)
        assert out <= 0.005 * planes, (k, planes, out)
        if grid_roots:  # exact grids: l1 == l2 to rounding at any threshold, and only there
            assert roots <= set(grid_roots), (k, roots)
        else:
            assert out + pair <= 0.005 * planes, (k, planes, out, pair)
    return worst


def test_left_out_share_per_case(oracle_lib):
    """At most 0.5 % of the plane leaves of any dump of any case are left out
    of the ill-conditioned fields ((l1 - l0) / l2 below map_dump.GAP_MIN, the
    oracle's own eigenvalues); the worst dump per case is printed. Leaves whose
    in-plane eigenvalues alone coincide ((l2 - l1) / l2 below GAP_MIN) stay
    under the oracle comparison in every field, their eigenvector pair as the
    projector of the plane it spans; they too are at most 0.5 % everywhere but
    in the insert-edge sequence, whose blocks are exact 0.18 m grids with
    l1 == l2 to rounding whatever the threshold (8 of ~450 plane leaves from
    scan 3 on, asserted to lie in the grid blocks' root voxels and nowhere
    else)."""
    for name in CASES:
        p, seq, nscan, orc = _oracle(name)
        full = []

        def stepper(k):
            _step(orc, seq, k)
            full.append(orc.stats()["fix_full"])
        print(name, "plane leaves / left out (worst dump):", _shares(orc, stepper, nscan))
        if name == "small-max-points":
            assert SMALL_MAX_POINTS < 100 and sum(full) > 0, full
        orc.close()
    # the release case's sequence, up to the release that erases roots (test_map_nodes_gpu)
    p = vgconfig.load("mid360")
    seq = sequence(p, "16line", 7)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0, release_dis=4))
    orc.seed(seq.gt_state(0))
    erased = []

    def stepper(k):
        _step(orc, seq, k)
        erased.append(orc.release_far()[0])
    print("release", _shares(orc, stepper, 22))
    assert max(erased) > 0, erased
    orc.close()
    p = E.config(vgconfig)
    seq, scans, keys = E.make(p)
    orc = oracle.Pipeline(vgconfig.to_c(p, use_threads=0, vnc_prep=0))
    orc.seed(seq.gt_state(0))
    print("insert edge shapes", _shares(orc, lambda k: orc.step(*scans[k]), len(scans),
                                        grid_roots=[tuple(key) for key in keys]))
    orc.close()


def test_bounds_follow_the_measurement():
    """profiles/map_nodes/observed.json: each ill-conditioned bound in map_dump.py is 100 x the
    maximum measured on the first case, rounded up to a power of ten, and at most 1e-6."""
    with open(os.path.join(REPO, "profiles", "map_nodes", "observed.json")) as f:
        j = json.load(f)
    assert j["gap_min"] == MD.GAP_MIN
    for field, bound in MD.ILL.items():
        assert bound <= MD.ILL_CAP
        assert j["bounds"][field] == bound == MD.ill_bound(j["observed"][field], field), field
