"""tests/frontier_ref.py, the restatement the GPU tests compare vg_frontiers with,
pinned without a device: its labels against scipy.ndimage.label with a 3 x 3
structure at the shapes the GPU tests use, the hand cases of the definition, the
generators' promised properties, the bindings' struct sizes against the header,
and frontier_order's ties."""
import ctypes

import numpy as np
import pytest

import clr_ref as cr
import frontier_ref as fr
import vgpu

# (nx, ny, seed, p_unknown) of tests/test_frontiers_gpu.py's random grids
SHAPES = [(61, 47, 7, 0.07), (130, 67, 11, 0.07), (67, 130, 11, 0.07)]


def _scipy_labels(m):
    """scipy's 8-connected labels of m, renamed to each component's smallest linear index; -1 off m."""
    from scipy import ndimage
    lab, n = ndimage.label(m, structure=np.ones((3, 3), dtype=int))
    idx = np.arange(m.size).reshape(m.shape)
    lo = ndimage.minimum(idx, lab, index=np.arange(1, n + 1)).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    return np.where(lab > 0, np.concatenate([[-1], lo])[lab], -1).astype(np.int32), n


@pytest.mark.parametrize("nx,ny,seed,p_unknown", SHAPES)
def test_labels_equal_scipy(nx, ny, seed, p_unknown):
    g = cr.random_grid(nx, ny, seed, p_unknown=p_unknown)
    m, _, _ = fr.mask(g)
    lab = fr.labels(m)
    want, n = _scipy_labels(m)
    assert np.array_equal(lab, want)
    rec = fr.records(lab)
    assert rec.size == n and rec["size"].sum() == m.sum() and (np.diff(rec["label"]) > 0).all()
    if nx > 64:      # what the GPU test relies on: many components, many of them across a tile border
        assert n >= 100 and fr.spanning(lab) >= 10


def test_with_cost_and_pot_equal_scipy():
    """The two optional tests only thin the mask out; the labels of the thinner mask equal scipy's too."""
    import nav_ref as nr
    g = cr.random_grid(130, 67, 11, p_unknown=0.07)
    c = cr.clearance(g, **cr.PARAMS["nav"])["cost"]
    pot = nr.potential(c, nr.trav_table(), [[int(np.argwhere(c == 0)[0][1]), int(np.argwhere(c == 0)[0][0])]])
    plain, _, _ = fr.mask(g)
    for kw in (dict(cost=c), dict(pot=pot), dict(cost=c, pot=pot), dict(cost=c, cost_max=40)):
        m, n_rc, n_ru = fr.mask(g, **kw)
        assert not (m & ~plain).any() and m.sum() + n_rc + n_ru == plain.sum() and 0 < m.sum() < plain.sum()
        assert np.array_equal(fr.labels(m), _scipy_labels(m)[0])
    lab, rec, s = fr.frontiers(g, cost=c, pot=pot)
    assert s["n_rejected_cost"] > 0 and s["n_rejected_unreached"] > 0
    p = pot.ravel()
    for r in rec:
        idx = np.flatnonzero(lab.ravel() == r["label"])
        assert r["best_pot"] == p[idx].min() and r["best_cell"] == idx[p[idx] == p[idx].min()][0]


def test_hand_cases():
    U, F, O = fr.UNKNOWN, fr.FREE, fr.OCCUPIED
    # two free cells touching only diagonally, each beside an unknown: one frontier
    g = np.array([[U, F, O],
                  [O, O, F],
                  [O, O, U]], dtype=np.int8)
    lab, rec, s = fr.frontiers(g)
    assert lab.ravel().tolist() == [-1, 1, -1, -1, -1, 1, -1, -1, -1] and s["n_components"] == 1
    assert rec[0].tolist()[:10] == (1, 2, 1, 0, 2, 1, 3, 1, -1, 0)
    # a free cell whose only unknown neighbour is diagonal is no frontier cell
    g = np.array([[U, O],
                  [O, F]], dtype=np.int8)
    assert not fr.mask(g)[0].any()
    # a free cell on the grid's edge with no unknown neighbour: outside the grid is not unknown
    g = np.array([[F, F, O]], dtype=np.int8)
    assert not fr.mask(g)[0].any()
    # the value 50 is free for vg_clearance and not free here
    g = np.array([[50, U, F]], dtype=np.int8)
    assert fr.mask(g)[0].ravel().tolist() == [False, False, True]
    # the cost test comes before the reach test
    g = np.array([[F, U, F]], dtype=np.int8)
    m, n_rc, n_ru = fr.mask(g, cost=np.array([[253, 255, 0]], dtype=np.uint8),
                            pot=np.array([[fr.UNREACHED, fr.UNREACHED, fr.UNREACHED]], dtype=np.uint32))
    assert not m.any() and (n_rc, n_ru) == (1, 1)


def test_generators():
    g = fr.serpentine_grid()
    lab, rec, s = fr.frontiers(g)
    assert g.shape == (65, 200) and s["n_components"] == 1 and rec[0]["label"] == 0 and rec[0]["size"] == 6630
    assert np.array_equal(lab, _scipy_labels(fr.mask(g)[0])[0])
    # the corridor changes tile along every free row: 3 borders a row, 33 rows
    on = lab >= 0
    assert int((on[:, 63] & on[:, 64]).sum() + (on[:, 127] & on[:, 128]).sum() + (on[:, 191] & on[:, 192]).sum()) == 99
    g = fr.rooms(256, 192, 3)
    lab, rec, s = fr.frontiers(g)
    assert s["n_components"] >= 10 and np.median(rec["size"]) >= 8 and fr.spanning(lab) >= 3
    assert np.array_equal(lab, _scipy_labels(fr.mask(g)[0])[0])


def test_struct_sizes_match_header(tmp_path):
    from test_abi import _c_layout
    for struct, cls in (("vg_frontier_params", vgpu.FrontierParams), ("vg_frontier_rec", vgpu.FrontierRec),
                        ("vg_frontier_summary", vgpu.FrontierSummary)):
        names = [f for f, _ in cls._fields_]
        size, offs = _c_layout(tmp_path, struct, names)
        assert ctypes.sizeof(cls) == size
        assert [getattr(cls, f).offset for f in names] == offs
    assert (ctypes.sizeof(vgpu.FrontierParams), ctypes.sizeof(vgpu.FrontierRec), ctypes.sizeof(vgpu.FrontierSummary)) == (56, 64, 128)
    assert vgpu.FRONTIER_REC.itemsize == 64 == fr.REC.itemsize and vgpu.FRONTIER_REC == fr.REC
    assert [vgpu.FRONTIER_REC.fields[f][1] for f, _ in vgpu.FrontierRec._fields_] == \
        [getattr(vgpu.FrontierRec, f).offset for f, _ in vgpu.FrontierRec._fields_]
    assert vgpu.FRONTIER_MAX_RECORDS == fr.MAX_RECORDS
    assert tuple(f for f, _ in vgpu.FrontierSummary._fields_ if f != "reserved") == fr.SUMMARY


def test_frontier_order_ties():
    r = np.zeros(5, dtype=fr.REC)
    r["label"] = [40, 3, 17, 9, 25]
    r["size"] = [5, 9, 5, 9, 1]
    r["best_cell"] = -1
    # without best: descending size, equal sizes by ascending label
    assert fr.frontier_order(r).tolist() == [1, 3, 2, 0, 4] == vgpu.frontier_order(r).tolist()
    r["best_cell"] = [41, 3, 18, 9, 25]
    r["best_pot"] = [700, 2 ** 32 - 2, 700, 0, 700]
    # with best: ascending best_pot (unsigned), equal ones by ascending label; size plays no part
    assert fr.frontier_order(r).tolist() == [3, 2, 4, 0, 1] == vgpu.frontier_order(r).tolist()
    assert vgpu.frontier_order(r[:0]).tolist() == [] == fr.frontier_order(r[:0]).tolist()
    g = cr.random_grid(61, 47, 7, p_unknown=0.07)
    _, rec, _ = fr.frontiers(g)
    assert fr.frontier_order(rec).tolist() == vgpu.frontier_order(rec).tolist()
