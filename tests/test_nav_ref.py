"""The navigation function's numpy restatement (tests/nav_ref.py) pinned without a
device: against scipy's Dijkstra on an edge list built here, cell pair by cell
pair, multi-source and with the no-corner-cutting rule; against hand-computed
values; and the Python helpers around vg_navfn that need no device."""
import ctypes

import numpy as np
import pytest

import nav_ref as nr
import vgpu
from test_abi import _c_layout

PLANES = [(61, 47, 7), (130, 130, 8), (33, 64, 9)]       # nx, ny, seed; the first is test_navfn_gpu's


def _dijkstra(cost, trav, goals):
    """pot by scipy over the definition's graph, its edges listed one by one."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra
    ny, nx = cost.shape
    t = trav.astype(np.int64)[cost]
    rows, cols, wts = [], [], []
    for ay in range(ny):
        for ax in range(nx):
            if not t[ay, ax]:
                continue
            for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 1)):      # each undirected edge once
                bx, by = ax + dx, ay + dy
                if not (0 <= bx < nx and 0 <= by < ny) or not t[by, bx]:
                    continue
                if dx and dy and not (t[ay, bx] and t[by, ax]):
                    continue
                rows.append(ay * nx + ax)
                cols.append(by * nx + bx)
                wts.append((17 if dx and dy else 12) * (t[ay, ax] + t[by, bx]))
    g, _ = nr.used_goals(cost, trav, goals)
    if not g.shape[0]:
        return np.full((ny, nx), nr.UNREACHED, dtype=np.uint32)
    m = coo_matrix((np.array(wts, dtype=np.float64), (rows, cols)), shape=(nx * ny, nx * ny)).tocsr()
    d = dijkstra(m, directed=False, indices=(g[:, 1] * nx + g[:, 0]).tolist(), min_only=True)
    d = np.where(t.ravel() > 0, d, np.inf)
    return np.where(np.isinf(d), nr.UNREACHED, np.minimum(d, nr.SAT)).astype(np.uint32).reshape(ny, nx)


@pytest.mark.parametrize("nx,ny,seed", PLANES)
@pytest.mark.parametrize("flags", [0, 1])
def test_potential_is_scipys_dijkstra(nx, ny, seed, flags):
    cost = nr.random_plane(nx, ny, seed)
    trav = nr.trav_table(flags=flags, unknown_as=100)
    goals = np.concatenate([nr.passable_cells(cost, trav, 2, seed), [[-1, 3], [nx, 0]]])
    lethal = np.argwhere(trav[cost] == 0)[0]
    goals = np.concatenate([goals, [[lethal[1], lethal[0]]]])
    pot = nr.potential(cost, trav, goals)
    assert np.array_equal(pot, _dijkstra(cost, trav, goals))
    s = nr.summary(cost, trav, goals, pot)
    assert (s["n_goals_used"], s["n_goals_ignored"]) == (2, 3) and 0 < s["cells_reached"] <= s["cells_passable"]
    assert (pot[trav[cost] == 0] == nr.UNREACHED).all() and s["cells_saturated"] == 0
    assert ((cost == 255) & (pot != nr.UNREACHED)).any() == bool(flags)


def test_default_table():
    t = nr.trav_table()
    assert t[0] == 50 and t[1] == 50 and t[2] == 51 and t[252] == 50 + 201 and not t[253:].any()
    assert np.array_equal(t, vgpu.nav_trav_table())
    kw = dict(flags=1, neutral=66, lethal_from=200, unknown_as=120, factor=3.0)
    t = nr.trav_table(**kw)
    assert t[199] == 66 + 597 and not t[200:255].any() and t[255] == t[120] == 426
    assert np.array_equal(t, vgpu.nav_trav_table(**kw))
    for bad in (dict(neutral=-1), dict(lethal_from=256), dict(unknown_as=255), dict(flags=2), dict(factor=-0.5),
                dict(factor=float("nan")), dict(factor=300.0), dict(neutral=65500, factor=1.0)):
        with pytest.raises(ValueError):
            vgpu.nav_trav_table(**bad)


def test_by_hand():
    """An open 3 x 3 plane of cost 0 (50 a cell): from the centre an edge cell is 12 (50 + 50), a corner 17 (50 +
    50). With the goal in a corner and the two cells beside it lethal, nothing else is reached: the only way out
    would cut the corner between them."""
    trav = nr.trav_table()
    c = np.zeros((3, 3), dtype=np.uint8)
    pot = nr.potential(c, trav, [[1, 1]])
    assert pot.tolist() == [[1700, 1200, 1700], [1200, 0, 1200], [1700, 1200, 1700]]
    pot = nr.potential(c, trav, [[0, 0]])
    assert pot.tolist() == [[0, 1200, 2400], [1200, 1700, 2900], [2400, 2900, 3400]]
    c[0, 1] = c[1, 0] = 254
    pot = nr.potential(c, trav, [[0, 0]])
    assert pot[0, 0] == 0 and pot[1, 1] == nr.UNREACHED and (pot.ravel()[1:] == nr.UNREACHED).all()
    c[1, 0] = 0                                                      # one of the pair opened: round the other way
    pot = nr.potential(c, trav, [[0, 0]])
    assert pot[1, 0] == 1200 and pot[1, 1] == 2400 and pot[0, 1] == nr.UNREACHED and pot[0, 2] == 2400 + 1200 + 1200
    cells, ln, status, pc = nr.descend(c, trav, pot, [[2, 0], [1, 0], [5, 5]], 8)
    assert cells[0, :ln[0]].tolist() == [2, 5, 4, 3, 0] and status.tolist() == [nr.REACHED, nr.NO_PATH, nr.NO_PATH]
    assert pc.tolist() == [4800, -1, -1] and ln.tolist() == [5, 0, 0]
    cells, ln, status, pc = nr.descend(c, trav, pot, [[2, 0]], 3)
    assert cells[0].tolist() == [2, 5, 4] and status[0] == nr.TRUNCATED and ln[0] == 3


def test_saturation_and_serpentine():
    """A corridor priced at 65535 a cell: 12 * 131070 a step, saturated past step 2730. The serpentine's far end:
    6631 orthogonal steps of 1200."""
    trav = np.full(256, 65535, dtype=np.uint16)
    c = np.zeros((1, 4000), dtype=np.uint8)
    pot = nr.potential(c, trav, [[0, 0]])
    k = np.arange(4000, dtype=np.int64)
    assert 12 * 131070 * 2730 < nr.SAT < 12 * 131070 * 2731
    assert np.array_equal(pot[0], np.where(k <= 2730, 12 * 131070 * k, nr.SAT))
    cells, ln, status, pc = nr.descend(c, trav, pot, [[3000, 0], [2000, 0], [2731, 0]], 4000)
    assert status.tolist() == [nr.STUCK, nr.REACHED, nr.REACHED] and ln.tolist() == [1, 2001, 2732] and pc[0] == nr.SAT
    s = nr.serpentine()
    pot = nr.potential(s, nr.trav_table(), [[0, 0]])
    assert nr.summary(s, nr.trav_table(), [[0, 0]], pot)["max_pot"] == 7_957_200 == 1200 * 6631
    assert pot[64, 199] == 7_957_200 and np.array_equal(pot, _dijkstra(s, nr.trav_table(), [[0, 0]]))


def test_struct_layouts_and_helpers(tmp_path):
    size, off = _c_layout(tmp_path, "vg_nav_params", [f for f, _ in vgpu.NavParams._fields_])
    assert size == ctypes.sizeof(vgpu.NavParams) == 64
    assert off == [getattr(vgpu.NavParams, f).offset for f, _ in vgpu.NavParams._fields_]
    size, off = _c_layout(tmp_path, "vg_nav_summary", [f for f, _ in vgpu.NavSummary._fields_])
    assert size == ctypes.sizeof(vgpu.NavSummary) == 128
    assert off == [getattr(vgpu.NavSummary, f).offset for f, _ in vgpu.NavSummary._fields_]
    assert (vgpu.NAV_SAT, vgpu.NAV_UNREACHED, vgpu.NAV_K_ORTHO, vgpu.NAV_K_DIAG) == (nr.SAT, nr.UNREACHED, 12, 17)
    assert (vgpu.NAV_REACHED, vgpu.NAV_NO_PATH, vgpu.NAV_TRUNCATED, vgpu.NAV_STUCK) == (0, 1, 2, 3)
    assert set(nr.REPRODUCIBLE) | set(vgpu.NAV_SCHEDULING) == {f for f, _ in vgpu.NavSummary._fields_} - {"reserved"}
    xy = vgpu.cells_to_world([0, 7, 23], nx=10, x0=-1.0, y0=2.0, res=0.5)
    assert xy.tolist() == [[-0.75, 2.25], [2.75, 2.25], [0.75, 3.25]]
