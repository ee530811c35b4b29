"""tests/view_ref.py, the restatement the GPU tests compare vg_view_gain with,
pinned without a device by properties that do not come from it: the open room's
circle count and symmetry, a closed diamond ring that nothing leaks through, the
diagonal rule in its four orientations, a 5 x 5 grid counted by eye, the
bindings' struct sizes against the header, and view_order's ties."""
import ctypes

import numpy as np
import pytest

import view_ref as vr
import vgpu

U, F, O = vr.UNKNOWN, vr.FREE, vr.OCCUPIED


@pytest.mark.parametrize("R,count", [(1, 5), (2, 13), (3, 29), (7, 149), (20, 1257), (64, 12853)])
def test_open_room(R, count):
    """An all-free grid with the window inside it: the visible set is the disc x^2 + y^2 <= R^2, whole, and so
    invariant under the eight reflections."""
    side = 2 * R + 5
    g = np.zeros((side, side), dtype=np.int8)
    c = side // 2
    rec, seen, s, n_diag = vr.view_gain(g, [[c, c]], R)
    assert vr.circle_count(R) == count
    assert rec[0]["n_visible"] == count == rec[0]["n_free"] and rec[0]["n_rays_open"] == 8 * R and n_diag == 0
    d = np.arange(side) - c
    assert np.array_equal(seen > 0, d[:, None] ** 2 + d[None, :] ** 2 <= R * R)
    vis = vr.visible(g, [[c, c]], R)[0][0]
    for w in (vis[::-1], vis[:, ::-1], vis.T, vis[::-1, ::-1].T):
        assert np.array_equal(w, vis)
    assert s == dict(n_views=1, n_ok=1, n_outside=0, n_blocked=0, rays=8 * R, max_unknown_seen=0, best_view=0,
                     cells_seen=count, unknown_seen=0)


def test_closed_ring():
    """An 8-connected closed diamond, one cell thick: from the centre and four off-centre cells inside, R = 30,
    nothing beyond it is visible; from the centre every cell inside is."""
    g, c = vr.diamond_ring()
    d = np.abs(np.arange(g.shape[0]) - c)
    l1 = d[:, None] + d[None, :]
    for k, (x, y) in enumerate(vr.RING_ORIGINS):
        rec, seen, s, _ = vr.view_gain(g, [[c + x, c + y]], 30)
        assert rec[0]["status"] == vr.OK and not (seen[l1 > vr.RING] > 0).any() and rec[0]["n_unknown"] == 0
        assert rec[0]["n_rays_open"] == 0 and rec[0]["n_occupied"] > 0
        if k == 0:
            assert (seen[l1 < vr.RING] == 1).all() and rec[0]["n_free"] == 181
            assert (seen[l1 == vr.RING] == 1).all() and rec[0]["n_occupied"] == 4 * vr.RING


@pytest.mark.parametrize("fx,fy", [(False, False), (True, False), (False, True), (True, True)])
def test_diagonal_rule(fx, fy):
    """Two occupied cells that touch diagonally block the diagonal step between them, in each orientation; one of
    them alone does not."""
    def flip(g):
        g = g[:, ::-1] if fx else g
        return np.ascontiguousarray(g[::-1] if fy else g)

    g = np.zeros((5, 5), dtype=np.int8)
    g[2, 3] = g[1, 2] = O                    # (3, 2) and (2, 1): the step (2, 2) -> (3, 1) squeezes between them
    rec, seen, s, n_diag = vr.view_gain(flip(g), [[2, 2]], 2)
    hidden = flip(np.arange(25).reshape(5, 5) == 1 * 5 + 3)
    assert seen[hidden] == 0 and n_diag == 3     # the targets (2, -1), (2, -2), (1, -2) all start with that step
    assert rec[0].tolist() == (2, 2, vr.OK, 10, 0, 8, 2, 16 - 3 - 2)
    for one in ((2, 3), (1, 2)):
        h = np.zeros((5, 5), dtype=np.int8)
        h[one] = O
        rec, seen, s, n_diag = vr.view_gain(flip(h), [[2, 2]], 2)
        assert seen[hidden] == 1 and n_diag == 0


def test_hand_cases():
    # origin (2, 2), R = 2: the disc has 13 cells. (2, 1) is occupied and hides (2, 0); (3, 2) and (4, 2) are unknown
    g = np.zeros((5, 5), dtype=np.int8)
    g[1, 2] = O
    g[2, 3] = g[2, 4] = U
    want = np.array([[0, 0, 0, 0, 0],
                     [0, 1, 1, 1, 0],
                     [1, 1, 1, 1, 1],
                     [0, 1, 1, 1, 0],
                     [0, 0, 1, 0, 0]], dtype=np.int32)
    rec, seen, s, n_diag = vr.view_gain(g, [[2, 2]], 2)
    assert np.array_equal(seen, want) and n_diag == 0
    assert rec[0].tolist() == (2, 2, vr.OK, 12, 2, 9, 1, 15)
    # max_unknown = 1: the ray east ends on (3, 2), open, and (4, 2) stays unseen; 2 is as 0 on a ray of two cells
    rec1, seen1, s1, _ = vr.view_gain(g, [[2, 2]], 2, max_unknown=1)
    want1 = want.copy()
    want1[2, 4] = 0
    assert np.array_equal(seen1, want1) and rec1[0].tolist() == (2, 2, vr.OK, 11, 1, 9, 1, 15)
    rec2, seen2, s2, _ = vr.view_gain(g, [[2, 2]], 2, max_unknown=2)
    assert rec2.tobytes() == rec.tobytes() and np.array_equal(seen2, seen)
    # an origin on an unknown cell counts its own cell; the value 50 is free
    g[2, 2], g[2, 1] = U, 50
    rec3, _, _, _ = vr.view_gain(g, [[2, 2]], 2)
    assert rec3[0].tolist() == (2, 2, vr.OK, 12, 3, 8, 1, 15)
    g[2, 2], g[2, 1] = F, F
    # origins outside the grid and on an occupied cell: zero counts, nothing seen; a cell named twice counts twice
    views = [[2, 2], [-1, 0], [2, 1], [2, 2], [5, 5], [0, 7]]
    rec, seen, s, _ = vr.view_gain(g, views, 2)
    assert rec["status"].tolist() == [vr.OK, vr.OUTSIDE, vr.BLOCKED, vr.OK, vr.OUTSIDE, vr.OUTSIDE]
    assert rec[1].tolist() == (-1, 0, vr.OUTSIDE, 0, 0, 0, 0, 0) and rec[2].tolist() == (2, 1, vr.BLOCKED, 0, 0, 0, 0, 0)
    assert np.array_equal(seen, 2 * want) and rec[3].tobytes() == rec[0].tobytes()
    assert s == dict(n_views=6, n_ok=2, n_outside=3, n_blocked=1, rays=32, max_unknown_seen=2, best_view=0,
                     cells_seen=12, unknown_seen=2)
    rec, seen, s, _ = vr.view_gain(g, [[9, 9], [2, 1]], 2)
    assert not seen.any() and s["best_view"] == -1 and s["max_unknown_seen"] == 0 and s["rays"] == 0
    # a corner: the window overhangs the grid, the rays end at its edge
    rec, seen, s, _ = vr.view_gain(np.zeros((5, 5), dtype=np.int8), [[0, 0]], 2)
    assert rec[0].tolist() == (0, 0, vr.OK, 6, 0, 6, 0, 16)


def test_struct_sizes_match_header(tmp_path):
    from test_abi import _c_layout
    for struct, cls in (("vg_view_params", vgpu.ViewParams), ("vg_view_rec", vgpu.ViewRec),
                        ("vg_view_summary", vgpu.ViewSummary)):
        names = [f for f, _ in cls._fields_]
        size, offs = _c_layout(tmp_path, struct, names)
        assert ctypes.sizeof(cls) == size
        assert [getattr(cls, f).offset for f in names] == offs
    assert (ctypes.sizeof(vgpu.ViewParams), ctypes.sizeof(vgpu.ViewRec), ctypes.sizeof(vgpu.ViewSummary)) == (56, 32, 128)
    assert vgpu.VIEW_REC.itemsize == 32 == vr.REC.itemsize and vgpu.VIEW_REC == vr.REC
    assert [vgpu.VIEW_REC.fields[f][1] for f, _ in vgpu.ViewRec._fields_] == \
        [getattr(vgpu.ViewRec, f).offset for f, _ in vgpu.ViewRec._fields_]
    assert (vgpu.VIEW_OK, vgpu.VIEW_OUTSIDE, vgpu.VIEW_BLOCKED, vgpu.VIEW_MAX_RADIUS) == (vr.OK, vr.OUTSIDE, vr.BLOCKED, vr.MAX_RADIUS)
    assert tuple(f for f, _ in vgpu.ViewSummary._fields_ if f != "reserved") == vr.SUMMARY
    assert "vg_view_gain" in vgpu.header_symbols()


def test_view_order_ties():
    r = np.zeros(7, dtype=vr.REC)
    r["n_unknown"] = [6, 3, 6, 0, 9, 2, 12]
    r["status"] = [vr.OK, vr.OK, vr.OK, vr.OK, vr.BLOCKED, vr.OK, vr.OK]
    # without pots: descending gain, equal gains by index; the blocked one and the one below min_gain leave
    assert vgpu.view_order(r).tolist() == [6, 0, 2, 1, 5] == vr.view_order(r).tolist()
    assert vgpu.view_order(r, min_gain=3).tolist() == [6, 0, 2, 1] == vr.view_order(r, min_gain=3).tolist()
    assert vgpu.view_order(r, min_gain=0).tolist() == [6, 0, 2, 1, 5, 3]
    # with pots: gain / (pot + 1). 6 / 2 == 3 / 1 == 12 / 4: the smaller pot first; 6 / 2 twice: the smaller index
    pots = np.array([1, 0, 1, 0, 0, 2 ** 32 - 1, 3], dtype=np.uint32)
    assert vgpu.view_order(r, pots).tolist() == [1, 0, 2, 6, 5] == vr.view_order(r, pots).tolist()
    # the products are exact where a double's are not: 2^31 - 1 unknown cells cannot occur, but pots near 2^32 do
    r2 = np.zeros(2, dtype=vr.REC)
    r2["n_unknown"] = [2 ** 18, 2 ** 18 - 1]
    p2 = np.array([2 ** 32 - 1, 2 ** 32 - 2 ** 14 - 2], dtype=np.uint32)
    assert vgpu.view_order(r2, p2).tolist() == vr.view_order(r2, p2).tolist()
    assert vgpu.view_order(r[:0]).tolist() == [] == vr.view_order(r[:0], pots[:0]).tolist()
    rng = np.random.default_rng(5)
    r3 = np.zeros(300, dtype=vr.REC)
    r3["n_unknown"] = rng.integers(0, 40, 300)
    r3["status"] = rng.integers(0, 3, 300)
    p3 = rng.integers(0, 30, 300).astype(np.uint32) * 1200
    assert vgpu.view_order(r3, p3).tolist() == vr.view_order(r3, p3).tolist()
    assert vgpu.view_order(r3).tolist() == vr.view_order(r3).tolist()
