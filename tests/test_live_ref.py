"""tests/live_ref.py, the numpy restatement of the live obstacle layer, pinned on
the CPU by hand-worked cases and by properties that do not come from it; and the
binding's records against the header (no device)."""
import ctypes

import numpy as np

import live_ref as lr
import view_ref as vr
import vgpu


def _rec(flags, a=(0, 0), b=(0, 0), m=(0, 0), cls=lr.DIFF_APPEARED):
    r = np.zeros(1, dtype=lr.REC)
    r["cls"], r["flags"] = cls, flags
    r["ax"], r["ay"], r["bx"], r["by"], r["mx"], r["my"] = a[0], a[1], b[0], b[1], m[0], m[1]
    return r


def test_ray_cells_are_the_view_gain_cells():
    """For every rim offset of radius R the cells are view gain's closed form, and their union inside the circle
    is view_ref's visible set of an all-free grid."""
    for R in (1, 2, 5, 9):
        t = vr.targets(R)
        seen = np.zeros((2 * R + 1, 2 * R + 1), dtype=bool)
        for dx, dy in t:
            c = lr.ray_cells((0, 0), (dx, dy), with_end=True)
            assert c.shape == (R + 1, 2) and tuple(c[0]) == (0, 0) and tuple(c[-1]) == (dx, dy)
            k = np.arange(R + 1)
            assert np.array_equal(c[:, 0], np.sign(dx) * ((2 * k * abs(dx) + R) // (2 * R)))
            assert np.array_equal(c[:, 1], np.sign(dy) * ((2 * k * abs(dy) + R) // (2 * R)))
            assert np.abs(np.diff(c, axis=0)).max() <= 1
            assert np.array_equal(lr.ray_cells((0, 0), (dx, dy)), c[:-1])
            inside = (c ** 2).sum(axis=1) <= R * R
            stop = inside.argmin() if not inside.all() else R + 1     # the view walk ends at the first cell outside
            seen[c[:stop, 1] + R, c[:stop, 0] + R] = True
        side = 4 * R + 1
        vis, _, _ = vr.visible(np.zeros((side, side), dtype=np.int8), [(2 * R, 2 * R)], R)
        assert np.array_equal(vis[0], seen)


def test_ray_cells_reflections():
    """The cell set is symmetric under the grid's eight reflections, from any start cell."""
    for a in ((0, 0), (3, -7)):
        for d in ((5, 2), (7, 7), (1, 6), (4, 0), (9, 4)):
            base = lr.ray_cells(a, (a[0] + d[0], a[1] + d[1]), with_end=True) - a
            for swap in (False, True):
                for fx in (1, -1):
                    for fy in (1, -1):
                        dd = (d[1], d[0]) if swap else d
                        dd = (fx * dd[0], fy * dd[1])
                        got = lr.ray_cells(a, (a[0] + dd[0], a[1] + dd[1]), with_end=True) - a
                        want = base[:, ::-1] if swap else base
                        assert np.array_equal(got, want * (fx, fy)), (a, d, swap, fx, fy)


def test_hand_worked_beams():
    """n = 0; an axis-aligned beam; an exact diagonal; a shallow beam by hand; the end cell is never cleared."""
    assert lr.ray_cells((4, 4), (4, 4)).shape == (0, 2)
    assert lr.ray_cells((1, 2), (5, 2)).tolist() == [[1, 2], [2, 2], [3, 2], [4, 2]]
    assert lr.ray_cells((1, 2), (1, -1)).tolist() == [[1, 2], [1, 1], [1, 0]]
    assert lr.ray_cells((0, 0), (-3, 3)).tolist() == [[0, 0], [-1, 1], [-2, 2]]
    # (0,0) -> (4,1): n = 4, y_k = (2 k + 4) div 8 = 0, 0, 1, 1, 1: rounding half away from zero at k = 2
    assert lr.ray_cells((0, 0), (4, 1), with_end=True).tolist() == [[0, 0], [1, 0], [2, 1], [3, 1], [4, 1]]
    hit, clear, cnt = lr.planes(_rec(lr.CLEARS | lr.MARKS, a=(0, 0), b=(4, 1), m=(4, 1)), 7, 6, 3)
    want = np.zeros((3, 6), dtype=np.int32)
    want[0, 0] = want[0, 1] = want[1, 2] = want[1, 3] = 7
    assert np.array_equal(clear, want) and clear[1, 4] == 0 and hit[1, 4] == 7 and hit.sum() == 7 and cnt == (1, 0, 1)
    # a == b clears nothing; a mark outside the grid is dropped and counted; a beam from outside clears what it crosses
    hit, clear, cnt = lr.planes(_rec(lr.CLEARS | lr.MARKS, a=(2, 2), b=(2, 2), m=(9, 0)), 3, 6, 3)
    assert not hit.any() and not clear.any() and cnt == (1, 1, 1)
    hit, clear, _ = lr.planes(_rec(lr.CLEARS, a=(-3, 1), b=(8, 1)), 3, 6, 3)
    assert np.array_equal(clear[1], np.full(6, 3)) and clear.sum() == 18
    # maxima: an older stamp never lowers a newer one, in either order
    r1, r2 = _rec(lr.CLEARS, a=(0, 0), b=(5, 0)), _rec(lr.CLEARS, a=(2, 0), b=(2, 2))
    h, c, _ = lr.planes(r1, 9, 6, 3)
    h, c, _ = lr.planes(r2, 4, 6, 3, h, c)
    h2, c2, _ = lr.planes(r2, 4, 6, 3)
    h2, c2, _ = lr.planes(r1, 9, 6, 3, h2, c2)
    assert np.array_equal(c, c2) and c[0].tolist() == [9, 9, 9, 9, 9, 0] and c[1].tolist() == [0, 0, 4, 0, 0, 0]


def _points(xyz, cls, **prm):
    pose = np.concatenate([np.eye(3).reshape(9), [0.5, 0.5, 0.0]])
    return lr.points(np.asarray(xyz, dtype=np.float64), pose, np.eye(3), np.zeros(3), np.asarray(cls), 0.0, 0.0, 1.0,
                     **prm)


def test_points_band_and_cut():
    """The sensor stands at (0.5, 0.5, 0) in cell (0, 0) of a 1 m lattice, band -0.5 .. 1."""
    band = dict(z_lo=-0.5, z_hi=1.0)
    # a level beam to (6.2, 0.5): marks (6, 0), clears from (0, 0) towards (6, 0)
    rec, unc = _points([[5.7, 0.0, 0.0]], [lr.DIFF_APPEARED], **band)
    assert not unc[0] and rec["flags"][0] == lr.MARKS | lr.CLEARS | lr.IN_BAND
    assert (rec["ax"][0], rec["ay"][0], rec["bx"][0], rec["by"][0], rec["mx"][0], rec["my"][0]) == (0, 0, 6, 0, 6, 0)
    # the same beam rising 2 m over 8: leaves the band at z = 1 after half its length, e = (4.5, 0.5): b = (4, 0);
    # its end is above the band and does not mark
    rec, _ = _points([[8.0, 0.0, 2.0]], [lr.DIFF_APPEARED], **band)
    assert rec["flags"][0] == lr.CLEARS | lr.LEFT_BAND and (rec["bx"][0], rec["mx"][0]) == (4, 8)
    # falling: leaves at z = -0.5 after a quarter: e = (2.5, 0.5)
    rec, _ = _points([[8.0, 0.0, -2.0]], [lr.DIFF_CONSISTENT], **band)
    assert rec["flags"][0] == lr.CLEARS | lr.LEFT_BAND and rec["bx"][0] == 2
    # the clear_max cut: level, 5.7 m long, cut at 3 m: e = (3.5, 0.5); the mark stays
    rec, _ = _points([[5.7, 0.0, 0.0]], [lr.DIFF_APPEARED], clear_max=3.0, **band)
    assert rec["flags"][0] == lr.MARKS | lr.CLEARS | lr.IN_BAND | lr.CUT and (rec["bx"][0], rec["mx"][0]) == (3, 6)
    # cut and band exit: whichever comes first names the flag
    rec, _ = _points([[8.0, 0.0, 2.0]], [lr.DIFF_APPEARED], clear_max=3.0, **band)
    assert rec["flags"][0] == lr.CLEARS | lr.CUT
    rec, _ = _points([[8.0, 0.0, 2.0]], [lr.DIFF_APPEARED], clear_max=7.0, **band)
    assert rec["flags"][0] == lr.CLEARS | lr.LEFT_BAND and rec["bx"][0] == 4
    # classes: only APPEARED marks, UNKNOWN with flags bit 0; r_min and mark_max gate the mark, not the beam
    cls = [lr.DIFF_UNKNOWN, lr.DIFF_CONSISTENT, lr.DIFF_APPEARED, lr.DIFF_VANISHED]
    rec, _ = _points([[5.7, 0.0, 0.0]] * 4, cls, **band)
    assert ((rec["flags"] & lr.MARKS) != 0).tolist() == [False, False, True, False]
    rec, _ = _points([[5.7, 0.0, 0.0]] * 4, cls, flags=1, **band)
    assert ((rec["flags"] & lr.MARKS) != 0).tolist() == [True, False, True, False]
    for kw in (dict(r_min=6.0), dict(mark_max=5.0, clear_max=9.0)):
        rec, _ = _points([[5.7, 0.0, 0.0]], [lr.DIFF_APPEARED], **band, **kw)
        assert rec["flags"][0] == lr.CLEARS | lr.IN_BAND
    # clear_max defaults to mark_max where that is set: the beam is cut there, e = (5.5, 0.5)
    rec, unc = _points([[5.7, 0.0, 0.0]], [lr.DIFF_APPEARED], mark_max=5.0, **band)
    assert rec["flags"][0] == lr.CLEARS | lr.IN_BAND | lr.CUT and rec["bx"][0] == 5 and not unc[0]
    # a point at the origin has no beam; a non-finite point has an empty record; a point on a lattice line is uncertain
    rec, unc = _points([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [5.5, 0.0, 0.0]], [lr.DIFF_UNKNOWN] * 3, **band)
    assert rec["flags"].tolist()[:2] == [lr.IN_BAND, 0] and unc.tolist() == [False, False, True]
    # the defaults: band -1 .. 1
    rec, _ = _points([[8.0, 0.0, 0.9], [8.0, 0.0, 1.1]], [lr.DIFF_APPEARED] * 2)
    assert ((rec["flags"] & lr.MARKS) != 0).tolist() == [True, False]


def test_live_rule_and_compose():
    """The three clauses, the tie hit == clear, expiry at now - hit == persist, and the compose's two flags."""
    hit = np.array([[0, 5, 5, 5, 3, 0]], dtype=np.int32)
    clr = np.array([[4, 0, 5, 6, 0, 0]], dtype=np.int32)
    #                never-hit; hit only; tie: live; cleared later; old hit; nothing
    assert lr.live(hit, clr, 6).tolist() == [[False, True, True, False, True, False]]
    assert lr.live(hit, clr, 6, persist=3).tolist() == [[False, True, True, False, False, False]]   # 6 - 3 == 3: gone
    assert lr.live(hit, clr, 5, persist=3).tolist() == [[False, True, True, False, True, False]]    # 5 - 3 < 3
    assert lr.live(hit, clr, 8, persist=3).tolist() == [[False] * 6]                                # 8 - 5 == 3
    base = np.array([[-1, -1, 0, 100, 0, -1]], dtype=np.int8)
    assert lr.compose(base, hit, clr, 6).tolist() == [[-1, 100, 100, 100, 100, -1]]
    assert lr.compose(base, hit, clr, 6, flags=1).tolist() == [[0, 100, 100, 100, 100, -1]]
    assert lr.compose(base, hit, clr, 8, persist=3, flags=1).tolist() == [[-1, -1, 0, 100, 0, -1]]   # 8 - 4 >= 3
    assert lr.compose(base, hit, clr, 6, persist=3, flags=1).tolist() == [[0, 100, 100, 100, 0, -1]]
    assert base.tolist() == [[-1, -1, 0, 100, 0, -1]]                                               # untouched


def test_binding_matches_the_header(tmp_path):
    """The header declares the entry points; the binding's records have the header's layout."""
    from test_abi import _c_layout
    assert all(s in vgpu.header_symbols() for s in ("vg_live_begin", "vg_live_mark", "vg_live_mark_dev",
                                                    "vg_live_compose", "vg_live_info", "vg_live_clear", "vg_live_end"))
    for struct, ct in (("vg_live_params", vgpu.LiveParams), ("vg_live_summary", vgpu.LiveSummary)):
        names = [f for f, _ in ct._fields_]
        size, offs = _c_layout(tmp_path, struct, names)
        assert ctypes.sizeof(ct) == size and [getattr(ct, f).offset for f in names] == offs
    names = list(vgpu.LIVE_POINT_DTYPE.names)
    size, offs = _c_layout(tmp_path, "vg_live_point", names)
    assert vgpu.LIVE_POINT_DTYPE.itemsize == size == 32 == lr.REC.itemsize
    assert [vgpu.LIVE_POINT_DTYPE.fields[f][1] for f in names] == offs
    assert lr.REC == vgpu.LIVE_POINT_DTYPE
    assert (vgpu.LIVE_MARKS, vgpu.LIVE_CLEARS, vgpu.LIVE_IN_BAND, vgpu.LIVE_CUT, vgpu.LIVE_LEFT_BAND) == (
        lr.MARKS, lr.CLEARS, lr.IN_BAND, lr.CUT, lr.LEFT_BAND)
