"""The ray-cast's numpy restatement (tests/raycast_ref.py) against hand-made
leaf records with known answers, and the layout of the four new C structs
against a C compiler (no GPU)."""
import ctypes

import numpy as np

import raycast_ref as rr
import vgpu
from test_abi import _c_layout


def _leaf(vc, ql, c, n):
    p = np.zeros(1, dtype=vgpu.MARKER_DTYPE)
    p["voxel_center"], p["quater_length"], p["center"], p["normal"] = vc, ql, c, n
    return p


WALL = _leaf((2.25, 0.25, 0.25), 0.125, (2.2, 0.3, 0.2), (1.0, 0.0, 0.0))   # the plane x = 2.2 in the cube [2, 2.5] x [0, 0.5]^2


def test_head_on():
    t, i, near = rr.cast(WALL, (0.0, 0.25, 0.25), [(1.0, 0.0, 0.0), (2.0, 0.0, 0.0)])
    assert np.allclose(t, 2.2, rtol=0, atol=1e-15) and list(i) == [0, 0] and not near.any()   # any length of d


def test_plane_met_outside_the_cube_is_a_miss():
    t, i, _ = rr.cast(WALL, (0.0, 0.75, 0.25), [(1.0, 0.0, 0.0)])   # meets x = 2.2 at y = 0.75
    assert np.isinf(t[0]) and i[0] == -1
    t, i, near = rr.cast(WALL, (0.0, 0.5, 0.25), [(1.0, 0.0, 0.0)])  # on the face y = 0.5: inclusive, and flagged
    assert t[0] == 2.2 and i[0] == 0 and near[0]


def test_the_nearer_of_two_cubes_wins():
    two = np.concatenate([_leaf((4.25, 0.25, 0.25), 0.125, (4.4, 0.25, 0.25), (-1.0, 0.0, 0.0)), WALL])
    t, i, _ = rr.cast(two, (0.0, 0.25, 0.25), [(1.0, 0.0, 0.0)])
    assert t[0] == 2.2 and i[0] == 1
    t, i, _ = rr.cast(two, (0.0, 0.25, 0.25), [(1.0, 0.0, 0.0)], t_min=2.2)   # the interval is open below
    assert abs(t[0] - 4.4) < 1e-15 and i[0] == 0
    t, i, _ = rr.cast(two, (3.0, 0.25, 0.25), [(1.0, 0.0, 0.0)])              # past the first plane: not behind
    assert abs(t[0] - 1.4) < 1e-15 and i[0] == 0
    t, i, _ = rr.cast(two, (0.0, 0.25, 0.25), [(1.0, 0.0, 0.0)], t_max=2.0)
    assert np.isinf(t[0]) and i[0] == -1


def test_a_grazing_plane_is_passed_through():
    s = np.sin(np.deg2rad(2.0))   # |n.d| = 0.0349 < 0.05
    graze = _leaf((2.25, 0.25, 0.25), 0.125, (2.25, 0.25, 0.25), (s, np.cos(np.deg2rad(2.0)), 0.0))
    both = np.concatenate([graze, _leaf((4.25, 0.25, 0.25), 0.125, (4.4, 0.25, 0.25), (1.0, 0.0, 0.0))])
    t, i, _ = rr.cast(both, (0.0, 0.25, 0.25), [(1.0, 0.0, 0.0)])
    assert abs(t[0] - 4.4) < 1e-15 and i[0] == 1
    t, i, _ = rr.cast(both, (0.0, 0.25, 0.25), [(1.0, 0.0, 0.0)], min_cos=0.03)
    assert abs(t[0] - 2.25) < 1e-12 and i[0] == 0


def test_diff_rule():
    h = np.zeros(5, dtype=vgpu.RAY_HIT_DTYPE)
    h["flags"] = (1, 1, 1, 0, 1)
    h["range"] = (10.0, 11.0, 8.0, 0.0, 13.0)   # the reach at 10 m: 11.53 m
    h["ndotd"], h["var"], h["leaf"] = -1.0, 0.0, (3, 4, 5, -1, 6)
    cls, leaf, r_map, gate, margin = rr.diff_rule(h, np.full(5, 10.0))
    assert list(cls) == [1, 2, 3, 0, 0] and list(leaf) == [3, 4, 5, -1, -1]   # 13 m: past the search's reach
    assert np.allclose(gate[:3], 3 * rr.DEPT) and gate[3] == 0 and r_map[4] == 0
    assert rr.diff_rule(h, np.full(5, 10.0), gate_floor=2.5)[0].tolist() == [1, 1, 1, 0, 0]


def test_new_struct_layouts_match_the_header(tmp_path):
    for name, st in (("vg_ray_params", vgpu.RayParams), ("vg_ray_hit", vgpu.RayHit),
                     ("vg_diff_params", vgpu.DiffParams), ("vg_diff_point", vgpu.DiffPoint),
                     ("vg_diff_summary", vgpu.DiffSummary)):
        names = [f for f, _ in st._fields_]
        size, offs = _c_layout(tmp_path, name, names)
        assert ctypes.sizeof(st) == size, name
        assert [getattr(st, f).offset for f in names] == offs, name
    assert ctypes.sizeof(vgpu.RayHit) == 64 == vgpu.RAY_HIT_DTYPE.itemsize
    assert ctypes.sizeof(vgpu.DiffPoint) == 32 == vgpu.DIFF_POINT_DTYPE.itemsize
    for dt, st in ((vgpu.RAY_HIT_DTYPE, vgpu.RayHit), (vgpu.DIFF_POINT_DTYPE, vgpu.DiffPoint)):
        assert [dt.fields[f][1] for f, _ in st._fields_] == [getattr(st, f).offset for f, _ in st._fields_]
