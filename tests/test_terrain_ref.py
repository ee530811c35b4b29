"""The terrain layer's numpy restatement (tests/terrain_ref.py) pinned on hand-made
rays and records, no device: a flat floor, a 30 degree ramp, a platform seen from
above and from below, a wall whose base cell has no elevation (the carried
reference), a negative g_sum (floor division), the pending free mark of a hit's
cell both ways, and the pieces around vgpu's terrain files and records.

One row of 8 cells of 1 m along x (y in (0, 1)), heights in centimetres (z_res =
0.01). The floor lies at z = 0.0037 so that no quantised height sits on an integer."""
import ctypes
import math

import numpy as np

import terrain_ref as tr
import vgpu

GEOM = dict(x0=0.0, y0=0.0, res=1.0, nx=8, ny=1)
O = (0.5, 0.5, 1.0037)   # a sensor 1 m above the floor


def ray(o, to, nz):
    """A ray from o that hits at the point `to` on a plane with normal[2] = nz: (o, dir, r, nz)."""
    v = np.subtract(to, o)
    return np.asarray(o, float), v, float(np.linalg.norm(v)), nz


def run(rays, elev=None, **kw):
    P = tr.defaults(**GEOM, z_res=0.01, **kw)
    o, d, r, nz = (np.array([x[i] for x in rays], dtype=np.float64) for i in range(4))
    out = tr.terrain(o, d, r, nz, P, elev=elev)
    assert not out["uncertain"].any()
    return out


def test_flat_floor():
    """Floor hits are ground and never obstacles; the cells before the hit are free while the ray is 0.15 .. 1.5 m
    above the ground, the last one (6 cm above it) is not."""
    out = run([ray(O, (2.5, 0.5, 0.0037), 1.0), ray(O, (4.5, 0.5, 0.0037), 1.0)], sensor_height=1.0)
    g_n, g_sum, g_min, g_max = out["planes"]
    assert g_n[0].tolist() == [0, 0, 1, 0, 1, 0, 0, 0] and not g_sum.any() and out["ground"].all()
    assert out["elev"][0].tolist() == [tr.NONE, tr.NONE, 0, tr.NONE, 0, tr.NONE, tr.NONE, tr.NONE]
    assert not out["step"].any() and out["stats"] == (2, 0, 0)
    assert not out["counts"][1].any() and not out["in_band"].any()
    # ray 1 (to 2.5): cells 0, 1 free, its piece in cell 2 is 0.125 m up; ray 2 (to 4.5): cells 0 .. 3, not 4
    assert out["counts"][0][0].tolist() == [2, 2, 1, 1, 0, 0, 0, 0]


def test_ramp():
    """A 30 degree ramp (normal[2] = cos 30 >= cos 35) is ground: elevations that rise, a step, no obstacle; a 40
    degree one is not ground, and its hit 0.29 m over the floor behind it is an obstacle."""
    t30 = math.tan(math.radians(30.0))
    hits = [(2.5, 0.5, 0.0037 + 0.5 * t30), (3.5, 0.5, 0.0037 + 1.5 * t30)]
    floor = ray(O, (1.5, 0.5, 0.0037), 1.0)
    out = run([floor] + [ray(O, h, math.cos(math.radians(30.0))) for h in hits], sensor_height=1.0)
    assert out["ground"].all() and not out["counts"][1].any()
    assert out["elev"][0, 1:4].tolist() == [0, 29, 86] and out["step"][0, 1:4].tolist() == [29, 57, 57]
    assert out["stats"] == (3, 57, 0)                  # 0.0037 + (0.2887, 0.8660): 29 and 86 cm
    out = run([floor] + [ray(O, h, math.cos(math.radians(40.0))) for h in hits[:1]], sensor_height=1.0)
    assert out["ground"].tolist() == [True, False] and out["in_band"].tolist() == [False, True]
    assert out["counts"][1][0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0] and out["carried"].tolist() == [False, True]


def test_platform_from_above_and_below():
    """A horizontal panel at 0.5037 m: ground from above (an elevation, no obstacle), an obstacle from below."""
    above = run([ray((0.5, 0.5, 1.5037), (3.5, 0.5, 0.5037), 1.0)], sensor_height=1.0)
    assert above["ground"].all() and above["elev"][0, 3] == 50 and not above["counts"][1].any()
    below = run([ray((0.5, 0.5, 0.2037), (3.5, 0.5, 0.5037), -1.0)], sensor_height=0.2)
    assert not below["ground"].any() and (below["elev"] == tr.NONE).all()
    assert below["in_band"].all() and below["counts"][1][0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert not below["carried"].any()                 # no elevation met: judged against q(o_z - sensor_height)
    assert below["counts"][0][0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0]   # 0.25, 0.35, 0.45 m up; the hit's cell held back


def test_wall_on_a_cell_without_elevation_and_the_pending_mark():
    """The wall's base cell (3) has no elevation: the hit is judged against cell 2's, carried along the ray; with
    sensor_height = 0 the start reference alone (100) would put it out of band. The hit's cell: a free piece and an
    in-band hit give n_occ only; a free piece and a hit above the band give n_free."""
    floor = ray(O, (2.5, 0.5, 0.0037), 1.0)
    wall = ray(O, (3.2, 0.5, 0.5037), 0.0)
    out = run([floor, wall], sensor_height=0.0)
    assert out["elev"][0, 2] == 0 and out["elev"][0, 3] == tr.NONE
    assert out["in_band"].tolist() == [False, True] and out["carried"].tolist() == [False, True]
    assert out["counts"][1][0].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    # the start reference is 100 (cells 0, 1: 90 - 100, 72 - 100: not free); from cell 2 on it is 0
    assert out["counts"][0][0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    high = ray(O, (3.9, 0.5, 1.5237), -1.0)            # 152 over the carried ground: above the band
    out = run([floor, high], sensor_height=1.0)
    assert out["in_band"].tolist() == [False, False] and not out["counts"][1].any()
    assert out["counts"][0][0].tolist() == [2, 2, 1, 1, 0, 0, 0, 0]    # cell 3: the piece 1.46 m up, released
    # flags bit 0 silences the free marks of the rays named, not their hits or the reference they carry
    P = tr.defaults(**GEOM, z_res=0.01, sensor_height=0.0, flags=1)
    rays = [floor, wall]
    o, d, r, nz = (np.array([x[i] for x in rays], dtype=np.float64) for i in range(4))
    out = tr.terrain(o, d, r, nz, P, silent=[False, True])
    assert out["counts"][1][0, 3] == 1 and out["counts"][0].sum() == 0


def test_negative_sum_floor_division():
    """floor(-7 / 2) = -4 (C's division would give -3), through the rays and through cells() alone."""
    o = (0.5, 0.5, 0.975)
    out = run([ray(o, (2.3, 0.5, -0.025), 1.0), ray(o, (2.7, 0.5, -0.035), 1.0)], sensor_height=1.0)
    g_n, g_sum, g_min, g_max = out["planes"]
    assert (g_n[0, 2], g_sum[0, 2], g_min[0, 2], g_max[0, 2]) == (2, -7, -4, -3)
    assert out["elev"][0, 2] == -4 and out["stats"] == (1, 0, 1)
    e, s, st = tr.cells([[2, 1, 3]], [[-7, 5, -9]], [[-4, 5, -3]], [[-3, 5, -3]], min_ground=2)
    assert e.tolist() == [[-4, tr.NONE, -3]] and s.tolist() == [[0, 0, 0]] and st == (2, 0, 1)
    e, s, st = tr.cells([[2, 1, 3]], [[-7, 5, -9]], [[-4, 5, -3]], [[-3, 5, -3]])
    assert e.tolist() == [[-4, 5, -3]] and s.tolist() == [[9, 9, 8]] and st == (3, 9, 1)


def test_quantisation_and_classification():
    """q floors, holds to +-2^30 and sends NaN out of range; the step rule sits on top of vg_occupancy's."""
    assert tr.q([-0.0005, 0.0, 0.0015, 1e300, -1e300, float("nan")], 0.001).tolist() == [-1, 0, 1, 2 ** 30, -2 ** 30,
                                                                                           -2 ** 30]
    counts = np.array([[[3, 0, 0, 2]], [[0, 1, 0, 0]]], dtype=np.int32)
    elev = np.array([[0, 0, tr.NONE, 0]], dtype=np.int32)
    step = np.array([[10, 40, 40, 31]], dtype=np.int32)
    assert tr.classify(counts, elev, step).tolist() == [[0, 100, -1, 0]]
    assert tr.classify(counts, elev, step, flags=2, smax=30).tolist() == [[0, 100, -1, 100]]
    P = tr.defaults(**GEOM, flags=2, step_max=0.3)
    assert (P["clo"], P["chi"], P["smax"], P["z_res"], P["g_lo"], P["g_hi"]) == (
        int(math.floor(0.15 / 0.001)), 1500, int(math.floor(0.3 / 0.001)), 0.001, -3.0, -0.1)


def test_records_and_files(tmp_path):
    """The ctypes mirrors' sizes, terrain_params' fields, and write_terrain / read_terrain."""
    assert ctypes.sizeof(vgpu.TerrainParams) == 224 and ctypes.sizeof(vgpu.TerrainSummary) == 128
    p = vgpu.terrain_params(x0=1.0, y0=2.0, res=0.5, nx=3, ny=4, sensor_height=0.7, step_max=0.2, flags=2, t_max=20.0)
    assert (p.x0, p.y0, p.res, p.nx, p.ny, p.sensor_height, p.step_max, p.flags, p.ray.t_max) == (
        1.0, 2.0, 0.5, 3, 4, 0.7, 0.2, 2, 20.0)
    assert vgpu.TER_NONE == tr.NONE == -2 ** 31
    e = np.array([[1, -2, vgpu.TER_NONE], [70000, 0, -70000]], dtype=np.int32)
    pre = str(tmp_path / "ter")
    vgpu.write_terrain(pre, e, -1.5, 2.25, 0.05, 0.001)
    assert open(pre + ".elev", "rb").read() == e.astype("<i4").tobytes()
    back, x0, y0, res, z_res = vgpu.read_terrain(pre)
    assert np.array_equal(back, e) and back.dtype == np.int32 and (x0, y0, res, z_res) == (-1.5, 2.25, 0.05, 0.001)


def test_struct_layout_matches_header(tmp_path):
    """vg_terrain_params and vg_terrain_summary: the documented sizes, no implicit padding (every field starts
    where the one before it ends) and the ctypes mirrors' offsets, from a C compiler."""
    from test_abi import _c_layout
    for struct, mirror, size in (("vg_terrain_params", vgpu.TerrainParams, 224),
                                 ("vg_terrain_summary", vgpu.TerrainSummary, 128)):
        names = [f for f, _ in mirror._fields_]
        c_size, offs = _c_layout(tmp_path, struct, names)
        assert c_size == ctypes.sizeof(mirror) == size
        assert offs == [getattr(mirror, f).offset for f in names]
        ends = [getattr(mirror, f).offset + getattr(mirror, f).size for f in names]
        assert offs[0] == 0 and offs[1:] == ends[:-1] and ends[-1] == size
