"""The occupancy grid's numpy restatement (tests/occ_ref.py) on a hand-made plane
set with known answers — a 4 m box room (walls x, y = +-2, floor z = -1, ceiling
z = 1) with one interior panel at x = 1, |y| <= 0.75 — and the Python helpers
around vg_occupancy that need no device: the direction fan, the grid's extent,
the map_server writer, the C structs' layout."""
import ctypes

import numpy as np

import occ_ref as oc
import vgpu
from test_abi import _c_layout

O = np.array([0.1, 0.05, 0.0])                                  # the sensor
GEOM = dict(x0=-3.01, y0=-3.01, res=0.25, nx=24, ny=24)          # no wall on a lattice line


def _tile(centres, normal):
    p = np.zeros(len(centres), dtype=vgpu.MARKER_DTYPE)
    p["voxel_center"] = p["center"] = centres
    p["quater_length"], p["normal"] = 0.125, normal                # cubes of edge 0.5, the plane through the centre
    return p


def _room():
    s = np.arange(-2.0, 2.01, 0.5)
    z = np.arange(-1.0, 1.01, 0.5)
    parts = []
    for sign in (-2.0, 2.0):
        parts.append(_tile([(sign, y, h) for y in s for h in z], (1.0, 0.0, 0.0)))
        parts.append(_tile([(x, sign, h) for x in s for h in z], (0.0, 1.0, 0.0)))
    for h in (-1.0, 1.0):
        parts.append(_tile([(x, y, h) for x in s for y in s], (0.0, 0.0, 1.0)))
    parts.append(_tile([(1.0, y, h) for y in (-0.5, 0.0, 0.5) for h in z], (1.0, 0.0, 0.0)))
    return np.concatenate(parts)


def _cell(x, y):
    return int(np.floor((y - GEOM["y0"]) / GEOM["res"])), int(np.floor((x - GEOM["x0"]) / GEOM["res"]))


_cache = {}


def _grids():
    if not _cache:
        dirs = vgpu.occupancy_dirs(n_az=720, elevations_deg=(-40, -10, 0, 10))
        for name, band in (("no_floor", (-0.3, 0.8)), ("floor", (-1.5, 0.8))):
            counts, unc, in_band, r, _, _ = oc.grid_ref(_room(), O[None, :], dirs, z_lo=band[0], z_hi=band[1], **GEOM)
            _cache[name] = (counts, oc.classify(counts), unc, r)
    return _cache


def test_room():
    counts, g, unc, r = _grids()["no_floor"]
    assert np.isfinite(r).all() and unc.mean() < 0.01               # a closed room: every ray hits
    assert g[_cell(O[0], O[1])] == 0 and g[_cell(0.5, 0.0)] == 0      # under the sensor; in front of the panel
    for y in np.arange(-1.9, 1.91, 0.2):
        assert g[_cell(-2.0, y)] == 100, y                            # the wall the panel does not shadow
    for y in (-0.7, 0.0, 0.7):
        assert g[_cell(1.0, y)] == 100
    for p in ((1.4, 0.0), (1.7, 0.3), (1.7, -0.3)):
        assert g[_cell(*p)] == -1 and not counts[:, _cell(*p)[0], _cell(*p)[1]].any()   # behind the panel
    assert g[_cell(2.6, 2.6)] == -1 and g[_cell(-2.6, 0.0)] == -1      # outside the room
    assert (g == 100).sum() + (g == 0).sum() + (g == -1).sum() == g.size
    # a ray marks a cell at most once: no cell holds more free marks than there are rays
    assert counts[0].max() <= r.size


def test_band_keeps_the_floor_out():
    g_no, g_fl = _grids()["no_floor"][1], _grids()["floor"][1]
    ys, xs = np.nonzero(g_no == 100)
    cx, cy = GEOM["x0"] + (xs + 0.5) * GEOM["res"], GEOM["y0"] + (ys + 0.5) * GEOM["res"]
    on_wall = (np.abs(np.abs(cx) - 2.0) < 0.25) | (np.abs(np.abs(cy) - 2.0) < 0.25) | ((np.abs(cx - 1.0) < 0.25) & (np.abs(cy) < 1.0))
    assert on_wall.all()
    # with the floor in the band the -40 degree ring lands 1 / tan(40) = 1.19 m out, in the middle of the room
    assert g_fl[_cell(O[0] - 1.19, O[1])] == 100 and g_no[_cell(O[0] - 1.19, O[1])] == 0
    assert not ((g_no == 100) & (g_fl != 100)).any()


def test_free_on_miss_and_flags():
    dirs = vgpu.occupancy_dirs(n_az=90, elevations_deg=(0,))
    r = np.full(90, np.inf)
    c0, _, _ = oc.marks(O, dirs, r, **GEOM)
    assert not c0.any()
    c1, unc, _ = oc.marks(O, dirs, r, free_on_miss=1.0, **GEOM)
    assert not c1[1].any() and c1[0].any() and oc.classify(c1)[_cell(O[0] + 0.9, O[1])] == 0
    ys, xs = np.nonzero(c1[0])
    far = np.hypot(GEOM["x0"] + (xs + 0.5) * GEOM["res"] - O[0], GEOM["y0"] + (ys + 0.5) * GEOM["res"] - O[1])
    assert far.max() < 1.0 + 0.25 * np.sqrt(0.5) + 1e-9
    # ended rays mark nothing, silent rays only their hit
    r = np.full(90, 1.5)
    ce, _, _ = oc.marks(O, dirs, r, ended=np.ones(90, bool), **GEOM)
    cs, _, _ = oc.marks(O, dirs, r, silent=np.ones(90, bool), **GEOM)
    ca, _, _ = oc.marks(O, dirs, r, **GEOM)
    assert not ce.any() and not cs[0].any() and cs[1].sum() == 90 and np.array_equal(cs[1], ca[1])
    assert not (ca[0].astype(bool) & ca[1].astype(bool) & (ca[0] > 90)).any()


def test_edge_rays():
    # straight down and straight up: only the cell the ray stands in, and only while the band holds some of it
    c, unc, _ = oc.marks(O, [(0.0, 0.0, -1.0), (0.0, 0.0, 1.0)], [np.inf, np.inf], free_on_miss=5.0, **GEOM)
    assert c[0].sum() == 2 and c[0][_cell(O[0], O[1])] == 2 and not unc.any()
    # d_y = 0 from a point exactly on an x-lattice line: ends, and is flagged
    on = np.array([GEOM["x0"] + 8 * GEOM["res"], 0.05, 0.0])
    for dx in (1.0, -1.0):
        c, unc, _ = oc.marks(on, [(dx, 0.0, 0.0)], [np.inf], free_on_miss=0.6, **GEOM)
        assert unc.all() and 2 <= c[0].sum() <= 4
    # a hit out of the band marks no occupied cell, and its own cell is then free like the others
    c, _, ib = oc.marks(O, [(1.0, 0.0, 0.5)], [1.0], z_lo=-0.3, z_hi=0.2, **GEOM)
    assert not ib.any() and not c[1].any() and c[0].sum() >= 1
    # the classification's order and ratio
    cnt = np.array([[[0, 3, 9, 0]], [[2, 1, 1, 0]]], dtype=np.int32)
    assert oc.classify(cnt).tolist() == [[100, 100, 100, -1]]
    assert oc.classify(cnt, occ_ratio=0.25).tolist() == [[100, 100, 0, -1]]
    assert oc.classify(cnt, min_occ=2, min_free=4).tolist() == [[100, -1, 0, -1]]


def test_dirs_and_grid_around():
    d = vgpu.occupancy_dirs()
    assert d.shape == (1080, 3) and np.allclose(np.linalg.norm(d, axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.allclose(d[:360, 2], np.sin(np.deg2rad(-10))) and not d[360:720, 2].any() and d[360, 0] == 1.0
    x0, y0, nx, ny = vgpu.grid_around([(0.3, -1.2, 5.0), (4.1, 2.0, 5.0)], 0.25, 1.0)
    assert (x0, y0) == (-0.75, -2.25) and x0 + nx * 0.25 >= 5.1 and y0 + ny * 0.25 >= 3.0 and (nx, ny) == (24, 21)


def test_pgm_yaml_round_trip(tmp_path):
    g = np.array([[100, 0, -1], [0, 0, 100]], dtype=np.int8)
    pre = str(tmp_path / "map")
    vgpu.write_occupancy(pre, g, -1.5, 2.25, 0.05)
    raw = open(pre + ".pgm", "rb").read()
    assert raw.startswith(b"P5\n3 2\n255\n") and raw[-6:] == bytes([254, 254, 0, 0, 254, 205])   # the largest y first
    y = open(pre + ".yaml").read()
    for line in ("image: map.pgm", "resolution: 0.05", "origin: [-1.5, 2.25, 0]", "negate: 0", "occupied_thresh: 0.65",
                 "free_thresh: 0.196"):
        assert line + "\n" in y, line
    back, x0, y0, res = vgpu.read_occupancy(pre)
    assert np.array_equal(back, g) and (x0, y0, res) == (-1.5, 2.25, 0.05)


def test_struct_layouts_match_the_header(tmp_path):
    for name, st, size in (("vg_occ_params", vgpu.OccParams, 176), ("vg_occ_summary", vgpu.OccSummary, 128)):
        names = [f for f, _ in st._fields_]
        csize, offs = _c_layout(tmp_path, name, names)
        assert ctypes.sizeof(st) == csize == size, name
        assert [getattr(st, f).offset for f in names] == offs, name
    hdr = open(vgpu.HEADER).read()
    assert "#define VG_OCC_UNKNOWN (-1)\n" in hdr and "#define VG_OCC_FREE 0\n" in hdr
    assert "#define VG_OCC_OCCUPIED 100\n" in hdr and "#define VG_OCC_MAX_CELLS (1 << 24)\n" in hdr
    assert bytes(vgpu.occ_params(z_lo=0.0, z_hi=0.0)) == bytes(176)
