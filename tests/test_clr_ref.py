"""The clearance field's numpy restatement (tests/clr_ref.py) pinned without a
device: against scipy's exact Euclidean distance transform, against its own
definition of `nearest`, on a 1 x 6 strip with hand-computed costs, and the
margin (boundary_free) that lets the GPU tests ask for byte-equal costs; with
them the Python helpers around vg_clearance that need no device."""
import ctypes
import math

import numpy as np
import pytest

import clr_ref as cr
import vgpu
from test_abi import _c_layout

GRIDS = [(61, 47, 7), (33, 64, 8), (5, 3, 9)]       # nx, ny, seed; the first is test_clearance_gpu's


@pytest.mark.parametrize("nx,ny,seed", GRIDS)
@pytest.mark.parametrize("flags", [0, 1])
def test_dist2_is_scipys_edt(nx, ny, seed, flags):
    from scipy import ndimage
    g = cr.random_grid(nx, ny, seed)
    obst = cr.obstacles(g, flags)
    assert obst.any() and not obst.all()
    dist2, _ = cr.transform(g, flags)
    edt = ndimage.distance_transform_edt(~obst)
    assert np.array_equal(dist2, np.rint(edt ** 2).astype(np.int32))
    assert (g == 50).any() and not obst[g == 50].any()              # another byte value is free


@pytest.mark.parametrize("nx,ny,seed", GRIDS)
@pytest.mark.parametrize("flags", [0, 1])
def test_nearest_attains_dist2_and_no_smaller_index_does(nx, ny, seed, flags):
    g = cr.random_grid(nx, ny, seed)
    dist2, nearest = cr.transform(g, flags)
    obst = cr.obstacles(g, flags).ravel()
    iy, ix = np.divmod(np.arange(nx * ny), nx)
    n = nearest.ravel()
    assert obst[n].all()
    assert np.array_equal((ix - n % nx) ** 2 + (iy - n // nx) ** 2, dist2.ravel())
    for i in np.flatnonzero(obst):                                   # no obstacle before `nearest` is as near
        before = n > i
        assert not ((ix[before] - i % nx) ** 2 + (iy[before] - i // nx) ** 2 <= dist2.ravel()[before]).any()


def test_empty_and_full():
    g = np.zeros((4, 6), dtype=np.int8)
    g[1, 2] = cr.UNKNOWN
    r = cr.clearance(g, **cr.PARAMS["nav"])
    assert (r["dist2"] == cr.NONE).all() and (r["nearest"] == -1).all()
    assert r["cost"][1, 2] == 255 and np.count_nonzero(r["cost"]) == 1
    assert cr.summary(g, 0, r["dist2"], r["cost"])["max_dist2"] == 0
    r = cr.clearance(g, flags=1, **cr.PARAMS["nav"])
    assert r["dist2"][1, 2] == 0 and (r["nearest"] == 8).all() and r["cost"][1, 2] == 254
    g[:] = cr.OCCUPIED
    r = cr.clearance(g, **cr.PARAMS["nav"])
    assert not r["dist2"].any() and np.array_equal(r["nearest"].ravel(), np.arange(24)) and (r["cost"] == 254).all()


def test_strip_costs_by_hand():
    """res 0.25, inscribed 0.33, inflation 1.9, scaling 3: d = 0, 0.25, 0.5, 0.75, 1, 1.25 m from the obstacle at
    the left end. 0.25 <= 0.33 is inscribed; then 252 exp(-3 (d - 0.33)) = 151.3, 71.5, 33.8, 15.9. The unknown
    cell at 0.25 m keeps its 253, the one at 0.75 m reads 255."""
    g = np.array([[100, -1, 0, -1, 0, 0]], dtype=np.int8)
    r = cr.clearance(g, **cr.PARAMS["nav"])
    assert r["dist2"].tolist() == [[0, 1, 4, 9, 16, 25]] and not r["nearest"].any()
    assert r["cost"].tolist() == [[254, 253, 151, 255, 33, 15]]
    assert [int(252.0 * math.exp(-3.0 * (d - 0.33))) for d in (0.5, 0.75, 1.0, 1.25)] == [151, 71, 33, 15]
    assert cr.cost_of(np.array([9, 57, 58]), **cr.PARAMS["nav"]).tolist() == [71, 2, 0]   # (1.9 / 0.25)^2 = 57.76; 252 exp(-3 (0.25 sqrt 57 - 0.33)) = 2.4
    assert cr.summary(g, 0, r["dist2"], r["cost"]) == dict(n_obstacles=1, n_unknown=2, cells_lethal=1, cells_inscribed=1,
                                                           cells_inflated=3, cells_free=0, cells_no_info=1, max_dist2=25)
    r1 = cr.clearance(g, flags=1, **cr.PARAMS["nav"])
    assert r1["dist2"].tolist() == [[0, 0, 1, 0, 1, 4]] and r1["nearest"].tolist() == [[0, 1, 1, 3, 3, 3]]
    assert r1["cost"].tolist() == [[254, 254, 253, 254, 253, 151]]


@pytest.mark.parametrize("name", sorted(cr.PARAMS))
def test_boundary_free_for_every_parameter_set(name):
    """Every dist2 the cost table of the set can hold, and two past it: none puts d on a radius or the skirt on an
    integer, so libm and numpy give the same byte."""
    p = cr.PARAMS[name]
    top = int((p["inflation_radius"] / p["res"]) ** 2) + 2
    assert cr.boundary_free(np.arange(0, top + 1), p) == top
    with pytest.raises(AssertionError):
        cr.boundary_free([4], dict(p, inscribed_radius=2 * p["res"], inflation_radius=8 * p["res"]))
    with pytest.raises(AssertionError):
        cr.boundary_free([4], dict(p, inscribed_radius=p["res"], inflation_radius=8 * p["res"], cost_scaling=0.0))


def test_struct_layouts(tmp_path):
    size, off = _c_layout(tmp_path, "vg_clr_params", [f for f, _ in vgpu.ClrParams._fields_])
    assert size == ctypes.sizeof(vgpu.ClrParams) == 80
    assert off == [getattr(vgpu.ClrParams, f).offset for f, _ in vgpu.ClrParams._fields_]
    size, off = _c_layout(tmp_path, "vg_clr_summary", [f for f, _ in vgpu.ClrSummary._fields_])
    assert size == ctypes.sizeof(vgpu.ClrSummary) == 128
    assert off == [getattr(vgpu.ClrSummary, f).offset for f, _ in vgpu.ClrSummary._fields_]
    assert (vgpu.CLR_NONE, vgpu.CLR_MAX_SIDE) == (cr.NONE, cr.MAX_SIDE)
    assert (vgpu.COST_FREE, vgpu.COST_INSCRIBED, vgpu.COST_LETHAL, vgpu.COST_NO_INFO) == (0, 253, 254, 255)


def test_costmap_files(tmp_path):
    c = np.arange(12, dtype=np.uint8).reshape(3, 4) + 250
    vgpu.write_costmap(str(tmp_path / "cm"), c, -1.5, 2.25, 0.05)
    raw = (tmp_path / "cm.pgm").read_bytes()
    assert raw.startswith(b"P5\n4 3\n255\n") and raw[-4:] == c[0].tobytes()      # the first row is written last
    got, x0, y0, res = vgpu.read_costmap(str(tmp_path / "cm"))
    assert np.array_equal(got, c) and (x0, y0, res) == (-1.5, 2.25, 0.05)
    assert "image: cm.pgm" in (tmp_path / "cm.yaml").read_text()
