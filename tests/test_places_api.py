"""vg_places_dirs, the place index's no-device export: unit vectors at the
documented angles, the counts, and VG_E_ARG at the limits (no GPU)."""
import ctypes
import math

import numpy as np
import pytest

import vgpu


def setup_module(_):
    vgpu.build()


def test_default_table_is_unit_vectors_at_the_documented_angles():
    d = vgpu.places_dirs()
    assert d.shape == (120 * 12, 3)
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() < 4e-16
    w, h, lo = 2 * math.pi / 120, math.radians(60.0) / 12, math.radians(-30.0)
    for e, a in [(0, 0), (0, 119), (5, 37), (11, 60), (11, 119)]:
        v = d[e * 120 + a]
        assert abs(math.atan2(v[1], v[0]) % (2 * math.pi) - (a + 0.5) * w) < 1e-14
        assert abs(math.asin(v[2]) - (lo + (e + 0.5) * h)) < 1e-14


def test_custom_bins_and_span():
    d = vgpu.places_dirs(n_az=7, n_el=3, el_min=-0.2, el_max=0.7)
    assert d.shape == (21, 3)
    el = np.arcsin(d[:, 2]).reshape(3, 7)
    assert np.allclose(el, (-0.2 + (np.arange(3) + 0.5) * 0.3)[:, None], atol=1e-14)
    az = (np.arctan2(d[:, 1], d[:, 0]) % (2 * math.pi)).reshape(3, 7)
    assert np.allclose(az, ((np.arange(7) + 0.5) * 2 * math.pi / 7)[None, :], atol=1e-14)


def test_counts_and_cap():
    L = vgpu.lib()
    p = vgpu.places_params(n_az=256, n_el=16)
    n = ctypes.c_int(0)
    assert L.vg_places_dirs(ctypes.byref(p), None, 0, ctypes.byref(n)) == 0 and n.value == 4096
    out = np.full((5, 3), 7.0)
    assert L.vg_places_dirs(ctypes.byref(p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 4,
                            ctypes.byref(n)) == 0
    assert n.value == 4096 and np.all(out[4] == 7.0) and np.all(np.abs(np.linalg.norm(out[:4], axis=1) - 1) < 4e-16)
    assert L.vg_places_dirs(None, None, 0, ctypes.byref(n)) == 0 and n.value == 1440   # NULL: the defaults


@pytest.mark.parametrize("bad", [dict(n_az=257), dict(n_el=33), dict(n_az=256, n_el=17), dict(el_min=0.5, el_max=0.5),
                                 dict(el_min=0.5, el_max=0.1), dict(el_min=-2.0, el_max=0.1)])
def test_limits_are_arg_errors(bad):
    with pytest.raises(vgpu.VgError) as ei:
        vgpu.places_dirs(**bad)
    assert "(-1)" in str(ei.value)


def test_null_count_and_negative_cap():
    L = vgpu.lib()
    p = vgpu.places_params()
    n = ctypes.c_int(0)
    assert L.vg_places_dirs(ctypes.byref(p), None, 0, None) == -1
    assert L.vg_places_dirs(ctypes.byref(p), None, -1, ctypes.byref(n)) == -1


def test_record_layouts():
    assert ctypes.sizeof(vgpu.PlacesParams) == 144
    assert vgpu.PLACE_CANDIDATE_DTYPE.itemsize == 48
    assert vgpu.place_lattice((-18, -8), (18, 8), 1.0, 1.5).shape == (629, 3)
