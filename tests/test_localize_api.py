"""The localisation calls' host side, no device: struct layouts against the
header, the hypothesis grid's count and order (vg_reloc_grid), and NodeCore's
parameter defaults."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import vgpu
from test_abi import _c_layout


@pytest.fixture(scope="module", autouse=True)
def _built():
    vgpu.build()


def test_pose_score_layout(tmp_path):
    names = [f for f, _ in vgpu.PoseScore._fields_]
    size, offs = _c_layout(tmp_path, "vg_pose_score", names)
    assert size == 80 == ctypes.sizeof(vgpu.PoseScore) == vgpu.POSE_SCORE_DTYPE.itemsize
    assert [getattr(vgpu.PoseScore, f).offset for f in names] == offs
    assert [vgpu.POSE_SCORE_DTYPE.fields[f][1] for f in names] == offs
    names = [f for f, _ in vgpu.PointMatch._fields_]
    size, offs = _c_layout(tmp_path, "vg_point_match", names)
    assert size == 24 == ctypes.sizeof(vgpu.PointMatch) == vgpu.POINT_MATCH_DTYPE.itemsize
    assert [getattr(vgpu.PointMatch, f).offset for f in names] == offs


def test_reloc_params_layout(tmp_path):
    names = [f for f, _ in vgpu.RelocParams._fields_]
    size, offs = _c_layout(tmp_path, "vg_reloc_params", names)
    assert size == ctypes.sizeof(vgpu.RelocParams) == 96
    assert [getattr(vgpu.RelocParams, f).offset for f in names] == offs


def test_grid_count_and_order():
    g = vgpu.reloc_grid(half_xy=2.0, step_xy=0.25, half_yaw=math.radians(30), step_yaw=math.radians(2.5))
    assert g.shape == (17 * 17 * 25, 4)
    # every cell exactly once
    cells = {(round(x / 0.25), round(y / 0.25), round(w / math.radians(2.5))) for x, y, _, w in g}
    assert len(cells) == g.shape[0] and np.all(g[:, 2] == 0)
    assert np.abs(g[:, :2]).max() == 2.0 and abs(np.abs(g[:, 3]).max() - math.radians(30)) < 1e-12
    # yaw outside the plane: the first 289 share the lowest yaw; inside it 4 x 4 patches, x fastest
    assert np.all(g[:289, 3] == g[0, 3]) and g[289, 3] > g[0, 3]
    first = g[:16, :2] / 0.25 + 8
    assert [tuple(v) for v in first] == [(i, j) for j in range(4) for i in range(4)]
    # the first four pose tiles of 16 are whole 4 x 4 patches (the 17th column's and row's patches are
    # narrower, so later tiles straddle consecutive patches)
    plane = g[:289, :2] / 0.25
    for t in range(0, 64, 16):
        tile = plane[t:t + 16]
        assert np.ptp(tile[:, 0]) <= 3 and np.ptp(tile[:, 1]) <= 3
    # z and the degenerate axes
    g = vgpu.reloc_grid(half_xy=0.5, step_xy=0.25, half_z=0.2, step_z=0.1)
    assert g.shape == (25 * 5, 4) and np.all(g[:25, 2] == g[0, 2]) and g[0, 2] == -0.2 and np.all(g[:, 3] == 0)
    assert vgpu.reloc_grid().tolist() == [[0, 0, 0, 0]]
    assert vgpu.reloc_grid(half_xy=1.0, step_xy=0.0).shape == (1, 4)
    assert vgpu.reloc_grid(half_xy=0.3, step_xy=0.25).shape == (9, 4)  # floor(half / step)
    # the limit: 65,536 hypotheses
    assert vgpu.reloc_grid(half_xy=127.5, step_xy=1.0).shape[0] == 65536 - 511  # 255 x 255
    for bad in (dict(half_xy=128.0, step_xy=1.0), dict(half_xy=-1.0, step_xy=0.25),
                dict(half_xy=2.0, step_xy=0.25, half_yaw=math.pi, step_yaw=math.radians(1))):
        with pytest.raises(vgpu.VgError):
            vgpu.reloc_grid(**bad)


def test_node_core_defaults(tmp_path):
    """General.localization_mode defaults to 0 and General.map_path to empty:
    behaviour with the defaults is unchanged."""
    inc = os.path.join(vgpu.REPO, "include")
    src = tmp_path / "nc.cpp"
    src.write_text('#include <cstdio>\n#include "vina_node_core.hpp"\n'
                   'int main(){ vina_gpu::NodeParams p; std::printf("%d|%s|\\n", p.localization_mode, p.map_path.c_str());'
                   ' return 0; }\n')
    exe = tmp_path / "nc"
    subprocess.check_call(["g++", "-std=c++17", "-I", inc, "-o", str(exe), str(src), "-L",
                           os.path.dirname(vgpu.LIB), "-lvina_gpu", "-Wl,-rpath," + os.path.dirname(vgpu.LIB)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "0||"
