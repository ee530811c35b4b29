"""The place index's design, checked on the CPU before any kernel: with place
descriptors built from the scene's true ranges (synth.Scene.cast along
vg_places_dirs' directions) on a 1 m lattice, the numpy restatement
(tests/place_ref.py) of the scan binning and the integer match puts the
lattice node nearest the true position among the 16 best (place, shift)
records, at the true yaw, for a scan near the checkpoint (31) and one further
along (45). The room's box is 180-degree symmetric and only the panels break
the symmetry, which is why the index returns a top-k and not one answer."""
import math

import numpy as np
import pytest

import loc_common as lc
import place_ref as pr
import vgpu

K = 16
YAW = math.radians(137.0)

_cache = {}


def _places():
    if not _cache:
        vgpu.build()
        s = lc.seq()
        p = pr.params()
        D = vgpu.places_dirs()
        pos = pr.lattice((-18.0, -8.0), (18.0, 8.0), 1.0, 1.5)
        r, _ = s.scene.cast(np.repeat(pos, D.shape[0], axis=0), np.tile(D, (pos.shape[0], 1)), max_range=p["t_max"])
        _cache.update(seq=s, prm=p, pos=pos, desc=pr.quantise(r).reshape(pos.shape[0], p["n_el"], p["n_az"]))
    return _cache


@pytest.mark.parametrize("k", [31, 45])
def test_true_place_in_top_k(k):
    c = _places()
    s, p, pos = c["seq"], c["prm"], c["pos"]
    eR, et = lc.ext()
    R, t = s.gt_pose(k)
    R_level = pr.rot_up(YAW) @ R           # the true attitude re-yawed: roll and pitch right, yaw unknown
    sd, _ = pr.scan_descriptor(s.scan(k)[0], R_level, eR, p)
    scores = pr.match_scores(c["desc"], sd, int(round(p["clip"] * pr.Q)))
    valid = pr.hit_bins(c["desc"]) >= p["min_bins"]
    top = pr.top_k(scores, valid, K)
    org = t + R @ et
    near = int(np.argmin(np.linalg.norm(pos[:, :2] - org[:2], axis=1)))
    w = 2.0 * math.pi / p["n_az"]
    true_shift = ((-YAW) % (2.0 * math.pi)) / w   # R = Rz(-YAW) R_level
    hits = [(i, rec) for i, rec in enumerate(top) if rec[1] == near]
    print("scan %d: true node %d, true shift %.2f, its records in the top %d: %s; best %s" %
          (k, near, true_shift, K, hits, top[0]))
    assert hits, (near, top)
    d = min(abs(rec[2] - true_shift) for _, rec in hits)
    assert min(d, p["n_az"] - d) <= 1.0, (true_shift, hits)
