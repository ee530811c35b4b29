"""synth.Scene.cast tests the panels only on the rays whose plane hit is the
nearest so far. The scans every test and the bench run on must not move by a
bit: the ranges and surface ids equal the plain all-rays formulation's, for
one origin (scan) and for per-ray origins (scan_raw)."""
import numpy as np
import pytest

import synth


def _cast_all_rays(scene, o, d, max_range=80.0):
    """The ray caster with every panel test over every ray."""
    n = d.shape[0]
    o2 = np.broadcast_to(o, d.shape)
    best = np.full(n, np.inf)
    sid = np.full(n, -1, dtype=np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        for ax in range(3):
            for k, bound in enumerate((scene.box_lo[ax], scene.box_hi[ax])):
                t = (bound - o2[:, ax]) / d[:, ax]
                ok = (t > 1e-6) & (t < best)
                best = np.where(ok, t, best)
                sid = np.where(ok, 2 * ax + k, sid)
        for j, (c, nrm, a, b, ha, hb) in enumerate(scene.panels):
            den = d @ nrm
            t = ((c[None, :] - o2) @ nrm) / den
            p = o2 + t[:, None] * d
            q = p - c[None, :]
            ok = (t > 1e-6) & (t < best) & (np.abs(q @ a) <= ha) & (np.abs(q @ b) <= hb)
            best = np.where(ok, t, best)
            sid = np.where(ok, 6 + j, sid)
    best[best > max_range] = np.inf
    return best, sid


@pytest.mark.parametrize("lidar,seq_id,k", [("tiny", 1, 0), ("16line", 3, 7), ("64line", 0, 41), ("64line", 5, 300)])
def test_cast_equals_all_rays_formulation(lidar, seq_id, k):
    seq = synth.Sequence(lidar, seq_id, blind=0.5)
    te = seq.t_end(k)
    R, p = seq.traj.rot(te), seq.traj.pos(te)
    dw = seq.dirs @ (R @ seq.ext_R).T
    o = R @ seq.ext_t + p
    r0, s0 = _cast_all_rays(seq.scene, o, dw)
    r1, s1 = seq.scene.cast(o, dw)
    assert np.isfinite(r0).sum() > 0.5 * r0.size and (s0 >= 6).sum() > 0  # walls and panels are hit
    assert np.array_equal(r0.view(np.uint64), r1.view(np.uint64)) and np.array_equal(s0, s1)
    # per-ray origins (the raw sweep)
    on = o[None, :] + 0.01 * np.random.default_rng(k).normal(size=dw.shape)
    r0, s0 = _cast_all_rays(seq.scene, on, dw)
    r1, s1 = seq.scene.cast(on, dw)
    assert np.array_equal(r0.view(np.uint64), r1.view(np.uint64)) and np.array_equal(s0, s1)
