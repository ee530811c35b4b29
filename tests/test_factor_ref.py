"""tests/factor_ref.py (the 50-digit LiDAR factor the device's factor passes
are compared with, test_ba_factor_gpu.py) pinned on the CPU: against the
oracle's fp64 restatement on plane voxels at W = 2, 3, 11, its gradient against
central differences of its own lambda_min at 50 digits (the perturbation of
test_oracle_kat.py's _boxplus: R <- R Exp(e), p <- p + e), and the properties
the input generators promise."""
import mpmath as mp
import numpy as np
import pytest

import factor_ref as fr
import hp_ref
from test_oracle_kat import _plane_voxel, _pack


def _np(m):
    return hp_ref.to_np(m)


@pytest.mark.parametrize("W", [2, 3, 11])
def test_reference_matches_oracle(oracle_lib, W):
    rng = np.random.default_rng(40 + W)
    clus, fix, ps = _plane_voxel(rng, W)
    poses = _pack(ps)
    lam, J, H = oracle_lib.kat_lidar_factor(clus, fix, poses)
    eig, pcr = oracle_lib.kat_lidar_eig(clus, fix, poses)
    o = fr.evaluate(clus, fix, poses)
    Hr, Jr = _np(o["H"]), _np(o["J"]).ravel()
    assert np.abs(Hr - Hr.T).max() <= 1e-40 * np.abs(Hr).max()
    assert abs(lam - float(o["lam"])) <= 1e-12 * float(o["w"][2])
    assert np.abs(J - Jr).max() <= 1e-11 * np.abs(Jr).max()
    assert np.abs(H - Hr).max() <= 1e-10 * np.abs(Hr).max()
    assert np.abs(eig[:3] - [float(x) for x in o["w"]]).max() <= 1e-12 * float(o["w"][2])
    U = eig[3:].reshape(3, 3)
    for k in range(3):
        assert abs(abs(float(U[:, k] @ _np(o["U"])[:, k])) - 1.0) < 1e-12
    P, v, N = o["pcr"]
    assert N == pcr[12] == fix[12] + clus[:, 12].sum()
    assert np.abs(pcr[:9] - _np(P).ravel()).max() <= 1e-13 * np.abs(pcr[:9]).max()
    assert np.abs(pcr[9:12] - _np(v).ravel()).max() <= 1e-13 * np.abs(pcr[9:12]).max()


@pytest.mark.parametrize("W", [2, 3])
def test_gradient_is_the_derivative_of_lambda_min(W):
    rng = np.random.default_rng(7 + W)
    true, poses = fr.window(rng, W)
    clus, fix = fr.plane_factor(rng, true)
    J = fr.evaluate(clus, fix, poses)["J"]
    ps = fr._poses(poses)
    h = mp.mpf(10) ** -15
    scale = max(abs(x) for x in J)
    for i in range(W):
        for k in range(6):
            def at(s):
                q = list(ps)
                R, p = q[i]
                e = mp.zeros(3, 1)
                e[k % 3] = s
                if k < 3:  # R Exp(e): Rodrigues on the axis e / |e|
                    K = hp_ref.hat(e / abs(s))
                    q[i] = (R * (mp.eye(3) + mp.sin(abs(s)) * K + (1 - mp.cos(abs(s))) * K * K), p)
                else:
                    q[i] = (R, p + e)
                return fr.lambda_min(clus, fix, q)
            fd = (at(h) - at(-h)) / (2 * h)
            assert abs(fd - J[6 * i + k]) <= mp.mpf(10) ** -25 * scale, (i, k, fd, J[6 * i + k])


def test_hessian_is_the_symmetrised_derivative_of_the_gradient():
    """One column per block kind (a rotation and a translation of frame 0) at W = 2: the central difference
    of J, symmetrised as test_oracle_kat.py does (the -1/2 hat(g) term), against H's column."""
    W = 2
    rng = np.random.default_rng(11)
    true, poses = fr.window(rng, W)
    clus, fix = fr.plane_factor(rng, true)
    o = fr.evaluate(clus, fix, poses)
    ps = fr._poses(poses)
    h = mp.mpf(10) ** -15
    cols = {}
    for c in range(6 * W):
        i, k = divmod(c, 6)

        def at(s):
            q = list(ps)
            R, p = q[i]
            e = mp.zeros(3, 1)
            e[k % 3] = s
            if k < 3:
                K = hp_ref.hat(e / abs(s))
                q[i] = (R * (mp.eye(3) + mp.sin(abs(s)) * K + (1 - mp.cos(abs(s))) * K * K), p)
            else:
                q[i] = (R, p + e)
            return fr.evaluate(clus, fix, q)["J"]
        cols[c] = (at(h) - at(-h)) / (2 * h)
    fd = mp.zeros(6 * W, 6 * W)
    for c in range(6 * W):
        fd[:, c] = cols[c]
    hs = (fd + fd.T) / 2
    scale = max(abs(x) for x in o["H"])
    assert max(abs(x) for x in (hs - o["H"])) <= mp.mpf(10) ** -25 * scale


def test_layouts():
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((9, 3))
    c = fr.cluster_of(pts)
    assert np.array_equal(c[:9].reshape(3, 3), c[:9].reshape(3, 3).T) and c[12] == 9
    assert np.allclose(c[:9].reshape(3, 3), pts.T @ pts) and np.allclose(c[9:12], pts.sum(0))
    d = fr.to_dev(c)
    assert d.tolist() == [c[0], c[1], c[2], c[4], c[5], c[8], c[9], c[10], c[11], 9.0]
    assert np.array_equal(fr.expm([0, 0, 0]), np.eye(3))
    R = fr.expm([0.3, -0.2, 0.5])
    assert np.allclose(R @ R.T, np.eye(3)) and np.isclose(np.linalg.det(R), 1.0)


@pytest.mark.parametrize("W", [2, 5, 11])
def test_generators(W):
    rng = np.random.default_rng(W)
    true, poses = fr.window(rng, W)
    assert poses.shape == (W, 12)
    clus, fix = fr.plane_factor(rng, true)
    assert len(set(clus[:, 12].tolist())) == W and fix[12] == 20  # every frame's N differs
    w = fr.eigen(fr.merge(clus, fix, poses))[0]
    assert 0 < w[0] < w[1] < w[2]
    # sparse frames: only the named frames populated, an empty fixed cluster allowed, merged N > 0
    for frames, n_fix in (((0,), 0), ((W // 2,), 20), ((W - 1,), 0), ((0, W - 1), 0)):
        clus, fix = fr.plane_factor(rng, true, fr.sparse_counts(W, frames), n_fix)
        assert [i for i in range(W) if clus[i, 12] != 0] == sorted(set(frames))
        assert not clus[[i for i in range(W) if i not in frames]].any()
        assert fr.merge(clus, fix, poses)[2] == clus[:, 12].sum() + n_fix > 0
    # centred 500 m out
    clus, fix = fr.plane_factor(rng, true, centre=[300.0, -400.0, 10.0])
    P, v, N = fr.merge(clus, fix, poses)
    assert abs(hp_ref.norm(v / N) - 500) < 5
    # eigenvalue gaps as stated, at the poses the passes run at (perturbed by 1e-6)
    true, poses = fr.window(rng, W, perturb=1e-6)
    for ratio in (1e3, 2.0, 1 + 1e-3):
        clus, fix = fr.gap_factor(rng, true, ratio)
        w = fr.eigen(fr.merge(clus, fix, poses))[0]
        got = float(w[1] / w[0])
        assert abs((got - 1) / (ratio - 1) - 1) < 0.05, (ratio, got)
        assert abs(float(w[2] / w[1]) - 4) < 0.01
