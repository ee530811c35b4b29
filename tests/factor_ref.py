"""50-digit reference (mpmath) of the LM's LiDAR factor, evaluated on the exact
fp64 inputs, and the factor sets tests/test_ba_factor_gpu.py runs on the device.

The reference follows the reference project's text: PointCluster::transform
and cov (types.hpp:144-175), evaluate_only_residual's merge onto the fixed
cluster in frame order (factors.cpp:137-150) and acc_evaluate2 for one factor
(factors.cpp:22-126); the eigen system comes from mpmath.eigsy, ascending.
Nothing here comes from oracle/ or from the device code; tests/test_factor_ref.py
pins this module against the oracle and against central differences of its own
lambda_min.

Layouts. A cluster is 13 doubles [P 9 row-major, v 3, N] (oracle.kat_lidar_factor's),
poses are (W, 12) [R 9, p 3]; to_dev / states give the device's 10-double
cluster [P xx xy xz yy yz zz, v 3, N] and 24-double frame state."""
import math

import mpmath as mp
import numpy as np

import hp_ref

mp.mp.dps = 50
M = hp_ref.M


# ---- the reference ---------------------------------------------------------------------------------------

def _clu(c):
    c = np.asarray(c, dtype=np.float64)
    return M(c[:9].reshape(3, 3)), M(c[9:12]), int(c[12])


def _poses(poses):
    """(W, 12) fp64, or a list of (R, p) mpmath pairs (the finite differences) -> list of (R, p)."""
    if isinstance(poses, list):
        return poses
    poses = np.asarray(poses, dtype=np.float64)
    return [(M(x[:9].reshape(3, 3)), M(x[9:12])) for x in poses]


def transform(c, R, p):
    """PointCluster::transform (types.hpp:168-174) of the cluster (P, v, N)."""
    P, v, N = c
    Rv = R * v
    rp = Rv * p.T
    return R * P * R.T + rp + rp.T + N * p * p.T, Rv + N * p, N


def merge(clus, fix, poses):
    """The fixed cluster plus every populated frame's cluster at its pose, in frame order
    (factors.cpp:138-145) -> (P, v, N)."""
    P, v, N = _clu(fix)
    for c, (R, p) in zip(clus, _poses(poses)):
        c = _clu(c)
        if c[2] != 0:
            t = transform(c, R, p)
            P, v, N = P + t[0], v + t[1], N + t[2]
    return P, v, N


def cov(c):
    P, v, N = c
    ce = v / N
    return P / N - ce * ce.T


def eigen(c):
    """Ascending eigenvalues and the eigenvectors in columns of the merged cluster's covariance."""
    return hp_ref.eig3(cov(c))


def lambda_min(clus, fix, poses):
    return eigen(merge(clus, fix, poses))[0][0]


def evaluate(clus, fix, poses):
    """acc_evaluate2 (factors.cpp:22-126) for one factor with coe = 1, at the eigen system and merged
    cluster of `poses` (what evaluate_only_residual leaves). Returns a dict: lam (lambda_min), J (6W x 1),
    H (6W x 6W, both triangles), w (3 eigenvalues), U (3 x 3), pcr (P, v, N)."""
    ps = _poses(poses)
    W = len(ps)
    add = merge(clus, fix, ps)
    lmbd, U = eigen(add)
    NN = add[2]
    vBar = add[1] / NN
    u = [U[:, k] for k in range(3)]
    uk = u[0]
    ukukT = uk * uk.T
    umumT = mp.zeros(3, 3)
    for i in (1, 2):
        umumT += 2 / (lmbd[0] - lmbd[i]) * u[i] * u[i].T
    I33 = mp.eye(3)
    H, J = mp.zeros(6 * W, 6 * W), mp.zeros(6 * W, 1)
    Auk, viRiTuk, viRiTukukT, n = [None] * W, [None] * W, [None] * W, [0] * W
    for i in range(W):
        Pi, vi, ni = _clu(clus[i])
        n[i] = ni
        if ni == 0:
            continue
        Ri, pi = ps[i]
        vihat = hp_ref.hat(vi)
        RiTuk = Ri.T * uk
        RiTukhat = hp_ref.hat(RiTuk)
        PiRiTuk = Pi * RiTuk
        viRiTuk[i] = vihat * RiTuk
        viRiTukukT[i] = viRiTuk[i] * uk.T
        ti_v = pi - vBar
        ukTti_v = (uk.T * ti_v)[0]
        combo1 = hp_ref.hat(PiRiTuk) + vihat * ukTti_v
        combo2 = Ri * vi + ni * ti_v
        A = mp.zeros(3, 6)
        A[:, 0:3] = (Ri * Pi + ti_v * vi.T) * RiTukhat - Ri * combo1
        A[:, 3:6] = combo2 * uk.T + (combo2.T * uk)[0] * I33
        A = A / NN
        Auk[i] = A
        jjt = A.T * uk
        J[6 * i: 6 * i + 6, 0] = jjt
        HRt = mp.mpf(2) / NN * (1 - mp.mpf(ni) / NN) * viRiTukukT[i]
        Hb = A.T * umumT * A
        Hb[0:3, 0:3] += (mp.mpf(2) / NN * (combo1 - RiTukhat * Pi) * RiTukhat
                         - mp.mpf(2) / NN / NN * viRiTuk[i] * viRiTuk[i].T - hp_ref.hat(jjt[0:3, 0]) / 2)
        Hb[0:3, 3:6] += HRt
        Hb[3:6, 0:3] += HRt.T
        Hb[3:6, 3:6] += mp.mpf(2) / NN * (ni - mp.mpf(ni) * ni / NN) * ukukT
        H[6 * i: 6 * i + 6, 6 * i: 6 * i + 6] = Hb
    for i in range(W - 1):
        if n[i] == 0:
            continue
        AtU = Auk[i].T * umumT
        for j in range(i + 1, W):
            if n[j] == 0:
                continue
            Hb = AtU * Auk[j]
            Hb[0:3, 0:3] += -mp.mpf(2) / NN / NN * viRiTuk[i] * viRiTuk[j].T
            Hb[0:3, 3:6] += -mp.mpf(2) * n[j] / NN / NN * viRiTukukT[i]
            Hb[3:6, 0:3] += -mp.mpf(2) * n[i] / NN / NN * viRiTukukT[j].T
            Hb[3:6, 3:6] += -mp.mpf(2) * n[i] * n[j] / NN / NN * ukukT
            H[6 * i: 6 * i + 6, 6 * j: 6 * j + 6] = Hb
            H[6 * j: 6 * j + 6, 6 * i: 6 * i + 6] = Hb.T
    return {"lam": lmbd[0], "J": J, "H": H, "w": lmbd, "U": U, "pcr": add}


def evaluate_sum(factors, poses):
    """The sum of evaluate over (clus, fix) pairs -> (H, J, lam) and the per-factor results."""
    per = [evaluate(c, f, poses) for c, f in factors]
    W = len(_poses(poses))
    H, J, lam = mp.zeros(6 * W, 6 * W), mp.zeros(6 * W, 1), mp.mpf(0)
    for o in per:
        H, J, lam = H + o["H"], J + o["J"], lam + o["lam"]
    return H, J, lam, per


# ---- layouts ---------------------------------------------------------------------------------------------

def cluster_of(pts):
    """Points (k, 3) -> [P 9, v 3, N], P exactly symmetric (each product summed once)."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    P = np.zeros((3, 3))
    for i in range(3):
        for j in range(i, 3):
            P[i, j] = P[j, i] = math.fsum(pts[:, i] * pts[:, j])
    v = [math.fsum(pts[:, i]) for i in range(3)]
    return np.r_[P.ravel(), v, len(pts)]


def to_dev(c):
    """[P 9, v 3, N] (..., 13) -> the device's [P xx xy xz yy yz zz, v 3, N] (..., 10)."""
    c = np.asarray(c, dtype=np.float64)
    return c[..., [0, 1, 2, 4, 5, 8, 9, 10, 11, 12]]


def states(poses, rng):
    """(W, 12) poses -> (W, 24) frame states; v, bg, ba, g filled with values the passes must ignore."""
    poses = np.asarray(poses, dtype=np.float64)
    xs = rng.standard_normal((poses.shape[0], 24))
    xs[:, :12] = poses
    return xs


def pack(ps):
    return np.array([np.r_[R.ravel(), p] for R, p in ps])


# ---- inputs ----------------------------------------------------------------------------------------------

def expm(w):
    w = np.asarray(w, dtype=np.float64)
    a = float(np.linalg.norm(w))
    if a < 1e-12:
        return np.eye(3)
    k = w / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def window(rng, W, perturb=0.01):
    """W true poses and the window poses the passes run at (the true ones moved by `perturb` rad / m)."""
    true = [(expm(rng.normal(0, 0.3, 3)), rng.normal(0, 1, 3)) for _ in range(W)]
    used = [(R @ expm(rng.normal(0, perturb, 3)), p + rng.normal(0, perturb, 3)) for R, p in true]
    return true, pack(used)


def _split(rng, pts, true, counts, n_fix):
    """Deal the world points to the frames (counts[i] each, 0 = an empty frame) and the fixed cluster;
    frame clusters are taken in the frame's own coordinates R^T (p_w - p)."""
    assert sum(counts) + n_fix == len(pts)
    pts = pts[rng.permutation(len(pts))]
    clus, o = [], 0
    for (R, p), k in zip(true, counts):
        clus.append(cluster_of((pts[o: o + k] - p) @ R) if k else np.zeros(13))
        o += k
    fix = cluster_of(pts[o:]) if n_fix else np.zeros(13)
    return np.array(clus), fix


def plane_factor(rng, true, counts=None, n_fix=20, centre=None):
    """One voxel: a noisy plane patch of random orientation (1 cm noise on a 2 m patch) seen from the
    frames of `true`; counts[i] points in frame i (default 25 + 3 i: every frame's N differs), n_fix in
    the fixed cluster."""
    W = len(true)
    counts = [25 + 3 * i for i in range(W)] if counts is None else list(counts)
    k = sum(counts) + n_fix
    Q = expm(rng.normal(0, 1.0, 3))
    c = rng.normal(0, 3, 3) if centre is None else np.asarray(centre, dtype=np.float64)
    local = np.c_[rng.uniform(-1, 1, (k, 2)), rng.normal(0, 0.01, k)]
    return _split(rng, local @ Q.T + c, true, counts, n_fix)


def gap_factor(rng, true, ratio, counts=None, n_fix=20):
    """One voxel whose point set has the covariance Q diag(l1 / ratio, l1, 4 l1) Q^T, l1 = 0.04, to fp64
    rounding (random points whitened, then shaped): lambda_1 / lambda_0 = ratio at the true poses."""
    W = len(true)
    counts = [25 + 3 * i for i in range(W)] if counts is None else list(counts)
    k = sum(counts) + n_fix
    x = rng.standard_normal((k, 3))
    x -= x.mean(0)
    w, V = np.linalg.eigh(x.T @ x / k)
    white = x @ V @ np.diag(w ** -0.5) @ V.T
    Q = expm(rng.normal(0, 1.0, 3))
    l1 = 0.04
    pts = white @ (Q @ np.diag(np.sqrt([l1 / ratio, l1, 4 * l1])) @ Q.T) + rng.normal(0, 3, 3)
    return _split(rng, pts, true, counts, n_fix)


def sparse_counts(W, frames):
    """Points per frame with only `frames` populated (distinct N)."""
    return [31 + 5 * i if i in frames else 0 for i in range(W)]
