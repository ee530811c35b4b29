"""Input sets of the device linear-algebra and IEKF-update tests (seeded, so the
CPU self-test of the reference and the GPU tests see the same items)."""
import numpy as np

# mid360.yaml: min_eigen_value, 1 / plane_eigen_value_thre
MIN_EIG, THRE = 0.0025, 0.25
ANGLES = [0.0, 1e-12, 0.9e-9, 1.1e-9, 0.9e-7, 1.1e-7, 1e-4, 0.9e-3, 1.1e-3, 0.5, 3.0, np.pi - 1e-6]


def _rot(rng):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def _spec(rng, w):
    U = _rot(rng)
    A = U @ np.diag(w) @ U.T
    return 0.5 * (A + A.T)


def eig3_cases():
    """class -> (n, 3, 3); the first two classes are the well-conditioned ones
    (the oracle's set, test_oracle_math.py)."""
    rng = np.random.default_rng(11)
    c = {}
    A = rng.normal(size=(120, 3, 3)) * (10.0 ** rng.uniform(-4, 2, 120))[:, None, None]
    c["random"] = 0.5 * (A + A.transpose(0, 2, 1))
    c["plane"] = np.array([_spec(rng, [1e-6, 0.04, 0.2]) for _ in range(60)])
    c["equal_low"] = np.array([_spec(rng, [lam, lam, mu]) for lam, mu in
                               [(0.01, 0.3), (1.0, 2.0), (1e-6, 1.0), (3.0, 1e3)] for _ in range(8)])
    c["equal_high"] = np.array([_spec(rng, [lam, mu, mu]) for lam, mu in
                                [(0.01, 0.3), (1.0, 2.0), (1e-6, 1.0), (3.0, 1e3)] for _ in range(8)])
    c["scaled_identity"] = np.array([s * np.eye(3) for s in (1.0, 0.3, 1e-6, 7e5)])
    c["diagonal_unsorted"] = np.array([np.diag(d) for d in
                                       ([3.0, 1.0, 2.0], [2.0, 3.0, 1.0], [1.0, 3.0, 2.0], [5.0, -1.0, 0.25],
                                        [0.2, 0.04, 1e-6], [1.0, 1.0, 0.5])])
    u = rng.normal(size=(16, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    c["rank1"] = np.array([s * np.outer(a, a) for a, s in zip(u, 10.0 ** rng.uniform(-3, 2, 16))])
    c["zero"] = np.zeros((1, 3, 3))
    t = []
    for p, q in ((0, 1), (0, 2), (1, 2)):  # (a_qq - a_pp) / (2 a_pq) overflows: the isinf(theta) branch
        for sgn in (1.0, -1.0):
            A = np.diag([1.0, 2.0, 3.0])
            A[p, q] = A[q, p] = sgn * 1e-300
            t.append(A)
    c["tiny_offdiag"] = np.array(t)
    A = rng.normal(size=(16, 3, 3)) * 1e8
    c["scale_1e8"] = 0.5 * (A + A.transpose(0, 2, 1))
    for name, g in (("gap_1e-6", 1e-6), ("gap_1e-9", 1e-9), ("gap_1e-12", 1e-12)):
        c[name] = np.array([_spec(rng, [1.0, 1.0 + g, 2.5]) if k % 2 else _spec(rng, [0.3, 2.0, 2.0 * (1 + g)])
                            for k in range(12)])
    return c


WELL_EIG3 = ("random", "plane")
# classes whose eigenvectors are pinned (distinct eigenvalues)
DISTINCT_EIG3 = ("random", "plane", "diagonal_unsorted", "tiny_offdiag", "scale_1e8", "gap_1e-6", "gap_1e-9")


def _cluster(pts):
    P = np.zeros((3, 3))
    v = np.zeros(3)
    for p in pts:  # PointCluster::push
        P += np.outer(p, p)
        v += p
    return np.array([P[0, 0], P[0, 1], P[0, 2], P[1, 1], P[1, 2], P[2, 2], v[0], v[1], v[2], len(pts)])


def cluster_cases():
    """class -> (n, 10) point clusters [P 6, v 3, N]: 20..300 points with 1 cm
    spread on a plane, on a line, and one repeated point, centred 0, 5 and 50 m
    from the origin."""
    rng = np.random.default_rng(12)
    c = {}
    for dist in (0.0, 5.0, 50.0):
        planes, lines, points = [], [], []
        for _ in range(24):
            n = int(rng.integers(20, 301))
            U = _rot(rng)
            d = rng.normal(size=3)
            ctr = dist * d / np.linalg.norm(d)
            q = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.normal(0, 0.01, n)], 1)
            planes.append(_cluster(ctr + q @ U.T))
            q = np.stack([rng.uniform(-0.5, 0.5, n), rng.normal(0, 0.01, n), rng.normal(0, 0.01, n)], 1)
            lines.append(_cluster(ctr + q @ U.T))
        for _ in range(8):
            n = int(rng.integers(20, 301))
            d = rng.normal(size=3)
            # coordinates on a 2^-8 grid: P = N p p^T and v = N p are exact, the covariance is exactly zero
            p = np.round(dist * d / np.linalg.norm(d) * 256) / 256
            points.append(_cluster(np.tile(p, (n, 1))))
        c["plane_%gm" % dist] = np.array(planes)
        c["line_%gm" % dist] = np.array(lines)
        c["point_%gm" % dist] = np.array(points)
    return c


def so3_vectors():
    """(n, 3) rotation vectors: ANGLES on random axes (none within 1 % of a branch threshold)."""
    rng = np.random.default_rng(13)
    out = []
    for a in ANGLES:
        for _ in range(6):
            u = rng.normal(size=3)
            out.append(a * u / np.linalg.norm(u))
    return np.array(out)


def rodrigues(w):
    """fp64 rotation matrix of a rotation vector (test input only: the references take the matrix as given)."""
    a = np.linalg.norm(w)
    if a == 0.0:
        return np.eye(3)
    u = w / a
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def so3_matrices():
    """(n, 3, 3): rotations of ANGLES, and rotations either side of Log's
    tr > 3 - 1e-6 cut-off (angles 0.9e-3 / 1.1e-3: tr = 3 - a^2) and of the
    quaternion branch t > 0 (tr = 1 + 2 cos a: angles 2 pi / 3 -+ 0.02)."""
    rng = np.random.default_rng(14)
    out = [rodrigues(w) for w in so3_vectors()]
    for a in (0.9e-3, 0.99e-3 * 0.99, 1.02e-3, 1.1e-3, 2 * np.pi / 3 - 0.02, 2 * np.pi / 3 + 0.02, 2.5, 3.1):
        for _ in range(6):
            u = rng.normal(size=3)
            out.append(rodrigues(a * u / np.linalg.norm(u)))
    return np.array(out)


BLOCKS = ((0, 3), (3, 6), (6, 9), (9, 15))  # rotation, position, velocity, biases


def block_scaled(rng, n, lo, hi):
    """D A D: A = M M^T / n + I (well conditioned), D constant per state block, log-spaced lo..hi."""
    Mx = rng.normal(size=(n, n))
    A = Mx @ Mx.T / n + np.eye(n)
    d = np.ones(n)
    blocks = [b for b in BLOCKS if b[0] < n]
    sc = 10.0 ** rng.permutation(np.linspace(np.log10(lo), np.log10(hi), len(blocks)))
    for (a, b), s in zip(blocks, sc):
        d[a:min(b, n)] = s
    return (A * d[:, None]) * d[None, :]


def inverse_cases(n):
    rng = np.random.default_rng(15 + n)
    spd = []
    for _ in range(12):
        Mx = rng.normal(size=(n, n))
        spd.append(Mx @ Mx.T + 1e-3 * np.eye(n))
    return {"spd": np.array(spd), "block_scaled": np.array([block_scaled(rng, n, 1e-5, 1e1) for _ in range(12)])}


def qr_cases():
    """class -> list of (A m x 3, b m): the kd-tree LIO's plane fit A n = -1."""
    rng = np.random.default_rng(16)
    c = {"plane": [], "collinear": [], "tie": []}
    for k in range(24):
        m = 5 if k < 12 else int(rng.integers(3, 9))
        U = _rot(rng)
        ctr = rng.uniform(-20, 20, 3)
        q = np.stack([rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m), rng.normal(0, 0.01, m)], 1)
        c["plane"].append((ctr + q @ U.T, -np.ones(m)))
    for k in range(12):  # a line inside a coordinate plane: one column exactly zero, rank 2
        z = k % 3
        a, b = [j for j in range(3) if j != z]
        t = rng.uniform(-1, 1, 5)
        th = rng.uniform(0, np.pi)
        A = np.zeros((5, 3))
        A[:, a] = rng.uniform(-5, 5) + t * np.cos(th)
        A[:, b] = rng.uniform(-5, 5) + t * np.sin(th)
        c["collinear"].append((A, -np.ones(5)))
    for k in range(12):  # two columns of exactly equal norm (entries on a 1/8 grid: the squares sum exactly)
        col = np.round(rng.uniform(-4, 4, 5) * 8) / 8
        A = np.zeros((5, 3))
        A[:, 0] = col
        A[:, 1] = rng.permutation(col) * rng.choice([-1.0, 1.0], 5)
        A[:, 2] = np.round(rng.uniform(-2, 2, 5) * 8) / 8
        if k % 2:
            A = A[:, [2, 0, 1]]
        c["tie"].append((A, -np.ones(5)))
    return c


def transform_cases():
    rng = np.random.default_rng(17)
    clu = cluster_cases()
    out = []
    for name in ("plane_0m", "plane_5m", "line_50m"):
        for c in clu[name][:8]:
            out.append(np.concatenate([c, _rot(rng).reshape(-1), rng.uniform(-30, 30, 3)]))
    return np.array(out)
