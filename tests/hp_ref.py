"""50-digit references (mpmath) of the small-matrix math and of the IEKF update,
evaluated on the exact fp64 inputs. They follow the reference project's formulas
and branches (math.hpp:12-88 for SO(3), types.hpp:115-175 for the point cluster,
odometry.cpp:192-254 for the update); eigen-decompositions come from
mpmath.eigsy, inverses and least squares from mpmath's LU / QR. Nothing here
comes from oracle/ or from the device code; tests/test_hp_ref.py pins this
module against numpy / scipy and the oracle.

Inputs are numpy fp64 arrays; results are mpmath matrices (or lists of mpf).
`err` gives the largest |device - reference| as a float."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50

# thresholds exactly as the fp64 constants the code compares with
_C1E9, _C1E7, _C1E3 = mp.mpf(1e-9), mp.mpf(1e-7), mp.mpf(0.001)
_CTR = mp.mpf(3.0 - 1e-6)


def M(a):
    """numpy fp64 array -> mpmath matrix (exact); an mpmath matrix passes through."""
    if isinstance(a, mp.matrix):
        return a
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in a])


def to_np(m):
    return np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])


def err(dev, ref):
    """max |dev - ref| (dev: numpy fp64, ref: mpmath matrix of the same shape, or flattened)."""
    d = np.asarray(dev, dtype=np.float64)
    r = [ref[i, j] for i in range(ref.rows) for j in range(ref.cols)]
    d = d.reshape(-1)
    assert d.size == len(r), (d.size, len(r))
    return float(max(abs(mp.mpf(float(x)) - y) for x, y in zip(d, r)))


def maxabs(ref):
    return float(max(abs(ref[i, j]) for i in range(ref.rows) for j in range(ref.cols)))


def hat(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def norm(v):
    return mp.sqrt(sum(x * x for x in v))


def eig3(A):
    """Ascending eigenvalues (list) and eigenvectors in columns (matrix) of the
    symmetric part of A (numpy fp64, or an mpmath matrix)."""
    A = A if isinstance(A, mp.matrix) else M(A)
    A = (A + A.T) / 2
    E, Q = mp.eigsy(A)
    order = sorted(range(3), key=lambda i: E[i])
    w = [E[i] for i in order]
    V = mp.matrix(3, 3)
    for j, i in enumerate(order):
        for k in range(3):
            V[k, j] = Q[k, i]
    return w, V


def Exp(v):
    v = M(v)
    n = norm(v)
    if n >= _C1E9:
        K = hat(v / n)
        return mp.eye(3) + mp.sin(n) * K + (1 - mp.cos(n)) * K * K
    return mp.eye(3)


def Exp_dt(w, dt):
    w = M(w)
    n = norm(w)
    if n > _C1E7:
        K = hat(w / n)
        a = n * (dt if isinstance(dt, mp.mpf) else mp.mpf(float(dt)))
        return mp.eye(3) + mp.sin(a) * K + (1 - mp.cos(a)) * K * K
    return mp.eye(3)


def _Log(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    theta = mp.mpf(0) if tr > _CTR else mp.acos((tr - 1) / 2)
    K = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return K / 2 if abs(theta) < _C1E3 else K * (theta / mp.sin(theta) / 2)


def Log(R):
    """The reference project's Log evaluated exactly (not the true matrix logarithm)."""
    return _Log(M(R))


def jr(v):
    v = M(v)
    a = norm(v)
    if a < _C1E9:
        return mp.eye(3)
    u = v / a
    ra = mp.sin(a) / a
    return ra * mp.eye(3) + (1 - ra) * u * u.T - (1 - mp.cos(a)) / a * hat(u)


def angle_axis(m):
    """Eigen::AngleAxisd(Matrix3d): through the quaternion (Eigen's branches)."""
    m = M(m)
    q = [mp.mpf(0)] * 4
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = mp.sqrt(t + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = mp.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    n = mp.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2)
    if n != 0:
        ang = 2 * mp.atan2(n, abs(q[3]))
        if q[3] < 0:
            n = -n
        return ang, mp.matrix([q[0] / n, q[1] / n, q[2] / n])
    return mp.mpf(0), mp.matrix([1, 0, 0])


def jr_inv(R):
    ang, ax = angle_axis(R)
    if ang < _C1E9:
        return mp.eye(3)
    ctt = ang / 2 / mp.tan(ang / 2)
    return ctt * mp.eye(3) + (1 - ctt) * ax * ax.T + ang / 2 * hat(ax)


def inverse(A):
    return mp.inverse(M(A))


def lstsq(A, b):
    """Least-squares solution of A x = b (m x 3), zero on columns of A that are
    exactly zero (the rank cut of a column-pivoted QR in exact arithmetic)."""
    A = np.asarray(A, dtype=np.float64)
    keep = [j for j in range(A.shape[1]) if np.any(A[:, j] != 0.0)]
    x = mp.matrix(A.shape[1], 1)
    if keep:
        y, _ = mp.qr_solve(M(A[:, keep]), M(b))
        for k, j in enumerate(keep):
            x[j] = y[k]
    return x


def _clu(c):
    """[P xx xy xz yy yz zz, v 3, N] -> P (3 x 3), v, N."""
    c = [mp.mpf(float(x)) for x in np.asarray(c, dtype=np.float64)]
    P = mp.matrix([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    return P, mp.matrix(c[6:9]), int(c[9])


def clu_cov(c):
    P, v, N = _clu(c)
    ce = v / N
    return P / N - ce * ce.T


def clu_transform(c, R, t):
    """-> [P 6, v 3, N] as a 10 x 1 matrix."""
    P, v, N = _clu(c)
    R, t = M(R), M(t)
    Rv = R * v
    rp = Rv * t.T
    P2 = R * P * R.T + rp + rp.T + N * t * t.T
    v2 = Rv + N * t
    return mp.matrix([P2[0, 0], P2[0, 1], P2[0, 2], P2[1, 1], P2[1, 2], P2[2, 2], v2[0], v2[1], v2[2], N])


def plane_decisions(ev, min_eig, thre):
    """The comparisons of the recut (ev0 < min_eigen_value, ev0 / ev2 < thre,
    ev0 / ev1 > 0.12) on exact eigenvalues, and the smallest relative distance
    of a compared value from its threshold. A 0 / 0 compares false, as a NaN does."""
    cm, ct, cc = mp.mpf(float(min_eig)), mp.mpf(float(thre)), mp.mpf(0.12)
    dec, margin = [], mp.inf
    for val, thr, gt in ((ev[0], cm, False), (None if ev[2] == 0 else ev[0] / ev[2], ct, False),
                         (None if ev[1] == 0 else ev[0] / ev[1], cc, True)):
        if val is None:
            dec.append(False)
            continue
        dec.append(bool(val > thr) if gt else bool(val < thr))
        margin = min(margin, abs(val - thr) / thr)
    return dec, float(margin)


_K6 = {}


def iekf_update(sums, x_curr, x_prop, it, rematch, max_iter=4):
    """odometry.cpp:192-227 on the sums of one iteration (HTH upper 21, HTz 6,
    ...) and the 250-double states. Returns dict: R, p, v, bg, ba (after
    x_curr += solution), sol (15), G6 (15 x 6), cov (after the update when the
    IEKF stops, else unchanged), rematch, done."""
    s = np.asarray(sums, dtype=np.float64)
    xc, xp = np.asarray(x_curr, dtype=np.float64), np.asarray(x_prop, dtype=np.float64)
    HTH = mp.matrix(6, 6)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            HTH[i, j] = HTH[j, i] = mp.mpf(float(s[k]))
            k += 1
    HTz = M(s[21:27])
    cov = M(xc[25:250].reshape(15, 15))
    H15 = mp.matrix(15, 15)
    H15[0:6, 0:6] = HTH
    key = (s[:21].tobytes(), xc[25:250].tobytes())  # (the gain does not depend on it / rematch / x_prop)
    if key not in _K6:
        _K6[key] = mp.inverse(H15 + mp.inverse(cov))[0:15, 0:6]
    K6 = _K6[key]
    G6 = K6 * HTH
    Rc, Rp = M(xc[1:10].reshape(3, 3)), M(xp[1:10].reshape(3, 3))
    vec = mp.matrix(15, 1)
    lg = _Log(Rc.T * Rp)
    for i in range(3):
        vec[i] = lg[i]
    for i in range(12):
        vec[3 + i] = mp.mpf(float(xp[10 + i])) - mp.mpf(float(xc[10 + i]))
    sol = K6 * HTz + vec - G6 * vec[0:6, 0]
    n3 = norm(sol[0:3, 0])
    if n3 >= _C1E9:
        Kh = hat(sol[0:3, 0] / n3)
        E = mp.eye(3) + mp.sin(n3) * Kh + (1 - mp.cos(n3)) * Kh * Kh
    else:
        E = mp.eye(3)
    out = {"R": Rc * E, "sol": sol, "G6": G6}
    for name, o in (("p", 0), ("v", 3), ("bg", 6), ("ba", 9)):
        out[name] = mp.matrix([mp.mpf(float(xc[10 + o + i])) + sol[3 + o + i] for i in range(3)])
    conv = (n3 * mp.mpf(57.3) < mp.mpf(0.01)) and (norm(sol[3:6, 0]) * 100 < mp.mpf(0.015))
    out["conv_margin"] = float(min(abs(n3 * mp.mpf(57.3) / mp.mpf(0.01) - 1),
                                   abs(norm(sol[3:6, 0]) * 100 / mp.mpf(0.015) - 1)))
    if conv or (rematch == 0 and it == max_iter - 2):
        rematch += 1
    done = rematch >= 2 or it == max_iter - 1
    if done:
        G = mp.matrix(15, 15)
        G[0:15, 0:6] = G6
        cov = (mp.eye(15) - G) * cov
    out["cov"], out["rematch"], out["done"] = cov, rematch, int(done)
    return out
