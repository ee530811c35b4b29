"""The reference project's own routes in plain fp64 numpy (libm / LAPACK): the
yardstick e_f64 of the device tests' edge classes. Same formulas and branches as
hp_ref.py."""
import numpy as np


def hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def Exp(v):
    n = np.linalg.norm(v)
    if n >= 1e-9:
        K = hat(v / n)
        return np.eye(3) + np.sin(n) * K + (1.0 - np.cos(n)) * K @ K
    return np.eye(3)


def Exp_dt(w, dt):
    n = np.linalg.norm(w)
    if n > 1e-7:
        K = hat(w / n)
        a = n * dt
        return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * K @ K
    return np.eye(3)


def Log(R):
    tr = np.trace(R)
    theta = 0.0 if tr > 3.0 - 1e-6 else np.arccos(0.5 * (tr - 1))
    K = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return 0.5 * K if abs(theta) < 0.001 else 0.5 * theta / np.sin(theta) * K


def jr(v):
    a = np.linalg.norm(v)
    if a < 1e-9:
        return np.eye(3)
    u = v / a
    ra = np.sin(a) / a
    return ra * np.eye(3) + (1 - ra) * np.outer(u, u) - (1 - np.cos(a)) / a * hat(u)


def jr_inv(R):
    q = np.zeros(4)  # Eigen::AngleAxisd(Matrix3d), through the quaternion
    t = np.trace(R)
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[:3] = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    n = np.linalg.norm(q[:3])
    if n == 0.0:
        return np.eye(3)
    ang = 2.0 * np.arctan2(n, abs(q[3]))
    ax = q[:3] / (-n if q[3] < 0 else n)
    if ang < 1e-9:
        return np.eye(3)
    ctt = ang / 2 / np.tan(ang / 2)
    return ctt * np.eye(3) + (1 - ctt) * np.outer(ax, ax) + ang / 2 * hat(ax)


def clu_cov(c):
    P = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    ce = c[6:9] / c[9]
    return P / c[9] - np.outer(ce, ce)


def clu_transform(c, R, t):
    P = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
    N = c[9]
    Rv = R @ c[6:9]
    rp = np.outer(Rv, t)
    P2 = R @ P @ R.T + rp + rp.T + N * np.outer(t, t)
    v2 = Rv + N * t
    return np.array([P2[0, 0], P2[0, 1], P2[0, 2], P2[1, 1], P2[1, 2], P2[2, 2], v2[0], v2[1], v2[2], N])


def iekf_update(sums, x_curr, x_prop, it, rematch, max_iter=4):
    """odometry.cpp:192-227 with two numpy.linalg.inv of 15 x 15."""
    s, xc, xp = np.asarray(sums), np.asarray(x_curr), np.asarray(x_prop)
    HTH = np.zeros((6, 6))
    HTH[np.triu_indices(6)] = s[:21]
    HTH = HTH + HTH.T - np.diag(np.diag(HTH))
    cov = xc[25:250].reshape(15, 15)
    H15 = np.zeros((15, 15))
    H15[:6, :6] = HTH
    K6 = np.linalg.inv(H15 + np.linalg.inv(cov))[:, :6]
    G6 = K6 @ HTH
    Rc, Rp = xc[1:10].reshape(3, 3), xp[1:10].reshape(3, 3)
    vec = np.concatenate([Log(Rc.T @ Rp), xp[10:22] - xc[10:22]])
    sol = K6 @ s[21:27] + vec - G6 @ vec[:6]
    out = {"R": Rc @ Exp(sol[:3]), "sol": sol, "G6": G6, "p": xc[10:13] + sol[3:6], "v": xc[13:16] + sol[6:9],
           "bg": xc[16:19] + sol[9:12], "ba": xc[19:22] + sol[12:15]}
    conv = (np.linalg.norm(sol[:3]) * 57.3 < 0.01) and (np.linalg.norm(sol[3:6]) * 100 < 0.015)
    if conv or (rematch == 0 and it == max_iter - 2):
        rematch += 1
    done = rematch >= 2 or it == max_iter - 1
    if done:
        G = np.zeros((15, 15))
        G[:, :6] = G6
        cov = (np.eye(15) - G) @ cov
    out["cov"], out["rematch"], out["done"] = cov, rematch, int(done)
    return out
