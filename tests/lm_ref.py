"""Reference of one LM step between the Hessian pass and the residual pass,
and of the LM bookkeeping, written from the reference project's
LI_BA_Optimizer (optimizers.cpp:171-245 divide_thread / hess_plus, 430-517
damping_iter) and Eigen's LDLT (Cholesky/LDLT.h: the pivot of step k is the
first largest |diagonal| among positions k.., transposed with position k; the
solve divides by D where |D| > DBL_MIN and puts 0 elsewhere). Plain numpy and
mpmath; nothing here comes from oracle/ or from the device code.
tests/test_lm_ref.py pins `solve` against the oracle's ldlt_solve and
`assemble` against a brute-force accumulation.

Layouts (the device's, csrc/ba_factor.hip, ba_solve.hip): hl = the 6W x 6W LiDAR Hessian as packed
lower rows, then the 6W gradient, then the residual; imuout = (W-1) x 931, per
IMU factor the 30 x 30 J^T C J (row-major), the 30 gradient entries, r^T C r;
a frame's state = R 9 (row-major), p, v, bg, ba, g; a bias record = bg 3, ba 3,
then their backups.

solve: mpmath LU at 50 digits up to MP_MAX unknowns, numpy's LU with two
rounds of iterative refinement (residual in np.longdouble) above. Timed on the
development CPU: mpmath 15 unknowns 0.02 s, 30 unknowns 0.07 s, 60 unknowns
0.5 s, 135 unknowns 5.6 s (150: cubic in the size, above that); numpy with
refinement under 0.01 s at every size, and equal to mpmath's fp64 result on
those systems. So W = 2 and 3 (15, 30 unknowns) take mpmath, W = 10 and 11
(135, 150 unknowns) numpy."""
import mpmath as mp
import numpy as np

import hp_ref

mp.mp.dps = 50
DIM = 15
MP_MAX = 60


def lo(i, j):
    """Index of entry (i, j) in packed lower rows."""
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


def pack_lower(H):
    n = H.shape[0]
    return np.array([H[i, j] for i in range(n) for j in range(i + 1)], dtype=np.float64)


def unpack_lower(p, n):
    H = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            H[i, j] = H[j, i] = p[lo(i, j)]
    return H


def assemble(hl, imuout, W, imu_coef):
    """divide_thread (optimizers.cpp:186-245): Hess / JacT / residual from the
    IMU factors in ascending order, times imu_coef (the residual times
    imu_coef * 0.5), then hess_plus adds the LiDAR 6 x 6 blocks and gradient.
    Returns H (15W x 15W; the lower triangle is authoritative — Eigen's LDLT
    reads nothing else — and is mirrored), J, res1."""
    hl = np.asarray(hl, dtype=np.float64)
    imu = np.asarray(imuout, dtype=np.float64).reshape(W - 1, 931)
    n, L = DIM * W, 6 * W
    H, J, res = np.zeros((n, n)), np.zeros(n), 0.0
    for i in range(W - 1):
        H[DIM * i: DIM * i + 2 * DIM, DIM * i: DIM * i + 2 * DIM] += imu[i, :900].reshape(30, 30)
        J[DIM * i: DIM * i + 2 * DIM] += imu[i, 900:930]
        res += imu[i, 930]
    H *= imu_coef
    J *= imu_coef
    res *= imu_coef * 0.5
    nl = L * (L + 1) // 2
    hs = unpack_lower(hl[:nl], L)
    for i in range(W):
        J[DIM * i: DIM * i + 6] += hl[nl + 6 * i: nl + 6 * i + 6]
        for j in range(W):
            H[DIM * i: DIM * i + 6, DIM * j: DIM * j + 6] += hs[6 * i: 6 * i + 6, 6 * j: 6 * j + 6]
    res += hl[nl + L]
    H = np.tril(H) + np.tril(H, -1).T
    return H, J, float(res)


def gauge_damp(H, J, u):
    """optimizers.cpp:460-466: the gauge frame's unit rows and columns and zero
    gradient, D = the gauged diagonal, A = Hess + u D (each diagonal entry
    D + u * D in fp64, two roundings). Returns A, the gauged J, D."""
    A = np.array(H, dtype=np.float64)
    Jg = np.array(J, dtype=np.float64)
    A[:DIM, :] = 0.0
    A[:, :DIM] = 0.0
    A[np.arange(DIM), np.arange(DIM)] = 1.0
    Jg[:DIM] = 0.0
    D = A.diagonal().copy()
    A[np.diag_indices_from(A)] = D + u * D
    return A, Jg, D


def pivot_order(D, u, structural, W=None):
    """The order in which the unknowns of frames 1..W-1 are eliminated.
    structural: v / bg / ba of frames 1..W-1 in frame order, then their poses.
    Else Eigen's: at step k the first largest |D + u D| among positions k..n-1
    is taken and transposed with position k (all 15W unknowns take part, the
    gauge frame's 1 + u too); the gauge frame's unknowns are then left out."""
    D = np.asarray(D, dtype=np.float64)
    n = D.size
    if structural:
        W = n // DIM
        return ([DIM * j + v for j in range(1, W) for v in range(6, DIM)] +
                [DIM * j + v for j in range(1, W) for v in range(6)])
    key = np.abs(D + u * D)
    perm = list(range(n))
    for k in range(n):
        p = k
        for i in range(k + 1, n):
            if key[perm[i]] > key[perm[p]]:
                p = i
        perm[k], perm[p] = perm[p], perm[k]
    return [e for e in perm if e >= DIM]


def solve(A, b):
    """x with A x = b for symmetric A (lower triangle read). An unknown whose
    row, column and diagonal are exactly zero is decoupled with a zero pivot:
    Eigen's LDLT solve gives it 0 (D^+), and the rest solve the reduced system.
    mpmath at 50 digits up to MP_MAX unknowns, refined numpy LU above (module
    docstring). Returns fp64."""
    A = np.asarray(A, dtype=np.float64)
    A = np.tril(A) + np.tril(A, -1).T
    b = np.asarray(b, dtype=np.float64)
    keep = [i for i in range(A.shape[0]) if np.any(A[i] != 0.0)]
    x = np.zeros(A.shape[0])
    As, bs = A[np.ix_(keep, keep)], b[keep]
    if len(keep) <= MP_MAX:
        xs = mp.lu_solve(hp_ref.M(As), hp_ref.M(bs))
        x[keep] = [float(v) for v in xs]
        return x
    xs = np.linalg.solve(As, bs)
    Al, bl = As.astype(np.longdouble), bs.astype(np.longdouble)
    for _ in range(2):
        r = bl - Al @ xs.astype(np.longdouble)
        xs = xs + np.linalg.solve(As, r.astype(np.float64))
    x[keep] = xs
    return x


def step(hl, imuout, W, imu_coef, u):
    """dx of one LM step from the raw inputs (assemble, gauge_damp, solve)."""
    H, J, _ = assemble(hl, imuout, W, imu_coef)
    A, Jg, D = gauge_damp(H, J, u)
    return solve(A, -Jg), D, Jg


def trial(xs, bias, dx):
    """optimizers.cpp:468-478 at a given dx: per frame R Exp(dx_R) at 50 digits
    (a list of mpmath matrices), the other states (W x 24 fp64, the rotation
    entries left 0): p, v, bg, ba each one fp64 addition, g copied; and the
    bias records (update_state, imu_preintegration.cpp:239-246): backup <- the
    old values, current <- old + dx."""
    xs = np.asarray(xs, dtype=np.float64).reshape(-1, 24)
    dx = np.asarray(dx, dtype=np.float64)
    W = xs.shape[0]
    Rs, rest = [], np.zeros((W, 24))
    for j in range(W):
        d = dx[DIM * j: DIM * j + DIM]
        Rs.append(hp_ref.M(xs[j, :9].reshape(3, 3)) * hp_ref.Exp(d[:3]))
        rest[j, 9:21] = xs[j, 9:21] + d[3:15]
        rest[j, 21:24] = xs[j, 21:24]
    b = np.array(bias, dtype=np.float64).reshape(W - 1, 12)
    for j in range(W - 1):
        b[j, 6:12] = b[j, 0:6]
        b[j, 0:6] = b[j, 0:6] + dx[DIM * j + 9: DIM * j + 15]
    return Rs, rest, b


def q1(dx, u, D, J):
    """0.5 dx . (u D dx - J) (optimizers.cpp:480) at 50 digits on the fp64
    inputs, and the sum of the moduli of its 2 x 15W products
    0.5 dx_r u D_r dx_r and 0.5 dx_r J_r (the scale of a rounding bound)."""
    f = [mp.mpf(float(v)) for v in dx]
    um = mp.mpf(float(u))
    s, a = mp.mpf(0), mp.mpf(0)
    for r in range(len(f)):
        t1, t2 = f[r] * um * mp.mpf(float(D[r])) * f[r] / 2, f[r] * mp.mpf(float(J[r])) / 2
        s += t1 - t2
        a += abs(t1) + abs(t2)
    return s, a


STATE_KEYS = ("u", "v", "res1", "res2", "q1", "calc_hess", "done", "iters", "nhess", "fin", "skip")


def control(state, r1_terms, r2_terms, imu_coef):
    """optimizers.cpp:483-515 in fp64 on the LM state (a dict over STATE_KEYS):
    residual2 = the IMU residuals r1_terms summed in order, times
    imu_coef * 0.5 (only_residual, 350-376), plus the LiDAR partials r2_terms;
    accept or reject with the updates of u and v (the cube correctly rounded);
    `done` is the loop's break, `iters` / `nhess` count the passes through the
    loop and through divide_thread, `fin` says the loop has ended (break, or 10
    iterations) unless the run is skipped. Returns (state, accept): accept 1 /
    0, or -1 with the state unchanged when the loop had ended already."""
    s = dict(state)
    if s["done"]:
        s["fin"] = 0 if s["skip"] else 1
        return s, -1
    if s["calc_hess"]:
        s["nhess"] += 1
    r1 = 0.0
    for t in r1_terms:
        r1 += float(t)
    r1 *= imu_coef * 0.5
    r2 = 0.0
    for t in r2_terms:
        r2 += float(t)
    residual1, residual2 = s["res1"], r1 + r2
    s["res2"] = residual2
    q = residual1 - residual2
    if q > 0:
        accept = 1
        one_three = 1.0 / 3
        q = q / s["q1"]
        s["v"] = 2.0
        q = 1 - float(mp.mpf(2 * q - 1) ** 3)
        s["u"] = s["u"] * (one_three if q < one_three else q)
        s["calc_hess"] = 1
    else:
        accept = 0
        s["u"] = s["u"] * s["v"]
        s["v"] = 2 * s["v"]
        s["calc_hess"] = 0
    s["iters"] += 1
    if abs((residual1 - residual2) / residual1) < 1e-6:
        s["done"] = 1
    s["fin"] = 1 if (s["done"] or s["iters"] >= 10) and not s["skip"] else 0
    return s, accept


def control_states(accept, xs, xt, bias):
    """x_stats = x_stats_temp on an accepted step (492); the IMU factors' bias
    increments go back to their backups on a rejected one (507-511)."""
    xs, bias = np.array(xs, dtype=np.float64), np.array(bias, dtype=np.float64)
    if accept == 1:
        xs = np.array(xt, dtype=np.float64).reshape(xs.shape)
    elif accept == 0:
        bias[:, 0:6] = bias[:, 6:12]
    return xs, bias
