"""numpy restatement of the localisability sums (vina_gpu.h "Localisability") on
top of vg_raycast's records: per ray J = [n ; (r d) x n], s2 = c^2 (var +
dept_err^2 + (r sin(beam_err))^2 (1 - c^2) / c^2) + floor_var, w = 1 / s2, H =
sum w J J^T with math.fsum. The ray-caster itself is pinned to brute force by
test_raycast_gpu.py, so what this checks is the term and the reduction."""
import math

import numpy as np

import raycast_ref as rr

EPS = 2.0 ** -52
MIN_HITS = 16


def unit(dirs):
    """dirs / |dirs| with the device's expression tree (dot3: a0 b0 + a1 b1 + a2 b2, then sqrt)."""
    d = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return d / dn[:, None]


def terms(hits, rd, r, floor_var=0.0, use=None):
    """Per ray (J (n, 6), w (n,), ok (n,)): hits: vg_raycast's records; rd: r d (n, 3); r: the range of the
    beam-noise term; use: a mask of the rays that may contribute (None: every hit)."""
    rd = np.asarray(rd, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(r, dtype=np.float64)
    hit = (hits["flags"] & 1) != 0
    if use is not None:
        hit = hit & use
    n = hits["normal"]
    c2 = hits["ndotd"] * hits["ndotd"]
    with np.errstate(all="ignore"):
        s2 = c2 * (hits["var"] + rr.DEPT * rr.DEPT + (r * r * rr.BEAM_DV) * (1.0 - c2) / c2) + floor_var
    ok = hit & np.isfinite(s2) & (s2 > 0.0)
    J = np.concatenate([n, np.cross(rd, n)], axis=1)
    w = np.where(ok, 1.0 / np.where(ok, s2, 1.0), 0.0)
    return J, w, ok


def info_sum(J, w, ok):
    """(H (6, 6) symmetric, n_hits, sum_w): each entry the exactly rounded sum of its terms (w J_i) J_j."""
    H = np.zeros((6, 6))
    Jk, wk = J[ok], w[ok]
    for i in range(6):
        wj = wk * Jk[:, i]
        for j in range(i, 6):
            H[i, j] = H[j, i] = math.fsum(wj * Jk[:, j])
    return H, int(ok.sum()), math.fsum(wk)


def place_ref(ctx, origin, dirs, floor_var=0.0, **ray):
    """The reference record of one place from ctx.raycast of its D rays: (H, n_hits, sum_w, hits)."""
    hits = ctx.raycast(origin, dirs, **ray)
    J, w, ok = terms(hits, hits["range"][:, None] * unit(dirs), hits["range"], floor_var)
    return info_sum(J, w, ok) + (hits,)


def bound(H_ref, terms_n):
    """|H_ij - ref_ij| <= (n + 32) 2^-52 sqrt(H_ii H_jj): by Cauchy-Schwarz sum |w J_i J_j| <= sqrt(H_ii H_jj),
    an n-term f64 sum in any order errs by at most n eps of that, and 32 covers each term's few ulps."""
    dg = np.sqrt(np.diag(H_ref))
    return (terms_n + 32) * EPS * np.outer(dg, dg)


def schur(H):
    """(S_t, S_r) of a 6 x 6 H ordered [p, theta]."""
    Hpp, Hpt, Htt = H[:3, :3], H[:3, 3:], H[3:, 3:]
    return Hpp - Hpt @ np.linalg.inv(Htt) @ Hpt.T, Htt - Hpt.T @ np.linalg.inv(Hpp) @ Hpt
