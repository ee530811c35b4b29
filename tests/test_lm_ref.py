"""tests/lm_ref.py (the LM step's reference) pinned on the CPU: its solve
against the oracle's restatement of Eigen's LDLT (orc_ldlt_solve) on the
systems test_ba_solve_gpu.py uses — a plain solve and the left-looking pivoted
LDLT agree to the conditioning of M M^T + lam I (~1e2-1e3, so 1e-10 relative
in the scaled unknowns) — and on a system with a decoupled zero-pivot unknown,
where the oracle's answer (0 for that unknown) is the specification; its
assembly against a brute-force accumulation of zero-padded 30 x 30 blocks at
15k offsets on integer data (every sum exact); its pivot order on a worked
example of Eigen's transpositions."""
import numpy as np
import pytest

import lm_ref
import oracle

TOL = 1e-10


def _spd(m, rng):
    M = rng.standard_normal((m, m))
    A = M @ M.T + m * np.eye(m)
    d = 10.0 ** rng.uniform(-2, 4, m)
    return d, (A * d[:, None]) * d[None, :]


def _indef(m, rng):
    M = rng.standard_normal((m, m))
    A = 0.5 * (M + M.T)
    A[np.diag_indices(m)] = rng.choice([-1.0, 1.0], m) * (4 * m + rng.uniform(0, m, m))
    d = 10.0 ** rng.uniform(-1, 3, m)
    return d, (A * d[:, None]) * d[None, :]


@pytest.mark.parametrize("m", [15, 30, 135, 150])  # mpmath below lm_ref.MP_MAX, refined numpy above
@pytest.mark.parametrize("kind", ["spd", "indefinite"])
def test_solve_matches_oracle_ldlt(oracle_lib, m, kind):
    rng = np.random.default_rng(7 * m + (kind == "spd"))
    d, A = (_spd if kind == "spd" else _indef)(m, rng)
    b = rng.standard_normal(m) * d
    x, ref = lm_ref.solve(A, b), oracle.ldlt_solve(A, b)
    err = np.abs(d * (x - ref)).max() / np.abs(d * ref).max()
    print(m, kind, "err %.2e" % err)
    assert err < TOL


@pytest.mark.parametrize("m", [30, 135])
def test_solve_zero_pivot_matches_oracle(oracle_lib, m):
    rng = np.random.default_rng(m)
    d, A = _spd(m, rng)
    b = rng.standard_normal(m) * d
    z = m // 3
    A[z, :] = 0.0
    A[:, z] = 0.0
    b[z] = 0.0
    x, ref = lm_ref.solve(A, b), oracle.ldlt_solve(A, b)
    assert x[z] == 0.0 and ref[z] == 0.0
    assert np.abs(d * (x - ref)).max() / np.abs(d * ref).max() < TOL
    keep = [i for i in range(m) if i != z]
    red = np.linalg.solve(A[np.ix_(keep, keep)], b[keep])
    assert np.abs(d[keep] * (x[keep] - red)).max() / np.abs(d[keep] * red).max() < TOL


@pytest.mark.parametrize("W", [2, 3, 5])
def test_assemble_matches_brute_force(W):
    rng = np.random.default_rng(W)
    n, L = 15 * W, 6 * W
    hs = rng.integers(-50, 50, (L, L)).astype(np.float64)
    hs = np.tril(hs) + np.tril(hs, -1).T
    hl = np.concatenate([lm_ref.pack_lower(hs), rng.integers(-50, 50, L + 1).astype(np.float64)])
    imu = rng.integers(-50, 50, (W - 1, 931)).astype(np.float64)
    coef = 0.25
    H, J, res = lm_ref.assemble(hl, imu, W, coef)
    Hb, Jb, rb = np.zeros((n, n)), np.zeros(n), 0.0
    for k in range(W - 1):
        pad = np.zeros((n, n))
        pad[15 * k: 15 * k + 30, 15 * k: 15 * k + 30] = imu[k, :900].reshape(30, 30)
        Hb += coef * pad
        g = np.zeros(n)
        g[15 * k: 15 * k + 30] = imu[k, 900:930]
        Jb += coef * g
        rb += 0.5 * coef * imu[k, 930]
    S = np.zeros((n, L))  # LiDAR unknown 6i + r is unknown 15i + r
    for i in range(W):
        S[15 * i: 15 * i + 6, 6 * i: 6 * i + 6] = np.eye(6)
    Hb += S @ hs @ S.T
    Jb += S @ hl[L * (L + 1) // 2: L * (L + 1) // 2 + L]
    rb += hl[-1]
    assert np.array_equal(np.tril(H), np.tril(Hb)) and np.array_equal(H, H.T)
    assert np.array_equal(J, Jb) and res == rb


def test_pivot_order_follows_eigens_transpositions():
    W = 2
    D = np.ones(30)
    D[15:] = np.arange(100.0, 85.0, -1.0)  # distinct, above the gauge frame's 1 + u: descending order
    assert lm_ref.pivot_order(D, 0.01, False) == list(range(15, 30))
    # 3, 3, 5 at positions 27, 28, 29 (all above the gauge frame's): step 12 takes 29 and moves the
    # entry of position 12 there; the equal entries 27, 28 keep their positions, so 27 comes first
    D[27:30] = [3.0, 3.0, 5.0]
    D[15:27] = np.arange(100.0, 88.0, -1.0)
    o = lm_ref.pivot_order(D, 0.01, False)
    assert o[:12] == list(range(15, 27)) and o[12:] == [29, 27, 28]
    # every entry below the gauge frame's, which therefore goes first and stays in place; the equal
    # entries 15 and 16 are the smallest. Step 15 takes 29 and moves 15 to position 29, step 16
    # takes 28 and moves 16 to position 28: at the end 16 stands before 15
    D[15:30] = [0.5, 0.5] + list(np.linspace(0.6, 0.7, 11)) + [0.8, 0.9]
    o = lm_ref.pivot_order(D, 0.01, False)
    key = np.abs(D + 0.01 * D)
    assert sorted(o) == list(range(15, 30)) and np.all(np.diff(key[o]) <= 0)
    assert o[:2] == [29, 28] and o[-2:] == [16, 15]
    assert lm_ref.pivot_order(D, 0.01, True) == list(range(21, 30)) + list(range(15, 21))
