"""Pin tests/hp_ref.py (the 50-digit references of the device tests) itself:
against numpy / scipy on well-conditioned random inputs, against the oracle's
eig3 / inverse15 / orc_so3 on test_oracle_math.py's input sets, and the plane
decisions' threshold band on the device test's cluster set. CPU only."""
import numpy as np
from scipy.spatial.transform import Rotation

import f64_ref
import hp_ref
import la_cases
import oracle


def _sym(rng, n, scale=1.0):
    A = rng.normal(size=(n, n)) * scale
    return 0.5 * (A + A.T)


def test_eig3_matches_numpy_and_oracle(oracle_lib):
    rng = np.random.default_rng(1)  # test_oracle_math.py's set
    for k in range(60):
        A = _sym(rng, 3, 10.0 ** rng.uniform(-4, 2))
        if k % 3 == 0:
            U, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            A = U @ np.diag([1e-6, 0.04, 0.2]) @ U.T
        w, V = hp_ref.eig3(A)
        wf, Vf = np.array([float(x) for x in w]), hp_ref.to_np(V)
        wn = np.linalg.eigvalsh(A)
        s = max(1.0, np.abs(wn).max())
        assert np.all(np.diff(wf) >= 0)
        assert np.abs(wf - wn).max() <= 1e-13 * s
        assert np.abs(wf - oracle.eig3(A)[0]).max() <= 1e-13 * s
        As = (hp_ref.M(A) + hp_ref.M(A).T) / 2
        assert hp_ref.maxabs(As * V - V * hp_ref.mp.diag(w)) < 1e-40 * s
        assert hp_ref.maxabs(V.T * V - hp_ref.mp.eye(3)) < 1e-40
        assert np.abs(Vf.T @ Vf - np.eye(3)).max() < 1e-15


def test_inverse_and_lstsq_match_numpy(oracle_lib):
    rng = np.random.default_rng(2)  # test_oracle_math.py's set
    for _ in range(5):
        Mx = rng.normal(size=(15, 15))
        A = Mx @ Mx.T + 1e-3 * np.eye(15)
        inv = hp_ref.to_np(hp_ref.inverse(A))
        assert np.allclose(inv, np.linalg.inv(A), rtol=1e-9, atol=1e-9)
        assert np.allclose(inv, oracle.inverse15(A), rtol=1e-9, atol=1e-9)
        assert hp_ref.maxabs(hp_ref.M(A) * hp_ref.inverse(A) - hp_ref.mp.eye(15)) < 1e-35
    for m in (3, 5, 8):
        A, b = rng.normal(size=(m, 3)), rng.normal(size=m)
        x = hp_ref.to_np(hp_ref.lstsq(A, b))[:, 0]
        assert np.allclose(x, np.linalg.lstsq(A, b, rcond=None)[0], rtol=1e-10, atol=1e-12)
    A = rng.normal(size=(5, 3))
    A[:, 1] = 0.0  # a zero column: the basic solution leaves it at zero
    x = hp_ref.to_np(hp_ref.lstsq(A, -np.ones(5)))[:, 0]
    assert x[1] == 0.0 and np.allclose(x[[0, 2]], np.linalg.lstsq(A[:, [0, 2]], -np.ones(5), rcond=None)[0])


def test_so3_matches_scipy_and_oracle(oracle_lib):
    L = oracle.lib()
    rng = np.random.default_rng(3)  # test_oracle_math.py's set
    for _ in range(50):
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * rng.uniform(1e-6, 3.0)
        R, lg, J, Ji = (np.zeros(9), np.zeros(3), np.zeros(9), np.zeros(9))
        L.orc_so3(oracle._d(w), oracle._d(R), oracle._d(lg), oracle._d(J), oracle._d(Ji))
        Rs = Rotation.from_rotvec(w).as_matrix()
        assert hp_ref.err(Rs, hp_ref.Exp(w)) < 1e-15
        assert hp_ref.err(R, hp_ref.Exp(w)) < 1e-15
        assert hp_ref.err(Rs, hp_ref.Exp_dt(w / 0.37, 0.37)) < 1e-15
        # the project's Log is the true logarithm beyond its small-angle branch (|w| > 1e-3 here)
        ang = np.linalg.norm(w)
        if ang > 2e-3:
            assert hp_ref.err(Rotation.from_matrix(R.reshape(3, 3)).as_rotvec(), hp_ref.Log(R.reshape(3, 3))) \
                < 1e-9
        assert hp_ref.err(lg, hp_ref.Log(R.reshape(3, 3))) < 1e-9
        assert hp_ref.err(J, hp_ref.jr(w)) < 1e-14
        assert hp_ref.err(Ji, hp_ref.jr_inv(R.reshape(3, 3))) < 1e-9
        # jr_inv(Exp(w)) inverts jr(w), with the exponential taken at 50 digits too
        assert hp_ref.maxabs(hp_ref.jr_inv(hp_ref.to_np(hp_ref.Exp(w))) * hp_ref.jr(w) - hp_ref.mp.eye(3)) < 1e-14
        # the fp64 yardstick agrees with the reference as well
        assert hp_ref.err(f64_ref.jr_inv(R.reshape(3, 3)), hp_ref.jr_inv(R.reshape(3, 3))) < 1e-9
        assert hp_ref.err(f64_ref.Log(R.reshape(3, 3)), hp_ref.Log(R.reshape(3, 3))) < 1e-9


def test_so3_branches():
    assert hp_ref.maxabs(hp_ref.Exp(np.array([0.9e-9, 0, 0])) - hp_ref.mp.eye(3)) == 0
    assert hp_ref.maxabs(hp_ref.Exp(np.array([1.1e-9, 0, 0])) - hp_ref.mp.eye(3)) > 1e-9
    assert hp_ref.maxabs(hp_ref.Exp_dt(np.array([0.9e-7, 0, 0]), 1e6) - hp_ref.mp.eye(3)) == 0
    assert hp_ref.maxabs(hp_ref.Exp_dt(np.array([1.1e-7, 0, 0]), 1e6) - hp_ref.mp.eye(3)) > 1e-2
    R = la_cases.rodrigues(np.array([0.0, 0.9e-3, 0.0]))  # inside the cut-off: 0.5 K, not the logarithm
    K = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    assert hp_ref.err(K, hp_ref.Log(R)) == 0.0


def test_cluster_matches_numpy():
    clu = la_cases.cluster_cases()
    for name in ("plane_0m", "line_5m"):
        for c in clu[name][:6]:
            assert hp_ref.err(f64_ref.clu_cov(c), hp_ref.clu_cov(c)) < 1e-12
    for x in la_cases.transform_cases()[:6]:
        ref = hp_ref.clu_transform(x[:10], x[10:19].reshape(3, 3), x[19:22])
        f = f64_ref.clu_transform(x[:10], x[10:19].reshape(3, 3), x[19:22])
        assert hp_ref.err(f, ref) <= 1e-13 * hp_ref.maxabs(ref)
        # a transformed cluster's covariance is the rotated covariance
        R = hp_ref.M(x[10:19].reshape(3, 3))
        c0, c1 = hp_ref.clu_cov(x[:10]), hp_ref.clu_cov(hp_ref.to_np(ref)[:, 0])
        assert hp_ref.maxabs(c1 - R * c0 * R.T) < 1e-9
    for c in clu["point_50m"]:
        assert hp_ref.maxabs(hp_ref.clu_cov(c)) == 0


def test_plane_decision_band():
    """At most 1 % of the cluster items lie within 1e-9 (relative) of a
    threshold of the recut's comparisons, and the classes decide as built."""
    n = band = 0
    for name, cs in la_cases.cluster_cases().items():
        for c in cs:
            w, _ = hp_ref.eig3(hp_ref.clu_cov(c))
            dec, margin = hp_ref.plane_decisions(w, la_cases.MIN_EIG, la_cases.THRE)
            n += 1
            band += margin < 1e-9
            if name.startswith("plane"):
                assert dec == [True, True, False], (name, dec)
            if name.startswith("point"):
                assert dec == [True, False, False], (name, dec)
    assert n > 100 and band <= 0.01 * n, (n, band)


def test_iekf_update_matches_numpy():
    import synth
    rng = np.random.default_rng(4)
    seq = synth.Sequence("tiny", seq_id=1, blind=0.5)
    xc = seq.gt_state(0)
    xp = xc.copy()
    xp[1:10] = (xc[1:10].reshape(3, 3) @ la_cases.rodrigues(rng.normal(size=3) * 1e-2)).reshape(-1)
    xp[10:22] += rng.normal(size=12) * 1e-2
    J = rng.normal(size=(40, 6))
    sums = np.zeros(34)
    sums[:21] = (J.T @ J * 50.0)[np.triu_indices(6)]
    sums[21:27] = J.T @ rng.normal(size=40) * 0.5
    for it, rm in ((0, 0), (2, 0), (3, 1)):
        a, b = hp_ref.iekf_update(sums, xc, xp, it, rm), f64_ref.iekf_update(sums, xc, xp, it, rm)
        assert (a["rematch"], a["done"]) == (b["rematch"], b["done"])
        for k in ("R", "p", "v", "bg", "ba", "G6", "cov", "sol"):
            assert hp_ref.err(b[k], a[k]) < 1e-10 * max(1.0, hp_ref.maxabs(a[k])), k
    # no match: the state becomes x_prop (x_curr + (x_prop - x_curr)), G = 0
    a = hp_ref.iekf_update(np.zeros(34), xc, xp, 0, 0)
    assert hp_ref.maxabs(a["G6"]) == 0
    assert hp_ref.err(xp[10:13], a["p"]) < 1e-30 and hp_ref.err(xp[1:10], a["R"]) < 1e-12
