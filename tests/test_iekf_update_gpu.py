"""k_iekf_update (vg_iekf.h: the 6 x 6 push-through solve on one wave, and the
ordered reduction in front of it) run alone on given sums (vgx_iekf_update),
against the reference's algorithm, K_1 = (H_T_H + cov^-1)^-1 with two 15 x 15
inverses (odometry.cpp:192-227), evaluated at 50 digits (hp_ref.iekf_update).

The update (the 34 final sums given). HTH / HTz / nnt from synthetic planes
and 2,000 points: eight normals, one normal (rank 1), two (rank 2), no match
(all sums zero: G6 must be exactly 0 and the state x_curr + (x_prop - x_curr)),
and the eight-normal sums scaled to sum R_inv = 1e12; each with the seed
covariance of synth.gt_state and with a block-scaled D A D covariance (blocks
1e-10..1e-2); it in {0, 2, 3} x rematch in {0, 1}, with a far (not converged)
and a near (converged) x_prop. iters, matches, rematch and done are checked
exactly against odometry.cpp:205-227 (solution norms at least a factor 2 from
the 0.01 deg / 0.015 cm limits); the covariance is compared when the IEKF
stops and must be untouched otherwise.

Errors per group (R, p, v, bg, ba, the 3-row blocks of G6, the 3 x 3 blocks
of the covariance) in units of the group's largest reference entry; e_f64 is
the same two-inverse route in fp64 numpy (f64_ref.iekf_update). Asserted per
class: e_dev / max(e_f64, 2^-53) <= BOUND, the next power of two above twice
the worst ratio measured on an MI355X (beside each bound; above 64 would be a
finding). One was: "big/scaled" measured 388 (G's position rows, e_dev 5.6e-14
against e_f64 1.4e-16): with the covariance blocks decades apart the rows of
I + HTH cov66 differ by as much, and partial pivoting picked poor pivots. The
solve now runs in the covariance's units (power-of-two scaling, exact: results
with rotation and position variances of one scale are unchanged bit for bit),
which brought the class to 6.4.

The reduction (block partials given): nb in {1, 7, 8, 64, 512} x n_points in
{1, 255, 256, 771, nb * 256}; rows of chunks beyond ceil(n_points / 256) are
+0 as k_iekf writes them (chunk of row b: (b % 8) * (nb / 8) + b / 8 when nb
is a multiple of 8, else b), the others hold entries of mixed sign over eight
decades. A selector state (R = I, zero state, cov(6 + i, i) = 1, everything
else 0) makes the update hand the sums back exactly: G6 rows 6..11 = HTH,
v / bg = HTz, nnt and matches directly. Bound per sum, derived:
(rows - 1) 2^-53 sum |x_i| against math.fsum."""
import math

import numpy as np
import pytest

import f64_ref
import hp_ref
import la_cases
import synth
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

# class -> bound; measured ratio on an MI355X beside it
BOUND = {
    "eight/seed": 8,  # 2.145
    "eight/scaled": 4,  # 1.492
    "rank1/seed": 8,  # 3.728
    "rank1/scaled": 4,  # 1.556
    "rank2/seed": 8,  # 3.102
    "rank2/scaled": 8,  # 2.444
    "none/seed": 4,  # 1.19
    "none/scaled": 2,  # 0.6624
    "big/seed": 8,  # 2.229
    "big/scaled": 16,  # 6.443 (388.4 before the solve was equilibrated, vg_iekf.h)
}


@pytest.fixture(scope="module")
def ctx():
    c = vgpu.Context(vgconfig.to_c(vgconfig.load("mid360")), max_points=20_000, max_nodes=100_000,
                     max_fix_points=200_000, hash_log2=16)
    yield c
    c.close()


def _sums(rng, R, normals, npts, resi_sigma, total=None):
    """The point loop's sums (odometry.cpp:134-147) for npts points on planes with the given normals."""
    s = np.zeros(34)
    if not len(normals):
        return s
    HTH, HTz, nnt = np.zeros((6, 6)), np.zeros(6), np.zeros((3, 3))
    pts = rng.uniform(-10, 10, (npts, 3))
    w = 1.0 / (0.0005 + rng.uniform(0.0, 0.01, npts))
    if total is not None:
        w *= total / w.sum()
    for p, wi in zip(pts, w):
        n = normals[rng.integers(len(normals))]
        jac = np.concatenate([f64_ref.hat(p) @ R.T @ n, n])
        HTH += wi * np.outer(jac, jac)
        HTz -= wi * jac * rng.normal(0, resi_sigma)
        nnt += np.outer(n, n)
    s[:21] = HTH[np.triu_indices(6)]
    s[21:27] = HTz
    s[27:33] = nnt[np.triu_indices(3)]
    s[33] = npts
    return s


def _cases():
    rng = np.random.default_rng(21)
    x0 = synth.Sequence("tiny", seq_id=1, blind=0.5).gt_state(3)
    R = x0[1:10].reshape(3, 3)
    nrm = rng.normal(size=(8, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    covs = {"seed": x0[25:].reshape(15, 15).copy(), "scaled": la_cases.block_scaled(rng, 15, 1e-5, 1e-1)}
    out = []
    for near in (False, True):
        sig = 1e-9 if near else 0.1
        sums = {"eight": _sums(rng, R, nrm, 2000, sig), "rank1": _sums(rng, R, nrm[:1], 2000, sig),
                "rank2": _sums(rng, R, nrm[:2], 2000, sig), "none": np.zeros(34),
                "big": _sums(rng, R, nrm, 2000, sig, total=1e12)}
        for sname, s in sums.items():
            for cname, cov in covs.items():
                xc = x0.copy()
                xc[25:] = cov.reshape(-1)
                xp = xc.copy()
                d = sig * np.ones(15)  # the prior's offset from x_curr
                xp[1:10] = (R @ la_cases.rodrigues(d[:3] * rng.normal(size=3))).reshape(-1)
                xp[10:22] += d[3:] * rng.normal(size=12)
                out.append((sname + "/" + cname, near, s, xc, xp))
    return out


def _groups(ref, x, G6):
    """(device / fp64 value, reference) per group."""
    g = [(x[1:10], ref["R"]), (x[10:13], ref["p"]), (x[13:16], ref["v"]), (x[16:19], ref["bg"]),
         (x[19:22], ref["ba"])]
    g += [(G6[3 * b:3 * b + 3], ref["G6"][3 * b:3 * b + 3, :]) for b in range(5)]
    if ref["done"]:
        cov = x[25:].reshape(15, 15)
        g += [(cov[3 * a:3 * a + 3, 3 * b:3 * b + 3], ref["cov"][3 * a:3 * a + 3, 3 * b:3 * b + 3])
              for a in range(5) for b in range(5)]
    return g


def test_update_against_two_inverse_reference(ctx):
    worst = {k: 0.0 for k in BOUND}
    fig = {k: (0.0, 0.0) for k in BOUND}
    for cls, near, s, xc, xp in _cases():
        for it in (0, 2, 3):
            for rm in (0, 1):
                ref = hp_ref.iekf_update(s, xc, xp, it, rm)
                assert ref["conv_margin"] > 0.5, (cls, near, ref["conv_margin"])  # well away from the limits
                f = f64_ref.iekf_update(s, xc, xp, it, rm)
                x, G6, nnt, fl = ctx.iekf_update(s, 2000, xc, xp, it, rm)
                assert list(fl) == [it + 1, int(s[33]), ref["rematch"], ref["done"]], (cls, near, it, rm, fl)
                assert np.array_equal(nnt, s[27:33]) and x[0] == xc[0] and np.array_equal(x[22:25], xc[22:25])
                if not ref["done"]:
                    assert np.array_equal(x[25:], xc[25:]), "covariance untouched before the IEKF stops"
                if cls.startswith("none"):
                    assert np.all(G6 == 0.0)
                xf = np.concatenate([[xc[0]], f["R"].reshape(-1), f["p"], f["v"], f["bg"], f["ba"], xc[22:25],
                                     f["cov"].reshape(-1)])
                for (dv, rv), (fv, _) in zip(_groups(ref, x, G6), _groups(ref, xf, f["G6"])):
                    scale = hp_ref.maxabs(rv)
                    if scale == 0.0:
                        assert np.all(np.asarray(dv) == 0.0), (cls, it, rm)
                        continue
                    ed, ef = hp_ref.err(dv, rv) / scale, hp_ref.err(fv, rv) / scale
                    r = ed / max(ef, U)
                    if r > worst[cls]:
                        worst[cls], fig[cls] = r, (ed, ef)
    for cls in BOUND:
        print("RATIO %-14s e_dev %.3e e_f64 %.3e ratio %.4g" % (cls, fig[cls][0], fig[cls][1], worst[cls]))
    for cls in BOUND:
        assert worst[cls] <= BOUND[cls], (cls, worst[cls], fig[cls])


def _chunk(b, nb):
    return (b % 8) * (nb // 8) + b // 8 if nb % 8 == 0 else b


@pytest.mark.parametrize("nb", [1, 7, 8, 64, 512])
def test_ordered_reduction(ctx, nb):
    rng = np.random.default_rng(100 + nb)
    xc = np.zeros(250)
    xc[1:10] = np.eye(3).reshape(-1)
    cov = np.zeros((15, 15))
    cov[6:12, 0:6] = np.eye(6)  # the selector: K6 rows 6..11 = I, so G6 rows 6..11 = HTH and v, bg = HTz
    xc[25:] = cov.reshape(-1)
    for n_points in (1, 255, 256, 257 * 3, nb * 256):
        nact = min(nb, (n_points + 255) // 256)
        P = np.zeros((nb, 34))
        act = [b for b in range(nb) if _chunk(b, nb) < nact]
        assert len(act) == nact
        P[act] = rng.choice([-1.0, 1.0], (nact, 34)) * 10.0 ** rng.uniform(-4, 4, (nact, 34))
        P[act, 33] = rng.integers(-10 ** 6, 10 ** 6, nact)
        x, G6, nnt, fl = ctx.iekf_update(P, n_points, xc, xc, 0, 0, reduce=True)
        got = np.zeros(34)
        k = 0
        for i in range(6):
            for j in range(i, 6):
                got[k] = G6[6 + i, j]
                assert G6[6 + j, i] == G6[6 + i, j]
                k += 1
        got[21:27] = x[13:19]
        got[27:33] = nnt
        got[33] = fl[1]
        for c in range(34):
            want = math.fsum(P[act, c])
            bound = (nact - 1) * U * np.abs(P[act, c]).sum()
            assert abs(got[c] - want) <= bound, (nb, n_points, c, got[c], want, bound)
        assert list(fl) == [1, int(math.fsum(P[act, 33])), 1, 0]
        assert np.array_equal(x[1:13], xc[1:13]) and np.array_equal(x[25:], xc[25:])
