"""The LM step between the Hessian pass and the residual pass, and the LM
bookkeeping, kernel by kernel against tests/lm_ref.py (written from
optimizers.cpp:430-517 and Eigen's LDLT; pinned on the CPU by
tests/test_lm_ref.py):

* vgx_ba_step runs k_ba_prep then k_ba_solve through the launch helper an LM
  iteration uses, on given LiDAR / IMU systems, window states, bias records and
  u, v, calc_hess: the assembly, the gauge frame, the damping, both pivot
  orders (vgx_debug 31), the tile image with its padding, res1, the retry
  branch, the un-permutation, the trial states, the bias records and q1;
* vgx_ba_control runs k_ba_control on a given LM state: accept / reject, u, v,
  calc_hess, done, iters, nhess, fin, xs <- xt and the bias restore. The
  unsharded product path runs the same ba_control_body inside k_ba_resid's IMU
  workgroup; that fused entry needs a live map and stays covered end to end
  only (test_pipeline_gpu.py).

W = 2 (one IMU block, one 16 x 16 tile with 15 real rows), 3 (the first
overlap of two IMU blocks), 10 (the bench window: 135 unknowns padded to 144)
and 11 (the LDS limit). imu_coef is 2^-13 (a power of two near mid360's 1e-4),
so the assembly of integer data is exact. The gauge frame's rows of the stored
system are never written by the device (they are not factored), so Hcalc is
compared on the unknowns of frames 1..W-1.

Bounds. Step (b, e): 1e-10 relative in the scaled unknowns, the solver's own
bound (test_ba_solve_gpu.py). Trial rotations (f): the device's error against
the 50-digit R Exp(dx) at most 4 times fp64 numpy's, the factor
test_device_la_gpu.py grants Exp and the 3 x 3 products; everything additive
exact. q1 (g): n 2^-53 sum|terms|, n = 15W, the bound of a fixed-order sum
(terms: the 2n products of lm_ref.q1). Control (h): exact, u after an accepted
step within 4 ulp (pow).

Observed on an MI355X (printed by every run): b step error <= 1.6e-15 under
either order, spd and indefinite alike, the two orders within 1.5e-15 of each
other; e <= 9.7e-16 against the reference and the oracle; f rotation error
<= 1.3e-16 where fp64 numpy's is <= 1.0e-16 (ratio <= 1.5); g |q1 - reference|
<= 0.03 of the bound.

No workload of the suite rejects an LM step: the oracle on the CPU, over every
sequence test_pipeline_gpu.py, test_ba_hessian_gpu.py and the gravity / long /
path cases step, counts 0 scans with ba_iters above the Hessian passes (mid360
16line x 16: 0 of 7 LM scans; mid360 64line x 30: 0 of 21; mid360 128line x 14:
0 of 5; mid360 1M x 11: 0 of 2; velodyne 16line x 16: 0 of 7; gravity-scale
16line x 14: 0 of 5; path 16line x 16: 0 of 7; W = 11 16line x 15: 0 of 5; long
16line x 240: 0 of 231; HILTI and robosense run no LM). So the calc_hess == 0
branch and the bias restore run under a check only here (d, h)."""
import numpy as np
import pytest

import f64_ref
import hp_ref
import lm_ref
import oracle
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu
TOL = 1e-10
COEF = 2.0 ** -13
U53 = 2.0 ** -53
WINS = [2, 3, 10, 11]
US = [0.01, 0.01 / 3, 1e3]
RESID_BLOCKS = 512  # k_ba_resid's workgroup count (vg_ba.h kResidBlocks; test_control_rejects_too_many_partials)

_ctxs = {}


@pytest.fixture(scope="module")
def ctx_for():
    def get(W):
        if W not in _ctxs:
            p = vgconfig.load("mid360")
            p["LocalBA"]["win_size"] = W
            p["LocalBA"]["imu_coef"] = COEF
            _ctxs[W] = vgpu.Context(vgconfig.to_c(p), max_points=20_000, max_nodes=100_000, max_fix_points=200_000,
                                    hash_log2=16)
        return _ctxs[W]
    yield get
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()


def _order(ctx, structural):
    ctx.debug(31, 1 if structural else 0)


# ---- inputs ------------------------------------------------------------------------------------------

def _mask(W):
    """Entries the assembled system can hold: same or adjacent frames (an IMU block), or two pose slots."""
    n = 15 * W
    f, pose = np.arange(n) // 15, (np.arange(n) % 15) < 6
    return (np.abs(f[:, None] - f[None, :]) <= 1) | (pose[:, None] & pose[None, :])


def _split(T, g, r_imu, r_lidar, W):
    """hl and imuout that assemble to the symmetric T (15W x 15W, within _mask), the gradient g and the
    residual parts: every entry is shared equally among the IMU blocks that cover it and, for pose
    slots, the LiDAR part; the IMU parts are divided by imu_coef (exact: a power of two)."""
    n, L = 15 * W, 6 * W
    cnt = np.zeros((n, n))
    cg = np.zeros(n)
    for k in range(W - 1):
        cnt[15 * k: 15 * k + 30, 15 * k: 15 * k + 30] += 1
        cg[15 * k: 15 * k + 30] += 1
    pose = np.array([15 * (i // 6) + i % 6 for i in range(L)])
    cnt[np.ix_(pose, pose)] += 1
    cg[pose] += 1
    assert np.all(T[cnt == 0] == 0.0)
    share, gshare = T / np.maximum(cnt, 1), g / cg
    imu = np.zeros((W - 1, 931))
    for k in range(W - 1):
        imu[k, :900] = (share[15 * k: 15 * k + 30, 15 * k: 15 * k + 30] / COEF).reshape(-1)
        imu[k, 900:930] = gshare[15 * k: 15 * k + 30] / COEF
        imu[k, 930] = r_imu[k]
    hl = np.concatenate([lm_ref.pack_lower(share[np.ix_(pose, pose)]), gshare[pose], [r_lidar]])
    return hl, imu


def _system(W, kind, rng):
    """A realistic system in the structure the LM assembles: 'spd' = the sum of M M^T + lam I pieces (one
    per IMU block, one LiDAR), 'indefinite' = symmetric, diagonally dominant with diagonal signs mixed;
    both scaled by D over decades (the constructions of test_ba_solve_gpu.py). Returns d, T, g."""
    n, L = 15 * W, 6 * W
    if kind == "spd":
        T = np.zeros((n, n))
        for k in range(W - 1):
            M = rng.standard_normal((30, 30))
            T[15 * k: 15 * k + 30, 15 * k: 15 * k + 30] += M @ M.T + 30 * np.eye(30)
        M = rng.standard_normal((L, L))
        pose = np.array([15 * (i // 6) + i % 6 for i in range(L)])
        T[np.ix_(pose, pose)] += M @ M.T + L * np.eye(L)
        d = 10.0 ** rng.uniform(-2, 4, n)
    else:
        M = rng.standard_normal((n, n))
        T = 0.5 * (M + M.T) * _mask(W)
        T[np.diag_indices(n)] = rng.choice([-1.0, 1.0], n) * (4 * n + rng.uniform(0, n, n))
        d = 10.0 ** rng.uniform(-1, 3, n)
    T = (T * d[:, None]) * d[None, :]
    return d, T, rng.standard_normal(n) * d


def _states(W, rng, scale=1.0):
    xs = np.zeros((W, 24))
    for j in range(W):
        xs[j, :9] = f64_ref.Exp(rng.standard_normal(3)).reshape(-1)
        xs[j, 9:24] = rng.standard_normal(15) * scale
    return xs, rng.standard_normal((W - 1, 12))


def _inputs(W, kind, seed, zero=()):
    rng = np.random.default_rng(seed)
    d, T, g = _system(W, kind, rng)
    for z in zero:
        T[z, :] = 0.0
        T[:, z] = 0.0
        g[z] = 0.0
    hl, imu = _split(T, g, rng.uniform(1, 2, W - 1), rng.uniform(1, 2), W)
    xs, bias = _states(W, rng)
    return d, hl, imu, xs, bias


def _scaled_err(d, x, ref):
    return float(np.abs(d[15:] * (x[15:] - ref[15:])).max() / np.abs(d[15:] * ref[15:]).max())


# ---- a. assembly, bit for bit ------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_assembly_is_exact_on_integer_data(ctx_for, W):
    ctx = ctx_for(W)
    n, L = 15 * W, 6 * W
    nout = L * (L + 1) // 2 + L + 1
    hl = np.arange(1, nout + 1, dtype=np.float64)  # distinct; the diagonal entries are positive
    imu = np.zeros((W - 1, 931))
    for k in range(W - 1):  # a value range per block (a block of the wrong frame cannot cancel), entries distinct
        imu[k] = 10000.0 * (k + 1) + np.arange(931)
    xs, bias = _states(W, np.random.default_rng(W))
    H, J, res1 = lm_ref.assemble(hl, imu, W, COEF)
    for structural in (True, False):
        _order(ctx, structural)
        o = ctx.ba_step(W, hl, imu, xs, bias, 0.01)
        Hd = lm_ref.unpack_lower(o["Hcalc"], n)
        assert np.array_equal(Hd[15:, 15:], H[15:, 15:]), (W, structural)
        assert np.array_equal(o["Jcalc"], J) and o["res1"] == res1, (W, structural)
        assert np.all(o["dxi"][:15] == 0.0)


# ---- b. the step against the reference ---------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
@pytest.mark.parametrize("kind", ["spd", "indefinite"])
def test_step_matches_reference(ctx_for, W, kind):
    ctx = ctx_for(W)
    d, hl, imu, xs, bias = _inputs(W, kind, 100 * W + (kind == "spd"))
    for u in US:
        ref, _, _ = lm_ref.step(hl, imu, W, COEF, u)
        dx = {}
        for structural in (True, False):
            _order(ctx, structural)
            dx[structural] = ctx.ba_step(W, hl, imu, xs, bias, u)["dxi"]
            assert np.all(dx[structural][:15] == 0.0)
            assert np.all(np.isfinite(dx[structural]))
        es, ee, eo = _scaled_err(d, dx[True], ref), _scaled_err(d, dx[False], ref), _scaled_err(d, dx[True],
                                                                                                dx[False])
        print("STEP W %d %s u %.3g: structural %.2e eigen %.2e between %.2e" % (W, kind, u, es, ee, eo))
        assert es < TOL and ee < TOL and eo < TOL, (W, kind, u, es, ee, eo)


# ---- c. pivot order -----------------------------------------------------------------------------------

def _diag_system(W, D, rng):
    """A diagonal system with the diagonal D (15W) held by one IMU block per frame (so it assembles
    without rounding) and a random gradient."""
    imu = np.zeros((W - 1, 931))
    for j in range(W):
        k, h = (0, 0) if j == 0 else (j - 1, 15)
        for v in range(15):
            imu[k, (h + v) * 30 + h + v] = D[15 * j + v] / COEF
            imu[k, 900 + h + v] = rng.standard_normal() / COEF
    L = 6 * W
    return np.zeros(L * (L + 1) // 2 + L + 1), imu


def _pivot_diagonals(W, u, rng):
    """name -> the diagonal of frames 1..W-1. Every case holds entries whose |D + u D| are equal."""
    m = 15 * W - 15
    out = {}
    # exact ties above and below the gauge frame's 1 + u, and with it
    D = rng.choice([0.25, 0.5, 1.0, 3.0, 3.0, 7.0, 1e3], m)
    D[rng.permutation(m)[: m // 3]] = rng.uniform(0.1, 10.0, m // 3)
    out["ties"] = D
    # negative entries, +x and -x tied in modulus
    D = rng.uniform(0.1, 10.0, m) * rng.choice([-1.0, 1.0], m)
    h = m // 2
    D[h: 2 * h] = -D[:h]
    out["negative"] = rng.permutation(D)
    # neighbours in fp64, 1..3 ulp apart, just below a power of two: distinct in |D|, and D + u D lands in
    # the next binade, where the spacing doubles, so rounding alone ties some pairs and orders the others
    D = rng.uniform(0.992, 0.999, m) * 2.0 ** rng.integers(-2, 3, m)
    for i in range(0, m - 1, 2):
        D[i + 1] = D[i]
        for _ in range(int(rng.integers(1, 4))):
            D[i + 1] = np.nextafter(D[i + 1], np.inf)
    out["rounding"] = rng.permutation(D)
    return out


@pytest.mark.parametrize("W", WINS)
def test_pivot_order(ctx_for, W):
    ctx = ctx_for(W)
    rng = np.random.default_rng(31 * W)
    xs, bias = _states(W, rng)
    u = 0.01
    differs = 0  # cases in which Eigen's order is not "descending, equal entries by index"
    for name, Dm in _pivot_diagonals(W, u, rng).items():
        D = np.concatenate([rng.uniform(0.5, 2.0, 15), Dm])  # the gauge frame's own diagonal is replaced by 1
        hl, imu = _diag_system(W, D, rng)
        H, J, _ = lm_ref.assemble(hl, imu, W, COEF)
        assert np.array_equal(H.diagonal(), D)
        _, Jg, Dg = lm_ref.gauge_damp(H, J, u)
        key = np.abs(Dg + u * Dg)[15:]
        assert len(set(key.tolist())) < key.size, name  # the case holds ties
        if name == "rounding":
            assert len(set(np.abs(Dm).tolist())) == Dm.size
        want = lm_ref.pivot_order(Dg, u, False)
        differs += want != sorted(want, key=lambda i: (-key[i - 15], i))
        _order(ctx, False)
        o = ctx.ba_step(W, hl, imu, xs, bias, u)
        assert o["ipg"].tolist() == want, (W, name)
        ref = -Jg / (Dg + u * Dg)
        assert np.all(o["dxi"][:15] == 0.0)
        assert np.abs(o["dxi"] - ref).max() <= 16 * U53 * np.abs(ref).max(), (W, name)
        _order(ctx, True)
        o = ctx.ba_step(W, hl, imu, xs, bias, u)
        assert o["ipg"].tolist() == lm_ref.pivot_order(Dg, u, True), (W, name)
        assert o["ipg"].tolist() == ([15 * j + v for j in range(1, W) for v in range(6, 15)] +
                                     [15 * j + v for j in range(1, W) for v in range(6)])
        assert np.abs(o["dxi"] - ref).max() <= 16 * U53 * np.abs(ref).max(), (W, name)
    assert differs > 0 or W < 10


# ---- d. the retry path --------------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
@pytest.mark.parametrize("structural", [True, False])
def test_retry_rereads_the_stored_system(ctx_for, W, structural):
    ctx = ctx_for(W)
    _order(ctx, structural)
    _, hl, imu, xs, bias = _inputs(W, "spd", 7 * W)
    _, hl2, imu2, _, _ = _inputs(W, "indefinite", 7 * W + 1)
    u0, v = 0.01, 2.0
    u1 = u0 * v
    fresh = ctx.ba_step(W, hl, imu, xs, bias, u1, v, 1)
    ctx.ba_step(W, hl2, imu2, xs, bias, u0, v, 1)  # another system in between: the store is overwritten
    first = ctx.ba_step(W, hl, imu, xs, bias, u0, v, 1)
    retry = ctx.ba_step(W, np.full_like(hl, np.nan), np.full_like(imu, np.nan), xs, bias, u1, 2 * v, 0)
    for key in ("dxi", "xt", "bias", "ipg"):
        assert np.array_equal(retry[key], fresh[key]), (W, structural, key)
    assert retry["q1"] == fresh["q1"] and np.isfinite(retry["q1"])
    n = 15 * W
    keep = np.array([lm_ref.lo(i, j) for i in range(15, n) for j in range(15, i + 1)])
    assert np.array_equal(retry["Hcalc"][keep], first["Hcalc"][keep])
    assert np.array_equal(retry["Jcalc"], first["Jcalc"])
    assert not np.array_equal(fresh["dxi"], first["dxi"])


# ---- e. a decoupled unknown ---------------------------------------------------------------------------

@pytest.mark.parametrize("W", WINS)
def test_decoupled_unknown_is_zero(oracle_lib, ctx_for, W):
    ctx = ctx_for(W)
    for z in (15 + 7, 15 * (W - 1) + 2):  # a velocity of frame 1, a rotation of the last frame
        d, hl, imu, xs, bias = _inputs(W, "spd", 50 * W + z, zero=(z,))
        H, J, _ = lm_ref.assemble(hl, imu, W, COEF)
        assert not H[z].any() and J[z] == 0.0
        A, Jg, _ = lm_ref.gauge_damp(H, J, 0.01)
        ref = lm_ref.solve(A, -Jg)
        orc = oracle.ldlt_solve(A, -Jg)
        assert ref[z] == 0.0 and orc[z] == 0.0 and _scaled_err(d, ref, orc) < TOL
        for structural in (True, False):
            _order(ctx, structural)
            dx = ctx.ba_step(W, hl, imu, xs, bias, 0.01)["dxi"]
            assert dx[z] == 0.0 and np.all(dx[:15] == 0.0), (W, z, structural, dx[z])
            e1, e2 = _scaled_err(d, dx, ref), _scaled_err(d, dx, orc)
            print("DECOUPLED W %d z %d structural %d: %.2e (reference) %.2e (oracle)" % (W, z, structural, e1, e2))
            assert e1 < TOL and e2 < TOL


# ---- f, g. trial states, bias records, q1 -------------------------------------------------------------

def _tail_frames(W):
    """(the frame whose rotation increment is solved to exactly 0, the frame whose increment is below
    Exp's small-angle branch point 1e-9); the gauge frame's increment is 0 at every W, and the last
    frame always keeps a rotation above the branch point."""
    return (1, 2) if W >= 10 else ((None, 1) if W == 3 else (None, None))


def _tail_inputs(W, seed):
    """A system with the rotations of _tail_frames decoupled from the rest: a zero gradient (dx = 0
    exactly), or one that gives |dx| ~ 5e-10."""
    rng = np.random.default_rng(seed)
    d, T, g = _system(W, "spd", rng)
    zero, tiny = _tail_frames(W)
    for f, grad in ((zero, 0.0), (tiny, 1e-6)):
        for z in ([] if f is None else range(15 * f, 15 * f + 3)):
            T[z, :] = 0.0
            T[:, z] = 0.0
            T[z, z] = 1e4
            g[z] = grad * (z % 15 + 2)
    hl, imu = _split(T, g, rng.uniform(1, 2, W - 1), rng.uniform(1, 2), W)
    xs, bias = _states(W, rng, scale=3.0)
    return hl, imu, xs, bias


@pytest.mark.parametrize("W", WINS)
@pytest.mark.parametrize("structural", [True, False])
def test_trial_states_bias_records_and_q1(ctx_for, W, structural):
    ctx = ctx_for(W)
    _order(ctx, structural)
    hl, imu, xs, bias = _tail_inputs(W, 900 + W)
    u = 0.01
    o = ctx.ba_step(W, hl, imu, xs, bias, u)
    dx = o["dxi"]
    assert np.all(dx[:15] == 0.0)
    zero, tiny = _tail_frames(W)
    if zero is not None:
        assert np.all(dx[15 * zero: 15 * zero + 3] == 0.0)
    if tiny is not None:
        assert 0.0 < np.linalg.norm(dx[15 * tiny: 15 * tiny + 3]) < 1e-9
    assert np.linalg.norm(dx[15 * (W - 1): 15 * (W - 1) + 3]) > 1e-8  # a rotation above the branch point
    Rs, rest, bref = lm_ref.trial(xs, bias, dx)
    e_dev = e_f64 = 0.0
    for j in range(W):
        e_dev = max(e_dev, hp_ref.err(o["xt"][j, :9], Rs[j]))
        e_f64 = max(e_f64, hp_ref.err((xs[j, :9].reshape(3, 3) @ f64_ref.Exp(dx[15 * j: 15 * j + 3])).reshape(-1),
                                      Rs[j]))
    print("TRIAL W %d structural %d: rotation error %.2e, numpy %.2e" % (W, structural, e_dev, e_f64))
    assert e_dev <= 4 * max(e_f64, U53)
    for j in [f for f in (0, zero, tiny) if f is not None]:  # identity increments: the rotation is copied
        assert np.array_equal(o["xt"][j, :9], xs[j, :9]), j
    assert np.array_equal(o["xt"][:, 9:24], rest[:, 9:24])
    assert np.array_equal(o["xt"][:, 21:24], xs[:, 21:24])
    assert np.array_equal(o["bias"], bref)
    assert np.array_equal(o["bias"][:, 6:12], bias[:, 0:6])
    assert np.array_equal(o["bias"][:, 0:3], bias[:, 0:3] + dx.reshape(W, 15)[: W - 1, 9:12])
    assert np.array_equal(o["bias"][:, 3:6], bias[:, 3:6] + dx.reshape(W, 15)[: W - 1, 12:15])
    # q1 on the device's own dx
    H, J, _ = lm_ref.assemble(hl, imu, W, COEF)
    _, Jg, Dg = lm_ref.gauge_damp(H, J, u)
    q, a = lm_ref.q1(dx, u, Dg, Jg)
    bound = 15 * W * U53 * float(a)
    e = float(abs(hp_ref.mp.mpf(o["q1"]) - q))
    print("Q1 W %d structural %d: |q1 - ref| %.2e bound %.2e (%.3f of it), q1 %.6e" % (W, structural, e, bound,
                                                                                      e / bound, o["q1"]))
    assert e <= bound and o["q1"] != 0.0


# ---- h. control -----------------------------------------------------------------------------------------

def _state(**kw):
    s = {"u": 0.01, "v": 2.0, "res1": 0.0, "res2": 0.0, "q1": 1.0, "calc_hess": 1, "done": 0, "iters": 0,
         "nhess": 0, "fin": 0, "skip": 0}
    s.update(kw)
    return s


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def _control_check(ctx, W, state, imures, rpart, xs, xt, bias, want_accept, ulp_u=0):
    got, xs_d, bias_d, acc = ctx.ba_control(W, state, imures, rpart, xs, xt, bias)
    ref, acc_r = lm_ref.control(state, imures, rpart, COEF)
    xs_r, bias_r = lm_ref.control_states(acc_r, xs, xt, bias)
    assert acc == acc_r == want_accept, (acc, acc_r, want_accept)
    for k in lm_ref.STATE_KEYS:
        if k == "u" and ulp_u:
            assert _ulps(got[k], ref[k]) <= ulp_u, (k, got[k], ref[k])
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.array_equal(xs_d, xs_r) and np.array_equal(bias_d, bias_r)
    return got, xs_d, bias_d


@pytest.mark.parametrize("W,nrb", [(3, RESID_BLOCKS), (10, RESID_BLOCKS), (3, 301), (2, 1)])
def test_control(ctx_for, W, nrb):
    ctx = ctx_for(W)
    rng = np.random.default_rng(W + nrb)
    xs, bias = _states(W, rng)
    xt, _ = _states(W, rng)
    imures = rng.uniform(1.0, 2.0, W - 1)
    rpart = rng.integers(0, 1000, nrb).astype(np.float64)  # integer partials: any summation order is exact
    r1 = 0.0
    for t in imures:
        r1 += t
    res2 = r1 * (COEF * 0.5) + rpart.sum()

    # accept, the gain ratio on both sides of the 1/3 clamp: 1 - (2 rho - 1)^3 = 1 at rho = 0.5, 0.271 at 0.95
    for rho, clamped in ((0.5, False), (0.95, True)):
        s = _state(res1=res2 + 8.0, q1=8.0 / rho, u=0.02, v=8.0, calc_hess=0, iters=3, nhess=2)
        got, xs_d, _ = _control_check(ctx, W, s, imures, rpart, xs, xt, bias, 1, ulp_u=4)
        assert (got["u"] == 0.02 * (1.0 / 3)) == clamped and got["v"] == 2.0 and got["nhess"] == 2
        assert np.array_equal(xs_d, xt) and got["calc_hess"] == 1 and not got["done"]
    # reject twice in a row: v 2 -> 4 -> 8, u x 2 then x 4, the bias records go back to their backups
    s = _state(res1=res2 - 5.0, q1=3.0)
    got, xs_d, bias_d = _control_check(ctx, W, s, imures, rpart, xs, xt, bias, 0)
    assert (got["u"], got["v"], got["calc_hess"], got["nhess"], got["iters"]) == (0.02, 4.0, 0, 1, 1)
    assert np.array_equal(bias_d[:, 0:6], bias[:, 6:12]) and np.array_equal(xs_d, xs)
    got, _, _ = _control_check(ctx, W, got, imures, rpart, xs, xt, bias, 0)
    assert (got["u"], got["v"], got["calc_hess"], got["nhess"], got["iters"]) == (0.08, 8.0, 0, 1, 2)
    # residual1 == residual2: rejected, and the LM ends
    got, _, _ = _control_check(ctx, W, _state(res1=res2), imures, rpart, xs, xt, bias, 0)
    assert got["done"] == 1 and got["fin"] == 1 and got["calc_hess"] == 0
    # an accepted step that ends the LM by |dr / r1| < 1e-6
    s = _state(res1=res2 * (1 + 2.0 ** -21), q1=1.0)
    assert 0 < (s["res1"] - res2) / s["res1"] < 1e-6
    got, xs_d, _ = _control_check(ctx, W, s, imures, rpart, xs, xt, bias, 1, ulp_u=4)
    assert got["done"] == 1 and got["fin"] == 1 and np.array_equal(xs_d, xt)
    # the tenth iteration: fin without done
    got, _, _ = _control_check(ctx, W, _state(res1=res2 + 8.0, q1=16.0, iters=9), imures, rpart, xs, xt, bias, 1,
                               ulp_u=4)
    assert (got["iters"], got["fin"], got["done"]) == (10, 1, 0)
    got, _, _ = _control_check(ctx, W, _state(res1=res2 + 8.0, q1=16.0, iters=8), imures, rpart, xs, xt, bias, 1,
                               ulp_u=4)
    assert (got["iters"], got["fin"]) == (9, 0)
    # already ended: nothing changes
    s = _state(res1=res2 + 8.0, q1=16.0, done=1, fin=1, iters=4, nhess=3, res2=1.5)
    got, xs_d, bias_d = _control_check(ctx, W, s, imures, rpart, xs, xt, bias, -1)
    assert got == s and np.array_equal(xs_d, xs) and np.array_equal(bias_d, bias)


def test_control_rejects_too_many_partials(ctx_for):
    """RESID_BLOCKS is the product's count: one more partial than k_ba_resid's workgroups is refused
    before any launch."""
    ctx = ctx_for(3)
    xs, bias = _states(3, np.random.default_rng(0))
    with pytest.raises(vgpu.VgError):
        ctx.ba_control(3, _state(res1=1.0), np.ones(2), np.ones(RESID_BLOCKS + 1), xs, xs, bias)
