"""tests/imu_ref.py pinned by answers that do not come from this project:
closed forms, the dense transition product, central differences at 50 digits
(step 1e-20: truncation ~1e-40 of the third derivative, far below the 1e-30
asked for), the merge identity of the preintegrated deltas; and the fp64 twin
against the 50-digit route on every case the GPU tests and the record test use
(1e-9 of each group's largest entry: the cap that keeps their ratio bounds
meaningful). CPU only."""
import mpmath as mp
import numpy as np
import pytest

import err_ref
import hp_ref
import imu_cases
import imu_ref
from imu_ref import HP

mp.mp.dps = 50
H = mp.mpf(10) ** -20
TOL = mp.mpf(10) ** -30


def _maxabs(m):
    return max(abs(m[i, j]) for i in range(m.rows) for j in range(m.cols))


def _near(a, b, tol=TOL):
    scale = max(_maxabs(b), mp.mpf(1))
    assert _maxabs(a - b) <= tol * scale, float(_maxabs(a - b) / scale)


def _true_exp(v):
    """The exact exponential of hat(v) (no small-angle branch)."""
    n = hp_ref.norm(v)
    K = hp_ref.hat(v / n)
    return mp.eye(3) + mp.sin(n) * K + (1 - mp.cos(n)) * K * K


# ---- propagate -------------------------------------------------------------------------------------------

def _const_case(n=9, dt=0.0078125):  # dt = 2^-7: the stamps are exact
    w, a = np.array([0.3, -0.2, 0.5]), np.array([0.4, 0.1, 9.9])
    imu = np.zeros((n, 7))
    imu[:, 0] = 100.0 + dt * np.arange(n)
    imu[:, 1:4], imu[:, 4:7] = w, a
    x = np.r_[np.eye(3).ravel(), [1, 2, 3], [0.5, -0.5, 0.1], np.zeros(6), [0, 0, -9.8]]
    return x, imu, w, a, dt


def test_propagate_constant_rate_closed_form():
    x, imu, w, a, dt = _const_case()
    end = imu[-1, 0] + 0.00390625
    o = imu_ref.propagate(x, np.eye(15) * 1e-4, imu, 100.0, end, 1.0, (0, 0, 0, 0))
    T = mp.mpf(end) - 100
    _near(o["R"], _true_exp(hp_ref.M(w) * T))  # R = Exp(w T) for a constant body rate
    # v and p against the same recursion written out with the closed-form R_k = Exp(w k dt)
    g, v, p = hp_ref.M([0, 0, -9.8]), hp_ref.M(x[12:15]), hp_ref.M(x[9:12])
    h = mp.mpf(dt)
    for k in range(len(imu) - 1):
        acc = _true_exp(hp_ref.M(w) * (k * h)) * hp_ref.M(a) + g if k else hp_ref.M(a) + g
        p, v = p + v * h + acc * h * h / 2, v + acc * h
    tail = mp.mpf(0.00390625)
    _near(o["v"], v + acc * tail)
    _near(o["p"], p + v * tail + acc * tail * tail / 2)
    assert o["steps"] == len(imu) - 1 and o["defined"]


def test_propagate_end_before_last_sample():
    """note = -1 (line 89): dt = note (end - imu_end) is positive and note dt the signed step."""
    x, imu, w, a, dt = _const_case()
    back = mp.mpf(0.00390625)
    o = imu_ref.propagate(x, np.eye(15), imu, 100.0, imu[-1, 0] - 0.00390625, 1.0, (0, 0, 0, 0))
    full = imu_ref.propagate(x, np.eye(15), imu, 100.0, imu[-1, 0], 1.0, (0, 0, 0, 0))  # end == imu_end: dt = 0
    _near(o["R"], full["R"] * _true_exp(hp_ref.M(w) * -back))
    _near(full["R"], _true_exp(hp_ref.M(w) * (mp.mpf(imu[-1, 0]) - 100)))


def test_propagate_covariance_is_the_dense_transition_product():
    rng = np.random.default_rng(1)
    case = [c for c in imu_cases.prop_cases() if c["name"] == "n3"][0]
    A = rng.normal(size=(15, 15))
    cov = A @ A.T
    o = imu_ref.propagate(case["x"][:24], cov, case["imu"], case["last_end"], case["end"], 1.0, (0, 0, 0, 0))
    _near(o["cov"], o["Phi"] * hp_ref.M(cov) * o["Phi"].T)
    n = imu_ref.propagate(case["x"][:24], cov, case["imu"], case["last_end"], case["end"], 1.0, imu_cases.mid360()["odo"])
    _near(n["cov"], n["cov"].T)
    d = n["cov"] - o["cov"]  # the noise's contribution is positive semi-definite and symmetric
    _near(d, d.T)
    assert min(mp.eigsy((d + d.T) / 2, eigvals_only=True)) > -TOL


def test_propagate_skip_rule_and_degenerate_lists():
    c = {k["name"]: k for k in imu_cases.prop_cases()}
    s = c["skip48"]
    o = imu_ref.propagate(s["x"][:24], s["x"][24:], s["imu"], s["last_end"], s["end"], 1.0, (0, 0, 0, 0))
    assert o["steps"] == 41  # pairs with heads 0..5 skipped: the straddling pair goes by its head stamp
    late = imu_ref.propagate(s["x"][:24], s["x"][24:], s["imu"][6:], s["last_end"], s["end"], 1.0, (0, 0, 0, 0))
    _near(o["cov"], late["cov"])
    _near(o["p"], late["p"])
    for name in ("allskip3", "n1"):
        k = c[name]
        u = imu_ref.propagate(k["x"][:24], k["x"][24:], k["imu"], k["last_end"], k["end"], 1.0, (0, 0, 0, 0))
        assert not u["defined"] and u["R"] is None and u["steps"] == 0
        assert hp_ref.err(k["x"][24:], u["cov"]) == 0.0
    k = c["n0"]
    u = imu_ref.propagate(k["x"][:24], k["x"][24:], k["imu"], k["last_end"], k["end"], 1.0, (1, 1, 1, 1))
    assert u["defined"] and hp_ref.err(k["x"][:9], u["R"]) == 0.0 and hp_ref.err(k["x"][24:], u["cov"]) == 0.0


# ---- preintegrate ----------------------------------------------------------------------------------------

def _pre_inputs():
    rng = np.random.default_rng(2)
    imu = imu_cases.samples(rng, 9, 0.0078125, 0.8)
    return np.array([0.01, -0.02, 0.005]), np.array([0.05, 0.02, -0.03]), imu


def test_bias_jacobians_against_central_differences():
    bg, ba, imu = _pre_inputs()
    Z = np.zeros((6, 6))

    def run(dbg, dba):
        return imu_ref.integrate(hp_ref.M(bg) + dbg, hp_ref.M(ba) + dba, imu, 1.0, Z, Z)

    s0 = imu_ref.integrate(bg, ba, imu, 1.0, Z, Z)
    zero = mp.zeros(3, 1)
    for j in range(3):
        e = mp.zeros(3, 1)
        e[j] = H
        pg, mg = run(e, zero), run(-e, zero)
        pa, ma = run(zero, e), run(zero, -e)
        # R_delta(bg + d) = R_delta Exp(R_bg d): column j of R_bg is the vee of R^T dR / d bg_j
        S = s0["R_delta"].T * (pg["R_delta"] - mg["R_delta"]) / (2 * H)
        _near(mp.matrix([S[2, 1], S[0, 2], S[1, 0]]), s0["R_bg"][:, j])
        _near((pg["p_delta"] - mg["p_delta"]) / (2 * H), s0["p_bg"][:, j])
        _near((pg["v_delta"] - mg["v_delta"]) / (2 * H), s0["v_bg"][:, j])
        _near((pa["p_delta"] - ma["p_delta"]) / (2 * H), s0["p_ba"][:, j])
        _near((pa["v_delta"] - ma["v_delta"]) / (2 * H), s0["v_ba"][:, j])
        _near(pa["R_delta"], s0["R_delta"])  # no dependence on ba


def test_split_and_merge_gives_the_whole_list():
    bg, ba, imu = _pre_inputs()
    Z = np.zeros((6, 6))
    whole = imu_ref.integrate(bg, ba, imu, 1.0, Z, Z)
    for cut in (1, 4, 7):
        a, b = imu_ref.integrate(bg, ba, imu[:cut + 1], 1.0, Z, Z), imu_ref.integrate(bg, ba, imu[cut:], 1.0, Z, Z)
        m = imu_ref.merge_deltas(a, b)
        for k in ("R_delta", "p_delta", "v_delta"):
            _near(m[k], whole[k])
        assert abs(m["dtime"] - whole["dtime"]) < TOL


def test_record_layout_and_inverse():
    bg, ba, imu = _pre_inputs()
    nz = imu_cases.mid360()
    s = imu_ref.integrate(bg, ba, imu, 1.0, nz["meas"], nz["walk"])
    rec = imu_ref.record(s)
    assert len(rec) == 289 and rec[61] == rec[62] == rec[63] == 0 and rec[60] == s["dtime"]
    assert rec[9 + 1] == s["p_delta"][1] and rec[15 + 3 * 1 + 2] == s["R_bg"][1, 2] and rec[51 + 8] == s["v_ba"][2, 2]
    C = mp.matrix(15, 15)
    for i in range(15):
        for j in range(15):
            C[i, j] = rec[64 + 15 * i + j]
    _near(C * s["cov"], mp.eye(15), mp.mpf(10) ** -25)
    _near(s["cov"], s["cov"].T)


# ---- give_evaluate ---------------------------------------------------------------------------------------

def _orth(R):
    """Gram-Schmidt on the rows."""
    a = [R[i, :] for i in range(3)]
    a[0] = a[0] / mp.sqrt((a[0] * a[0].T)[0])
    a[1] = a[1] - (a[1] * a[0].T)[0] * a[0]
    a[1] = a[1] / mp.sqrt((a[1] * a[1].T)[0])
    a[2] = a[2] - (a[2] * a[0].T)[0] * a[0] - (a[2] * a[1].T)[0] * a[1]
    a[2] = a[2] / mp.sqrt((a[2] * a[2].T)[0])
    return mp.matrix([[a[i][j] for j in range(3)] for i in range(3)])


def _retract(st, d, o):
    """The window's retraction on block o of a frame: R Exp(d) for the rotation, additive for the rest."""
    R, p, v, bg, ba, g = st
    if o == 0:
        return (R * _true_exp(d), p, v, bg, ba, g)
    parts = [R, p, v, bg, ba, g]
    parts[o] = parts[o] + d
    return tuple(parts)


@pytest.mark.parametrize("which", [("pre/0.5", 1e-2), ("spd/3.0", 1e-2), ("pre/5e-4", 1e-2), ("spd/2e-3", 1e-2)])
def test_jacobian_against_central_differences(which):
    cls, dbg_size = which
    found = None
    for c in imu_cases.factor_cases():
        for k, name in enumerate(c["cls_s"]):
            if name == cls and abs(np.linalg.norm(c["bias"][k, :3]) - dbg_size) < 1e-12:
                found = (c["rec"][k], c["bias"][k], c["xs"][k], c["xs"][k + 1])
    assert found, which
    rec, bias, x1, x2 = found
    r = imu_ref._rec_dict(HP, rec)
    dbg, dba = hp_ref.M(bias[0:3]), hp_ref.M(bias[3:6])
    st1, st2 = imu_ref._frame(HP, x1), imu_ref._frame(HP, x2)
    # the Jacobian's identities hold for rotations: the fp64 matrices are orthogonal to 1e-16 only, so they
    # are made orthogonal to 50 digits first (this is a test of the formulas, on whatever inputs)
    r["R_delta"] = _orth(r["R_delta"])
    st1, st2 = (_orth(st1[0]),) + st1[1:], (_orth(st2[0]),) + st2[1:]
    ev = imu_ref.evaluate(r, dbg, dba, st1, st2)
    J = ev["joc"]
    # (dbg = 1e-2 in every case: at dbg = 0 the reference's Exp(R_bg dbg) returns I for any |R_bg dbg| < 1e-9,
    # so a difference quotient of its own residual in dbg would read 0 there)
    for blk in range(10):
        first, o = blk < 5, blk % 5
        for j in range(3):
            d = mp.zeros(3, 1)
            d[j] = H
            if first and o == 3:  # column block 9: dbg += d (the bias record), and bg1 moves the bias residual
                rp = imu_ref.residual(r, dbg + d, dba, _retract(st1, d, 3), st2)[0]
                rm = imu_ref.residual(r, dbg - d, dba, _retract(st1, -d, 3), st2)[0]
            elif first and o == 4:
                rp = imu_ref.residual(r, dbg, dba + d, _retract(st1, d, 4), st2)[0]
                rm = imu_ref.residual(r, dbg, dba - d, _retract(st1, -d, 4), st2)[0]
            elif first:
                rp = imu_ref.residual(r, dbg, dba, _retract(st1, d, o), st2)[0]
                rm = imu_ref.residual(r, dbg, dba, _retract(st1, -d, o), st2)[0]
            else:
                rp = imu_ref.residual(r, dbg, dba, st1, _retract(st2, d, o))[0]
                rm = imu_ref.residual(r, dbg, dba, st1, _retract(st2, -d, o))[0]
            num = (rp - rm) / (2 * H)
            col = J[:, 3 * blk + j]
            scale = max(_maxabs(col), mp.mpf(1))
            # rows 3.. are exact derivatives; the rotation rows are exact where Log is the true logarithm
            assert _maxabs(num[3:15, 0] - col[3:15, 0]) <= TOL * scale, (which, blk, j)
            assert _maxabs(num[0:3, 0] - col[0:3, 0]) <= mp.mpf(ROT_TOL[cls]) * scale, (
                which, blk, j, float(_maxabs(num[0:3, 0] - col[0:3, 0]) / scale))
    C = r["cov_inv"]
    _near(ev["gg"], J.T * C * ev["rr"])
    _near(ev["jtj"], ev["jtj"].T, mp.mpf(10) ** -40)
    assert abs(ev["res"] - (ev["rr"].T * C * ev["rr"])[0, 0]) <= TOL * abs(ev["res"])


# how far the reference's rotation Jacobian may stand from the derivative of its own residual. Above the 1e-3
# switch Log is the true logarithm and jr_inv, jr are its exact Jacobians; below it Log returns the vee part,
# sin(theta) / theta short of the logarithm: theta^2 / 6 = 4e-8 at 5e-4.
ROT_TOL = {"pre/0.5": 1e-25, "spd/3.0": 1e-25, "pre/5e-4": 1e-6, "spd/2e-3": 1e-25}


# ---- the fp64 twin on the tests' cases -------------------------------------------------------------------

CAP = 1e-9


def test_twin_on_propagation_cases():
    for c in imu_cases.prop_cases():
        hp, f = imu_cases.ref_prop(c)
        assert hp["defined"] == f["defined"] == (c["cls"] != "undefined" and c["name"] != "n1"), c["name"]
        if not hp["defined"]:
            continue
        for (name, a), (_, b) in zip(imu_cases.prop_groups(hp["R"], hp["p"], hp["v"], hp["cov"]),
                                     imu_cases.prop_groups(f["R"], f["p"], f["v"], f["cov"])):
            e, scale = imu_cases.rel_err(b, a)
            assert e <= CAP, (c["name"], name, e)


def test_twin_on_factor_cases():
    for c in imu_cases.factor_cases():
        for xs, cls in ((c["xs"], c["cls_s"]), (c["xt"], c["cls_t"])):
            for k in range(c["W"] - 1):
                hp, f = imu_cases.ref_factor(c["rec"][k], c["bias"][k], xs[k], xs[k + 1])
                lg = hp_ref.norm(hp["rr"][0:3, 0])
                assert lg <= 3.0 + 1e-6, (cls[k], float(lg))
                for (name, a), (_, b) in zip(imu_cases.factor_groups(hp["jtj"], hp["gg"], hp["res"]),
                                             imu_cases.factor_groups(f["jtj"], f["gg"], f["res"])):
                    e, scale = imu_cases.rel_err(b, a)
                    assert e <= CAP, (c["W"], c["head"], k, cls[k], name, e)


def test_derived_bound_holds_for_the_fp64_route():
    """tests/err_ref.py carries f64_ref's values, and on every factor case the fp64 route's gg and r^T C r
    stand within a fifth of the bound the device test allows (the running bound); the bound itself is
    below 1e-8 of each gg block's largest entry, so it still separates a rounding from a mistake."""
    err_ref.self_check()
    for c in imu_cases.factor_cases():
        for xs in (c["xs"], c["xt"]):
            for k in range(c["W"] - 1):
                hp, f = imu_cases.ref_factor(c["rec"][k], c["bias"][k], xs[k], xs[k + 1])
                e = imu_ref.give_evaluate(c["rec"][k], c["bias"][k], xs[k], xs[k + 1], B=err_ref.ERR)
                assert np.array_equal(e["gg"].v, imu_ref.to_np(f["gg"])) or np.allclose(
                    e["gg"].v, imu_ref.to_np(f["gg"]), rtol=1e-9, atol=0)
                ref = imu_ref.to_np(hp["gg"])[:, 0]
                bound = e["gg"].e[:, 0]
                assert np.all(np.abs(imu_ref.to_np(f["gg"])[:, 0] - ref) <= 0.2 * bound), (c["W"], c["head"], k)
                assert abs(float(f["res"]) - float(hp["res"])) <= 0.2 * float(e["res"].e)
                for a in range(10):
                    assert bound[3 * a:3 * a + 3].max() <= 1e-8 * np.abs(ref[3 * a:3 * a + 3]).max(), (c["W"], k, a)
                assert float(e["res"].e) <= 1e-8 * float(hp["res"])


def test_twin_on_record_cases():
    for c in imu_cases.record_cases():
        hp, f = imu_cases.ref_record(c)
        for (name, a), (_, b) in zip(imu_cases.record_groups(hp), imu_cases.record_groups(f)):
            e, scale = imu_cases.rel_err(b, a)
            assert e <= CAP, (c["name"], name, e)
