"""The IMU side on the device, alone on given inputs, against tests/imu_ref.py
at 50 digits (written from the reference project's text, pinned by
tests/test_imu_ref.py; nothing of oracle/ or the host code in it).

k_scan_prop (state.hip; vgx_scan_prop), with the mid360 noises from the seed
state of synth.gt_state (imu_cases.prop_cases): 0, 1, 2, 3, 47 and 48 = kPropMax
samples; at 48 five early stamps and a pair straddling last_end (the skip rule
goes by the head stamp); the scan end after and before the last stamp; a pair
with dt = 0; rates 0, 1e-9 (below Exp's 1e-7 switch), 0.3 and 6 rad/s; the seed
covariance and a block-scaled one (blocks 1e-10..1e-2). In every case the
device equals the host's propagate() bit for bit (the claim of state.hip's
header) and x_prop equals x_curr; no sample leaves the block untouched; with
every pair skipped, or one sample, the reference reads uninitialised vectors
(imu_ekf.cpp:91): only device == host and finite there. 49 samples are refused
before any launch.

The IMU workgroups of k_ba_hess, k_ba_resid and k_ba_resid_hess (ba_factor.hip;
vgx_ba_imu) for W in {2, 3, 5, 8, 11} and ring heads {0, 7, 31, 32 - (W-1) + 1}
(the last folds inside the window; at W = 2 it is no slot of the ring):
records of imu_ref.preintegrate and records with a dense SPD cov_inv (diagonal
1e2..1e12), dbg in {0, 1e-12, 1e-2}, dba in {0, 0.1}, rotation residuals 0,
1e-10, 5e-4, 2e-3 (either side of Log's switch), 0.5 and 3.0 rad, xt different
from xs (imu_cases.factor_cases).

Errors per group (R, p, v, the 3 x 3 blocks of cov; the 3 x 3 blocks of jtj)
in units of the group's largest reference entry; e_f64 is the same route in
fp64 numpy. Asserted per class: e_dev / max(e_f64, 2^-53) <= BOUND, the next
power of two above twice the worst ratio measured on an MI355X (beside each
bound; above 64 would be a finding). Asymmetry of cov and jtj counts as an
error of the same group.

The sums gg = joc^T C r and r^T C r (the Hessian workgroups' and the residual
lanes') take a derived bound instead: per entry, the running error bound of
the reference's formulas evaluated in fp64 from the exact inputs
(tests/err_ref.py: u per operation, 4 ulp per library function, n u |A| |B|
per product; the terms it drops are u times itself). On these cases it is
1e-12 to 4e-9 of the group's largest entry; the fp64 route uses a fifth of it
at most (tests/test_imu_ref.py), the device a quarter (0.254 measured). Why not the ratio: it measured 82
on one gg block (W2 head0 k0 at xt, class spd/5e-4: e_dev 2.353e-13, e_f64
2.868e-15). That record's dense cov_inv puts 3.9e11 on one rotation axis and
the entries of res_r are of size 1 whatever the residual, so one rounding
(2^-53) of them moves the block by 6.0e-13 of its largest entry; e_dev is 0.4
such roundings, and the fp64 route's r happened to be 6.6e-19 off on that
axis, 170 times better than one rounding. A yardstick that can be that lucky
bounds nothing there; what the inputs' rounding allows does."""
import numpy as np
import pytest

import err_ref
import imu_cases
import imu_ref
import vgconfig
import vgpu

pytestmark = pytest.mark.gpu
U = imu_cases.U

# class -> bound; measured ratio on an MI355X beside it
PROP_BOUND = {
    "count": 8,  # 2.313
    "skip": 16,  # 6.497
    "endbefore": 8,  # 2.736
    "dtzero": 8,  # 2.646
    "scaled": 8,  # 2.005
    "rate0": 4,  # 1.322
    "rate1e-9": 8,  # 2.26
    "rate6": 8,  # 3.606
}
FACTOR_BOUND = {  # (the 3 x 3 blocks of jtj; gg and r^T C r used at most 0.254 of their derived bound)
    "pre/0": 32,  # 10.76
    "pre/1e-10": 32,  # 13.09
    "pre/5e-4": 16,  # 7.901
    "pre/2e-3": 16,  # 7.283
    "pre/0.5": 32,  # 9.876
    "pre/3.0": 32,  # 10.63
    "spd/0": 16,  # 5.65
    "spd/1e-10": 16,  # 7.545
    "spd/5e-4": 16,  # 4.483
    "spd/2e-3": 16,  # 4.22
    "spd/0.5": 16,  # 5.172
    "spd/3.0": 16,  # 6.405
}
_ctxs = {}


@pytest.fixture(scope="module")
def ctx_for():
    def get(W):
        if W not in _ctxs:
            p = vgconfig.load("mid360")
            p["LocalBA"]["win_size"] = W
            _ctxs[W] = vgpu.Context(vgconfig.to_c(p), max_points=20_000, max_nodes=20_000, max_fix_points=50_000,
                                    hash_log2=14)
        return _ctxs[W]
    yield get
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()


class Worst:
    def __init__(self, classes):
        self.w = {k: (0.0, 0.0, 0.0, "") for k in classes}

    def add(self, cls, ed, ef, what):
        r = ed / max(ef, U)
        if r > self.w[cls][0]:
            self.w[cls] = (r, ed, ef, what)

    def check(self, bound):
        for cls in bound:
            print("RATIO %-10s e_dev %.3e e_f64 %.3e ratio %.4g (%s)" % ((cls,) + self.w[cls][1:3] +
                                                                        (self.w[cls][0], self.w[cls][3])))
        for cls in bound:
            assert self.w[cls][0] <= bound[cls], (cls, self.w[cls])


# ---- k_scan_prop -----------------------------------------------------------------------------------------

def test_scan_prop(ctx_for):
    ctx = ctx_for(11)
    worst = Worst(PROP_BOUND)
    for c in imu_cases.prop_cases():
        xc, xp, host = ctx.scan_prop(c["x"], c["imu"], c["last_end"], c["beg"], c["end"])
        assert np.array_equal(xc.view(np.uint64), host.view(np.uint64)), ("device != host", c["name"])
        assert np.array_equal(xp.view(np.uint64), xc.view(np.uint64)), ("x_prop != x_curr", c["name"])
        assert np.all(np.isfinite(xc)), c["name"]
        assert np.array_equal(xc[15:24], c["x"][15:24]), ("biases / gravity moved", c["name"])
        if len(c["imu"]) == 0:
            assert np.array_equal(xc.view(np.uint64), c["x"].view(np.uint64)), "no sample: the block is untouched"
            continue
        hp, f = imu_cases.ref_prop(c)
        if not hp["defined"]:
            assert np.array_equal(xc[24:], c["x"][24:]), ("no pair ran: the covariance stays", c["name"])
            continue
        cov = xc[24:].reshape(15, 15)
        dev = imu_cases.prop_groups(xc[0:9].reshape(3, 3), xc[9:12], xc[12:15], cov)
        sym = dict(imu_cases.prop_groups(xc[0:9].reshape(3, 3), xc[9:12], xc[12:15], cov.T))
        ref = imu_cases.prop_groups(hp["R"], hp["p"], hp["v"], hp["cov"])
        twin = imu_cases.prop_groups(f["R"], f["p"], f["v"], f["cov"])
        for (name, d), (_, a), (_, b) in zip(dev, ref, twin):
            ed, scale = imu_cases.rel_err(d, a)
            ef, _ = imu_cases.rel_err(b, a)
            if scale == 0.0:
                assert ed == 0.0, (c["name"], name)
                continue
            worst.add(c["cls"], ed, ef, c["name"] + " " + name)
            if name.startswith("cov"):  # symmetry: block (a, b) against block (b, a) transposed
                worst.add(c["cls"], float(np.abs(d - sym[name]).max()) / scale, ef, c["name"] + " " + name + " asym")
    worst.check(PROP_BOUND)


def test_scan_prop_refuses_more_samples_than_its_arrays_hold(ctx_for):
    ctx = ctx_for(11)
    c = imu_cases.prop_cases()[0]
    rng = np.random.default_rng(5)
    for n in (vgpu.PROP_MAX + 1, 1000):
        with pytest.raises(vgpu.VgError, match=r"\(-1\)"):
            ctx.scan_prop(c["x"], imu_cases.samples(rng, n, 0.005, 0.3), 100.0, 100.0, 101.0)
    xc, xp, host = ctx.scan_prop(c["x"], imu_cases.samples(rng, vgpu.PROP_MAX, 0.005, 0.3), 100.0, 100.0, 100.3)
    assert np.array_equal(xc, host)


# ---- the LM's IMU factor blocks --------------------------------------------------------------------------

def _split(row):
    return row[:900].reshape(30, 30), row[900:930].reshape(30, 1), row[930]


@pytest.mark.parametrize("W", imu_cases.WINDOWS)
def test_imu_factor_blocks(ctx_for, W):
    ctx = ctx_for(W)
    worst = Worst(FACTOR_BOUND)
    derived = 0.0
    poison = -7.25e300
    for c in [k for k in imu_cases.factor_cases() if k["W"] == W]:
        n = W - 1
        o = ctx.ba_imu(W, c["head"], c["rec"], c["bias"], c["xs"], c["xt"], poison=poison)
        at_t = ctx.ba_imu(W, c["head"], c["rec"], c["bias"], c["xt"], c["xs"], poison=poison)
        tag = "W%d head%d" % (W, c["head"])
        # rows past W-1 untouched
        for buf in (o["hess"], o["rh_out"], o["resid"], o["rh_res"]):
            assert np.all(buf[n:] == poison), tag
            assert not np.any(buf[:n] == poison), tag
        # (c) equals (b)'s residuals and a k_ba_hess run at xt, bit for bit
        assert np.array_equal(o["rh_res"][:n].view(np.uint64), o["resid"][:n].view(np.uint64)), tag
        assert np.array_equal(o["rh_out"][:n].view(np.uint64), at_t["hess"][:n].view(np.uint64)), tag
        assert not np.array_equal(o["hess"][:n], o["rh_out"][:n]), tag
        for k in range(n):
            for xs, cls, row, rlane in ((c["xs"], c["cls_s"][k], o["hess"][k], None),
                                        (c["xt"], c["cls_t"][k], o["rh_out"][k], o["resid"][k])):
                hp, f = imu_cases.ref_factor(c["rec"][k], c["bias"][k], xs[k], xs[k + 1])
                jtj, gg, res = _split(row)
                dev = imu_cases.factor_groups(jtj, gg, res)
                sym = dict(imu_cases.factor_groups(jtj.T, gg, res))
                ref = imu_cases.factor_groups(hp["jtj"], hp["gg"], hp["res"])
                twin = imu_cases.factor_groups(f["jtj"], f["gg"], f["res"])
                eb = imu_ref.give_evaluate(c["rec"][k], c["bias"][k], xs[k], xs[k + 1], B=err_ref.ERR)
                bgg, bres = eb["gg"].e[:, 0], float(eb["res"].e)
                egg = np.abs(gg[:, 0] - imu_ref.to_np(hp["gg"])[:, 0])
                eres = max(abs(v - float(hp["res"])) for v in ((res,) if rlane is None else (res, rlane)))
                derived = max(derived, float((egg / bgg).max()), eres / bres)
                assert np.all(egg <= bgg), ("%s k%d gg" % (tag, k), cls, float((egg / bgg).max()))
                assert eres <= bres, ("%s k%d res" % (tag, k), cls, eres, bres)  # (b) too: the lanes' r^T C r at xt
                for (name, d), (_, a), (_, b) in zip(dev, ref, twin):
                    if not name.startswith("jtj"):
                        continue
                    ed, scale = imu_cases.rel_err(d, a)
                    ef, _ = imu_cases.rel_err(b, a)
                    what = "%s k%d %s" % (tag, k, name)
                    if scale == 0.0:
                        assert ed == 0.0, what
                        continue
                    worst.add(cls, ed, ef, what)
                    worst.add(cls, float(np.abs(d - sym[name]).max()) / scale, ef, what + " asym")
    print("DERIVED W%d: gg / r^T C r use at most %.3g of their bound" % (W, derived))
    worst.check({k: v for k, v in FACTOR_BOUND.items() if worst.w[k][3]})  # (the classes this W's factors drew)


def test_jacobian_zero_pattern(ctx_for):
    """cov_inv = e_q e_q^T selects row q of joc: jtj = joc[q]^T joc[q], so jtj[c, c] = joc[q, c]^2 and
    jtj[c0, c] / sqrt(jtj[c0, c0]) reads the row back with its signs. The entries the reference leaves 0 are
    0 exactly; the others are the reference's within 1e-12 of the row's largest. cov_inv = I: the 3 x 3 blocks
    of jtj whose column blocks share no row block of joc are 0 exactly."""
    ctx = ctx_for(2)
    c = [k for k in imu_cases.factor_cases() if k["W"] == 2 and k["head"] == 7][0]
    for kind in (0, 3):
        rec = imu_cases.record_pool()["pre"][kind].copy()
        bias = c["bias"].copy()
        bias[0, 0:3] = [6e-3, -5e-3, 4e-3]
        bias[0, 3:6] = [0.05, 0.02, -0.07]
        joc = imu_ref.to_np(imu_ref.give_evaluate(rec, bias[0], c["xs"][0], c["xs"][1])["joc"])
        for q in range(15):
            r = rec.copy()
            r[64:] = 0.0
            r[64 + 16 * q] = 1.0
            o = ctx.ba_imu(2, 7, r[None, :], bias, c["xs"], c["xt"])
            jtj = o["hess"][0][:900].reshape(30, 30)
            d = np.diag(jtj)
            assert np.array_equal(d == 0.0, joc[q] == 0.0), (kind, q, np.flatnonzero((d == 0.0) != (joc[q] == 0.0)))
            c0 = int(np.argmax(np.abs(joc[q])))
            row = jtj[c0] / np.sqrt(d[c0]) * np.sign(joc[q, c0])
            assert np.abs(row - joc[q]).max() <= 1e-12 * np.abs(joc[q]).max(), (kind, q)
        r = rec.copy()
        r[64:] = np.eye(15).reshape(-1)
        jtj = ctx.ba_imu(2, 7, r[None, :], bias, c["xs"], c["xt"])["hess"][0][:900].reshape(30, 30)
        nz = np.array([[np.any(joc[3 * a:3 * a + 3, 3 * b:3 * b + 3] != 0.0) for b in range(10)] for a in range(5)])
        share = (nz.T.astype(int) @ nz.astype(int)) > 0
        assert not share.all() and share.sum() > 20
        for a in range(10):
            for b in range(10):
                blk = jtj[3 * a:3 * a + 3, 3 * b:3 * b + 3]
                assert share[a, b] or np.all(blk == 0.0), (kind, a, b)
                assert not share[a, b] or np.any(blk != 0.0), (kind, a, b)


def test_ba_imu_refuses_a_head_outside_the_ring(ctx_for):
    ctx = ctx_for(2)
    c = [k for k in imu_cases.factor_cases() if k["W"] == 2][0]
    for head in (-1, imu_cases.MAX_WIN):
        with pytest.raises(vgpu.VgError, match=r"\(-1\)"):
            ctx.ba_imu(2, head, c["rec"], c["bias"], c["xs"], c["xt"])
