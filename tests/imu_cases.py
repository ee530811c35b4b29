"""Inputs of the IMU tests (seeded), shared by tests/test_imu_ref.py (the fp64
twin's agreement with the 50-digit route on exactly these cases),
tests/test_imu_record.py and tests/test_imu_gpu.py. References are computed
once per process (ref_*) and handed out unchanged."""
import itertools

import mpmath as mp
import numpy as np

import f64_ref
import hp_ref
import imu_ref
import la_cases
import synth
import vgconfig

U = 2.0 ** -53
MAX_WIN = 32  # the device's IMU record ring (kMaxWin)
T0 = 100.0    # stamps near 100 s: differences of 5 ms carry 2^-46 s of rounding, as a real drive's do


def mid360():
    p = vgconfig.load("mid360")
    o, b = p["Odometry"], p["LocalBA"]
    return {"odo": (o["cov_gyr"], o["cov_acc"], o["rdw_gyr"], o["rdw_acc"]),
            "meas": imu_ref.noise6(b["cov_gyr"], b["cov_acc"]), "walk": imu_ref.noise6(b["rdw_gyr"], b["rdw_acc"])}


def _unit(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def samples(rng, n, dt, rate, R0=np.eye(3), t0=T0, noisy=True):
    """n samples dt apart: gyro `rate` rad/s about one axis, the accelerometer reading of a body at rest in R0
    plus 0.5 m/s^2 of motion; with `noisy` both carry sample noise (off: the gyro is exactly constant)."""
    ax = _unit(rng)
    imu = np.zeros((n, 7))
    imu[:, 0] = t0 + dt * np.arange(n)
    imu[:, 1:4] = rate * ax
    imu[:, 4:7] = R0.T @ np.array([0.0, 0.0, 9.8]) + rng.normal(0, 0.5, 3)
    if noisy:
        imu[:, 1:4] += rng.normal(0, 0.01, (n, 3))
        imu[:, 4:7] += rng.normal(0, 0.05, (n, 3))
    return imu


# ---- propagation -----------------------------------------------------------------------------------------

def prop_cases():
    """-> list of dicts: name, cls (the bound's class), x (249), imu (n, 7), last_end, beg, end."""
    rng = np.random.default_rng(31)
    x0 = synth.Sequence("tiny", seq_id=1, blind=0.5).gt_state(3)[1:].copy()
    x0[15:18] = [1e-3, -2e-3, 5e-4]  # bg
    x0[18:21] = [0.02, -0.01, 0.03]  # ba
    R0 = x0[:9].reshape(3, 3)
    scaled = la_cases.block_scaled(rng, 15, 1e-5, 1e-1)
    out = []

    def add(name, cls, imu, last_end=T0, end_off=0.002, cov=None, x=None):
        x = (x0 if x is None else x).copy()
        if cov is not None:
            x[24:] = cov.reshape(-1)
        end = (imu[-1, 0] if len(imu) else T0) + end_off
        out.append({"name": name, "cls": cls, "x": x, "imu": imu, "last_end": last_end, "beg": T0, "end": end})

    for n in (0, 1, 2, 3, 47, 48):
        add("n%d" % n, "count", samples(rng, n, 0.005, 0.3, R0))
    skip = samples(rng, 48, 0.005, 0.3, R0)  # stamps 0..4 early, the pair (5, 6) straddles last_end
    add("skip48", "skip", skip, last_end=skip[5, 0] + 0.002)
    add("skip48/scaled", "skip", skip, last_end=skip[5, 0] + 0.002, cov=scaled)
    add("allskip3", "undefined", samples(rng, 3, 0.005, 0.3, R0), last_end=T0 + 1.0)
    for n in (3, 48):
        add("endbefore%d" % n, "endbefore", samples(rng, n, 0.005, 0.3, R0), end_off=-0.002)
        z = samples(rng, n, 0.005, 0.3, R0)
        z[n // 2:, 0] = z[n // 2 - 1:-1, 0].copy()  # stamps n/2 - 1 and n/2 coincide: a pair with dt = 0
        add("dtzero%d" % n, "dtzero", z)
        add("scaled%d" % n, "scaled", samples(rng, n, 0.005, 0.3, R0), cov=scaled)
    xz = x0.copy()
    xz[15:18] = 0.0  # no gyro bias: the averaged rate is the samples' exactly
    for rate, tag in ((0.0, "0"), (1e-9, "1e-9"), (6.0, "6")):
        add("rate" + tag, "rate" + tag, samples(rng, 12, 0.005, rate, R0, noisy=rate > 1.0), x=xz)
    return out


PROP_CLASSES = ("count", "skip", "endbefore", "dtzero", "scaled", "rate0", "rate1e-9", "rate6")
_prop_ref = {}


def ref_prop(case):
    """(50-digit result, fp64 twin's) of a propagation case."""
    if case["name"] not in _prop_ref:
        noises = mid360()["odo"]
        a = (case["x"][:24], case["x"][24:], case["imu"], case["last_end"], case["end"], 1.0, noises)
        _prop_ref[case["name"]] = (imu_ref.propagate(*a), imu_ref.propagate(*a, B=imu_ref.F64))
    return _prop_ref[case["name"]]


def prop_groups(R, p, v, cov):
    """[(name, values)] of a propagation result (either arithmetic, or numpy)."""
    g = [("R", R), ("p", p), ("v", v)]
    g += [("cov%d%d" % (a, b), cov[3 * a:3 * a + 3, 3 * b:3 * b + 3]) for a in range(5) for b in range(5)]
    return g


# ---- factors ---------------------------------------------------------------------------------------------

THETAS = ((0.0, "0"), (1e-10, "1e-10"), (5e-4, "5e-4"), (2e-3, "2e-3"), (0.5, "0.5"), (3.0, "3.0"))
DBG, DBA = (0.0, 1e-12, 1e-2), (0.0, 0.1)
WINDOWS = (2, 3, 5, 8, 11)
FACTOR_CLASSES = tuple(k + "/" + t for k in ("pre", "spd") for _, t in THETAS)
_pool = {}


def heads(W):
    """0, 7, the last slot, and the head whose window folds the ring at its second record (W = 2 has one
    record and that head would be MAX_WIN itself, outside the ring: three heads there)."""
    return tuple(h for h in (0, 7, MAX_WIN - 1, MAX_WIN - (W - 1) + 1) if h < MAX_WIN)


def record_pool():
    """Six records of imu_ref.preintegrate (10..20 samples, the mid360 noises, rounded to fp64), and each
    one again with a dense SPD cov_inv D A D, A well conditioned, D^2 log-spaced 1e2..1e12 in shuffled order."""
    if not _pool:
        rng = np.random.default_rng(32)
        nz = mid360()
        pre, spd = [], []
        for n in (10, 12, 14, 16, 18, 20):
            imu = samples(rng, n, 0.005, 0.3 + 0.2 * rng.random())
            r = imu_ref.rec_np(imu_ref.preintegrate(rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3), imu, 1.0,
                                                    nz["meas"], nz["walk"]))
            pre.append(r)
            Mx = rng.normal(size=(15, 15))
            A = Mx @ Mx.T / 15 + np.eye(15)
            d = rng.permutation(10.0 ** np.linspace(1, 6, 15))
            C = (A * d[:, None]) * d[None, :]
            s = r.copy()
            s[64:] = (0.5 * (C + C.T)).reshape(-1)
            spd.append(s)
        _pool["pre"], _pool["spd"] = pre, spd
    return _pool


def _window(rng, W, recs, bias, thetas):
    """W frame states whose factor k has a rotation residual of thetas[k] rad about a random axis and
    translation / velocity residuals of a few cm (fp64 construction: test input only)."""
    xs = np.zeros((W, 24))
    R, p, v = la_cases.rodrigues(rng.normal(0, 0.5, 3)), rng.normal(0, 2, 3), rng.normal(0, 1, 3)
    for k in range(W):
        bg, ba, g = rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3), np.array([0, 0, -9.8]) + rng.normal(0, 0.01, 3)
        xs[k] = np.r_[R.ravel(), p, v, bg, ba, g]
        if k == W - 1:
            break
        r = recs[k]
        Rd, pd, vd, Rbg, dt = r[0:9].reshape(3, 3), r[9:12], r[12:15], r[15:24].reshape(3, 3), r[60]
        Rc = Rd @ f64_ref.Exp(Rbg @ bias[k, :3])
        p, v = (p + v * dt + 0.5 * g * dt * dt + R @ (pd + rng.normal(0, 0.05, 3)),
                v + g * dt + R @ (vd + rng.normal(0, 0.05, 3)))
        R = R @ Rc @ la_cases.rodrigues(thetas[k] * _unit(rng))
    return xs


def factor_cases():
    """-> list of dicts, one per (W, head): W, head, rec (W-1, 289), bias (W-1, 12), xs, xt (W, 24), cls_s and
    cls_t (per factor: its class at xs and at xt). The 72 combinations of record kind, rotation residual, dbg
    and dba are dealt to the factors in a fixed shuffled order; at xt every factor has the next residual of
    THETAS, so the two passes never agree."""
    rng = np.random.default_rng(33)
    pool = record_pool()
    combos = list(itertools.product(("pre", "spd"), range(len(THETAS)), DBG, DBA))
    order = rng.permutation(len(combos))
    out, c = [], 0
    for W in WINDOWS:
        for head in heads(W):
            rec, bias, th_s, th_t, cls_s, cls_t = [], np.zeros((W - 1, 12)), [], [], [], []
            for k in range(W - 1):
                kind, ti, dbg, dba = combos[order[c % len(combos)]]
                c += 1
                rec.append(pool[kind][rng.integers(6)])
                bias[k, 0:3] = dbg * _unit(rng)
                bias[k, 3:6] = dba * _unit(rng)
                bias[k, 6:12] = rng.normal(size=6)  # the backups: never read by the passes
                tj = (ti + 1) % len(THETAS)
                th_s.append(THETAS[ti][0])
                th_t.append(THETAS[tj][0])
                cls_s.append(kind + "/" + THETAS[ti][1])
                cls_t.append(kind + "/" + THETAS[tj][1])
            rec = np.array(rec)
            out.append({"W": W, "head": head, "rec": rec, "bias": bias, "xs": _window(rng, W, rec, bias, th_s),
                        "xt": _window(rng, W, rec, bias, th_t), "cls_s": cls_s, "cls_t": cls_t})
    return out


_fac_ref = {}


def ref_factor(rec, bias, x1, x2):
    """(50-digit give_evaluate, fp64 twin's) of one factor."""
    key = (rec.tobytes(), bias[:6].tobytes(), x1.tobytes(), x2.tobytes())
    if key not in _fac_ref:
        _fac_ref[key] = (imu_ref.give_evaluate(rec, bias, x1, x2), imu_ref.give_evaluate(rec, bias, x1, x2, B=imu_ref.F64))
    return _fac_ref[key]


def factor_groups(jtj, gg, res):
    """[(name, values)]: the 3 x 3 blocks of jtj, the 3-vectors of gg and r^T C r."""
    g = [("jtj%d,%d" % (a, b), jtj[3 * a:3 * a + 3, 3 * b:3 * b + 3]) for a in range(10) for b in range(10)]
    g += [("gg%d" % a, gg[3 * a:3 * a + 3, 0:1]) for a in range(10)]
    return g + [("res", [res])]


# ---- the record ------------------------------------------------------------------------------------------

NOISE_SCALED = ((1e2, 1e-2), (1e-12, 1e-6))  # (meas gyr, acc), (walk gyr, acc): cov's diagonal blocks span 12 decades


def record_cases():
    """-> list of dicts: name, cls, bg, ba, imu, meas, walk (6 x 6). 2 and 11 samples in every combination of
    dt, gyro rate and noises; 48 samples on four of them (not 0.1 s steps with the scaled noises: over 4.7 s the
    fp64 twin's own inverse is off by 1.1e-9 of a block, past the 1e-9 cap of tests/test_imu_ref.py)."""
    rng = np.random.default_rng(34)
    nz = mid360()
    noises = {"mid360": (nz["meas"], nz["walk"]),
              "scaled": (imu_ref.noise6(*NOISE_SCALED[0]), imu_ref.noise6(*NOISE_SCALED[1]))}
    combos = list(itertools.product((2, 11), (0.005, 0.1), (0.0, 1e-9, 3.0), ("mid360", "scaled")))
    combos += [(48, 0.005, 3.0, "mid360"), (48, 0.005, 3.0, "scaled"), (48, 0.1, 0.0, "mid360"), (48, 0.1, 1e-9, "mid360")]
    out = []
    for n, dt, rate, nk in combos:
        exact = rate < 1.0  # rate 0 / 1e-9: no gyro bias and no sample noise, so Exp and jr take their identity branches
        out.append({"name": "n%d/dt%g/w%g/%s" % (n, dt, rate, nk), "cls": nk + ("/n2" if n == 2 else ""),
                    "bg": np.zeros(3) if exact else rng.normal(0, 1e-3, 3), "ba": rng.normal(0, 1e-2, 3),
                    "imu": samples(rng, n, dt, rate, noisy=not exact), "meas": noises[nk][0], "walk": noises[nk][1]})
    return out


RECORD_CLASSES = ("mid360", "scaled", "mid360/n2", "scaled/n2")
_rec_ref = {}


def ref_record(case):
    """(50-digit record as a list of mpf, fp64 twin's as numpy). With 2 samples cov is singular in exact
    arithmetic (one step: the position rows of its noise Jacobian are dt / 2 times the velocity rows): the
    cov_inv part of both is None."""
    if case["name"] not in _rec_ref:
        a = (case["bg"], case["ba"], case["imu"], 1.0, case["meas"], case["walk"])
        if len(case["imu"]) == 2:
            s, f = imu_ref.integrate(*a), imu_ref.integrate(*a, B=imu_ref.F64)
            try:
                mp.inverse(s["cov"])
                raise AssertionError("a one-step covariance has rank 6")
            except ZeroDivisionError:
                pass
            s["cov"], f["cov"] = mp.eye(15), np.eye(15)
            hp, fl = imu_ref.record(s), imu_ref.rec_np(imu_ref.record(f, imu_ref.F64))
            hp[64:], fl = [None] * 225, fl[:64]
        else:
            hp, fl = imu_ref.preintegrate(*a), imu_ref.rec_np(imu_ref.preintegrate(*a, B=imu_ref.F64))
        _rec_ref[case["name"]] = (hp, fl)
    return _rec_ref[case["name"]]


def record_groups(rec):
    """[(name, list of values)] of a record (list of mpf or numpy): each delta and Jacobian block, dtime, and
    the 3 x 3 blocks of cov_inv when it is there."""
    g = [(name, list(rec[o:o + n])) for name, o, n in imu_ref.REC_FIELDS] + [("dtime", [rec[60]])]
    if len(rec) > 64 and rec[64] is not None:
        g += [("cinv%d%d" % (a, b), [rec[64 + (3 * a + i) * 15 + 3 * b + j] for i in range(3) for j in range(3)])
              for a in range(5) for b in range(5)]
    return g


# ---- errors ----------------------------------------------------------------------------------------------

def _flat(v):
    if isinstance(v, mp.matrix):
        return [v[i, j] for i in range(v.rows) for j in range(v.cols)]
    if isinstance(v, (list, tuple)):
        return list(v)
    return list(np.asarray(v, dtype=np.float64).reshape(-1))


def rel_err(val, ref):
    """(largest |val - ref| over the group in units of the group's largest |ref|, that scale); a zero group
    gives (inf or 0, 0): the caller asserts exact zeros there."""
    r = [x if isinstance(x, mp.mpf) else mp.mpf(float(x)) for x in _flat(ref)]
    d = [mp.mpf(float(x)) for x in _flat(val)]
    assert len(r) == len(d), (len(r), len(d))
    scale = max(abs(x) for x in r)
    e = max(abs(a - b) for a, b in zip(d, r))
    if scale == 0:
        return (0.0 if e == 0 else float("inf")), 0.0
    return float(e / scale), float(scale)
