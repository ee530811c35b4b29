"""Reference of the IMU side of the estimator, written from the reference
project's text: IMUEKF::motion_blur's state and covariance propagation
(imu_ekf.cpp:28-94), IMU_PRE::push_imu / add_imu (imu_preintegration.cpp:31-95),
IMU_PRE::give_evaluate (97-163) and the delta lines of IMU_PRE::merge
(269-273). Every routine runs on the exact fp64 inputs in one of two
arithmetics: HP (mpmath at 50 digits, hp_ref's Exp / Exp_dt / Log / jr / jr_inv
/ inverse) and F64 (numpy fp64, f64_ref's: the yardstick e_f64 of the device
tests). F and Q are dense 15 x 15 and the covariance step is the dense product.
Nothing here comes from oracle/ or from the device code; tests/test_imu_ref.py
pins this module by closed forms and central differences.

Layouts. A frame state is 24 doubles [R 9 row-major, p, v, bg, ba, g]; an IMU
sample is [t, gyr 3, acc 3]; a preintegration record is 289 doubles (the
device's, vg_imu.h:17-19): R_delta 9, p_delta 3, v_delta 3, R_bg 9, p_bg 9, p_ba
9, v_bg 9, v_ba 9, dtime, three pad, cov_inv 225; a bias record is [dbg 3, dba
3, their backups 6]. Vectors are columns (3 x 1) in both arithmetics."""
import functools

import mpmath as mp
import numpy as np

import f64_ref
import hp_ref

mp.mp.dps = 50
REC = 289
REC_FIELDS = (("R_delta", 0, 9), ("p_delta", 9, 3), ("v_delta", 12, 3), ("R_bg", 15, 9), ("p_bg", 24, 9),
              ("p_ba", 33, 9), ("v_bg", 42, 9), ("v_ba", 51, 9))


class HP:
    """mpmath at 50 digits."""
    name = "hp"
    num = staticmethod(lambda x: x if isinstance(x, mp.mpf) else mp.mpf(float(x)))
    mat = staticmethod(hp_ref.M)
    zeros = staticmethod(lambda r, c: mp.zeros(r, c))
    eye = staticmethod(lambda n: mp.eye(n))
    mm = staticmethod(lambda *ms: functools.reduce(lambda a, b: a * b, ms))
    hat = staticmethod(hp_ref.hat)
    Exp = staticmethod(hp_ref.Exp)
    Exp_dt = staticmethod(hp_ref.Exp_dt)
    Log = staticmethod(hp_ref._Log)
    jr = staticmethod(hp_ref.jr)
    jr_inv = staticmethod(hp_ref.jr_inv)
    inverse = staticmethod(lambda A: mp.inverse(A))
    sym = staticmethod(lambda A: A)


class F64:
    """numpy fp64 (libm / LAPACK)."""
    name = "f64"
    num = staticmethod(float)

    @staticmethod
    def mat(a):
        a = np.array(a, dtype=np.float64)
        return a[:, None] if a.ndim == 1 else a

    zeros = staticmethod(lambda r, c: np.zeros((r, c)))
    eye = staticmethod(lambda n: np.eye(n))
    mm = staticmethod(lambda *ms: functools.reduce(lambda a, b: a @ b, ms))
    hat = staticmethod(lambda v: f64_ref.hat(v[:, 0]))
    Exp = staticmethod(lambda v: f64_ref.Exp(v[:, 0]))
    Exp_dt = staticmethod(lambda w, dt: f64_ref.Exp_dt(w[:, 0], dt))
    Log = staticmethod(lambda R: f64_ref.Log(R)[:, None])
    jr = staticmethod(lambda v: f64_ref.jr(v[:, 0]))
    jr_inv = staticmethod(f64_ref.jr_inv)
    inverse = staticmethod(np.linalg.inv)


def to_np(m):
    """A result of either arithmetic -> numpy fp64 (rounded)."""
    return hp_ref.to_np(m) if isinstance(m, mp.matrix) else np.asarray(m, dtype=np.float64)


def _frame(B, x):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return (B.mat(x[0:9].reshape(3, 3)),) + tuple(B.mat(x[o:o + 3]) for o in (9, 12, 15, 18, 21))


# ---- propagation -----------------------------------------------------------------------------------------

def propagate(x, cov, imu, last_end, end, sg, noises, B=HP):
    """imu_ekf.cpp:28-94 from the frame state x (24) and cov (15 x 15) over the samples imu (n, 7), the
    caller's list with last_imu already in front (line 17). noises = (cov_gyr, cov_acc, cov_bias_gyr,
    cov_bias_acc), each one number for the three axes. Returns a dict: R, p, v, cov, Phi (the product of the
    per-step F, newest on the left), steps (pairs not skipped) and defined. No sample at all leaves
    everything as given (the reference never sees that: its list holds last_imu). With samples but every
    pair skipped, or one sample, line 91-93 read acc_imu and angvel_avr uninitialised: defined is False and
    R, p, v are None."""
    R, p, v, bg, ba, g = _frame(B, x)
    cov = B.mat(np.asarray(cov, dtype=np.float64).reshape(15, 15))
    imu = np.asarray(imu, dtype=np.float64).reshape(-1, 7)
    cg, ca, rg, ra = (B.num(q) for q in noises)
    sg, half = B.num(sg), B.num(0.5)
    I3 = B.eye(3)
    acc_imu = angvel = None
    Phi, steps = B.eye(15), 0
    for k in range(len(imu) - 1):  # line 33
        head, tail = imu[k], imu[k + 1]
        if head[0] < last_end:  # line 38: the skip rule, on the head stamp
            continue
        angvel = half * (B.mat(head[1:4]) + B.mat(tail[1:4])) - bg  # 43-50
        acc_avr = half * (B.mat(head[4:7]) + B.mat(tail[4:7])) * sg - ba  # 46-51
        acc_imu = B.mm(R, acc_avr) + g  # 52
        cur = head[0]
        if cur < last_end:  # 55
            cur = last_end
        dt = B.num(tail[0]) - B.num(cur)  # 60
        F, Q = B.eye(15), B.zeros(15, 15)  # 68-69
        F[0:3, 0:3] = B.Exp_dt(angvel, -dt)  # 71
        F[0:3, 9:12] = -I3 * dt
        F[3:6, 6:9] = I3 * dt
        F[6:9, 0:3] = -B.mm(R, B.hat(acc_avr)) * dt
        F[6:9, 12:15] = -R * dt
        Q[0:3, 0:3] = I3 * (cg * dt * dt)  # 76
        Q[6:9, 6:9] = B.mm(R, I3 * ca, R.T) * dt * dt
        Q[9:12, 9:12] = I3 * (rg * dt * dt)
        Q[12:15, 12:15] = I3 * (ra * dt * dt)
        cov = B.mm(F, cov, F.T) + Q  # 81
        Phi = B.mm(F, Phi)
        p = p + v * dt + half * acc_imu * dt * dt  # 83
        v = v + acc_imu * dt
        R = B.mm(R, B.Exp_dt(angvel, dt))
        steps += 1
    out = {"cov": cov, "Phi": Phi, "steps": steps, "defined": True, "R": R, "p": p, "v": v}
    if len(imu) == 0:
        return out
    if acc_imu is None:
        out.update(defined=False, R=None, p=None, v=None)
        return out
    imu_end = imu[-1, 0]  # 88
    note = B.num(1.0 if end > imu_end else -1.0)
    dt = note * (B.num(end) - B.num(imu_end))  # 90
    out["v"] = v + note * acc_imu * dt
    out["R"] = B.mm(R, B.Exp_dt(note * angvel, dt))
    out["p"] = p + note * v * dt + note * half * acc_imu * dt * dt
    return out


# ---- preintegration --------------------------------------------------------------------------------------

def noise6(a, b):
    """diag(a, a, a, b, b, b) as noiseMeas / noiseWalk are filled (gyro part first)."""
    N = np.zeros((6, 6))
    N[range(3), range(3)] = a
    N[range(3, 6), range(3, 6)] = b
    return N


def integrate(bg, ba, imu, sg, noiseMeas, noiseWalk, B=HP):
    """push_imu / add_imu (imu_preintegration.cpp:31-95) from a fresh IMU_PRE (7-29). Returns a dict of
    R_delta, p_delta, v_delta, R_bg, p_bg, p_ba, v_bg, v_ba, dtime and cov (15 x 15)."""
    bg, ba = B.mat(bg), B.mat(ba)  # (HP: mpmath columns pass through, for the finite differences)
    imu = np.asarray(imu, dtype=np.float64).reshape(-1, 7)
    nm, nw = B.mat(np.asarray(noiseMeas).reshape(6, 6)), B.mat(np.asarray(noiseWalk).reshape(6, 6))
    sg, half = B.num(sg), B.num(0.5)
    I3 = B.eye(3)
    s = {"R_delta": B.eye(3), "p_delta": B.zeros(3, 1), "v_delta": B.zeros(3, 1), "dtime": B.num(0.0),
         "cov": B.zeros(15, 15)}
    for k in ("R_bg", "p_bg", "p_ba", "v_bg", "v_ba"):
        s[k] = B.zeros(3, 3)
    for k in range(1, len(imu)):  # line 36
        prev, curr = imu[k - 1], imu[k]
        dt = B.num(curr[0]) - B.num(prev[0])  # 41
        gyr = half * (B.mat(prev[1:4]) + B.mat(curr[1:4])) - bg  # 43-50
        acc = half * (B.mat(prev[4:7]) + B.mat(curr[4:7])) * sg - ba  # 46-51
        # add_imu
        s["dtime"] = s["dtime"] + dt  # 59
        rinc = B.Exp_dt(gyr, dt)  # 61
        rj = B.jr(gyr * dt)
        rdt = s["R_delta"] * dt  # 64
        rdt2 = s["R_delta"] * (half * dt * dt)
        ask = B.hat(acc)
        s["p_ba"] = s["p_ba"] + s["v_ba"] * dt - rdt2  # 70
        s["p_bg"] = s["p_bg"] + s["v_bg"] * dt - B.mm(rdt2, ask, s["R_bg"])
        s["v_ba"] = s["v_ba"] - rdt
        s["v_bg"] = s["v_bg"] - B.mm(rdt, ask, s["R_bg"])
        s["R_bg"] = B.mm(rinc.T, s["R_bg"]) - rj * dt  # 74
        A, Bm = B.eye(9), B.zeros(9, 6)  # 76-77
        A[0:3, 0:3] = rinc.T
        A[3:6, 0:3] = -B.mm(rdt2, ask)
        A[3:6, 6:9] = I3 * dt
        A[6:9, 0:3] = -B.mm(rdt, ask)
        Bm[0:3, 0:3] = rj * dt  # 84
        Bm[3:6, 3:6] = rdt2
        Bm[6:9, 3:6] = rdt
        cov = s["cov"]
        c99 = B.mm(A, cov[0:9, 0:9], A.T) + B.mm(Bm, nm, Bm.T)  # 88
        cov[0:9, 0:9] = c99
        cov[9:15, 9:15] = cov[9:15, 9:15] + nw * dt  # 90
        s["p_delta"] = s["p_delta"] + s["v_delta"] * dt + B.mm(rdt2, acc)  # 92
        s["v_delta"] = s["v_delta"] + B.mm(rdt, acc)
        s["R_delta"] = B.mm(s["R_delta"], rinc)
    return s


def merge_deltas(a, b, B=HP):
    """IMU_PRE::merge's deltas (imu_preintegration.cpp:269-273): a followed by b."""
    return {"p_delta": a["p_delta"] + a["v_delta"] * b["dtime"] + B.mm(a["R_delta"], b["p_delta"]),
            "v_delta": a["v_delta"] + B.mm(a["R_delta"], b["v_delta"]),
            "R_delta": B.mm(a["R_delta"], b["R_delta"]), "dtime": a["dtime"] + b["dtime"]}


def record(s, B=HP):
    """The 289 entries of the record of an integrate() result; cov_inv = cov.inverse()
    (imu_preintegration.cpp:126) in B's arithmetic. A list of B's numbers."""
    out = [B.num(0.0)] * REC
    for name, o, n in REC_FIELDS:
        m = s[name]
        vals = [m[i, j] for i in range(3) for j in range(3)] if n == 9 else [m[i, 0] for i in range(3)]
        out[o:o + n] = vals
    out[60] = s["dtime"]
    ci = B.inverse(s["cov"])
    out[64:] = [ci[i, j] for i in range(15) for j in range(15)]
    return out


def preintegrate(bg, ba, imu, sg, noiseMeas, noiseWalk, B=HP):
    """integrate() then record(): the device-layout record, cov_inv inverted in B's arithmetic (HP: at 50
    digits)."""
    return record(integrate(bg, ba, imu, sg, noiseMeas, noiseWalk, B), B)


def rec_np(rec):
    return np.array([float(x) for x in rec], dtype=np.float64)


# ---- the factor ------------------------------------------------------------------------------------------

def residual(rec, dbg, dba, st1, st2, B=HP):
    """Lines 105-124 on B's values: rec a dict of R_delta .. v_ba, dtime; st = (R, p, v, bg, ba, g).
    Returns rr (15 x 1) and the intermediates the Jacobian needs."""
    R1, p1, v1, bg1, ba1, g1 = st1
    R2, p2, v2, bg2, ba2, _ = st2
    dtime, half = rec["dtime"], B.num(0.5)
    R_correct = B.mm(rec["R_delta"], B.Exp(B.mm(rec["R_bg"], dbg)))  # 105
    t_correct = rec["p_delta"] + B.mm(rec["p_bg"], dbg) + B.mm(rec["p_ba"], dba)
    v_correct = rec["v_delta"] + B.mm(rec["v_bg"], dbg) + B.mm(rec["v_ba"], dba)
    res_r = B.mm(R_correct.T, R1.T, R2)  # 109
    exp_v = B.mm(R1.T, v2 - v1 - g1 * dtime)
    res_v = exp_v - v_correct
    exp_t = B.mm(R1.T, p2 - p1 - v1 * dtime - g1 * (half * dtime * dtime))
    res_t = exp_t - t_correct
    rr = B.zeros(15, 1)
    rr[0:3, 0:1] = B.Log(res_r)  # 120
    rr[3:6, 0:1] = res_t
    rr[6:9, 0:1] = res_v
    rr[9:12, 0:1] = bg2 - bg1
    rr[12:15, 0:1] = ba2 - ba1
    return rr, res_r, exp_t, exp_v


def _rec_dict(B, rec):
    rec = np.asarray(rec, dtype=np.float64).reshape(REC)
    d = {name: B.mat(rec[o:o + n].reshape(3, 3) if n == 9 else rec[o:o + n]) for name, o, n in REC_FIELDS}
    d["dtime"] = B.num(rec[60])
    d["cov_inv"] = B.mat(rec[64:].reshape(15, 15))
    return d


def give_evaluate(rec, bias, x1, x2, jac=True, B=HP):
    """IMU_PRE::give_evaluate (imu_preintegration.cpp:97-163) on a record (289; its cov_inv stands for
    line 126's cov.inverse()), a bias record (dbg, dba in front) and the frame states x1, x2 (24). Returns a
    dict: res = rr^T cov_inv rr, rr (15 x 1) and, with jac, joc (15 x 30), jtj (30 x 30), gg (30 x 1)."""
    r = _rec_dict(B, rec)
    bias = np.asarray(bias, dtype=np.float64).reshape(-1)
    return evaluate(r, B.mat(bias[0:3]), B.mat(bias[3:6]), _frame(B, x1), _frame(B, x2), jac, B)


def evaluate(r, dbg, dba, st1, st2, jac=True, B=HP):
    """give_evaluate on B's values (r: _rec_dict's; st: _frame's)."""
    rr, res_r, exp_t, exp_v = residual(r, dbg, dba, st1, st2, B)
    C = r["cov_inv"]
    out = {"rr": rr, "res": B.mm(rr.T, B.mm(C, rr))[0, 0]}  # 162
    if not jac:
        return out
    R1, R2, I3 = st1[0], st2[0], B.eye(3)
    JR_inv = B.jr_inv(res_r)  # 130
    joc = B.zeros(15, 30)
    joc[0:3, 0:3] = -B.mm(JR_inv, R2.T, R1)  # 132
    joc[0:3, 15:18] = JR_inv
    joc[0:3, 9:12] = -B.mm(JR_inv, res_r.T, B.jr(B.mm(r["R_bg"], dbg)), r["R_bg"])  # 134
    joc[3:6, 0:3] = B.hat(exp_t)  # 136
    joc[3:6, 3:6] = -R1.T
    joc[3:6, 6:9] = -R1.T * r["dtime"]
    joc[3:6, 9:12] = -r["p_bg"]
    joc[3:6, 12:15] = -r["p_ba"]
    joc[3:6, 18:21] = R1.T  # 141
    joc[6:9, 0:3] = B.hat(exp_v)  # 143
    joc[6:9, 6:9] = -R1.T
    joc[6:9, 9:12] = -r["v_bg"]
    joc[6:9, 12:15] = -r["v_ba"]
    joc[6:9, 21:24] = R1.T  # 147
    joc[9:12, 9:12] = -I3  # 149
    joc[12:15, 12:15] = -I3
    joc[9:12, 24:27] = I3
    joc[12:15, 27:30] = I3
    out["joc"] = joc
    out["jtj"] = B.mm(joc.T, C, joc)  # 158
    out["gg"] = B.mm(joc.T, C, rr)
    return out
