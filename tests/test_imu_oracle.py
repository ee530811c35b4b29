"""The oracle's IMU code against tests/imu_ref.py at 50 digits (CPU only): its
propagate() (oracle.Pipeline.kat_prop) on every propagation case of
imu_cases.prop_cases, and its IMU_PRE (oracle.kat_imu: push_imu, the bias
deltas, give_evaluate's rr, joc and r^T C r with its own inverse of cov) on
preintegrations of 10 and 20 samples at rotation residuals either side of
Log's switch, 0.5 and 3.0 rad, with and without bias deltas. The oracle is an
fp64 route of the same formulas, so it is held to what tests/test_imu_ref.py
holds the fp64 twin to: 1e-9 of each group's largest reference entry."""
import numpy as np

import hp_ref
import imu_cases
import imu_ref
import oracle
import vgconfig

CAP = 1e-9


def test_oracle_propagate_against_imu_ref(oracle_lib):
    pl = oracle.Pipeline(vgconfig.to_c(vgconfig.load("mid360"), use_threads=0, vnc_prep=0))
    for c in imu_cases.prop_cases():
        s = pl.kat_prop(np.r_[0.0, c["x"]], c["imu"], c["last_end"], c["beg"], c["end"])
        x = s[1:]
        assert s[0] == c["end"] and np.array_equal(x[15:24], c["x"][15:24]), c["name"]
        if len(c["imu"]) == 0:
            assert np.array_equal(x, c["x"]), c["name"]
            continue
        hp, _ = imu_cases.ref_prop(c)
        if not hp["defined"]:
            assert np.array_equal(x[24:], c["x"][24:]), c["name"]
            continue
        got = imu_cases.prop_groups(x[0:9].reshape(3, 3), x[9:12], x[12:15], x[24:].reshape(15, 15))
        ref = imu_cases.prop_groups(hp["R"], hp["p"], hp["v"], hp["cov"])
        for (name, d), (_, a) in zip(got, ref):
            e, scale = imu_cases.rel_err(d, a)
            assert e <= CAP, (c["name"], name, e)
    pl.close()


def test_oracle_give_evaluate_against_imu_ref(oracle_lib):
    rng = np.random.default_rng(35)
    nz = imu_cases.mid360()
    p = vgconfig.load("mid360")["LocalBA"]
    noise = np.array([p["cov_gyr"], p["cov_acc"], p["rdw_gyr"], p["rdw_acc"]])
    for n in (10, 20):
        imu = imu_cases.samples(rng, n, 0.005, 0.4)
        b0 = np.r_[rng.normal(0, 1e-3, 3), rng.normal(0, 1e-2, 3)]
        s = imu_ref.integrate(b0[:3], b0[3:], imu, 1.0, nz["meas"], nz["walk"])
        rec = imu_ref.record(s)
        r = {k: s[k] for k in s}
        r["cov_inv"] = hp_ref.mp.matrix(15, 15)
        for i in range(15):
            for j in range(15):
                r["cov_inv"][i, j] = rec[64 + 15 * i + j]
        rnp = imu_ref.rec_np(rec)
        for theta in (5e-4, 2e-3, 0.5, 3.0):
            for db in (np.zeros(6), np.r_[1e-2 * imu_cases._unit(rng), 0.1 * imu_cases._unit(rng)]):
                bias = np.r_[db, np.zeros(6)][None, :]
                xs = imu_cases._window(rng, 2, rnp[None, :], bias, [theta])
                cost, rr, J = oracle.kat_imu(imu, b0, db, xs[0], xs[1], noise)
                ev = imu_ref.evaluate(r, hp_ref.M(db[:3]), hp_ref.M(db[3:]), imu_ref._frame(imu_ref.HP, xs[0]),
                                      imu_ref._frame(imu_ref.HP, xs[1]))
                tag = (n, theta, float(np.abs(db).max()))
                assert imu_cases.rel_err(rr, ev["rr"])[0] <= CAP, tag
                for a in range(5):
                    for b in range(10):
                        blk = ev["joc"][3 * a:3 * a + 3, 3 * b:3 * b + 3]
                        e, scale = imu_cases.rel_err(J[3 * a:3 * a + 3, 3 * b:3 * b + 3], blk)
                        assert e <= CAP if scale else e == 0.0, (tag, a, b, e)
                assert abs(cost - float(ev["res"])) <= CAP * float(ev["res"]), (tag, cost, float(ev["res"]))
