"""HImuPre::push_imu + record() (vg_host.h; host code, run through
vgx_imu_record without a device) against imu_ref.preintegrate at 50 digits:
the deltas, the bias Jacobians and cov_inv = inverse(cov), which every IMU
factor of the LM reads. Cases (imu_cases.record_cases): 2, 11 and 48 samples,
steps of 5 ms and 0.1 s, gyro rates 0, 1e-9 (below Exp's 1e-7 switch) and 3
rad/s, the mid360 noises and noises that spread cov's blocks over 12 decades.

Errors per group (each delta and Jacobian block, dtime, the 3 x 3 blocks of
cov_inv) in units of the group's largest reference entry; e_f64 is the same
route in fp64 numpy (numpy.linalg.inv). Asserted per class: e_host / max(e_f64,
2^-53) <= BOUND, the next power of two above twice the worst ratio measured on
a CPU host (beside each bound; above 64 would be a finding). e_f64 is
numpy / LAPACK's: another BLAS build can move it. With 2
samples cov has rank 6 in exact arithmetic (imu_cases.ref_record), its inverse
is not defined and only the first 64 entries are compared."""
import numpy as np

import imu_cases
import vgpu

U = imu_cases.U

# class -> bound; measured ratio beside it
BOUND = {
    "mid360": 16,  # 5.196
    "scaled": 16,  # 6.514
    "mid360/n2": 4,  # 1
    "scaled/n2": 4,  # 1
}


def test_record_against_preintegrate():
    worst = {k: (0.0, 0.0, 0.0, "") for k in BOUND}
    for c in imu_cases.record_cases():
        hp, f = imu_cases.ref_record(c)
        rec = vgpu.imu_record(c["bg"], c["ba"], c["imu"], 1.0, c["meas"], c["walk"])
        assert np.all(rec[61:64] == 0.0)
        n2 = len(c["imu"]) == 2
        if not n2:
            C = rec[64:].reshape(15, 15)
            assert np.all(np.isfinite(C))
        for (name, a), (_, d), (_, b) in zip(imu_cases.record_groups(hp), imu_cases.record_groups(rec[:64] if n2 else rec),
                                             imu_cases.record_groups(f)):
            ed, scale = imu_cases.rel_err(d, a)
            ef, _ = imu_cases.rel_err(b, a)
            if scale == 0.0:
                assert ed == 0.0, (c["name"], name)
                continue
            r = ed / max(ef, U)
            if r > worst[c["cls"]][0]:
                worst[c["cls"]] = (r, ed, ef, c["name"] + " " + name)
    for cls in BOUND:
        print("RATIO %-10s e_host %.3e e_f64 %.3e ratio %.4g (%s)" % ((cls,) + worst[cls][1:3] + (worst[cls][0], worst[cls][3])))
    for cls in BOUND:
        assert worst[cls][0] <= BOUND[cls], (cls, worst[cls])
