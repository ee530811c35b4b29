// imu_prop.cpp — the host IMU propagation: IMUEKF::motion_blur's state and
// covariance part (imu_ekf.cpp:28-94) on the host mirror's x_curr. Used when a
// scan does not propagate on the device (state.hip k_scan_prop, the same
// expression trees; pipeline.cpp prop_on_device): the deskew path, which
// needs the IMU poses on the host, the stage-level API, and a fused step with
// the device propagation off or more than kPropMax IMU samples. The per-point
// deskew (114-144) is SURVEY row f1 (pipeline.cpp stage_deskew).
#include <cstring>
#include <vector>

#include "vg_host.h"

namespace vg {

// one row of a sparse 15x15 matrix: its non-zero columns, ascending
struct SpRow {
  int n;
  int k[7];
  double v[7];
};
// F C F^T + Q with F given by its rows; every sum in ascending column order
// (the dense product's order, zero terms dropped)
static M15 sandwich(const SpRow* F, const M15& C, const M15& Q) {
  M15 A, out;
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = F[i].v[0] * C(F[i].k[0], j);
      for (int t = 1; t < F[i].n; t++) s += F[i].v[t] * C(F[i].k[t], j);
      A(i, j) = s;
    }
  for (int i = 0; i < 15; i++)
    for (int j = 0; j < 15; j++) {
      double s = A(i, F[j].k[0]) * F[j].v[0];
      for (int t = 1; t < F[j].n; t++) s += A(i, F[j].k[t]) * F[j].v[t];
      out(i, j) = s + Q(i, j);
    }
  return out;
}

void propagate(vg_ctx* ctx, HostPipe* P, const std::vector<Imu>& imus, double pcl_beg, double pcl_end) {
  P->poses.clear();
  const vg_config& c = ctx->cfg;
  HX& xc = P->x_curr;
  V3 acc_imu = V3::Z(), angvel = V3::Z(), acc_avr, vel = xc.v, pos = xc.p;
  M3 R_imu = xc.R;
  double dt = 0;
  for (size_t k = 0; k + 1 < imus.size(); k++) {
    const Imu& head = imus[k];
    const Imu& tail = imus[k + 1];
    if (head.t < P->last_pcl_end_time) continue;
    for (int j = 0; j < 3; j++) {
      angvel[j] = 0.5 * (head.gyr[j] + tail.gyr[j]);
      acc_avr[j] = 0.5 * (head.acc[j] + tail.acc[j]);
    }
    angvel = sub(angvel, xc.bg);
    acc_avr = sub(scl(acc_avr, P->sg), xc.ba);  // imu_ekf.cpp:51
    acc_imu = add(mul(R_imu, acc_avr), xc.g);
    double cur = head.t;
    if (cur < P->last_pcl_end_time) cur = P->last_pcl_end_time;
    dt = tail.t - cur;
    {  // imu_poses.emplace_back(offt, R_imu, pos_imu, vel_imu, angvel_avr, acc_imu) (imu_ekf.cpp:64)
      double rec[22];
      rec[0] = cur - pcl_beg;
      memcpy(rec + 1, R_imu.a, 72);
      memcpy(rec + 10, pos.a, 24);
      memcpy(rec + 13, vel.a, 24);
      memcpy(rec + 16, angvel.a, 24);
      memcpy(rec + 19, acc_imu.a, 24);
      P->poses.insert(P->poses.end(), rec, rec + 22);
    }
    M3 ask = hat(acc_avr);
    M3 Exp_f = Exp(angvel, dt);
    M15 cw = M15::Z();
    M3 F00 = Exp(angvel, -dt), F60 = scl(mul(R_imu, ask), -dt), F612 = scl(R_imu, -dt);
    M3 ca = M3::Z();
    for (int j = 0; j < 3; j++) ca(j, j) = c.odo_cov_acc;
    M3 cw66 = scl(mul(mul(R_imu, ca), tr(R_imu)), dt * dt);
    for (int r = 0; r < 3; r++) {
      for (int q = 0; q < 3; q++) cw(6 + r, 6 + q) = cw66(r, q);
      cw(r, r) = c.odo_cov_gyr * dt * dt;
      cw(9 + r, 9 + r) = c.odo_rdw_gyr * dt * dt;
      cw(12 + r, 12 + r) = c.odo_rdw_acc * dt * dt;
    }
    // cov = F cov F^T + cw (imu_ekf.cpp:79) with F's non-zeros only: F is the
    // identity but for rows 0-2 (F00, -dt I), 3-5 (I, dt I) and 6-8 (F60, I,
    // F612). Terms are summed in ascending column order, as the dense product
    // does, and the zero terms it adds are exact no-ops: same bits, 5x fewer
    // flops on the host's per-scan critical path.
    SpRow Fr[15];
    for (int r = 0; r < 3; r++) {
      Fr[r] = SpRow{4, {0, 1, 2, 9 + r}, {F00(r, 0), F00(r, 1), F00(r, 2), -dt}};
      Fr[3 + r] = SpRow{2, {3 + r, 6 + r}, {1.0, dt}};
      Fr[6 + r] = SpRow{7, {0, 1, 2, 6 + r, 12, 13, 14}, {F60(r, 0), F60(r, 1), F60(r, 2), 1.0, F612(r, 0),
                                                           F612(r, 1), F612(r, 2)}};
    }
    for (int r = 9; r < 15; r++) Fr[r] = SpRow{1, {r}, {1.0}};
    xc.cov = sandwich(Fr, xc.cov, cw);
    pos = add(add(pos, scl(vel, dt)), scl(acc_imu, 0.5 * dt * dt));
    vel = add(vel, scl(acc_imu, dt));
    R_imu = mul(R_imu, Exp_f);
  }
  if (!imus.empty()) {
    double note = pcl_end > imus.back().t ? 1.0 : -1.0;
    dt = note * (pcl_end - imus.back().t);
    xc.v = add(vel, scl(acc_imu, note * dt));
    xc.R = mul(R_imu, Exp(scl(angvel, note), dt));
    xc.p = add(add(pos, scl(vel, note * dt)), scl(acc_imu, note * 0.5 * dt * dt));
  }
  xc.t = pcl_end;
  P->last_pcl_end_time = pcl_end;
}

// Test-only (vgx_scan_prop): k_scan_prop alone on a given x_curr block (x_in,
// kXC: the frame state and the covariance) and n <= kPropMax samples, launched
// through state_scan_begin without scan pointers or hand-off flags, with the
// arguments stage_propagate gives it (prop_arg_fill: the noises and the gravity
// scale are the context's). Out: DState::xc and xp after the launch, and the
// block the host's propagate() makes of the same inputs on a scratch HostPipe.
// More samples than the kernel's arrays hold never reach a launch.
int scan_prop_test(vg_ctx* ctx, const double* x_in, int n, const double* imu, double last_end, double beg, double end,
                   double* xc_out, double* xp_out, double* host_out) {
  if (sharded(ctx)) {
    ctx->err = "vgx_scan_prop: sharded context";
    return VG_E_STATE;
  }
  if (n < 0 || n > kPropMax) {
    ctx->err = "vgx_scan_prop: sample count outside [0, kPropMax]";
    return VG_E_ARG;
  }
  const HostPipe* P = hp(ctx);
  std::vector<PropArg> arg(1);
  memset(&arg[0], 0, sizeof(PropArg));
  prop_arg_fill(arg[0], ctx->cfg, P->sg, last_end, imu, n, beg, end);
  DState* st = ctx->st;
  VG_HIP(hipMemcpy(st->xc, x_in, kXC * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipDeviceSynchronize());  // (the context's stream does not wait for the null stream)
  VG_TRY(state_scan_begin(ctx, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &arg[0]));
  VG_HIP(hipStreamSynchronize(ctx->stream));
  VG_HIP(hipMemcpy(xc_out, st->xc, kXC * sizeof(double), hipMemcpyDeviceToHost));
  VG_HIP(hipMemcpy(xp_out, st->xp, kXC * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<HostPipe> S(1);
  hx_get_block(S[0].x_curr, x_in);
  S[0].last_pcl_end_time = last_end;
  S[0].sg = P->sg;
  propagate(ctx, &S[0], to_imus(imu, n), beg, end);
  hx_put_block(S[0].x_curr, host_out);
  return VG_OK;
}

// Test-only (vgx_imu_record): HImuPre::push_imu + record() on given biases,
// samples (n x 7), gravity scale and 6 x 6 noises. Host code only.
int imu_record_test(const double* bg, const double* ba, const double* imu, int n, double sg, const double* noise_meas,
                    const double* noise_walk, double* rec) {
  M6 nm, nw;
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      nm(r, c) = noise_meas[r * 6 + c];
      nw(r, c) = noise_walk[r * 6 + c];
    }
  HImuPre q(v3(bg[0], bg[1], bg[2]), v3(ba[0], ba[1], ba[2]));
  q.push_imu(to_imus(imu, n), nm, nw, sg);
  q.record(rec);
  return VG_OK;
}

}  // namespace vg
