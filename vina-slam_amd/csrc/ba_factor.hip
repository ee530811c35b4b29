// ba_factor.hip — the LM's factor passes and bookkeeping (SURVEY §8(a) rows
// A11, A12): the point-cluster factor LidarFactor::acc_evaluate2 /
// evaluate_only_residual (factors.cpp:22-158), IMU_PRE::give_evaluate
// (imu_preintegration.cpp:97-163) and damping_iter's accept / reject
// (optimizers.cpp:480-515). Kernels: k_ba_hess, k_ba_hfinal, k_ba_control,
// k_ba_resid, k_ba_resid_hess, k_ba_rsum, k_ba_init, k_ba_init_hess. The
// iteration they make up is described at the head of ba.hip, which drives them
// through the launch functions at the end of this file (vg_ba.h).
#include "vg_ba.h"

#include "vg_imu.h"  // imu_residual (host and device)

namespace vg {

__device__ __forceinline__ void factor_basics(const double* e, const Clu& pcr, double* f) {
  // f: umumT(9) ukukT(9) uk(3) NN lmbd0
  V3 u[3];
  for (int k = 0; k < 3; k++) u[k] = v3(e[3 + 0 * 3 + k], e[3 + 1 * 3 + k], e[3 + 2 * 3 + k]);
  M3 um;
  um.zero();
  for (int i = 1; i < 3; i++) {
    M3 o = outer3(u[i], u[i]);
    double c = 2.0 / (e[0] - e[i]);
    for (int t = 0; t < 9; t++) um[t] += o[t] * c;
  }
  M3 uu = outer3(u[0], u[0]);
  for (int t = 0; t < 9; t++) {
    f[t] = um[t];
    f[9 + t] = uu[t];
  }
  for (int t = 0; t < 3; t++) f[18 + t] = u[0][t];
  f[21] = (double)pcr.N;
  f[22] = 1.0;  // coe (octree.cpp:507)
  f[23] = e[0];
}

// IMU record k of DState's ring (pushed by k_push_state, slid by moving the head)
__device__ __forceinline__ const double* imu_rec(const double* imurec, int head, int k) {
  return &imurec[(size_t)((head + k) % kMaxWin) * kImuRec];
}
// give_evaluate with jac_enable at the current state; out per factor: jtj 900, gg 30, res 1
__device__ void imu_factor_block(int k, const double* __restrict__ imurec, int head, const double* __restrict__ bias,
                                 const double* __restrict__ xs, double* __restrict__ out) {
  __shared__ double joc[450], rr[15], P[450], C[225];
  const double* rec = imu_rec(imurec, head, k);
  if (threadIdx.x == 0) imu_residual(rec, &bias[k * 12], &xs[(size_t)k * kX], &xs[(size_t)(k + 1) * kX], rr, joc);
  for (int t = threadIdx.x; t < 225; t += blockDim.x) C[t] = rec[64 + t];
  __syncthreads();
  // P = joc^T C (30 x 15)
  for (int t = threadIdx.x; t < 450; t += blockDim.x) {
    int r = t / 15, l = t % 15;
    double s = joc[0 * 30 + r] * C[0 * 15 + l];
    for (int q = 1; q < 15; q++) s += joc[q * 30 + r] * C[q * 15 + l];
    P[t] = s;
  }
  __syncthreads();
  double* o = &out[(size_t)k * 931];
  for (int t = threadIdx.x; t < 900; t += blockDim.x) {
    int r = t / 30, c = t % 30;
    double s = P[r * 15 + 0] * joc[0 * 30 + c];
    for (int l = 1; l < 15; l++) s += P[r * 15 + l] * joc[l * 30 + c];
    o[t] = s;
  }
  if (threadIdx.x < 30) {
    int r = threadIdx.x;
    double s = P[r * 15 + 0] * rr[0];
    for (int l = 1; l < 15; l++) s += P[r * 15 + l] * rr[l];
    o[900 + r] = s;
  }
  if (threadIdx.x == 0) {
    double cr[15];
    for (int r = 0; r < 15; r++) {
      double s = C[r * 15] * rr[0];
      for (int l = 1; l < 15; l++) s += C[r * 15 + l] * rr[l];
      cr[r] = s;
    }
    double s = rr[0] * cr[0];
    for (int r = 1; r < 15; r++) s += rr[r] * cr[r];
    o[930] = s;
  }
}

// IMU residuals only (give_evaluate(..., false)) at the trial state
__device__ void imu_residual_lane(int k, const double* __restrict__ imurec, int head, const double* __restrict__ bias,
                                  const double* __restrict__ xt, double* __restrict__ res) {
  const double* rec = imu_rec(imurec, head, k);
  double rr[15];
  imu_residual(rec, &bias[k * 12], &xt[(size_t)k * kX], &xt[(size_t)(k + 1) * kX], rr, nullptr);
  double cr[15];
  for (int r = 0; r < 15; r++) {
    double s = rec[64 + r * 15] * rr[0];
    for (int l = 1; l < 15; l++) s += rec[64 + r * 15 + l] * rr[l];
    cr[r] = s;
  }
  double s = rr[0] * cr[0];
  for (int r = 1; r < 15; r++) s += rr[r] * cr[r];
  res[k] = s;
}

// acc_evaluate2 per (factor, frame) — factors.cpp:57-97. Outputs the
// diagonal 6x6 block Hb (lower, 21), the gradient piece jjt (6) and the three
// 6-vectors whose outer products make every off-diagonal block:
//   Auk_i^T umumT Auk_j = sum_{m=1,2} c_m (Auk_i^T u_m)(Auk_j^T u_m)^T,
//       umumT = sum_m c_m u_m u_m^T, c_m = 2/(lambda_0 - lambda_m)
//   the correction terms (factors.cpp:80-86) = -(2/NN^2) h_i h_j^T,
//       h_i = [viRiTuk; n_i uk]
__device__ __forceinline__ void factor_frame(const double* e, const Clu& pa, const Clu& s, const double* x,
                                             double* hb, double* jjt_o, double* g1, double* g2, double* h) {
  double f[kCompF];
  factor_basics(e, pa, f);
  const double NN = f[21];
  M3 umumT, ukukT;
  for (int k = 0; k < 9; k++) {
    umumT[k] = f[k];
    ukukT[k] = f[9 + k];
  }
  const V3 uk = v3(f[18], f[19], f[20]);
  const V3 vBar = v3(pa.v[0] / NN, pa.v[1] / NN, pa.v[2] / NN);
  const M3 Pi = clu_Pm(s);
  const V3 vi = clu_v(s);
  const M3 Ri = ld_m3(x);
  const double ni = (double)s.N;
  const M3 vihat = hat(vi);
  const V3 RiTuk = mul(tr(Ri), uk);
  const M3 RiTukhat = hat(RiTuk);
  const V3 PiRiTuk = mul(Pi, RiTuk);
  const V3 viRiTuk = mul(vihat, RiTuk);
  const V3 ti_v = sub(ld_v3(x + 9), vBar);
  const double ukTti_v = dot3(uk, ti_v);
  const M3 combo1 = add(hat(PiRiTuk), scl(vihat, ukTti_v));
  const V3 combo2 = add(mul(Ri, vi), scl(ti_v, ni));
  M<3, 6> A;
  M3 A1 = sub(mul(add(mul(Ri, Pi), outer3(ti_v, vi)), RiTukhat), mul(Ri, combo1));
  M3 A2 = add(outer3(combo2, uk), scl(M3::I(), dot3(combo2, uk)));
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      A(r, c) = A1(r, c) / NN;
      A(r, 3 + c) = A2(r, c) / NN;
    }
  V6 jjt = mul(tr(A), uk);
  // Hb = (A^T umumT) A + the corrections, only the lower triangle the output
  // keeps: every entry formed exactly as the full products form it (same
  // terms, same order), the upper 15 entries and their registers skipped
  // (the full 6x6 pushed k_ba_hess past 256 VGPRs: 50 spilled)
  M<6, 3> AtU = mul(tr(A), umumT);
  const double s2n = 2.0 / NN * (1.0 - ni / NN);  // HRt's scale
  const double c00s = 2.0 / NN, c00v = 2.0 / NN / NN;
  const double c11s = 2.0 / NN * (ni - ni * ni / NN);
  M3 L1;  // combo1 - RiTukhat Pi (c00's left factor, full: its rows meet RiTukhat's columns)
  {
    const M3 RP = mul(RiTukhat, Pi);
    for (int t = 0; t < 9; t++) L1[t] = combo1[t] - RP[t];
  }
  int q = 0;
  for (int r = 0; r < 6; r++)
    for (int c = 0; c <= r; c++) {
      double v = AtU(r, 0) * A(0, c);
      v += AtU(r, 1) * A(1, c);
      v += AtU(r, 2) * A(2, c);
      if (r < 3) {  // c00 = ((L1 RiTukhat) * 2/NN - (viRiTuk viRiTuk^T) * 2/NN/NN) - hat(jjt[0..3]) * 0.5
        double m = L1(r, 0) * RiTukhat(0, c);
        m += L1(r, 1) * RiTukhat(1, c);
        m += L1(r, 2) * RiTukhat(2, c);
        const V3 jt = v3(jjt[0], jjt[1], jjt[2]);
        const double hj = r == c ? 0.0 : (r == 1 ? (c == 0 ? jt[2] : 0.0) : (c == 0 ? -jt[1] : jt[0]));
        v += (m * c00s - (viRiTuk[r] * viRiTuk[c]) * c00v) - hj * 0.5;
      } else if (c < 3) {  // HRt(c, r - 3) (the lower off-diagonal block)
        v += (viRiTuk[c] * uk[r - 3]) * s2n;
      } else {
        v += ukukT(r - 3, c - 3) * c11s;
      }
      hb[q++] = v;
    }
  for (int k = 0; k < 6; k++) jjt_o[k] = jjt[k];
  const V3 u1 = v3(e[3 + 0 * 3 + 1], e[3 + 1 * 3 + 1], e[3 + 2 * 3 + 1]);
  const V3 u2 = v3(e[3 + 0 * 3 + 2], e[3 + 1 * 3 + 2], e[3 + 2 * 3 + 2]);
  for (int k = 0; k < 6; k++) {
    g1[k] = A(0, k) * u1[0] + A(1, k) * u1[1] + A(2, k) * u1[2];
    g2[k] = A(0, k) * u2[0] + A(1, k) * u2[1] + A(2, k) * u2[2];
  }
  for (int k = 0; k < 3; k++) {
    h[k] = viRiTuk[k];
    h[3 + k] = ni * uk[k];
  }
}

// outputs per chunk: 1830 lower entries of the 6W x 6W LiDAR Hessian
// (row-major lower), then 6W gradient, then the residual
__device__ __forceinline__ int lower_idx(int r, int c) { return r * (r + 1) / 2 + c; }

// One workgroup per chunk of factors, no HBM intermediates: lane (f, i)
// evaluates factor f of the sub-chunk at frame i, keeps the coe-weighted
// diagonal block / gradient in registers and writes its three rank-1 rows to
// X (LDS); the off-diagonal blocks are then X^T S X on v_mfma_f64_16x16x4
// (one wave per lower 16x16 output tile, accumulators live across
// sub-chunks). Chunk partials go to `part` (summed by k_ba_hfinal).
// kSpec (k_ba_resid_hess): the pass at the LM's trial state, `xs` = the trial
// states. The chunk first does k_ba_resid's work for its factors —
// evaluate_only_residual: frame clusters moved to the trial poses, merged onto
// pcr_fix in frame order, 3x3 eigen, fac_eig / fac_pcr written — with
// k_ba_resid's operations, then evaluates the Hessian from those values (LDS)
// instead of fac_eig / fac_pcr. ev0[0] / ev0[1] take each lane's smallest
// eigenvalues for the two residual chunks the Hessian chunk holds.
template <bool kSpec = false>
__device__ __forceinline__ void hess_chunk_eval(int ch, int nf, int W, const int* __restrict__ fac_node,
                                                const double* __restrict__ fac_eig, const Clu* __restrict__ fac_pcr,
                                                const Clu* __restrict__ pcrs, const int* __restrict__ mpring,
                                                const double* __restrict__ xs, double* __restrict__ part,
                                                const Clu* __restrict__ pcr_fix = nullptr,
                                                double* __restrict__ eig_out = nullptr,
                                                Clu* __restrict__ pcr_out = nullptr, double* ev0 = nullptr,
                                                const double* __restrict__ eig_src = nullptr,
                                                const Clu* __restrict__ pcr_src = nullptr,
                                                NodeHdr* __restrict__ hdr = nullptr) {
  __syncthreads();  // the previous chunk's reduction has read the LDS
  extern __shared__ __attribute__((aligned(16))) double X[];
  __shared__ double S[kHessThreads];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int FS = hess_fs(W), KS = hess_ks(W), NT = hess_nt(W), XS = hess_xs(W);
  const int L = 6 * W, nl = L * (L + 1) / 2, nout = nl + L + 1;
  const int f = tid / W, i = tid % W;
  const bool active = f < FS;
  const int a_begin = ch * hess_chunk(W);
  const int a_end = min(nf, a_begin + hess_chunk(W));
  const int ntl = NT * (NT + 1) / 2;
  __shared__ double s_e[kSpec ? 64 : 1][12];  // kSpec: the chunk's eigen systems and merged clusters at the trial
  __shared__ Clu s_pa[kSpec ? 64 : 1];
  if constexpr (kSpec) {
    Clu* s_t = reinterpret_cast<Clu*>(X);  // the moved frame clusters (X is filled below)
    {
      const int a = a_begin + f;
      if (active && a < a_end) {
        const Clu src = pcrs[(size_t)fac_node[a] * W + mpring[i]];
        Clu t;
        if (src.N != 0) {
          t = clu_transform(src, ld_m3(&xs[(size_t)i * kX]), ld_v3(&xs[(size_t)i * kX + 9]));
        } else {
          clu_zero(t);
          t.N = 0;
        }
        s_t[tid] = t;
      }
    }
    __syncthreads();
    const int a2 = a_begin + tid;
    if (tid < FS && a2 < a_end) {
      Clu sig = pcr_fix[fac_node[a2]];
      for (int k = 0; k < W; k++) {
        const Clu& t = s_t[tid * W + k];
        if (t.N != 0) clu_add(sig, t);
      }
      V3 ev;
      M3 U;
      eig3(clu_cov(sig), ev, U);
      double* e = &eig_out[(size_t)a2 * 12];
      for (int j = 0; j < 3; j++) e[j] = s_e[tid][j] = ev[j];
      for (int j = 0; j < 9; j++) e[3 + j] = s_e[tid][3 + j] = U[j];
      pcr_out[a2] = sig;
      s_pa[tid] = sig;
      ev0[tid < FS / 2 ? 0 : 1] += 1.0 * ev[0];  // k_ba_resid's acc (lane tid mod FS/2 of its chunk)
    }
    __syncthreads();  // s_t is read: X may be cleared
  }
  // A chunk is one sub-chunk (hess_chunk == hess_fs): the lane's factor_frame
  // writes its diagonal block and gradient straight into hb / jj (0 + coe x,
  // the accumulation's value), so no second copy is live beside the call
  // (it was: 256 VGPRs and ~50 spilled, scratch traffic ~5x the kernel's bytes)
  for (int t = tid; t < KS * XS; t += kHessThreads) X[t] = 0.0;
  for (int t = tid; t < KS; t += kHessThreads) S[t] = 0.0;
  __syncthreads();
  double hb[21], jj[6], res = 0.0;
  {
    const int a = a_begin + f;
    bool got = false;
    if (active && a < a_end) {
      const int node = fac_node[a];
      // eig_src (k_ba_init_hess): tras_opt's bookkeeping in this pass, the
      // factor's eigen system and cluster read from the map and copied out
      const double* e = kSpec ? s_e[f] : (eig_src ? &eig_src[(size_t)node * 12] : &fac_eig[(size_t)a * 12]);
      const Clu pa = kSpec ? s_pa[f] : (eig_src ? pcr_src[node] : fac_pcr[a]);
      if (!kSpec && eig_src && i == 0) {
        for (int j = 0; j < 12; j++) eig_out[(size_t)a * 12 + j] = e[j];
        pcr_out[a] = pa;
        hdr[node].opt_state = a;
      }
      const double coe = 1.0;  // octree.cpp:507
      if (i == 0) {
        res = 0.0 + coe * e[0];
        const double NN = (double)pa.N;
        S[3 * f + 0] = coe * (2.0 / (e[0] - e[1]));
        S[3 * f + 1] = coe * (2.0 / (e[0] - e[2]));
        S[3 * f + 2] = -coe * (2.0 / NN / NN);
      }
      const Clu sc = pcrs[(size_t)node * W + mpring[i]];
      if (sc.N != 0) {
        double g1[6], g2[6], h[6];
        factor_frame(e, pa, sc, &xs[(size_t)i * kX], hb, jj, g1, g2, h);
        for (int k = 0; k < 21; k++) hb[k] = 0.0 + coe * hb[k];
        for (int k = 0; k < 6; k++) jj[k] = 0.0 + coe * jj[k];
        double* x0 = &X[(size_t)(3 * f) * XS + 6 * i];
        for (int k = 0; k < 6; k++) {
          x0[k] = g1[k];
          x0[XS + k] = g2[k];
          x0[2 * XS + k] = h[k];
        }
        got = true;
      }
    }
    if (!got) {
      for (int k = 0; k < 21; k++) hb[k] = 0.0;
      for (int k = 0; k < 6; k++) jj[k] = 0.0;
    }
  }
  __syncthreads();
  v4d acc[4];  // <= 15 lower tiles (W <= 11) over the 8 waves (<= 2 per wave; 4 slots)
  for (int q = wave, slot = 0; q < ntl; q += kHessThreads / 64, slot++) {
    int TI = 0;
    while ((TI + 1) * (TI + 2) / 2 <= q) TI++;
    const int TJ = q - TI * (TI + 1) / 2;
    const int cc = lane & 15, rq = lane >> 4;
    v4d c = v4d{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < KS; k0 += 4) {
      const int k = k0 + rq;
      const double av = S[k] * X[(size_t)k * XS + 16 * TI + cc];
      const double bv = X[(size_t)k * XS + 16 * TJ + cc];
      c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
    }
    acc[slot] = c;
  }
  __syncthreads();
  double* out = &part[(size_t)ch * nout];
  // off-diagonal blocks from the MFMA tiles (diagonal 6x6 blocks come from Hb)
  for (int q = wave, slot = 0; q < ntl; q += kHessThreads / 64, slot++) {
    int TI = 0;
    while ((TI + 1) * (TI + 2) / 2 <= q) TI++;
    const int TJ = q - TI * (TI + 1) / 2;
    const int cc = lane & 15, rq = lane >> 4;
    for (int g = 0; g < 4; g++) {
      const int row = 16 * TI + rq + 4 * g, colx = 16 * TJ + cc;
      if (row < L && colx <= row && row / 6 != colx / 6) out[lower_idx(row, colx)] = acc[slot][g];
    }
  }
  // per-frame diagonal blocks, gradient and residual: ordered sum over f
  double* R = X;
  if (active) {
    for (int k = 0; k < 21; k++) R[tid * 28 + k] = hb[k];
    for (int k = 0; k < 6; k++) R[tid * 28 + 21 + k] = jj[k];
    R[tid * 28 + 27] = res;
  }
  __syncthreads();
  for (int e = tid; e < W * 27 + 1; e += kHessThreads) {
    if (e == W * 27) {
      double sres = 0.0;
      for (int ff = 0; ff < FS; ff++) sres += R[(ff * W) * 28 + 27];
      out[nl + L] = sres;
      continue;
    }
    const int fi = e / 27, k = e % 27;
    double sv = 0.0;
    for (int ff = 0; ff < FS; ff++) sv += R[(ff * W + fi) * 28 + k];
    if (k < 21) {
      int r = 0;
      while ((r + 1) * (r + 2) / 2 <= k) r++;
      const int c = k - r * (r + 1) / 2;
      out[lower_idx(6 * fi + r, 6 * fi + c)] = sv;
    } else {
      out[nl + 6 * fi + (k - 21)] = sv;
    }
  }
}

// The factor count is read on the device (*nfp): workgroups [0, G) loop over
// the chunks (chunk c -> partial c, whatever G), G + k evaluates IMU factor k.
__device__ __forceinline__ void hess_body(const int* __restrict__ nfp, int W, const int* __restrict__ fac_node,
                                          const double* __restrict__ fac_eig, const Clu* __restrict__ fac_pcr,
                                          const Clu* __restrict__ pcrs, const int* __restrict__ mpring,
                                          const double* __restrict__ xs, double* __restrict__ part,
                                          const BaState* __restrict__ st, int G, int nimu,
                                          const double* __restrict__ imurec, const int* __restrict__ imu_head,
                                          const double* __restrict__ bias, double* __restrict__ imuout) {
  if ((int)blockIdx.x >= G) {  // IMU factors ride in the same launch (give_evaluate, jac_enable)
    const int k = blockIdx.x - G;
    if (k < nimu) imu_factor_block(k, imurec, *imu_head, bias, xs, imuout);
    return;
  }
  const int nf = *nfp;
  const int nchunk = (nf + hess_chunk(W) - 1) / hess_chunk(W);
  for (int ch = blockIdx.x; ch < nchunk; ch += G) hess_chunk_eval(ch, nf, W, fac_node, fac_eig, fac_pcr, pcrs, mpring, xs, part);
}

__global__ void __launch_bounds__(kHessThreads) k_ba_hess(const int* __restrict__ nfp, int W,
                                                          const int* __restrict__ fac_node,
                                                          const double* __restrict__ fac_eig,
                                                          const Clu* __restrict__ fac_pcr, const Clu* __restrict__ pcrs,
                                                          const int* __restrict__ mpring, const double* __restrict__ xs,
                                                          double* __restrict__ part, const BaState* __restrict__ st,
                                                          int G, int nimu, const double* __restrict__ imurec,
                                                          const int* __restrict__ imu_head,
                                                          const double* __restrict__ bias, double* __restrict__ imuout,
                                                          KClock* __restrict__ clk) {
  if (st->done || !st->calc_hess) return;
  // in-kernel clock (vg_profile bit 2): slot (scan, LM iteration), start by
  // workgroup 0, every workgroup's end (KClock h_*)
  const bool clk_on = clk && clk->on;
  const int clk_slot = clk_on ? (clk->scan * 8 + (st->iters < 7 ? st->iters : 7)) & (kClkHRing - 1) : 0;
  if (clk_on && blockIdx.x == 0 && threadIdx.x == 0) {
    clk->h_t0[clk_slot] = (unsigned long long)wall_clock64();
    clk->h_exec[clk_slot] = 1;
  }
  hess_body(nfp, W, fac_node, fac_eig, fac_pcr, pcrs, mpring, xs, part, st, G, nimu, imurec, imu_head, bias, imuout);
  if (clk_on && blockIdx.x < kClkHBlocks) {
    __syncthreads();
    if (threadIdx.x == 0) clk->h_tend[clk_slot][blockIdx.x] = (unsigned long long)wall_clock64();
  }
}

// ordered sum of the chunk partials: 8 lanes per output split the chunks
// (stride 8), then a fixed 3-step shuffle tree (deterministic)
// xa.frame (sharded): `out` is the exchange frame, closed here (nout = its payload)
__global__ void __launch_bounds__(256) k_ba_hfinal(const int* __restrict__ nfp, int chunk, int nout,
                                                   const double* __restrict__ part, double* __restrict__ out,
                                                   const BaState* __restrict__ st, XchgArg xa) {
  if (xa.frame && blockIdx.x == 0 && threadIdx.x == 0) xchg_close(xa.frame, xa.n, 3, xa.seq);
  if (st->done || !st->calc_hess) return;
  const int nchunk = (*nfp + chunk - 1) / chunk;
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = gt >> 3, sub = gt & 7;
  double s = 0.0;
  if (e < nout) {  // chunks sub, sub + 8, ... in order; up to 32 loads issued per batch (one batch up to
                   // 256 chunks: one memory round trip), then added
    constexpr int kB = 32;
    for (int b = sub; b < nchunk; b += 8 * kB) {
      double v[kB];
#pragma unroll
      for (int k = 0; k < kB; k++) v[k] = b + 8 * k < nchunk ? part[(size_t)(b + 8 * k) * nout + e] : 0.0;
#pragma unroll
      for (int k = 0; k < kB; k++)
        if (b + 8 * k < nchunk) s += v[k];
    }
  }
  s += __shfl_down(s, 4, 8);
  s += __shfl_down(s, 2, 8);
  s += __shfl_down(s, 1, 8);
  if (e < nout && sub == 0) out[e] = s;
}

// `pre`: the lane's strided sum of the residual partials, already formed (k_ba_resid).
// The sums run over the first kResidThreads lanes whatever the workgroup size
// (k_ba_resid_hess's is 512), so the residual's order is k_ba_resid's.
__device__ __forceinline__ void ba_control_body(const CtlArg& c, const double* pre = nullptr) {
  __shared__ int accept;
  __shared__ double s_r[kResidThreads];
  const int nt = kResidThreads;
  {  // residual partials: lane-strided sums, then a fixed tree (deterministic)
    double part = 0.0;
    const bool ok = c.xworld <= 0 || xchg_ok(c.rpart, kShardSmall, c.xworld);  // (the frame's consumers read zeros)
    if (!ok && threadIdx.x == 0) atomicOr(c.xerr, 32);
    if (pre) part = *pre;
    else if (!c.st->done && ok) {  // a lane's loads in one batch, summed in the same order
      constexpr int kU = 4;
      for (int b0 = threadIdx.x; b0 < c.nrb; b0 += kU * nt) {
        double v[kU];
#pragma unroll
        for (int k = 0; k < kU; k++) v[k] = b0 + k * nt < c.nrb ? c.rpart[b0 + k * nt] : 0.0;
#pragma unroll
        for (int k = 0; k < kU; k++)
          if (b0 + k * nt < c.nrb) part += v[k];
      }
    }
    if ((int)threadIdx.x < nt) s_r[threadIdx.x] = part;
    __syncthreads();
    for (int w = nt >> 1; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) s_r[threadIdx.x] += s_r[threadIdx.x + w];
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    accept = -1;
    if (!c.st->done) {
      // (residual1 of divide_thread at the current state: k_ba_prep, on the Hessian iterations)
      if (c.st->calc_hess) c.st->nhess += 1;
      double r1 = 0.0;
      for (int k = 0; k < c.nimu; k++) r1 += c.imures[k];
      r1 *= c.imu_coef * 0.5;
      const double r2 = s_r[0];
      const double residual2 = r1 + r2;
      c.st->res2 = residual2;
      const double residual1 = c.st->res1;
      double q = residual1 - residual2;
      if (q > 0) {
        accept = 1;
        const double one_three = 1.0 / 3;
        q = q / c.st->q1;
        c.st->v = 2;
        q = 1 - pow(2 * q - 1, 3);
        c.st->u *= (q < one_three ? one_three : q);
        c.st->calc_hess = 1;
      } else {
        accept = 0;
        c.st->u = c.st->u * c.st->v;
        c.st->v = 2 * c.st->v;
        c.st->calc_hess = 0;
      }
      c.st->iters += 1;
      if (fabs((residual1 - residual2) / residual1) < 1e-6) c.st->done = 1;
    }
  }
  __syncthreads();
  if (accept == 1) {
    for (int t = threadIdx.x; t < c.W * kX; t += blockDim.x) c.xs[t] = c.xt[t];
  } else if (accept == 0) {
    for (int t = threadIdx.x; t < c.nimu * 6; t += blockDim.x) {
      int k = t / 6, j = t % 6;
      c.bias[k * 12 + j] = c.bias[k * 12 + 6 + j];
    }
  }
  if (threadIdx.x == 0) {  // LM flags -> host (read without draining the stream)
    c.st->fin = ((c.st->done || c.st->iters >= 10) && !c.st->skip) ? 1 : 0;
    const int seq = c.st->seq;  // one publication per launch, numbered on the device (graph replays)
    c.st->seq = seq + 1;
    // done and the iteration count in one word: the host reads them as one
    // (a queued-ahead iteration publishing between two separate reads could
    // pair one iteration's count with the next one's done, and sharded ranks
    // would then enqueue different iteration counts)
    pub_store(&c.pub->ba_word, c.st->iters * 2 + (c.st->done ? 1 : 0));
    pub_flag(&c.pub->seq_ba, seq);
  }
}
__global__ void __launch_bounds__(256) k_ba_control(CtlArg c) { ba_control_body(c); }

// The LM bookkeeping inside k_ba_resid, without a fence per workgroup (an
// agent-scope release writes back the XCD's L2): every residual slot starts
// as a sentinel NaN (k_ba_init, and the reader re-arms it), each workgroup
// stores its partial with one relaxed agent-scope 64-bit store, and the IMU
// workgroup (the last dispatched) polls the slots until none holds the
// sentinel, then runs k_ba_control's body on the values it read.
constexpr unsigned long long kRpartEmpty = 0x7ff4deadbeef0001ull;  // a NaN payload arithmetic never produces
__device__ __forceinline__ void rpart_put(double* slot, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void resid_bookkeeping(const CtlArg& c) {
  __shared__ int s_late;
  if (threadIdx.x == 0) s_late = 0;
  __syncthreads();
  double part = 0.0;  // k_ba_control's lane-strided order: slots t, t + 256, ...
  for (int b = threadIdx.x; b < c.nrb && (int)threadIdx.x < kResidThreads; b += kResidThreads) {
    unsigned long long* p = reinterpret_cast<unsigned long long*>(const_cast<double*>(c.rpart) + b);
    unsigned long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int spin = 0; v == kRpartEmpty; spin++) {
      if (spin > (1 << 22)) {  // ~seconds: a workgroup never stored (should not happen)
        s_late = 1;
        v = 0ull;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(p, kRpartEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
    part += __longlong_as_double((long long)v);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_late) atomicOr(c.err, 64);
  ba_control_body(c, &part);
}

// evaluate_only_residual (factors.cpp:128-158) at the trial poses. A chunk of
// 256/W factors per workgroup step: lane (f, i) moves factor f's frame-i
// cluster to the trial pose (independent work, in parallel), then lane f merges
// them onto pcr_fix in frame order (the reference's order) and takes the 3x3
// eigen-decomposition. Workgroup b < nrb takes chunks b, b + nrb, ... of the
// device factor count *nfp; its residual partial goes to rpart[b].
__global__ void __launch_bounds__(256, 2) k_ba_resid(const int* __restrict__ nfp, int W, const int* __restrict__ fac_node,
                                                  const Clu* __restrict__ pcr_fix, const Clu* __restrict__ pcrs,
                                                  const int* __restrict__ mpring, const double* __restrict__ xt,
                                                  double* __restrict__ fac_eig, Clu* __restrict__ fac_pcr,
                                                  double* __restrict__ rpart, const BaState* st, int nrb,
                                                  int nimu, const double* __restrict__ imurec,
                                                  const int* __restrict__ imu_head,
                                                  const double* __restrict__ bias, double* __restrict__ imures,
                                                  CtlArg ctl) {
  if (st->done) {  // converged: the bookkeeping still publishes the flags
    if (ctl.err && (int)blockIdx.x == nrb) ba_control_body(ctl);
    return;
  }
  if ((int)blockIdx.x >= nrb) {  // IMU residuals at the trial state in the same launch
    if ((int)threadIdx.x < nimu) imu_residual_lane(threadIdx.x, imurec, *imu_head, bias, xt, imures);
    if (ctl.err) {
      __syncthreads();  // imures, read by thread 0 of this workgroup
      resid_bookkeeping(ctl);
    }
    return;
  }
  __shared__ Clu s_t[256];
  __shared__ double red[4];
  const int FS = 256 / W;
  const int f = threadIdx.x / W, i = threadIdx.x % W;
  const int nf = *nfp;
  const int nchunk = (nf + FS - 1) / FS;
  double acc = 0.0;
  for (int ch = blockIdx.x; ch < nchunk; ch += nrb) {
    const int a = ch * FS + f;
    if (f < FS && a < nf) {
      const Clu src = pcrs[(size_t)fac_node[a] * W + mpring[i]];
      Clu t;
      if (src.N != 0) {
        t = clu_transform(src, ld_m3(&xt[(size_t)i * kX]), ld_v3(&xt[(size_t)i * kX + 9]));
      } else {
        clu_zero(t);
        t.N = 0;
      }
      s_t[threadIdx.x] = t;
    }
    __syncthreads();
    const int a2 = ch * FS + (int)threadIdx.x;
    if ((int)threadIdx.x < FS && a2 < nf) {
      Clu sig = pcr_fix[fac_node[a2]];
      for (int k = 0; k < W; k++) {
        const Clu& t = s_t[threadIdx.x * W + k];
        if (t.N != 0) clu_add(sig, t);
      }
      V3 ev;
      M3 U;
      eig3(clu_cov(sig), ev, U);
      double* e = &fac_eig[(size_t)a2 * 12];
      for (int j = 0; j < 3; j++) e[j] = ev[j];
      for (int j = 0; j < 9; j++) e[3 + j] = U[j];
      fac_pcr[a2] = sig;
      acc += 1.0 * ev[0];
    }
    __syncthreads();
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) rpart_put(&rpart[blockIdx.x], ((red[0] + red[1]) + red[2]) + red[3]);
}

// The first LM iteration's residual pass and, speculatively, the second
// iteration's Hessian pass at the same trial state, as one launch
// (vg_ctx::ba_resid_hess). An accepted step makes the trial the state
// (optimizers.cpp:480-492), so the second iteration's Hessian is the one of
// the trial poses: every chunk workgroup does k_ba_resid's work for its
// factors (hess_chunk_eval<true>) and goes straight on to their Hessian, so
// the second iteration needs no k_ba_hess launch. A rejected step leaves the
// Hessian unused (calc_hess = 0: k_ba_hfinal / k_ba_prep take the stored
// system). Layout: workgroups [0, kResidBlocks / 2) the Hessian chunks c, c +
// kResidBlocks / 2, ... (hess_fs = 2 x k_ba_resid's chunk: chunk c holds
// residual chunks 2c and 2c + 1, and this workgroup stores their residual
// partials exactly as k_ba_resid's workgroups 2c and 2c + 1 would); then the
// IMU residuals + the LM bookkeeping (resid_bookkeeping); then one workgroup
// per IMU factor's Hessian block (imu_factor_block at the trial). Results are
// bit-identical to k_ba_resid followed by k_ba_hess.
__global__ void __launch_bounds__(kHessThreads) k_ba_resid_hess(const int* __restrict__ nfp, int W,
                                                                const int* __restrict__ fac_node,
                                                                const Clu* __restrict__ pcr_fix,
                                                                const Clu* __restrict__ pcrs,
                                                                const int* __restrict__ mpring,
                                                                const double* __restrict__ xt,
                                                                double* __restrict__ fac_eig, Clu* __restrict__ fac_pcr,
                                                                double* __restrict__ part, double* __restrict__ rpart,
                                                                const BaState* st, int nimu,
                                                                const double* __restrict__ imurec,
                                                                const int* __restrict__ imu_head,
                                                                const double* __restrict__ bias,
                                                                double* __restrict__ imures, double* __restrict__ imuout,
                                                                CtlArg ctl) {
  const int G = kRhChunkWg;
  if (st->done) {  // converged: the bookkeeping still publishes the flags
    if (ctl.err && (int)blockIdx.x == G) ba_control_body(ctl);
    return;
  }
  if ((int)blockIdx.x == G) {  // IMU residuals at the trial state, then the bookkeeping (k_ba_resid's)
    if ((int)threadIdx.x < nimu) imu_residual_lane(threadIdx.x, imurec, *imu_head, bias, xt, imures);
    if (ctl.err) {  // (sharded: k_ba_rsum, the exchange and k_ba_control follow)
      __syncthreads();
      resid_bookkeeping(ctl);
    }
    return;
  }
  if ((int)blockIdx.x > G) {  // the IMU factors' Hessian blocks at the trial (k_ba_hess's IMU workgroups)
    const int k = blockIdx.x - G - 1;
    if (k < nimu) imu_factor_block(k, imurec, *imu_head, bias, xt, imuout);
    return;
  }
  const int nf = *nfp;
  const int nchunk = (nf + hess_chunk(W) - 1) / hess_chunk(W);
  double ev0[2] = {0.0, 0.0};
  for (int ch = blockIdx.x; ch < nchunk; ch += G)
    hess_chunk_eval<true>(ch, nf, W, fac_node, nullptr, nullptr, pcrs, mpring, xt, part, pcr_fix, fac_eig, fac_pcr,
                          ev0);
  // the residual partials of chunks 2c and 2c + 1 in k_ba_resid's form: lane l
  // of its wave 0 holds the chunk's factor l, the other waves hold zeros
  if (threadIdx.x < 64) {
    const int fr = 256 / W, lane = threadIdx.x;
    double r0 = ev0[0];
    double r1 = __shfl_down(ev0[1], fr, 64);
    if (lane >= fr) r1 = 0.0;
    for (int off = 32; off > 0; off >>= 1) r0 += __shfl_down(r0, off, 64);
    for (int off = 32; off > 0; off >>= 1) r1 += __shfl_down(r1, off, 64);
    double z = 0.0;  // waves 1-3 of k_ba_resid: an all-zero tree
    for (int off = 32; off > 0; off >>= 1) z += __shfl_down(z, off, 64);
    if (lane == 0) {
      rpart_put(&rpart[2 * blockIdx.x], ((r0 + z) + z) + z);
      rpart_put(&rpart[2 * blockIdx.x + 1], ((r1 + z) + z) + z);
    }
  }
}

// sharded mode: this shard's factor residual (ordered sum of the block
// partials) packed into the exchange frame (k_ba_control checks its guard)
// (the partials staged in LDS by every lane in one round of loads, then the
// same sequential sum on one lane)
__global__ void k_ba_rsum(int nrb, const double* __restrict__ rpart, const BaState* __restrict__ st, XchgArg xa) {
  __shared__ double sp[kResidBlocks];
  for (int i = threadIdx.x + 1; i < xa.n - 2; i += blockDim.x) xa.frame[i] = 0.0;
  const bool run = !st->done && nrb <= kResidBlocks;
  if (run) {
    constexpr int kU = kResidBlocks / 64;
    double v[kU];
#pragma unroll
    for (int k = 0; k < kU; k++) {
      const int b = threadIdx.x + 64 * k;
      v[k] = b < nrb ? rpart[b] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kU; k++) {
      const int b = threadIdx.x + 64 * k;
      if (b < nrb) sp[b] = v[k];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    if (run)
      for (int b = 0; b < nrb; b++) r += sp[b];
    else if (!st->done)
      for (int b = 0; b < nrb; b++) r += rpart[b];
    xa.frame[0] = r;
    xchg_close(xa.frame, xa.n, 4, xa.seq);
  }
}

// k_ba_init's part after the factor bookkeeping: the residual slots armed, the
// Hessian accumulators cleared (grid-stride gt / gn), then (wg0) the ring and
// the LM state
__device__ __forceinline__ void ba_init_common(int gt, int gn, bool wg0, BaState* st, double* __restrict__ hl,
                                               double* __restrict__ hl_part, int nout, const MpRing& ring,
                                               int* __restrict__ mpring, int W, int status, int seq0,
                                               double* __restrict__ rpart, int nrb, const int* __restrict__ ph,
                                               unsigned* __restrict__ rc_flag) {
  for (int b = gt; b < nrb; b += gn)  // empty residual slots (resid_bookkeeping)
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(rpart + b), kRpartEmpty, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  for (int t = gt; t < nout; t += gn) {
    hl[t] = 0.0;
    hl_part[t] = 0.0;
  }
  if (!wg0) return;
  if ((int)threadIdx.x < W) mpring[threadIdx.x] = ring.mp[threadIdx.x];
  if (threadIdx.x == 0) {
    const int skip = status ? 1 : 0;  // an asynchronous recut that needs the host: skip
    st->u = 0.01;
    st->v = 2;
    st->res1 = st->res2 = st->q1 = 0.0;
    st->calc_hess = 1;
    st->done = skip;
    st->skip = skip;
    st->iters = 0;
    st->nhess = 0;
    st->seq = ph ? ph[0] : seq0;
    st->fin = 0;
    if (ph) __hip_atomic_store(rc_flag, (unsigned)ph[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// LM state (optimizers.cpp:436-441), the reduced-Hessian accumulator, the ring.
// ph (the scan graph, pipeline.cpp): the per-scan numbers k_ins_prep copied
// from host-mapped memory into DState::ph — the LM's first flag number
// replaces seq0, and the recut-done flag the margi prefix waits for
// (vg_ctx::d_sync[3]) is raised here (the recut's kernels have ended)
// fin (an asynchronous recut, map_recut): tras_opt's factor bookkeeping
// (k_factor_finish_dev's work: opt_state = factor index, the factors' eigen
// and cluster copies) over the whole grid, beside the LM state in workgroup 0 —
// one launch fewer on the chain
__global__ void __launch_bounds__(256) k_ba_init(BaState* st, double* __restrict__ hl, double* __restrict__ hl_part,
                                                 int nout, MpRing ring, int* __restrict__ mpring, int W,
                                                 const int* __restrict__ rc_status, int seq0, double* __restrict__ rpart,
                                                 int nrb, const int* __restrict__ ph, unsigned* __restrict__ rc_flag,
                                                 int fin, DevMap m, const int* __restrict__ fac_node,
                                                 double* __restrict__ fac_eig, Clu* __restrict__ fac_pcr) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x, gn = gridDim.x * blockDim.x;
  const int status = rc_status ? *rc_status : 0;
  if (fin && !status) {
    const int nf = m.counters[kCntFactors];
    for (int a = gt; a < nf; a += gn) {
      const int node = fac_node[a];
      m.hdr[node].opt_state = a;
      for (int j = 0; j < 12; j++) fac_eig[(size_t)a * 12 + j] = m.eig[(size_t)node * 12 + j];
      fac_pcr[a] = m.pcr_add[node];
    }
  }
  ba_init_common(gt, gn, blockIdx.x == 0, st, hl, hl_part, nout, ring, mpring, W, status, seq0, rpart, nrb, ph,
                 rc_flag);
}

// k_ba_init + the first LM iteration's k_ba_hess as one launch (the scan
// graph, vg_ctx::ba_init_hess): workgroups [0, G) the Hessian chunks, which
// also do tras_opt's bookkeeping for their own factors when `fin` (each
// factor's eigen system and cluster read from the map, copied to fac_eig /
// fac_pcr, opt_state = factor index: k_ba_init's loop), with the ring from
// the arguments; then the IMU factors' blocks; the last workgroup does the
// rest of k_ba_init (ba_init_common). Nothing in the launch reads the LM state
// the last workgroup writes: the chunks decide on the recut status, the same
// test k_ba_init's skip is.
__global__ void __launch_bounds__(kHessThreads) k_ba_init_hess(
    const int* __restrict__ nfp, int W, const int* __restrict__ fac_node, double* __restrict__ fac_eig,
    Clu* __restrict__ fac_pcr, const Clu* __restrict__ pcrs, const double* __restrict__ xs, double* __restrict__ part,
    int G, int nimu, const double* __restrict__ imurec, const int* __restrict__ imu_head,
    const double* __restrict__ bias, double* __restrict__ imuout, KClock* __restrict__ clk, BaState* st,
    double* __restrict__ hl, double* __restrict__ hl_part, int nout, MpRing ring, int* __restrict__ mpring,
    const int* __restrict__ rc_status, double* __restrict__ rpart, int nrb, const int* __restrict__ ph,
    unsigned* __restrict__ rc_flag, int fin, DevMap m, int seq0) {
  const int status = rc_status ? *rc_status : 0;
  if ((int)blockIdx.x == G + nimu) {
    ba_init_common(threadIdx.x, blockDim.x, true, st, hl, hl_part, nout, ring, mpring, W, status, seq0, rpart, nrb, ph,
                   rc_flag);
    return;
  }
  if (status) return;  // the recut needs the host: the LM is skipped (k_ba_init's skip)
  if ((int)blockIdx.x >= G) {  // IMU factors (give_evaluate, jac_enable)
    imu_factor_block(blockIdx.x - G, imurec, *imu_head, bias, xs, imuout);
    return;
  }
  __shared__ int s_mp[kMaxW];
  if ((int)threadIdx.x < kMaxW) s_mp[threadIdx.x] = ring.mp[threadIdx.x];
  const bool clk_on = clk && clk->on;  // in-kernel clock (vg_profile bit 2): the LM's iteration 0 slot
  const int clk_slot = clk_on ? (clk->scan * 8) & (kClkHRing - 1) : 0;
  if (clk_on && blockIdx.x == 0 && threadIdx.x == 0) {
    clk->h_t0[clk_slot] = (unsigned long long)wall_clock64();
    clk->h_exec[clk_slot] = 1;
  }
  __syncthreads();  // s_mp
  const int nf = *nfp;
  const int nchunk = (nf + hess_chunk(W) - 1) / hess_chunk(W);
  for (int ch = blockIdx.x; ch < nchunk; ch += G)
    hess_chunk_eval<false>(ch, nf, W, fac_node, fac_eig, fac_pcr, pcrs, s_mp, xs, part, nullptr, fac_eig, fac_pcr,
                           nullptr, fin ? m.eig : nullptr, fin ? m.pcr_add : nullptr, fin ? m.hdr : nullptr);
  if (clk_on && blockIdx.x < kClkHBlocks) {
    __syncthreads();
    if (threadIdx.x == 0) clk->h_tend[clk_slot][blockIdx.x] = (unsigned long long)wall_clock64();
  }
}

// ---- launches (vg_ba.h): the grids, block sizes, LDS sizes and arguments of
// one LM iteration's factor kernels, for ba.hip's ba_iter_kernels
int ba_factor_setup(vg_ctx* ctx) {
  const int lds = (int)hess_lds_bytes(ctx->cfg.win_size);
  VG_HIP(hipFuncSetAttribute((const void*)k_ba_hess, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  VG_HIP(hipFuncSetAttribute((const void*)k_ba_resid_hess, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  VG_HIP(hipFuncSetAttribute((const void*)k_ba_init_hess, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  return VG_OK;
}

void launch_ba_init(vg_ctx* ctx, const BaDev& d, const MpRing& ring, int seq0, bool fin) {
  const int W = ctx->cfg.win_size, L = 6 * W, nout = L * (L + 1) / 2 + L + 1;
  k_ba_init<<<fin ? 64 : 1, 256, 0, ctx->stream>>>(d.st, d.hl, ctx->ba.hout_part, nout, ring, d.mpring, W,
                                                    map_rc_status(ctx), seq0, d.rpart, kResidBlocks,
                                                    seq0 > 0 ? nullptr : ctx->st->ph, ctx->d_sync + 3, fin ? 1 : 0,
                                                    ctx->map, ctx->ba.fac_node, ctx->ba.fac_eig, ctx->ba.fac_pcr);
}

void launch_ba_init_hess(vg_ctx* ctx, const BaDev& d, const InitHessArg& ih) {
  const int W = ctx->cfg.win_size, nimu = W - 1, L = 6 * W, nout = L * (L + 1) / 2 + L + 1, G = ba_hess_grid(ctx);
  k_ba_init_hess<<<G + nimu + 1, kHessThreads, hess_lds_bytes(W), ctx->stream>>>(
      ctx->map.counters + kCntFactors, W, ctx->ba.fac_node, ctx->ba.fac_eig, ctx->ba.fac_pcr, ctx->map.pcrs, d.xs,
      d.part, G, nimu, d.imurec, &ctx->st->imu_head, d.bias, d.imuout, &ctx->st->clk, d.st, d.hl, ctx->ba.hout_part,
      nout, ih.ring, d.mpring, map_rc_status(ctx), d.rpart, kResidBlocks, ih.seq0 > 0 ? nullptr : ctx->st->ph,
      ih.seq0 > 0 ? nullptr : ctx->d_sync + 3, ih.fin, ctx->map, ih.seq0);
}

void launch_ba_hess(vg_ctx* ctx, const BaDev& d) {
  const int W = ctx->cfg.win_size, nimu = W - 1, G = ba_hess_grid(ctx);
  k_ba_hess<<<G + nimu, kHessThreads, hess_lds_bytes(W), ctx->stream>>>(
      ctx->map.counters + kCntFactors, W, ctx->ba.fac_node, ctx->ba.fac_eig, ctx->ba.fac_pcr, ctx->map.pcrs, d.mpring,
      d.xs, d.part, d.st, G, nimu, d.imurec, &ctx->st->imu_head, d.bias, d.imuout, &ctx->st->clk);
}

void launch_ba_hfinal(vg_ctx* ctx, const BaDev& d, double* out, const XchgArg& xa) {
  const int W = ctx->cfg.win_size, L = 6 * W, nout = L * (L + 1) / 2 + L + 1;
  k_ba_hfinal<<<(nout * 8 + 255) / 256, 256, 0, ctx->stream>>>(ctx->map.counters + kCntFactors, hess_chunk(W), nout,
                                                                 d.part, out, d.st, xa);
}

void launch_ba_resid(vg_ctx* ctx, const BaDev& d, const CtlArg& ctl) {
  const int W = ctx->cfg.win_size, nimu = W - 1, nrb = kResidBlocks;
  k_ba_resid<<<nrb + 1, kResidThreads, 0, ctx->stream>>>(
      ctx->map.counters + kCntFactors, W, ctx->ba.fac_node, ctx->map.pcr_fix, ctx->map.pcrs, d.mpring, d.xt,
      ctx->ba.fac_eig, ctx->ba.fac_pcr, d.rpart, d.st, nrb, nimu, d.imurec, &ctx->st->imu_head, d.bias, d.imures, ctl);
}

void launch_ba_resid_hess(vg_ctx* ctx, const BaDev& d, const CtlArg& ctl) {
  const int W = ctx->cfg.win_size, nimu = W - 1;
  k_ba_resid_hess<<<kRhChunkWg + 1 + nimu, kHessThreads, hess_lds_bytes(W), ctx->stream>>>(
      ctx->map.counters + kCntFactors, W, ctx->ba.fac_node, ctx->map.pcr_fix, ctx->map.pcrs, d.mpring, d.xt,
      ctx->ba.fac_eig, ctx->ba.fac_pcr, d.part, d.rpart, d.st, nimu, d.imurec, &ctx->st->imu_head, d.bias, d.imures,
      d.imuout, ctl);
}

void launch_ba_rsum(vg_ctx* ctx, const BaDev& d, const XchgArg& xa) {
  k_ba_rsum<<<1, 64, 0, ctx->stream>>>(kResidBlocks, d.rpart, d.st, xa);
}

void launch_ba_control(vg_ctx* ctx, const CtlArg& ctl) { k_ba_control<<<1, 256, 0, ctx->stream>>>(ctl); }

// ---- LiDAR factor passes for a host-driven LM (the initialisation's
// LI_BA_OptimizerGravity, optimizers.cpp:640-743): the same kernels, no IMU
// factors (the host evaluates those), synchronous.
// poses: W x kX frame states (R 9, p 3, v 3, bg 3, ba 3, g 3) by ord.
// out (Hessian pass): the 6W x 6W LiDAR Hessian as packed lower rows, then the
// 6W gradient, then the residual (acc_evaluate2 summed over the factors);
// out (residual pass): the residual (evaluate_only_residual, which also stores
// each factor's eigen system and merged cluster at these poses, as the
// reference's does).
// G: the Hessian pass's chunk workgroups, nrb: the residual pass's workgroups
// (ba_lidar_pass: the LM's own; vgx_ba_factors may choose others)
static int lidar_pass(vg_ctx* ctx, bool hessian, const double* poses, const int* mp_ring, int G, int nrb, double* out) {
  const int W = ctx->cfg.win_size;
  hipStream_t s = ctx->stream;
  BaDev d = carve(ctx);
  const int L = 6 * W, nout = L * (L + 1) / 2 + L + 1;
  BaState bs;
  memset(&bs, 0, sizeof(bs));
  bs.calc_hess = 1;
  int ring[kMaxW];
  for (int i = 0; i < kMaxW; i++) ring[i] = i < W ? mp_ring[i] : 0;
  double* h = ctx->h_stage;  // pinned staging
  memcpy(h, poses, (size_t)W * kX * sizeof(double));
  memcpy(h + W * kX, &bs, sizeof(bs));
  memcpy(h + W * kX + 8, ring, sizeof(ring));
  double* target = hessian ? d.xs : d.xt;
  VG_HIP(hipMemcpyAsync(target, h, (size_t)W * kX * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.st, h + W * kX, sizeof(bs), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.mpring, h + W * kX + 8, sizeof(ring), hipMemcpyHostToDevice, s));
  const int* nfp = ctx->map.counters + kCntFactors;
  if (hessian) {
    k_ba_hess<<<G, kHessThreads, hess_lds_bytes(W), s>>>(nfp, W, ctx->ba.fac_node, ctx->ba.fac_eig, ctx->ba.fac_pcr,
                                                        ctx->map.pcrs, d.mpring, d.xs, d.part, d.st, G, 0, d.imurec,
                                                        &ctx->st->imu_head, d.bias, d.imuout, nullptr);
    k_ba_hfinal<<<(nout * 8 + 255) / 256, 256, 0, s>>>(nfp, hess_chunk(W), nout, d.part, d.hl, d.st, XchgArg{});
    VG_HIP(hipGetLastError());
    VG_HIP(hipMemcpyAsync(h, d.hl, nout * sizeof(double), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));
    memcpy(out, h, nout * sizeof(double));
    return VG_OK;
  }
  k_ba_resid<<<nrb, 256, 0, s>>>(nfp, W, ctx->ba.fac_node, ctx->map.pcr_fix, ctx->map.pcrs, d.mpring, d.xt,
                                 ctx->ba.fac_eig, ctx->ba.fac_pcr, d.rpart, d.st, nrb, 0, d.imurec, &ctx->st->imu_head,
                                 d.bias, d.imures, CtlArg{});
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(h, d.rpart, nrb * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  double r = 0.0;
  for (int b = 0; b < nrb; b++) r += h[b];
  *out = r;
  return VG_OK;
}

int ba_lidar_pass(vg_ctx* ctx, bool hessian, const double* poses, const int* mp_ring, double* out) {
  return lidar_pass(ctx, hessian, poses, mp_ring, ba_hess_grid(ctx), kResidBlocks, out);
}

// Test-only (vgx_ba_factors): both LiDAR factor passes on given factors,
// through lidar_pass. nf factors, factor a the voxel of node fac_node[a]; the
// nn nodes `nodes` carry their window clusters by physical slot (clus: nn x W x
// 10 — P xx xy xz yy yz zz, v 3, N — written to map.pcrs[node * W + slot]) and
// their fixed cluster (fix: nn x 10, to map.pcr_fix). The residual pass runs at
// `poses` (W x kX) with ring mp_ring and leaves fac_eig / fac_pcr as tras_opt
// hands them to the Hessian pass, which then runs at the same poses. G / nrb:
// the passes' workgroup counts, 0 for the LM's own. Out: hl (packed lower
// Hessian, gradient, residual), the residual pass's residual, fac_eig (nf x
// 12) and fac_pcr (nf x 10). The context must not be stepped afterwards.
int ba_factors_test(vg_ctx* ctx, int nf, const int* fac_node, int nn, const int* nodes, const double* clus,
                    const double* fix, const double* poses, const int* mp_ring, int G, int nrb, double* hl,
                    double* resid, double* eig, double* pcr) {
  const int W = ctx->cfg.win_size;
  if (sharded(ctx)) return VG_E_STATE;
  if (nf < 0 || nf > ctx->ba.cap_f || nn < 0 || nn > ctx->map.cap_nodes) return VG_E_ARG;
  if (G < 0 || G > kHessGridMax || nrb < 0 || nrb > kResidBlocks) return VG_E_ARG;
  for (int i = 0; i < W; i++)
    if (mp_ring[i] < 0 || mp_ring[i] >= W) return VG_E_ARG;
  std::vector<char> given((size_t)ctx->map.cap_nodes, 0);
  for (int k = 0; k < nn; k++) {
    if (nodes[k] < 0 || nodes[k] >= ctx->map.cap_nodes) return VG_E_ARG;
    given[nodes[k]] = 1;
  }
  for (int a = 0; a < nf; a++)  // a factor reads only clusters this call wrote
    if (fac_node[a] < 0 || fac_node[a] >= ctx->map.cap_nodes || !given[fac_node[a]]) return VG_E_ARG;
  hipStream_t s = ctx->stream;
  auto clu_of = [](const double* c) {
    Clu o;
    for (int i = 0; i < 6; i++) o.P[i] = c[i];
    for (int i = 0; i < 3; i++) o.v[i] = c[6 + i];
    o.N = (int)c[9];
    o.pad = 0;
    return o;
  };
  std::vector<Clu> hc((size_t)nn * (W + 1));
  for (int k = 0; k < nn; k++) {
    Clu* row = &hc[(size_t)k * (W + 1)];
    for (int j = 0; j < W; j++) row[j] = clu_of(&clus[((size_t)k * W + j) * 10]);
    row[W] = clu_of(&fix[(size_t)k * 10]);
    VG_HIP(hipMemcpyAsync(ctx->map.pcrs + (size_t)nodes[k] * W, row, (size_t)W * sizeof(Clu), hipMemcpyHostToDevice, s));
    VG_HIP(hipMemcpyAsync(ctx->map.pcr_fix + nodes[k], row + W, sizeof(Clu), hipMemcpyHostToDevice, s));
  }
  if (nf > 0) VG_HIP(hipMemcpyAsync(ctx->ba.fac_node, fac_node, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(ctx->map.counters + kCntFactors, &nf, sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(hipStreamSynchronize(s));
  VG_TRY(lidar_pass(ctx, false, poses, mp_ring, 0, nrb ? nrb : kResidBlocks, resid));
  std::vector<Clu> fp((size_t)nf);
  if (nf > 0) {
    VG_HIP(hipMemcpyAsync(eig, ctx->ba.fac_eig, (size_t)nf * 12 * sizeof(double), hipMemcpyDeviceToHost, s));
    VG_HIP(hipMemcpyAsync(fp.data(), ctx->ba.fac_pcr, (size_t)nf * sizeof(Clu), hipMemcpyDeviceToHost, s));
    VG_HIP(hipStreamSynchronize(s));
  }
  for (int a = 0; a < nf; a++) {
    for (int i = 0; i < 6; i++) pcr[(size_t)a * 10 + i] = fp[a].P[i];
    for (int i = 0; i < 3; i++) pcr[(size_t)a * 10 + 6 + i] = fp[a].v[i];
    pcr[(size_t)a * 10 + 9] = (double)fp[a].N;
  }
  return lidar_pass(ctx, true, poses, mp_ring, G ? G : ba_hess_grid(ctx), 0, hl);
}

// Test-only (vgx_ba_control): one k_ba_control launch (the LM bookkeeping,
// ba_control_body) on a given LM state — sd: u, v, res1, res2, q1; si:
// calc_hess, done, iters, nhess, fin, skip — the IMU residuals imures (W-1),
// nrb <= kResidBlocks residual partials, the window states xs, the trial
// states xt and the bias records. Returns the state, xs and the bias records
// after the launch. The context must not be stepped afterwards.
int ba_control_test(vg_ctx* ctx, double* sd, int* si, const double* imures, const double* rpart, int nrb, double* xs,
                    const double* xt, double* bias) {
  const int W = ctx->cfg.win_size, nimu = W - 1, L = 6 * W, nl = L * (L + 1) / 2;
  if (sharded(ctx)) return VG_E_STATE;
  if (nrb < 0 || nrb > kResidBlocks) return VG_E_ARG;
  hipStream_t s = ctx->stream;
  BaDev d = carve(ctx);
  BaState bs;
  memset(&bs, 0, sizeof(bs));
  bs.u = sd[0];
  bs.v = sd[1];
  bs.res1 = sd[2];
  bs.res2 = sd[3];
  bs.q1 = sd[4];
  bs.calc_hess = si[0];
  bs.done = si[1];
  bs.iters = si[2];
  bs.nhess = si[3];
  bs.fin = si[4];
  bs.skip = si[5];
  VG_HIP(hipMemcpyAsync(d.st, &bs, sizeof(bs), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.imures, imures, (size_t)nimu * sizeof(double), hipMemcpyHostToDevice, s));
  if (nrb > 0) VG_HIP(hipMemcpyAsync(d.rpart, rpart, (size_t)nrb * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.xs, xs, (size_t)W * kX * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.xt, xt, (size_t)W * kX * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.bias, bias, (size_t)nimu * 12 * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipStreamSynchronize(s));
  CtlArg ctl{W, nimu, nrb, nl + L, ctx->cfg.imu_coef, d.hl, d.imuout, d.imures, d.rpart, d.xs, d.xt, d.bias, d.st,
             ctx->d_pub, nullptr, 0, ctx->map.counters + kCntErr};
  k_ba_control<<<1, 256, 0, s>>>(ctl);
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(&bs, d.st, sizeof(bs), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(xs, d.xs, (size_t)W * kX * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(bias, d.bias, (size_t)nimu * 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  sd[0] = bs.u;
  sd[1] = bs.v;
  sd[2] = bs.res1;
  sd[3] = bs.res2;
  sd[4] = bs.q1;
  si[0] = bs.calc_hess;
  si[1] = bs.done;
  si[2] = bs.iters;
  si[3] = bs.nhess;
  si[4] = bs.fin;
  si[5] = bs.skip;
  return VG_OK;
}

// Test-only (vgx_ba_imu): the IMU factor workgroups of the LM's three factor
// passes on given records, through the launches the LM uses. The W-1 records
// (kBaImuRec each) go to ring slots (head + k) % kMaxWin of DState::imurec —
// every other slot holds `poison` — with imu_head = head; the bias records
// ((W-1) x 12), xs and xt (W x kX) as given; the factor count is 0, so the
// LiDAR workgroups have nothing to do. (a) k_ba_hess at xs, (b) k_ba_resid at
// xt, (c) k_ba_resid_hess at xt; (b) and (c) with an empty CtlArg (err = null:
// no bookkeeping runs; the LM state stays live, done = 0, because a finished
// state makes both kernels return before their IMU lanes). imuout and imures
// are filled with `poison` before each pass and returned whole (kMaxW x 931,
// kMaxW): rows from W-1 on must still hold it. The context must not be stepped
// afterwards.
int ba_imu_test(vg_ctx* ctx, int head, const double* rec, const double* bias, const double* xs, const double* xt,
                double poison, double* imuout_hess, double* imures_resid, double* imuout_rh, double* imures_rh) {
  const int W = ctx->cfg.win_size, nimu = W - 1;
  if (sharded(ctx)) return VG_E_STATE;
  if (head < 0 || head >= kMaxWin || nimu < 1 || nimu > kMaxW) return VG_E_ARG;
  hipStream_t s = ctx->stream;
  BaDev d = carve(ctx);
  DState* st = ctx->st;
  std::vector<double> ring((size_t)kMaxWin * kImuRec, poison), po((size_t)kMaxW * 931, poison);
  for (int k = 0; k < nimu; k++)
    memcpy(&ring[(size_t)((head + k) % kMaxWin) * kImuRec], &rec[(size_t)k * kImuRec], kImuRec * sizeof(double));
  BaState bs;
  memset(&bs, 0, sizeof(bs));
  bs.calc_hess = 1;
  const int zero = 0, ringmp[kMaxW] = {0};
  VG_HIP(hipMemcpy(st->imurec, ring.data(), ring.size() * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(&st->imu_head, &head, sizeof(int), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(d.bias, bias, (size_t)nimu * 12 * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(d.xs, xs, (size_t)W * kX * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(d.xt, xt, (size_t)W * kX * sizeof(double), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(d.st, &bs, sizeof(bs), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(d.mpring, ringmp, sizeof(ringmp), hipMemcpyHostToDevice));
  VG_HIP(hipMemcpy(ctx->map.counters + kCntFactors, &zero, sizeof(int), hipMemcpyHostToDevice));
  auto arm = [&]() -> int {  // (the context's stream does not wait for the null stream)
    VG_HIP(hipMemcpy(d.imuout, po.data(), (size_t)kMaxW * 931 * sizeof(double), hipMemcpyHostToDevice));
    VG_HIP(hipMemcpy(d.imures, po.data(), (size_t)kMaxW * sizeof(double), hipMemcpyHostToDevice));
    VG_HIP(hipDeviceSynchronize());
    return VG_OK;
  };
  auto fetch = [&](double* out, double* res) -> int {
    VG_HIP(hipGetLastError());
    VG_HIP(hipStreamSynchronize(s));
    if (out) VG_HIP(hipMemcpy(out, d.imuout, (size_t)kMaxW * 931 * sizeof(double), hipMemcpyDeviceToHost));
    if (res) VG_HIP(hipMemcpy(res, d.imures, (size_t)kMaxW * sizeof(double), hipMemcpyDeviceToHost));
    return VG_OK;
  };
  VG_TRY(arm());
  launch_ba_hess(ctx, d);
  VG_TRY(fetch(imuout_hess, nullptr));
  VG_TRY(arm());
  launch_ba_resid(ctx, d, CtlArg{});
  VG_TRY(fetch(nullptr, imures_resid));
  VG_TRY(arm());
  launch_ba_resid_hess(ctx, d, CtlArg{});
  VG_TRY(fetch(imuout_rh, imures_rh));
  return VG_OK;
}

// the factors' eigenvectors (column 0 = the plane normal) and count, host copy
int ba_factor_normals(vg_ctx* ctx, std::vector<double>& normals) {
  hipStream_t s = ctx->stream;  // stream-ordered: the context stream is non-blocking
  VG_HIP(hipMemcpyAsync(ctx->h_pinned, ctx->map.counters + kCntFactors, sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  const int nf = ctx->h_pinned[0];
  std::vector<double> e((size_t)nf * 12);
  if (nf > 0) VG_HIP(hipMemcpyAsync(e.data(), ctx->ba.fac_eig, e.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  normals.resize((size_t)nf * 3);
  for (int a = 0; a < nf; a++)
    for (int k = 0; k < 3; k++) normals[(size_t)a * 3 + k] = e[(size_t)a * 12 + 3 + k * 3];  // U(k, 0), row-major
  return VG_OK;
}

}  // namespace vg
