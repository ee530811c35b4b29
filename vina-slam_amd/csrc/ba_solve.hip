// ba_solve.hip — the LM's dense step: k_ba_prep
// assembles, gauges, damps and pivots the 15W x 15W system of
// LI_BA_Optimizer::damping_iter (optimizers.cpp:454-466), k_ba_solve factors it
// in LDS and forms the trial state and q1 (466-478). Apart from BaState the two
// share nothing with the factor passes (ba_factor.hip); ba.hip launches them
// through launch_prep_solve (vg_ba.h).
#include "vg_ba.h"

namespace vg {

// packed lower storage of the n x n system (Hcalc)
__device__ __forceinline__ int lo(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// ---- LDS tile store of the permuted system: lower block triangle of 16x16
// fp64 tiles, tile (I,J) (I >= J) at I(I+1)/2 + J, element (r,c) at
// r*16 + (c ^ r): rows and columns of a tile both read conflict-free, which
// the MFMA operand loads (16 rows of one column per lane group) need.
__device__ __forceinline__ int tix(int I, int J) { return I * (I + 1) / 2 + J; }
__device__ __forceinline__ int tel(int r, int c) { return r * 16 + (c ^ r); }

__device__ __forceinline__ double bcast(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo32 = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi32 = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi32 << 32) | (unsigned int)lo32);
}


// broadcast lane qd of every quad (DPP quad_perm) — qd must fold to a constant
template <int Q>
__device__ __forceinline__ double quad_bcast_c(double v) {
  const long long b = __double_as_longlong(v);
  const int lo32 = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), Q * 0x55, 0xf, 0xf, false);
  const int hi32 = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), Q * 0x55, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi32 << 32) | (unsigned int)lo32);
}
__device__ __forceinline__ double quad_bcast(double v, int qd) {
  switch (qd) {
    case 0: return quad_bcast_c<0>(v);
    case 1: return quad_bcast_c<1>(v);
    case 2: return quad_bcast_c<2>(v);
    default: return quad_bcast_c<3>(v);
  }
}

// one assembled lower entry (R >= C) of the 15W x 15W system in the host
// loop's accumulation order (divide_thread 215-222: IMU factors k ascending,
// x imu_coef, then hess_plus 171-179 adds the LiDAR 6x6 blocks)
__device__ __forceinline__ double asm_entry(int R, int C, int nimu, double imu_coef, const double* hl,
                                            const double* imuout, int L) {
  const int bR = R / 15, bC = C / 15, rR = R % 15, rC = C % 15;
  double v = 0.0;
  for (int k = bR > 0 ? bR - 1 : 0; k <= bC && k < nimu; k++)
    v += imuout[(size_t)k * 931 + (R - 15 * k) * 30 + (C - 15 * k)];
  v *= imu_coef;
  if (rR < 6 && rC < 6) {
    const int lr = bR * 6 + rR, lc = bC * 6 + rC;
    v += hl[lr * (lr + 1) / 2 + lc];
  }
  return v;
}
__device__ __forceinline__ double asm_grad(int t, int nimu, double imu_coef, const double* hl, const double* imuout,
                                           int L) {
  const int b = t / 15, r = t % 15;
  double v = 0.0;
  if (b >= 1 && b - 1 < nimu) v += imuout[(size_t)(b - 1) * 931 + 900 + r + 15];
  if (b < nimu) v += imuout[(size_t)b * 931 + 900 + r];
  v *= imu_coef;
  if (r < 6) v += hl[L * (L + 1) / 2 + b * 6 + r];
  return v;
}

// Wide preparation of the permuted, gauged, damped system: one block per
// 16x16 tile of the lower block triangle. Every block ranks the damped
// diagonal (Eigen's LDLT is left-looking, so its pivot order is the
// descending order of |diag|, see the oracle's ldlt_solve) and writes its
// tile of P A P^T to the tile image; on Hessian iterations it also stores
// the assembled entries it visits (each lower entry exactly once) for the
// damping-only retries. Block 0 writes the permuted right-hand side.
// The gauge frame's 15 variables (optimizers.cpp:460-463: unit rows and
// columns, zero gradient) are decoupled from the rest, so wherever Eigen's
// pivot order puts them their elimination changes nothing and their solution
// is 0: they are left out of the factored system (n - 15 unknowns).
__global__ void __launch_bounds__(256) k_ba_prep(int W, int nimu, double imu_coef, const double* __restrict__ hl,
                                                 const double* __restrict__ imuout, double* __restrict__ Hcalc,
                                                 double* __restrict__ Jcalc, double* __restrict__ timg,
                                                 double* __restrict__ bvec, double* __restrict__ dvec,
                                                 double* __restrict__ jvec, int* __restrict__ ipg,
                                                 BaState* __restrict__ st, int structural, int xworld,
                                                 int* __restrict__ xerr) {
  if (st->done) return;
  // sharded: `hl` is the all-reduced exchange frame; a guard mismatch ends the
  // LM (error bit 32: the scan fails with VG_E_STATE)
  if (xworld > 0 && !xchg_ok(hl, 3 * W * (6 * W + 1) + 6 * W + 1 + 2, xworld)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      atomicOr(xerr, 32);
      st->done = 1;
    }
    return;
  }
  constexpr int kN = kMaxNB * kTile;
  __shared__ double Dv[kN], Jg[kN];
  __shared__ int ip[kN], perm[kN];
  __shared__ int s_tie;
  const int n = 15 * W, L = 6 * W, m = n - 15, NB = (m + kTile - 1) / kTile, N = NB * kTile;
  const int tid = threadIdx.x, q = blockIdx.x;
  const bool calc = st->calc_hess != 0;
  const double u = st->u;
  if (tid == 0) s_tie = 0;
  for (int t = tid; t < n; t += blockDim.x)
    Dv[t] = t < 15 ? 1.0 : (calc ? asm_entry(t, t, nimu, imu_coef, hl, imuout, L) : Hcalc[lo(t, t)]);
  __syncthreads();
  for (int i = 15 + tid; i < n; i += blockDim.x) {
    if (structural) {  // v / bg / ba of frames 1..W-1 first (frame order), then their poses
      const int j = i / 15, v = i - 15 * j;
      ip[v >= 6 ? 9 * (j - 1) + (v - 6) : 9 * (W - 1) + 6 * (j - 1) + v] = i;
      continue;
    }
    // Eigen's order: rank of |D + u D| descending (equal entries: below)
    const unsigned long long ki = (unsigned long long)__double_as_longlong(fabs(Dv[i] + u * Dv[i]));
    int c = 0, tie = 0;
    for (int j = 15; j < n; j++) {
      const unsigned long long kj = (unsigned long long)__double_as_longlong(fabs(Dv[j] + u * Dv[j]));
      c += kj > ki;
      tie |= (kj == ki && j != i);
    }
    ip[c] = i;
    if (tie) s_tie = 1;
  }
  __syncthreads();
  // Equal entries: Eigen takes the first largest of the remaining positions
  // and transposes it with position k, so which of two equal entries comes
  // first depends on the transpositions before (the gauge frame's 1 + u among
  // them). Rare (exact fp64 equality): one lane replays the selection over all
  // n entries and keeps the order of the factored ones.
  if (!structural && s_tie) {
    if (tid == 0) {
      for (int t = 0; t < n; t++) perm[t] = t;
      int o = 0;
      for (int k = 0; k < n; k++) {
        int p = k;
        double best = fabs(Dv[perm[k]] + u * Dv[perm[k]]);
        for (int i = k + 1; i < n; i++) {
          const double a = fabs(Dv[perm[i]] + u * Dv[perm[i]]);
          if (a > best) {
            best = a;
            p = i;
          }
        }
        const int e = perm[p];
        perm[p] = perm[k];
        perm[k] = e;
        if (e >= 15) ip[o++] = e;
      }
    }
    __syncthreads();
  }
  int TI = 0;
  while ((TI + 1) * (TI + 2) / 2 <= q) TI++;
  const int TJ = q - TI * (TI + 1) / 2;
  for (int e = tid; e < 256; e += blockDim.x) {
    const int r = e >> 4, c = e & 15, R = TI * 16 + r, C = TJ * 16 + c;
    double v;
    if (R >= m || C >= m) {
      v = (R == C) ? 1.0 : 0.0;
    } else {
      const int pr = ip[R], pc = ip[C], a = pr > pc ? pr : pc, bb = pr > pc ? pc : pr;
      const double raw = calc ? asm_entry(a, bb, nimu, imu_coef, hl, imuout, L) : Hcalc[lo(a, bb)];
      if (calc && R >= C) Hcalc[lo(a, bb)] = raw;
      v = (pr == pc) ? Dv[pr] + u * Dv[pr] : raw;
    }
    timg[(size_t)q * 256 + tel(r, c)] = v;
  }
  if (q == 0) {
    // residual1 of divide_thread at the current state (optimizers.cpp:454), on
    // a lane the gradient loop below leaves idle (n < 256)
    if (calc && tid == (int)blockDim.x - 1) {
      double r = 0.0;
      for (int k = 0; k < nimu; k++) r += imuout[(size_t)k * 931 + 930];
      r *= imu_coef * 0.5;
      r += hl[L * (L + 1) / 2 + L];
      st->res1 = r;
    }
    for (int t = tid; t < n; t += blockDim.x) {
      const double raw = calc ? asm_grad(t, nimu, imu_coef, hl, imuout, L) : Jcalc[t];
      if (calc) Jcalc[t] = raw;
      Jg[t] = t < 15 ? 0.0 : raw;
      dvec[t] = Dv[t];
      if (t < m) ipg[t] = ip[t];
    }
    __syncthreads();
    for (int t = tid; t < N; t += blockDim.x) bvec[t] = t < m ? -Jg[ip[t]] : 0.0;
    for (int t = tid; t < n; t += blockDim.x) jvec[t] = Jg[t];
  }
}

// 4x4 symmetric sweep in registers, pivots in index order: b -> -b^-1. A
// pivot with |d| <= DBL_MIN contributes nothing (Eigen's LDLT leaves such a
// column undivided and its solve takes D^+, so that unknown's share is 0).
__device__ __forceinline__ void sweep4(double (&b)[4][4]) {
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const double d = b[p][p];
    double ip = __builtin_amdgcn_rcp(d);
    ip = fma(ip, fma(-d, ip, 1.0), ip);
    ip = fabs(d) > 2.2250738585072014e-308 ? ip : 0.0;
    double c[4];
#pragma unroll
    for (int i = 0; i < 4; i++) c[i] = b[i][p] * ip;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j <= i; j++)
        if (i != p && j != p) {
          b[i][j] = fma(-c[i], b[p][j], b[i][j]);
          b[j][i] = b[i][j];
        }
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i != p) b[i][p] = b[p][i] = c[i];
    b[p][p] = -ip;
  }
}
// v_i for a lane-varying i in [0, 4): flat selects (no divergent branches)
__device__ __forceinline__ double sel4(double v0, double v1, double v2, double v3, int i) {
  double r = v3;
  r = i == 2 ? v2 : r;
  r = i == 1 ? v1 : r;
  r = i == 0 ? v0 : r;
  return r;
}
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int C>
__device__ __forceinline__ double dpp_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo32 = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), C, 0xf, 0xf, false);
  const int hi32 = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), C, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi32 << 32) | (unsigned int)lo32);
}
// sum over the 16 lanes of each row (lanes with equal lane >> 4): DPP
// quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror; every lane
// adds the same pairs, so all 16 hold the same bits
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  return v;
}
// sum over lanes l, l^16, l^32, l^48 (the four rows): gfx950's
// v_permlane16_swap / v_permlane32_swap, (even + odd) then (low + high)
__device__ __forceinline__ double xrow_sum(double v) {
  long long b = __double_as_longlong(v);
  auto lo = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
  auto hi = __builtin_amdgcn_permlane16_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  v = __longlong_as_double(((long long)hi[0] << 32) | lo[0]) + __longlong_as_double(((long long)hi[1] << 32) | lo[1]);
  b = __double_as_longlong(v);
  lo = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
  hi = __builtin_amdgcn_permlane32_swap((unsigned)(b >> 32), (unsigned)(b >> 32), false, false);
  return __longlong_as_double(((long long)hi[0] << 32) | lo[0]) + __longlong_as_double(((long long)hi[1] << 32) | lo[1]);
}

// Block LDL^T solve of the prepared system P A P^T y = P b in one workgroup
// (the LDLT the reference runs at optimizers.cpp:466, pivot order from
// k_ba_prep: Eigen's, descending |diag|). 16 x 16 tiles, no further pivoting:
//   P A P^T = L D L^T with D = diag(S_KK) (the Schur-complement diagonal
//   tiles) and L_IK = S_IK S_KK^-1, so
//   forward  y_I -= L_IK y_K (rides along the trailing update),
//   diagonal w_K  = S_KK^-1 y_K,
//   backward x_K  = w_K - S_KK^-1 sum_{J>K} S_JK^T x_J.
// A diagonal tile is inverted in registers by one wave as a 4-column block
// sweep (Gauss-Jordan on the symmetric tile): each step inverts its 4 x 4
// pivot block (sweep4, redundantly per lane), exchanges one 16 x 4 panel
// through LDS and applies the rank-4 update with one v_mfma_f64_16x16x4; the
// pivot rows/columns are written directly (not as the difference of two
// rounded products). Tiles live in the D layout of that MFMA (lane (c, q)
// holds rows q + 4g of column c), which is also the layout a tile has after a
// trailing update, so the factor never leaves registers between the update
// and the inversion.
// Phase K (one workgroup barrier each): wave 0 computes -L_{K+1,K}^T, brings
// tile (K+1, K+1) and y_{K+1} up to date and inverts the tile (the critical
// chain); the twelve waves on the other three SIMDs take the rest of panel K's
// trailing update, row pieces of up to four tiles that each compute their
// row's -L_IK^T = S_KK^-1 S_IK^T once in registers (that transposed product
// is exactly the MFMA A-operand layout of the update), plus w_K. The backward
// substitution keeps acc_J in wave J's registers: one barrier per tile row.
// Rounding differs from Eigen's sequential recurrences (tolerance level).
__global__ void __launch_bounds__(1024) k_ba_solve(int W, int nimu, const double* __restrict__ timg,
                                                  const double* __restrict__ bvec, const double* __restrict__ dvec,
                                                  const double* __restrict__ jvec, const int* __restrict__ ipg,
                                                  const double* __restrict__ xs, double* __restrict__ xt,
                                                  double* __restrict__ bias, double* __restrict__ dxi_out,
                                                  BaState* __restrict__ st, KClock* __restrict__ clk) {
  if (st->done) return;
  const unsigned long long clk0 = wall_clock64();  // vg_profile bit 2 (KClock)
  extern __shared__ __attribute__((aligned(16))) double T[];
  constexpr int kN = kMaxNB * kTile;
  __shared__ double Jv[kN], Dv[kN], yv[kN], wv[kN], xv[kN], col[kN], sP[64], sG[64];
  __shared__ int ip[kN];
  const int n = 15 * W, m = n - 15;  // the gauge frame's unknowns are not factored (k_ba_prep)
  const int NB = (m + kTile - 1) / kTile, N = NB * kTile;
  const int ntile = NB * (NB + 1) / 2;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int cc = lane & 15, rq = lane >> 4;
  const double u = st->u;
#ifdef VG_PROBE
  __shared__ unsigned s_tmax;
  if (tid == 0) s_tmax = 0;
#endif
  VG_PROBE_BEGIN();

  // -S^-1 of a diagonal tile held in registers (D layout), on one wave
  auto diag = [&](v4d a) __attribute__((always_inline)) {
    const int cq = cc & 3, cb = cc >> 2;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      sP[rq * 16 + cc] = a[k];  // rows 4k..4k+3 of the tile
      wave_lds_sync();
      double b[4][4], p[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int j = 0; j < 4; j++) b[i][j] = sP[i * 16 + 4 * k + j];
        p[i] = sP[i * 16 + cc];  // A(4k+i, c) = A(c, 4k+i)
      }
      sweep4(b);  // -B^-1
      double bc[4];
#pragma unroll
      for (int j = 0; j < 4; j++) bc[j] = sel4(b[j][0], b[j][1], b[j][2], b[j][3], rq);  // -B^-1(j, q)
      double gq = 0.0;  // -G(c, q), G = A(:, K) B^-1
#pragma unroll
      for (int j = 0; j < 4; j++) gq = fma(p[j], bc[j], gq);
      const bool inK = cb == k;
      sG[cc * 4 + rq] = -gq;
      a = __builtin_amdgcn_mfma_f64_16x16x4f64(inK ? 0.0 : gq, inK ? 0.0 : a[k], a, 0, 0, 0);  // A_OO -= G A_KO
      wave_lds_sync();
      double go[4];
#pragma unroll
      for (int g = 0; g < 4; g++) go[g] = sG[(rq + 4 * g) * 4 + cq];
#pragma unroll
      for (int g = 0; g < 4; g++)
        if (g != k) a[g] = inK ? go[g] : a[g];  // A_OK <- G
      a[k] = inK ? sel4(bc[0], bc[1], bc[2], bc[3], cq) : -gq;  // A_KK <- -B^-1, A_KO <- B^-1 A_KO = G^T
    }
    return a;
  };
  // -L_IK^T = S_KK^-1 S_IK^T as (-S_KK^-1) S_IK^T: lane (c, q) reg g =
  // -L_IK(c, q + 4g). tv[ks] = (-S_KK^-1)(c, 4ks + q) (from the tile store, or
  // wave 0's registers: the inverse is symmetric, so its D-layout register g
  // is that A operand), sv[ks] = S_IK(c, 4ks + q). Two accumulation chains.
  auto mk_gt = [&](const v4d& tv, const v4d& sv) __attribute__((always_inline)) {
    const v4d z = v4d{0.0, 0.0, 0.0, 0.0};
    v4d g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[0], sv[0], z, 0, 0, 0);
    v4d g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[2], sv[2], z, 0, 0, 0);
    g1 = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[1], sv[1], g1, 0, 0, 0);
    g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(tv[3], sv[3], g2, 0, 0, 0);
    return g1 + g2;
  };
  // operand columns of a tile: lane (c, q) reg ks = tile(c, 4ks + q)
  auto ld_ops = [&](const double* t) __attribute__((always_inline)) {
    v4d o;
#pragma unroll
    for (int ks = 0; ks < 4; ks++) o[ks] = t[tel(cc, 4 * ks + rq)];
    return o;
  };
  // acc -= L_IK S_JK^T, sj = ld_ops(S_JK); two accumulation chains
  auto tile_upd = [&](v4d acc, const v4d& gt, const v4d& sj) __attribute__((always_inline)) {
    v4d a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(gt[2], sj[2], v4d{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gt[0], sj[0], acc, 0, 0, 0);
    a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(gt[3], sj[3], a2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gt[1], sj[1], acc, 0, 0, 0);
    return acc + a2;
  };
  // y_I -= L_IK y_K
  auto y_upd = [&](const v4d& gt, int K, int I) __attribute__((always_inline)) {
    double s = 0.0;
#pragma unroll
    for (int g = 0; g < 4; g++) s = fma(gt[g], yv[16 * K + rq + 4 * g], s);
    s = xrow_sum(s);
    if (rq == 0) yv[16 * I + cc] += s;
  };
  // w_K = S_KK^-1 y_K (into wv, and into xv as well for the last tile row)
  auto w_job = [&](int K, bool last) __attribute__((always_inline)) {
    const double* Ti = &T[tix(K, K) * 256];
    const double yk = yv[16 * K + cc];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const double s = -row16_sum(Ti[tel(rq + 4 * g, cc)] * yk);
      if (cc == 0) {
        wv[16 * K + rq + 4 * g] = s;
        if (last) xv[16 * K + rq + 4 * g] = s;
      }
    }
  };
  auto ld_tile = [&](const double* t) __attribute__((always_inline)) {
    v4d a;
#pragma unroll
    for (int g = 0; g < 4; g++) a[g] = t[tel(rq + 4 * g, cc)];
    return a;
  };
  auto st_tile = [&](double* t, const v4d& a) __attribute__((always_inline)) {
#pragma unroll
    for (int g = 0; g < 4; g++) t[tel(rq + 4 * g, cc)] = a[g];
  };
  // an all-zero tile (wave-uniform): its updates are exact no-ops and are
  // skipped. In the structural order (k_ba_prep) the v/bg/ba tiles far from the
  // diagonal are zero and stay zero (the IMU factors couple adjacent frames only)
  auto zero_tile = [&](const v4d& o) __attribute__((always_inline)) {
    const bool nz = o[0] != 0.0 || o[1] != 0.0 || o[2] != 0.0 || o[3] != 0.0;
    return __ballot(nz) == 0;
  };

  // wave 0 takes tile (0, 0) straight from the image and inverts it while the
  // other waves fill the tile store and the vectors
  v4d tinv;  // wave 0: -S_KK^-1 of the current panel, kept in registers
  if (wave == 0) {
    __builtin_amdgcn_s_setprio(3);  // the critical chain issues first on its SIMD
    tinv = diag(ld_tile(timg));
    st_tile(T, tinv);
  } else {
    const double2* src = reinterpret_cast<const double2*>(timg);
    double2* dst = reinterpret_cast<double2*>(T);
    for (int t = 128 + tid - 64; t < ntile * 128; t += nt - 64) dst[t] = src[t];
    for (int t = tid - 64; t < N; t += nt - 64) yv[t] = bvec[t];
    for (int t = tid - 64; t < n; t += nt - 64) {
      Dv[t] = dvec[t];
      Jv[t] = jvec[t];
      if (t < m) ip[t] = ipg[t];
    }
  }
  __syncthreads();
  VG_PROBE_MARK(3);

  // -L_IK^T of a phase goes to tile (I, K) in the next phase, once no wave
  // reads S_IK any more (the backward substitution needs L, not S): at most
  // two rows per wave and phase (wave-uniform bookkeeping)
  v4d pg0, pg1;
  int pt0 = -1, pt1 = -1;
  auto flush = [&]() __attribute__((always_inline)) {
    if (pt0 >= 0) st_tile(&T[pt0 * 256], pg0);
    if (pt1 >= 0) st_tile(&T[pt1 * 256], pg1);
    pt0 = pt1 = -1;
  };
  auto pend = [&](const v4d& gt, int t) __attribute__((always_inline)) {
    if (pt0 < 0) {
      pg0 = gt;
      pt0 = t;
    } else {
      pg1 = gt;
      pt1 = t;
    }
  };
  for (int K = 0; K + 1 < NB; K++) {
    flush();
    if (wave == 0) {
      const v4d s1 = ld_ops(&T[tix(K + 1, K) * 256]);
      v4d a = ld_tile(&T[tix(K + 1, K + 1) * 256]);
      const v4d gt = mk_gt(tinv, s1);
      a = tile_upd(a, gt, s1);
      pend(gt, tix(K + 1, K));
      VG_PROBE_MARK(10);
      tinv = diag(a);
      st_tile(&T[tix(K + 1, K + 1) * 256], tinv);
      VG_PROBE_MARK(11);
    } else if (wave & 3) {
      // the twelve waves off wave 0's SIMD: job 0 = w_K and y_{K+1}, then row
      // pieces of up to four tiles (the three other waves on wave 0's SIMD
      // stay idle: as helpers they slowed the critical chain more than they
      // shortened the trailing update, phase clocks 34.1 -> 35.5 us)
#ifdef VG_PROBE
      const unsigned long long tj0 = wall_clock64();
#endif
      const int wk = wave - (wave >> 2) - 1;
      constexpr int nwk = 12;
      const v4d tv = ld_ops(&T[tix(K, K) * 256]);
      int q = 0;
      if (q++ == wk) {
        w_job(K, false);
        y_upd(mk_gt(tv, ld_ops(&T[tix(K + 1, K) * 256])), K, K + 1);
      }
      for (int I = K + 2; I < NB; I++)
        for (int J0 = K + 1; J0 <= I; J0 += 4) {
          if (q++ % nwk != wk) continue;
          const v4d sik = ld_ops(&T[tix(I, K) * 256]);
          if (zero_tile(sik)) continue;  // L_IK = 0: no update, no y update, the tile stays 0 (= -L_IK^T)
          const v4d gt = mk_gt(tv, sik);
          const int J1 = J0 + 4 < I + 1 ? J0 + 4 : I + 1;
          for (int J = J0; J < J1; J++) {
            const v4d sjk = ld_ops(&T[tix(J, K) * 256]);
            if (zero_tile(sjk)) continue;
            double* Tij = &T[tix(I, J) * 256];
            st_tile(Tij, tile_upd(ld_tile(Tij), gt, sjk));
          }
          if (J0 == K + 1) {
            y_upd(gt, K, I);
            pend(gt, tix(I, K));
          }
        }
#ifdef VG_PROBE
      if (lane == 0) atomicMax(&s_tmax, (unsigned)(wall_clock64() - tj0));
#endif
    }
    __syncthreads();
#ifdef VG_PROBE
    if (tid == 0) {
      atomicAdd(&g_probe[12], (unsigned long long)s_tmax);  // the slowest trailing wave's job time
      s_tmax = 0;
    }
#endif
    VG_PROBE_MARK(6);
  }
  flush();
  if (wave == 0) w_job(NB - 1, true);
  __syncthreads();
  VG_PROBE_MARK(5);

  // backward: x_J = w_J + sum_{I>J} (-L_IJ^T) x_I, tile (I, J) now holding
  // -L_IJ^T; wave J keeps its lane shares pa[g] of rows q + 4g and completes
  // x_J at step J+1 (one 16-lane DPP sum per row group)
  {
    double pa[4] = {0.0, 0.0, 0.0, 0.0};
    for (int I = NB - 1; I >= 1; I--) {
      if (wave < I) {
        const double* Lt = &T[tix(I, wave) * 256];
        const double xi = xv[16 * I + cc];
#pragma unroll
        for (int g = 0; g < 4; g++) pa[g] = fma(Lt[tel(rq + 4 * g, cc)], xi, pa[g]);
        if (wave == I - 1) {
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const double t = row16_sum(pa[g]);
            if (cc == 0) xv[16 * (I - 1) + rq + 4 * g] = wv[16 * (I - 1) + rq + 4 * g] + t;
          }
        }
      }
      __syncthreads();
    }
  }
  VG_PROBE_MARK(7);
  for (int t = tid; t < n; t += nt) {
    if (t < m) col[ip[t]] = xv[t];
    else col[t - m] = 0.0;  // the gauge frame (t - m < 15)
  }
  __syncthreads();
  // trial states (optimizers.cpp:468-475) and IMU bias trial (477-478)
  if (tid < W) {
    const int j = tid;
    const double* x = &xs[(size_t)j * kX];
    double* o = &xt[(size_t)j * kX];
    M3 Rn = mul(ld_m3(x), Exp(v3(col[15 * j], col[15 * j + 1], col[15 * j + 2])));
    for (int t = 0; t < 9; t++) o[t] = Rn[t];
    for (int t = 0; t < 3; t++) {
      o[9 + t] = x[9 + t] + col[15 * j + 3 + t];
      o[12 + t] = x[12 + t] + col[15 * j + 6 + t];
      o[15 + t] = x[15 + t] + col[15 * j + 9 + t];
      o[18 + t] = x[18 + t] + col[15 * j + 12 + t];
      o[21 + t] = x[21 + t];
    }
    if (j < nimu) {
      double* b = &bias[j * 12];
      for (int t = 0; t < 3; t++) {
        b[6 + t] = b[t];
        b[9 + t] = b[3 + t];
        b[t] += col[15 * j + 9 + t];
        b[3 + t] += col[15 * j + 12 + t];
      }
    }
  }
  for (int t = tid; t < n; t += nt) dxi_out[t] = col[t];
  if (wave == 1) {  // q1 on its own wave (the trial states run on wave 0): lane-strided sums, fixed xor tree
    double q1 = 0.0;
    for (int r = lane; r < n; r += 64) q1 += col[r] * (u * Dv[r] * col[r] - Jv[r]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q1 += __shfl_xor(q1, off, 64);
    if (lane == 0) st->q1 = 0.5 * q1;
  }
  if (clk && clk->on) {
    __syncthreads();
    if (tid == 0) {
      clk->solve_ticks += (unsigned long long)wall_clock64() - clk0;
      clk->solve_n += 1;
    }
  }
  VG_PROBE_MARK(8);
#ifdef VG_PROBE
  if (tid == 0) atomicAdd(&g_probe[63], 1ull);
#endif
}

int ba_solve_setup(vg_ctx* ctx) {
  VG_HIP(hipFuncSetAttribute((const void*)k_ba_solve, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)solve_lds_bytes(ctx->cfg.win_size)));
  return VG_OK;
}

void launch_prep_solve(vg_ctx* ctx, const BaDev& d, const double* hlx, int xworld, hipEvent_t* ev) {
  const int W = ctx->cfg.win_size, nimu = W - 1;
  hipStream_t s = ctx->stream;
  const int NBt = (15 * W - 15 + kTile - 1) / kTile, ntile = NBt * (NBt + 1) / 2;
  k_ba_prep<<<ntile, 256, 0, s>>>(W, nimu, ctx->cfg.imu_coef, hlx, d.imuout, d.Hcalc, d.Jcalc, d.timg, d.bvec,
                                  d.dvec, d.jvec, d.ipg, d.st, ctx->ba_structural ? 1 : 0, xworld,
                                  ctx->map.counters + kCntErr);
  if (ev) (void)hipEventRecord(ev[0], s);
  k_ba_solve<<<1, 1024, solve_lds_bytes(W), s>>>(W, nimu, d.timg, d.bvec, d.dvec, d.jvec, d.ipg, d.xs, d.xt, d.bias,
                                                 d.dxi, d.st, &ctx->st->clk);
  if (ev) (void)hipEventRecord(ev[1], s);
}

// Test-only (vgx_ba_solve): k_ba_solve on a given m x m symmetric system
// (m = 15W - 15, row-major A, right-hand side b) in identity pivot order;
// x = the solution. Runs the kernel exactly as an LM iteration does (the
// trial-state tail writes the context's scratch trial states and bias
// records, so use a context that is not stepped afterwards).
int ba_solve_test(vg_ctx* ctx, const double* A, const double* b, double* x) {
  const int W = ctx->cfg.win_size, n = 15 * W, m = n - 15;
  const int NB = (m + kTile - 1) / kTile, N = NB * kTile, ntile = NB * (NB + 1) / 2;
  hipStream_t s = ctx->stream;
  BaDev d = carve(ctx);
  std::vector<double> img((size_t)ntile * 256), bv(N, 0.0), dv(n, 1.0), jv(n, 0.0);
  std::vector<int> ipv(N, 0);
  for (int I = 0; I < NB; I++)
    for (int J = 0; J <= I; J++)
      for (int r = 0; r < 16; r++)
        for (int c = 0; c < 16; c++) {
          const int R = I * 16 + r, C = J * 16 + c;
          const double v = (R < m && C < m) ? A[(size_t)R * m + C] : (R == C ? 1.0 : 0.0);
          img[(size_t)(I * (I + 1) / 2 + J) * 256 + r * 16 + (c ^ r)] = v;
        }
  for (int t = 0; t < m; t++) {
    bv[t] = b[t];
    ipv[t] = 15 + t;
  }
  BaState bs;
  memset(&bs, 0, sizeof(bs));
  VG_HIP(hipMemcpyAsync(d.timg, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.bvec, bv.data(), N * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.dvec, dv.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.jvec, jv.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.ipg, ipv.data(), N * sizeof(int), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.st, &bs, sizeof(bs), hipMemcpyHostToDevice, s));
  VG_HIP(hipStreamSynchronize(s));
  k_ba_solve<<<1, 1024, solve_lds_bytes(W), s>>>(W, W - 1, d.timg, d.bvec, d.dvec, d.jvec, d.ipg, d.xs, d.xt, d.bias,
                                                 d.dxi, d.st, nullptr);
  VG_HIP(hipGetLastError());
  std::vector<double> out(n);
  VG_HIP(hipMemcpyAsync(out.data(), d.dxi, n * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  for (int t = 0; t < m; t++) x[t] = out[15 + t];
  return VG_OK;
}

// Test-only (vgx_ba_step): one LM step's k_ba_prep + k_ba_solve, launched as
// ba_iter_kernels launches them (launch_prep_solve), on a given LiDAR system
// hl (packed lower 6W x 6W, 6W gradient, residual), IMU blocks imuout
// ((W-1) x 931), window states xs (W x 24), bias records (W-1) x 12 and the LM
// state's u, v, calc_hess. The stored system (Hcalc / Jcalc) stays on the
// device between calls, so a calc_hess = 0 call re-reads what the previous
// call stored. The window states and bias records are the context's own: use
// a context that is not stepped afterwards.
int ba_step_test(vg_ctx* ctx, const double* hl, const double* imuout, const double* xs, const double* bias, double u,
                 double v, int calc_hess, double* dxi, double* xt, double* bias_out, double* q1_res1, int* ipg,
                 double* Hcalc, double* Jcalc) {
  const int W = ctx->cfg.win_size, n = 15 * W, m = n - 15, nimu = W - 1;
  const int L = 6 * W, nout = L * (L + 1) / 2 + L + 1, nn = n * (n + 1) / 2;
  if (sharded(ctx)) return VG_E_STATE;
  hipStream_t s = ctx->stream;
  BaDev d = carve(ctx);
  BaState bs;
  memset(&bs, 0, sizeof(bs));
  bs.u = u;
  bs.v = v;
  bs.calc_hess = calc_hess;
  VG_HIP(hipMemcpyAsync(d.hl, hl, (size_t)nout * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.imuout, imuout, (size_t)nimu * 931 * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.xs, xs, (size_t)W * kX * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.bias, bias, (size_t)nimu * 12 * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(d.st, &bs, sizeof(bs), hipMemcpyHostToDevice, s));
  VG_HIP(hipStreamSynchronize(s));
  launch_prep_solve(ctx, d, d.hl, 0, nullptr);
  VG_HIP(hipGetLastError());
  std::vector<int> ipv(kMaxNB * kTile);
  VG_HIP(hipMemcpyAsync(dxi, d.dxi, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(xt, d.xt, (size_t)W * kX * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(bias_out, d.bias, (size_t)nimu * 12 * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(&bs, d.st, sizeof(bs), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(ipv.data(), d.ipg, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(Hcalc, d.Hcalc, (size_t)nn * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipMemcpyAsync(Jcalc, d.Jcalc, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  q1_res1[0] = bs.q1;
  q1_res1[1] = bs.res1;
  for (int t = 0; t < m; t++) ipg[t] = ipv[t];
  return VG_OK;
}

}  // namespace vg

#ifdef VG_PROBE
VG_PROBE_READER(vg_probe_read)
#endif
