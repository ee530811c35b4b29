// vg_ba.h — what the LM's three files share: ba_factor.hip (the factor passes
// and the LM bookkeeping), ba_solve.hip (the dense step) and ba.hip (the host
// driver). Kernels are launched only from the file that defines them (no
// relocatable device code): the driver goes through the launch functions below.
#pragma once
#include "vg_dev.h"

namespace vg {

constexpr int kMaxW = 16;
constexpr int kCompF = 24;    // per factor: umumT 9, ukukT 9, uk 3, NN, coe, lmbd0
constexpr int kImuRec = kBaImuRec;  // preintegration record + cov_inv

struct BaState {             // device-resident LM state
  double u, v, res1, res2, q1;
  int calc_hess, done, iters, seq;  // seq: the next LM publication number (k_ba_control)
  int nhess;                        // Hessian passes executed (I_H, SURVEY 8(d) byte model)
  int fin;                          // the run has finished (converged or 10 iterations): the margi tail's gate
  int skip, pad_[3];                // the recut needs the host (k_ba_init): the run is skipped, the gate stays shut
};
static_assert(sizeof(BaState) <= 16 * sizeof(double), "BaState is carved as 16 doubles");

typedef double v4d __attribute__((ext_vector_type(4)));

// x state per frame: R 9, p 3, v 3, bg 3, ba 3, g 3 = 24 doubles
constexpr int kX = 24;

constexpr int kHessThreads = 512;  // 8 waves: a chunk's (factor, frame) lanes in one pass
constexpr int kHessGridMax = 256;  // k_ba_hess chunk workgroups (more chunks loop)
constexpr int kResidBlocks = 512;  // k_ba_resid workgroups (more chunks loop)
constexpr int kResidThreads = 256;  // k_ba_resid's workgroup (its chunking and residual order)
// factors per sub-chunk: two of k_ba_resid's chunks (256 / W factors) where
// that fits the lanes and the 64-row cap (W >= 8), so a Hessian chunk holds
// whole residual chunks (k_ba_resid_hess); else min(512 / W, 64)
__host__ __device__ constexpr int hess_fs(int W) {
  return 2 * (256 / W) <= 64 && 2 * (256 / W) <= kHessThreads / W ? 2 * (256 / W)
                                                                    : (kHessThreads / W < 64 ? kHessThreads / W : 64);
}
__host__ __device__ constexpr bool resid_hess_ok(int W) { return hess_fs(W) == 2 * (256 / W) && 256 / W <= 64; }
__host__ __device__ constexpr int hess_ks(int W) { return (3 * hess_fs(W) + 3) / 4 * 4; }  // GEMM K per sub-chunk
__host__ __device__ constexpr int hess_nt(int W) { return (6 * W + 15) / 16; }           // 16-wide output tiles
__host__ __device__ constexpr int hess_xs(int W) { return hess_nt(W) * 16 + 16; }        // X row stride (+16: rows k, k+1 in opposite LDS halves)
__host__ __device__ constexpr int hess_chunk(int W) { return hess_fs(W); }      // factors per workgroup (one sub-chunk)
constexpr int kRhChunkWg = kResidBlocks / 2;  // k_ba_resid_hess's chunk workgroups

// the dense step's LDS tile store (ba_solve.hip): 16x16 fp64 tiles
constexpr int kTile = 16;
constexpr int kMaxNB = 11;  // 15W <= 176

// LM bookkeeping (optimizers.cpp:480-515): k_ba_control, or
// k_ba_resid's IMU workgroup (CtlArg::err set, unsharded; resid_bookkeeping)
struct CtlArg {
  int W, nimu, nrb, nl;
  double imu_coef;
  const double* hl;
  const double* imuout;
  const double* imures;
  const double* rpart;
  double* xs;
  const double* xt;
  double* bias;
  BaState* st;
  Pub* pub;
  int* err;   // k_ba_resid runs the bookkeeping (nullptr: k_ba_control follows); error bit 64 on a stalled hand-off
  int xworld;  // sharded: rpart is the all-reduced exchange frame, its guard checked here (mismatch: bit 32 in xerr)
  int* xerr;
};

struct MpRing {
  int mp[kMaxW];
};

// ih (the scan graph, k == 0): k_ba_init_hess replaces k_ba_init + k_ba_hess
struct InitHessArg {
  MpRing ring;
  int fin;
  int seq0;  // > 0: the LM's first flag number (a direct launch); 0: DState::ph (the scan graph)
};

struct BaDev {
  double* part;
  double* hl;
  double* imurec;
  double* bias;
  double* imuout;
  double* imures;
  double* Hcalc;
  double* timg;
  double* bvec;
  double* dvec;
  double* jvec;
  int* ipg;
  double* Jcalc;
  double* xs;
  double* xt;
  double* dxi;
  double* rpart;
  int* mpring;
  BaState* st;
};

// dynamic LDS of k_ba_hess: the X operand of a sub-chunk, reused as the
// per-lane (hb, jj, res) rows of the final reduction (512 x 28 doubles =
// 112 KB); with the static S[512] (4 KB) it must fit gfx950's 160 KB LDS,
// checked at context creation (ba_alloc) against the device limit
inline size_t hess_lds_bytes(int W) {
  const size_t gemm = (size_t)hess_ks(W) * hess_xs(W), red = (size_t)kHessThreads * 28;
  return (gemm > red ? gemm : red) * sizeof(double);
}
static_assert((size_t)kHessThreads * 28 * sizeof(double) + kHessThreads * sizeof(double) <= 160 * 1024,
              "k_ba_hess reduction rows exceed gfx950 LDS");

inline size_t solve_lds_bytes(int W) {
  const int NB = (15 * W - 15 + kTile - 1) / kTile;  // the gauge frame is not factored
  return (size_t)NB * (NB + 1) / 2 * 256 * sizeof(double);
}

// carve the scratch block in BaBufs::xs; the first 1024 doubles are the WinD /
// counts staging area used by the map stages. The window states, the IMU
// records and the bias records live in the device state (state.hip); the two
// holes where they were once carved stay, so that every member keeps its
// offset and the block stays inside what ba_alloc requests (which is larger
// and does not change either).
inline BaDev carve(vg_ctx* ctx) {
  BaBufs& b = ctx->ba;
  const int W = ctx->cfg.win_size;
  const int n = 15 * W, nn = n * (n + 1) / 2;
  double* p = b.xs + 1024;
  auto take = [&p](size_t doubles) {
    double* q = p;
    p += doubles;
    return q;
  };
  BaDev d;
  d.Hcalc = take(nn);
  d.timg = take(kMaxNB * (kMaxNB + 1) / 2 * 256);
  d.bvec = take(kMaxNB * kTile);
  d.dvec = take(kMaxNB * kTile);
  d.jvec = take(kMaxNB * kTile);
  d.ipg = (int*)take(kMaxNB * kTile);
  d.Jcalc = take(n);
  d.dxi = take(n);
  take(kMaxW * kX);  // hole
  d.xt = take(kMaxW * kX);
  take(kMaxW * kImuRec + kMaxW * 12);  // hole
  d.imuout = take(kMaxW * 931);
  d.imures = take(kMaxW);
  d.st = (BaState*)take(16);
  d.mpring = (int*)take(16);
  d.xs = ctx->st->xs;
  d.imurec = ctx->st->imurec;
  d.bias = ctx->st->bias;
  d.part = b.hpart;
  d.hl = b.hout;
  d.rpart = b.rpart;
  return d;
}

// ---- launches, one per kernel, each in the file that defines the kernel.
// ba_factor.hip (G: the Hessian passes' chunk workgroups)
inline int ba_hess_grid(vg_ctx* ctx) {
  return std::min(kHessGridMax, ctx->ba.cap_f / hess_chunk(ctx->cfg.win_size) + 1);
}
int ba_factor_setup(vg_ctx* ctx);  // the dynamic LDS limits of the three Hessian kernels
void launch_ba_init(vg_ctx* ctx, const BaDev& d, const MpRing& ring, int seq0, bool fin);
void launch_ba_init_hess(vg_ctx* ctx, const BaDev& d, const InitHessArg& ih);
void launch_ba_hess(vg_ctx* ctx, const BaDev& d);
void launch_ba_hfinal(vg_ctx* ctx, const BaDev& d, double* out, const XchgArg& xa);
void launch_ba_resid(vg_ctx* ctx, const BaDev& d, const CtlArg& ctl);
void launch_ba_resid_hess(vg_ctx* ctx, const BaDev& d, const CtlArg& ctl);
void launch_ba_rsum(vg_ctx* ctx, const BaDev& d, const XchgArg& xa);
void launch_ba_control(vg_ctx* ctx, const CtlArg& ctl);
// ba_solve.hip
int ba_solve_setup(vg_ctx* ctx);  // k_ba_solve's dynamic LDS limit
// k_ba_prep then k_ba_solve of one LM iteration on the system in `hlx` /
// d.imuout (ba_iter_kernels, and the test entry ba_step_test); ev: the event
// pair around k_ba_solve (vg_profile), or nullptr
void launch_prep_solve(vg_ctx* ctx, const BaDev& d, const double* hlx, int xworld, hipEvent_t* ev);

}  // namespace vg
