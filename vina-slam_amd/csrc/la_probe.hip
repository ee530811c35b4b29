// la_probe.hip — test-only: vg_la.h as compiled for the device, one item per
// thread on given fp64 inputs (vgx_la_eval; tests/test_device_la_gpu.py
// compares the results with a 50-digit reference). Never launched by the
// product path.
#include "vg_internal.h"
#include "vg_la.h"

namespace vg {
namespace {

// op: doubles read / written per item
//  0 eig3             A 9                          -> w 3, V 9 (row-major, eigenvectors in columns)
//  1 Exp(v)           v 3                          -> R 9
//  2 Exp(w, dt)       w 3, dt                      -> R 9
//  3 Log              R 9                          -> 3
//  4 jr               v 3                          -> 9
//  5 jr_inv           R 9                          -> 9
//  6 inverse<6>       A 36                         -> 36
//  7 inverse<15>      A 225                        -> 225
//  8 colpiv_qr_solve  m, A 8 x 3 (rows < m), b 8   -> x 3
//  9 clu_cov          P 6, v 3, N                  -> 9
// 10 clu_transform    P 6, v 3, N, R 9, t 3        -> P 6, v 3, N
constexpr int kLaOps = 11;
constexpr int kLaIn[kLaOps] = {9, 3, 4, 9, 3, 9, 36, 225, 33, 10, 22};
constexpr int kLaOut[kLaOps] = {12, 9, 9, 3, 9, 9, 36, 225, 3, 9, 10};

template <int R, int C>
__device__ __forceinline__ M<R, C> ld(const double* p) {
  M<R, C> m;
  for (int i = 0; i < R * C; i++) m[i] = p[i];
  return m;
}
template <int R, int C>
__device__ __forceinline__ void st(double* p, const M<R, C>& m) {
  for (int i = 0; i < R * C; i++) p[i] = m[i];
}
__device__ __forceinline__ Clu ld_clu(const double* p) {
  Clu c;
  for (int i = 0; i < 6; i++) c.P[i] = p[i];
  for (int i = 0; i < 3; i++) c.v[i] = p[6 + i];
  c.N = (int)p[9];
  c.pad = 0;
  return c;
}

template <int OP>
__global__ void __launch_bounds__(256) k_la_probe(const double* __restrict__ in, int is, double* __restrict__ out,
                                                  int os, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* a = in + (size_t)i * is;
  double* o = out + (size_t)i * os;
  if constexpr (OP == 0) {
    V3 w;
    M3 V;
    eig3(ld<3, 3>(a), w, V);
    st(o, w);
    st(o + 3, V);
  } else if constexpr (OP == 1) {
    st(o, Exp(ld<3, 1>(a)));
  } else if constexpr (OP == 2) {
    st(o, Exp(ld<3, 1>(a), a[3]));
  } else if constexpr (OP == 3) {
    st(o, Log(ld<3, 3>(a)));
  } else if constexpr (OP == 4) {
    st(o, jr(ld<3, 1>(a)));
  } else if constexpr (OP == 5) {
    st(o, jr_inv(ld<3, 3>(a)));
  } else if constexpr (OP == 6) {
    st(o, inverse<6>(ld<6, 6>(a)));
  } else if constexpr (OP == 7) {
    st(o, inverse<15>(ld<15, 15>(a)));
  } else if constexpr (OP == 8) {
    int m = (int)a[0];
    m = m < 3 ? 3 : (m > 8 ? 8 : m);
    colpiv_qr_solve(a + 1, m, a + 25, o);
  } else if constexpr (OP == 9) {
    st(o, clu_cov(ld_clu(a)));
  } else {
    const Clu c = clu_transform(ld_clu(a), ld<3, 3>(a + 10), ld<3, 1>(a + 19));
    for (int k = 0; k < 6; k++) o[k] = c.P[k];
    for (int k = 0; k < 3; k++) o[6 + k] = c.v[k];
    o[9] = (double)c.N;
  }
}

template <int OP>
void la_launch(int op, hipStream_t s, const double* in, int is, double* out, int os, int n) {
  if (op == OP) k_la_probe<OP><<<(n + 255) / 256, 256, 0, s>>>(in, is, out, os, n);
  if constexpr (OP + 1 < kLaOps) la_launch<OP + 1>(op, s, in, is, out, os, n);
}

}  // namespace
}  // namespace vg

// Test-only: `op` of the table above on n items, item i read from
// in[i * in_stride ...] and written to out[i * out_stride ...] (host arrays).
extern "C" int vgx_la_eval(vg_ctx* ctx, int op, const double* in, int in_stride, double* out, int out_stride, int n) {
  using namespace vg;
  if (!ctx || !in || !out || op < 0 || op >= kLaOps || n <= 0 || n > (1 << 16)) return VG_E_ARG;
  if (in_stride < kLaIn[op] || out_stride < kLaOut[op] || in_stride > 1024 || out_stride > 1024) return VG_E_ARG;
  VG_TRY(host_sync(ctx));
  const size_t nin = (size_t)n * in_stride * sizeof(double), nout = (size_t)n * out_stride * sizeof(double);
  DevBuf<double> d_in, d_out;
  hipError_t e = d_in.reserve((size_t)n * in_stride);
  if (e == hipSuccess) e = d_out.reserve((size_t)n * out_stride);
  if (e == hipSuccess) e = hipMemcpy(d_in, in, nin, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, nout);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // (the context's stream does not wait for the null stream)
  if (e == hipSuccess) {
    la_launch<0>(op, ctx->stream, d_in.p, in_stride, d_out.p, out_stride, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    ctx->err = std::string("vgx_la_eval: ") + hipGetErrorString(e);
    return VG_E_HIP;
  }
  return VG_OK;
}
