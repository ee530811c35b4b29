// places.hip — the place index (vina_gpu.h "Place index"): per sample position
// the polar range image the frozen map shows from there, a scan binned into the
// same image, and every place compared with the scan under every circular
// azimuth shift. The descriptor and its arithmetic: vg_place.h.
//
// k_place_cast: one lane per (place, bin), 256-thread workgroups, a workgroup
// inside one place, so a wave's ballot counts one place's hits (one integer
// atomic per wave). The ray is k_raycast's: ray_trace with the same operands,
// so a row equals vg_raycast's ranges quantised, and depends on the place and
// the map alone. Latency-bound gather, no LDS (raycast.hip's notes apply).
//
// k_place_scan: one lane per point. A workgroup's 256 points land in a private
// (sum, count) histogram of A E bins in LDS (uint32 pairs, 8 A E bytes: 11.5 KB
// at the defaults, 32 KB at the limits; 256 points x 65535 fit a uint32) through
// LDS integer atomics — neighbouring points of a spinning scan share bins, so
// the contention stays inside the CU — and the non-empty bins go out in one pass
// of global integer atomics (64-bit sum, 32-bit count). k_place_scan_finish, one
// workgroup, turns the sums into uint16 means and counts the non-empty bins.
//
// k_place_match: one workgroup per place, one lane per shift. The scan's
// descriptor and the place's rows are staged in LDS as uint16, each row twice
// in a row (2 A entries), so lane s reads entry a + s without a modulo: the
// lanes of a wave read consecutive 2-byte addresses (two lanes per bank word,
// no conflict) and the scan's value is a broadcast. The loop over the bins is
// uniform; an empty scan bin is skipped by every lane at once. The best shift
// and the best shift at least A / 4 bins away come from two fixed min-trees
// over (score << 32 | s) keys in LDS, so ties go to the lower s.
//
// Nothing here polls a flag, and nothing is shared between workgroups but the
// integer atomics named above.
#include <algorithm>
#include <climits>

#include "vg_place.h"

namespace vg {

__global__ void __launch_bounds__(kPlaceBlock) k_place_cast(double vs, DevMap m, const double* __restrict__ pos,
                                                            const double* __restrict__ dirs, int nb, int bpp,
                                                            RayPrm prm, uint16_t* __restrict__ desc,
                                                            int* __restrict__ hit) {
  const int place = blockIdx.x / bpp;
  const int bin = (blockIdx.x % bpp) * kPlaceBlock + threadIdx.x;
  unsigned q = 0;
  if (bin < nb) {
    const V3 o = ld_v3(pos + 3 * (size_t)place), d = ld_v3(dirs + 3 * (size_t)bin);
    vg_ray_hit r;
    ray_trace(m, vs, o, d, prm, r);
    if (r.flags & kRayHit) q = place_quant(r.range);
    desc[(size_t)place * nb + bin] = (uint16_t)q;
  }
  const unsigned long long b = __ballot(q > 0);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&hit[place], __popcll(b));
}

// h: nb sums, then nb counts
__global__ void __launch_bounds__(kPlaceBlock) k_place_scan(const float* __restrict__ xyz, int n, PlacePrm p,
                                                            PlaceFrame F, unsigned long long* __restrict__ gsum,
                                                            unsigned* __restrict__ gcnt) {
  extern __shared__ unsigned h[];
  const int nb = p.n_az * p.n_el;
  for (int i = threadIdx.x; i < 2 * nb; i += kPlaceBlock) h[i] = 0;
  __syncthreads();
  const int i = blockIdx.x * kPlaceBlock + threadIdx.x;
  if (i < n) {
    unsigned q = 0;
    const int bin = place_bin(p, F, (double)xyz[3 * (size_t)i], (double)xyz[3 * (size_t)i + 1],
                              (double)xyz[3 * (size_t)i + 2], q);
    if (bin >= 0 && bin < nb) {
      atomicAdd(&h[bin], q);
      atomicAdd(&h[nb + bin], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += kPlaceBlock) {
    const unsigned c = h[nb + b];
    if (c) {
      atomicAdd(&gsum[b], (unsigned long long)h[b]);
      atomicAdd(&gcnt[b], c);
    }
  }
}

__global__ void __launch_bounds__(kPlaceBlock) k_place_scan_finish(const unsigned long long* __restrict__ gsum,
                                                                   const unsigned* __restrict__ gcnt, int nb,
                                                                   uint16_t* __restrict__ scan,
                                                                   int* __restrict__ n_valid) {
  __shared__ int tot;
  if (threadIdx.x == 0) tot = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += kPlaceBlock) {  // (uniform trip count: every lane reaches the ballot)
    const int b = b0 + threadIdx.x;
    unsigned v = 0;
    if (b < nb) {
      const unsigned long long c = gcnt[b];
      if (c) {
        const unsigned long long mean = (gsum[b] + c / 2) / c;
        v = mean > 65535ull ? 65535u : (unsigned)mean;
      }
      scan[b] = (uint16_t)v;
    }
    const unsigned long long bal = __ballot(v > 0);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&tot, __popcll(bal));
  }
  __syncthreads();
  if (threadIdx.x == 0) *n_valid = tot;
}

// the minimum of the workgroup's keys (every thread gets it)
__device__ __forceinline__ long long place_min_tree(long long* red, long long key) {
  const int t = threadIdx.x;
  __syncthreads();  // (the previous tree's readers are done)
  red[t] = key;
  __syncthreads();
  for (int w = kPlaceBlock / 2; w > 0; w >>= 1) {
    if (t < w && red[t + w] < red[t]) red[t] = red[t + w];
    __syncthreads();
  }
  return red[0];
}

// sm: the scan's nb entries, then the place's E rows of 2 A entries. best: 4 ints per place
__global__ void __launch_bounds__(kPlaceBlock) k_place_match(const uint16_t* __restrict__ desc,
                                                             const int* __restrict__ hit,
                                                             const uint16_t* __restrict__ scan, int A, int E,
                                                             int min_bins, int clip_q, int* __restrict__ best,
                                                             int* __restrict__ scores) {
  extern __shared__ uint16_t sm[];
  __shared__ long long red[kPlaceBlock];
  const int place = blockIdx.x, s = threadIdx.x, nb = A * E;
  if (hit[place] < min_bins) {  // (uniform over the workgroup)
    if (s == 0) {
      best[4 * place] = best[4 * place + 2] = -1;
      best[4 * place + 1] = best[4 * place + 3] = INT_MAX;
    }
    if (scores && s < A) scores[(size_t)place * A + s] = INT_MAX;
    return;
  }
  uint16_t* sc = sm;
  uint16_t* pl = sm + nb;
  for (int i = s; i < nb; i += kPlaceBlock) sc[i] = scan[i];
  const uint16_t* row = desc + (size_t)place * nb;
  for (int i = s; i < 2 * nb; i += kPlaceBlock) {
    const int e = i / (2 * A), j = i - e * 2 * A;
    pl[i] = row[e * A + (j < A ? j : j - A)];
  }
  __syncthreads();
  int score = 0;
  if (s < A) {
    for (int e = 0; e < E; e++) {
      const uint16_t* pe = pl + e * 2 * A + s;
      const uint16_t* se = sc + e * A;
      for (int a = 0; a < A; a++) {
        const int sv = se[a];
        if (sv == 0) continue;
        const int pv = pe[a];
        int d = pv > sv ? pv - sv : sv - pv;
        d = d < clip_q ? d : clip_q;
        score += pv ? d : clip_q;
      }
    }
    if (scores) scores[(size_t)place * A + s] = score;
  }
  const long long none = LLONG_MAX;
  const long long key = s < A ? (((long long)score << 32) | (long long)s) : none;
  const long long k0 = place_min_tree(red, key);
  const int s0 = (int)(k0 & 0xffffffffll);
  int dist = s > s0 ? s - s0 : s0 - s;
  dist = dist < A - dist ? dist : A - dist;
  const long long k1 = place_min_tree(red, (s < A && 4 * dist >= A) ? key : none);
  if (s == 0) {
    best[4 * place] = s0;
    best[4 * place + 1] = (int)(k0 >> 32);
    best[4 * place + 2] = k1 == none ? -1 : (int)(k1 & 0xffffffffll);
    best[4 * place + 3] = k1 == none ? INT_MAX : (int)(k1 >> 32);
  }
}

// ---- host side

int places_prm_ok(const vg_places_params* prm, int* A, int* E) {
  PlacePrm q;
  if (!place_prm(prm, q)) return VG_E_ARG;
  if (A) *A = q.n_az;
  if (E) *E = q.n_el;
  return VG_OK;
}

int places_dirs(const vg_places_params* prm, double* out, int cap, int* count) {
  PlacePrm q;
  if (!place_prm(prm, q)) return VG_E_ARG;
  *count = q.n_az * q.n_el;
  if (!out) return VG_OK;
  for (int e = 0; e < q.n_el; e++)
    for (int a = 0; a < q.n_az; a++) {
      const int k = e * q.n_az + a;
      if (k < cap) place_dir(q, e, a, out + 3 * (size_t)k);
    }
  return VG_OK;
}

int places_build_dev(vg_ctx* ctx, PlaceIndex* I, const MP& mp) {
  static_assert(sizeof(vg_place_candidate) == 48 && sizeof(vg_places_params) == 144, "the records' documented sizes");
  PlacePrm q;
  if (!place_prm(&I->prm, q)) return VG_E_ARG;
  const int nb = q.n_az * q.n_el, M = I->M;
  I->A = q.n_az;
  I->E = q.n_el;
  hipStream_t s = ctx->stream;
  VG_HIP(I->d_pos.reserve((size_t)M * 3));
  VG_HIP(I->d_dirs.reserve((size_t)nb * 3));
  VG_HIP(I->d_desc.reserve((size_t)M * nb));
  VG_HIP(I->d_hit.reserve((size_t)M));
  VG_HIP(I->d_sum.reserve((size_t)nb));
  VG_HIP(I->d_cnt.reserve((size_t)nb));
  VG_HIP(I->d_scan.reserve((size_t)nb));
  VG_HIP(I->d_scan_valid.reserve(1));
  VG_HIP(I->d_best.reserve((size_t)M * 4));
  // the table of vg_places_dirs as (ex, ey, up) combinations: the table itself where gravity is along -z
  std::vector<double> dirs((size_t)nb * 3);
  const double* f = I->frame;
  for (int e = 0; e < q.n_el; e++)
    for (int a = 0; a < q.n_az; a++) {
      double d[3];
      place_dir(q, e, a, d);
      double* o = &dirs[3 * (size_t)(e * q.n_az + a)];
      for (int j = 0; j < 3; j++) o[j] = d[0] * f[j] + d[1] * f[3 + j] + d[2] * f[6 + j];
    }
  VG_HIP(hipMemcpyAsync(I->d_pos, I->pos.data(), (size_t)M * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemcpyAsync(I->d_dirs, dirs.data(), dirs.size() * sizeof(double), hipMemcpyHostToDevice, s));
  VG_HIP(hipMemsetAsync(I->d_hit, 0, (size_t)M * sizeof(int), s));
  const int bpp = (nb + kPlaceBlock - 1) / kPlaceBlock;
  VG_HIP(I->t_build.begin(s));
  k_place_cast<<<(unsigned)M * (unsigned)bpp, kPlaceBlock, 0, s>>>(mp.vs, ctx->map, I->d_pos, I->d_dirs, nb, bpp, q.ray,
                                                                   I->d_desc, I->d_hit);
  VG_HIP(I->t_build.end(s));
  VG_HIP(hipGetLastError());
  I->hit.assign((size_t)M, 0);
  VG_HIP(hipMemcpyAsync(I->hit.data(), I->d_hit, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));  // (dirs is read by the copy until here)
  I->n_valid = 0;
  for (int v : I->hit) I->n_valid += v >= q.min_bins ? 1 : 0;
  return VG_OK;
}

int places_scan_dev(vg_ctx* ctx, PlaceIndex* I, const MP& mp, const float* xyz, int n, const double* R_level9,
                    uint16_t* desc, int32_t* n_per_bin, int* n_valid) {
  PlacePrm q;
  if (!place_prm(&I->prm, q)) return VG_E_ARG;
  const int nb = q.n_az * q.n_el;
  VG_TRY(ray_bufs(ctx));
  RayBufs& b = ctx->ray;
  if (n > (int)b.out.cap) return VG_E_ARG;
  hipStream_t s = ctx->stream;
  PlaceFrame F;
  memcpy(F.f, I->frame, sizeof(F.f));
  M3 Rl, eR;
  memcpy(Rl.a, R_level9, 72);
  memcpy(eR.a, mp.extR, 72);
  const M3 Mx = mul(Rl, eR);
  memcpy(F.m, Mx.a, 72);
  float* d_xyz = reinterpret_cast<float*>(b.dir.p);
  if (n > 0) VG_HIP(hipMemcpyAsync(d_xyz, xyz, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, s));
  VG_HIP(I->t_query.begin(s));
  VG_HIP(hipMemsetAsync(I->d_sum, 0, (size_t)nb * sizeof(unsigned long long), s));
  VG_HIP(hipMemsetAsync(I->d_cnt, 0, (size_t)nb * sizeof(unsigned), s));
  if (n > 0)
    k_place_scan<<<(n + kPlaceBlock - 1) / kPlaceBlock, kPlaceBlock, 2 * (size_t)nb * sizeof(unsigned), s>>>(
        d_xyz, n, q, F, I->d_sum, I->d_cnt);
  k_place_scan_finish<<<1, kPlaceBlock, 0, s>>>(I->d_sum, I->d_cnt, nb, I->d_scan, I->d_scan_valid);
  VG_HIP(I->t_query.end(s));
  VG_HIP(hipGetLastError());
  if (desc) VG_HIP(hipMemcpyAsync(desc, I->d_scan, (size_t)nb * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
  if (n_per_bin) {
    static_assert(sizeof(int32_t) == sizeof(unsigned), "the counts are copied as they are");
    VG_HIP(hipMemcpyAsync(n_per_bin, I->d_cnt, (size_t)nb * sizeof(unsigned), hipMemcpyDeviceToHost, s));
  }
  int nv = 0;
  VG_HIP(hipMemcpyAsync(&nv, I->d_scan_valid, sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  if (n_valid) *n_valid = nv;
  return VG_OK;
}

int places_match_dev(vg_ctx* ctx, PlaceIndex* I, int* best, int32_t* scores_all) {
  PlacePrm q;
  if (!place_prm(&I->prm, q)) return VG_E_ARG;
  const int nb = q.n_az * q.n_el, M = I->M;
  hipStream_t s = ctx->stream;
  if (scores_all) VG_HIP(I->d_scores.reserve((size_t)M * q.n_az));
  k_place_match<<<M, kPlaceBlock, 3 * (size_t)nb * sizeof(uint16_t), s>>>(
      I->d_desc, I->d_hit, I->d_scan, q.n_az, q.n_el, q.min_bins, q.clip_q, I->d_best, scores_all ? I->d_scores.p : nullptr);
  VG_HIP(I->t_query.end(s));
  VG_HIP(hipGetLastError());
  VG_HIP(hipMemcpyAsync(best, I->d_best, (size_t)M * 4 * sizeof(int), hipMemcpyDeviceToHost, s));
  if (scores_all)
    VG_HIP(hipMemcpyAsync(scores_all, I->d_scores, (size_t)M * q.n_az * sizeof(int), hipMemcpyDeviceToHost, s));
  VG_HIP(hipStreamSynchronize(s));
  return VG_OK;
}

}  // namespace vg

// Test / measurement hook: the device time of the build's cast kernel and of
// the last query's kernels (scan pass to match pass; HIP events on the stream
// of the context that made the call), of the index of the map ctx reads
extern "C" int vgx_places_ms(vg_ctx* ctx, double* build_ms, double* query_ms) {
  if (!ctx) return VG_E_ARG;
  vg_ctx* owner = ctx->view_of ? ctx->view_of : ctx;
  std::lock_guard<std::mutex> lock(owner->places_mu);
  vg::PlaceIndex* I = owner->places;
  if (!I) return VG_E_STATE;
  if (build_ms) {
    I->t_build.clear();
    VG_HIP(I->t_build.collect());
    *build_ms = I->t_build.ms;
  }
  if (query_ms) {
    I->t_query.clear();
    if (I->t_query.armed()) VG_HIP(I->t_query.collect());  // (0: no query yet)
    *query_ms = I->t_query.ms;
  }
  return VG_OK;
}
