// vg_reduce.h — the device-side reductions behind the query layers' summaries,
// once: for 64-lane waves and integer types only (sums, minima and maxima that no
// order of the lanes changes; the double-precision sums of vg_info.h depend on
// their order and stay where they are). Every lane of the wave, for block_add of
// the workgroup, calls them, the lanes past the data with the identity.
#pragma once
#include <hip/hip_runtime.h>

namespace vg {

// the wave's sum, minimum and maximum of v; lane 0's result is the wave's
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_down(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// the number of the wave's lanes with pred to sum[slot]: one atomic, none for a zero
__device__ __forceinline__ void wave_count_add(unsigned long long* __restrict__ sum, int slot, bool pred) {
  const unsigned long long b = __ballot(pred);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&sum[slot], (unsigned long long)__popcll(b));
}

// the sum of v over a workgroup of kBlock lanes to sum[slot]: the waves' sums, LDS across the waves, one atomic
// (none for a zero)
template <int kBlock>
__device__ __forceinline__ void block_add(unsigned long long v, unsigned long long* sum, int slot) {
  __shared__ unsigned long long s_w[kBlock / 64];
  v = wave_sum(v);
  __syncthreads();  // (a call before this one has read s_w)
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < kBlock / 64; w++) t += s_w[w];
    if (t) atomicAdd(&sum[slot], t);
  }
}

}  // namespace vg
