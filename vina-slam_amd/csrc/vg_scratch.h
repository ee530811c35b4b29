// vg_scratch.h — the two owning types behind the query-side scratch (score,
// raycast, localisability, occupancy, terrain, clearance, navfn, frontiers, view
// gain, the change layer, the place index, markers, the fleet's tables and the
// transient device scratch of checkpoint / lifetime / la_probe). Self-contained:
// the HIP runtime API and the standard library, nothing of the context; what the
// query layers share on top of them is vg_query.h and vg_reduce.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>

namespace vg {

// A grow-only device allocation of `cap` elements. Contents do not survive
// growth; a failed reserve leaves the buffer empty, never half-set. Reads as
// its pointer wherever a T* is expected (kernel arguments, copies).
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  operator T*() const { return p; }

  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // room for n elements, exactly n when it has to allocate (at least one byte);
  // *regrown is set when the old allocation went away
  hipError_t reserve(size_t n, bool* regrown = nullptr) {
    if (n <= cap && p) return hipSuccess;
    release();
    if (regrown) *regrown = true;
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, n > 0 ? n * sizeof(T) : 1);
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q);
    cap = n;
    return hipSuccess;
  }
  // the same, doubling the capacity from `first` until it covers n
  hipError_t reserve_pow2(size_t n, size_t first = 1024) {
    if (n <= cap && p) return hipSuccess;
    size_t c = cap ? cap : first;
    while (c < n) c *= 2;
    return reserve(c);
  }
};

// Device time of a span of stream work: two events and the milliseconds
// collected so far. begin / end record around the span; collect adds the
// span's time once the caller has synchronised the stream.
struct KernelTimer {
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = 0.0;

  KernelTimer() = default;
  KernelTimer(const KernelTimer&) = delete;
  KernelTimer& operator=(const KernelTimer&) = delete;
  ~KernelTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }

  bool armed() const { return ev[1] != nullptr; }  // begin has run: the events exist
  hipError_t begin(hipStream_t s) {
    for (hipEvent_t& e : ev)
      if (!e) {
        const hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
      }
    return hipEventRecord(ev[0], s);
  }
  hipError_t end(hipStream_t s) { return hipEventRecord(ev[1], s); }
  hipError_t collect() {
    float t = 0;
    const hipError_t e = hipEventElapsedTime(&t, ev[0], ev[1]);
    if (e == hipSuccess) ms += t;
    return e;
  }
  void clear() { ms = 0.0; }
};

}  // namespace vg
