// scratch_check — csrc/vg_scratch.h on the host, stand-alone: the HIP entry
// points the header calls are stubs over malloc / free that count what lives,
// and a switch makes the k-th allocation fail. Built with ASan + UBSan by
// tests/test_scratch.py (LeakSanitizer at exit is the leak check); not linked
// against the HIP runtime.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
//       tools/scratch_check.cpp -o scratch_check && ./scratch_check
#include "../csrc/vg_scratch.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

static int g_live = 0, g_allocs = 0, g_frees = 0;  // device allocations
static int g_fail_at = 0;                          // > 0: the allocation that brings g_allocs to it fails
static size_t g_last_bytes = 0;
static int g_events = 0, g_records = 0;

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  g_allocs++;
  if (g_allocs == g_fail_at) return hipErrorOutOfMemory;
  *p = malloc(bytes);
  g_last_bytes = bytes;
  g_live++;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (p) g_live--, g_frees++;
  free(p);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = static_cast<hipEvent_t>(malloc(1));
  g_events++;
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  free(e);
  g_events--;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
  if (!e) return hipErrorInvalidHandle;
  g_records++;
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  if (!a || !b) return hipErrorInvalidHandle;
  *ms = 1.5f;
  return hipSuccess;
}
}

static int g_bad = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      g_bad++;                                                      \
    }                                                               \
  } while (0)

using vg::DevBuf;
using vg::KernelTimer;

static void check_reserve() {
  DevBuf<double> b;
  CHECK(b.p == nullptr && b.cap == 0);
  bool regrown = false;
  CHECK(b.reserve(10, &regrown) == hipSuccess && regrown && b.cap == 10 && g_last_bytes == 80);
  double* first = b.p;
  const int allocs = g_allocs;
  regrown = false;
  CHECK(b.reserve(10, &regrown) == hipSuccess && b.reserve(3, &regrown) == hipSuccess);  // within capacity: nothing
  CHECK(!regrown && b.p == first && b.cap == 10 && g_allocs == allocs);
  CHECK(b.reserve(11, &regrown) == hipSuccess && regrown && b.cap == 11 && g_allocs == allocs + 1 && g_live == 1);
  static_cast<double*>(b)[10] = 1.0;  // (ASan: the last element is inside)
  DevBuf<char> z;
  CHECK(z.reserve(0) == hipSuccess && z.p && z.cap == 0 && g_last_bytes == 1);  // at least one byte
  const int a2 = g_allocs;
  CHECK(z.reserve(0) == hipSuccess && g_allocs == a2);
  b.release();
  CHECK(b.p == nullptr && b.cap == 0 && g_live == 1);
}

static void check_pow2() {
  DevBuf<float> b;
  const size_t need[] = {1, 1024, 1025, 2048, 2049, 5000, 3};
  const size_t want[] = {1024, 1024, 2048, 2048, 4096, 8192, 8192};
  for (int i = 0; i < 7; i++) CHECK(b.reserve_pow2(need[i]) == hipSuccess && b.cap == want[i]);
  DevBuf<float> c;
  CHECK(c.reserve_pow2(100, 16) == hipSuccess && c.cap == 128);
}

static void check_failure() {
  DevBuf<int> b;
  CHECK(b.reserve(4) == hipSuccess);
  g_fail_at = g_allocs + 1;
  bool regrown = false;
  CHECK(b.reserve(8, &regrown) == hipErrorOutOfMemory);
  CHECK(b.p == nullptr && b.cap == 0 && regrown && g_live == 0);  // empty, never half-set; the old plane is gone
  CHECK(b.reserve(8) == hipSuccess && b.cap == 8 && g_live == 1);
  g_fail_at = 0;
}

static void check_moves() {
  const int frees = g_frees;
  {
    DevBuf<int> a;
    CHECK(a.reserve(5) == hipSuccess);
    int* p = a.p;
    DevBuf<int> b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 5);
    DevBuf<int> c;
    CHECK(c.reserve(7) == hipSuccess);
    c = std::move(b);  // c's own allocation goes, b's arrives
    CHECK(g_frees == frees + 1 && c.p == p && c.cap == 5 && b.p == nullptr && b.cap == 0);
    DevBuf<int>& self = c;
    c = std::move(self);
    CHECK(c.p == p && c.cap == 5);
  }
  CHECK(g_frees == frees + 2 && g_live == 0);
}

// the staging of vg_localizability as info_bufs sets it up: four buffers, each reserved on its own. The third
// allocation fails; the retry must end with four live allocations and nothing lost
struct Four {
  DevBuf<double> pos, dirs;
  DevBuf<char> out, part;
};
static hipError_t four_bufs(Four& b) {
  hipError_t e;
  if ((e = b.pos.reserve(4096 * 3)) != hipSuccess) return e;
  if ((e = b.dirs.reserve(4096 * 3)) != hipSuccess) return e;
  if ((e = b.out.reserve(4096 * 416)) != hipSuccess) return e;
  return b.part.reserve(100 * 184);
}
static void check_partial_failure() {
  {
    Four b;
    g_fail_at = g_allocs + 3;
    CHECK(four_bufs(b) == hipErrorOutOfMemory);
    CHECK(b.pos.p && b.dirs.p && !b.out.p && !b.part.p && g_live == 2);
    g_fail_at = 0;
    const int allocs = g_allocs;
    CHECK(four_bufs(b) == hipSuccess);
    CHECK(g_allocs == allocs + 2 && g_live == 4);  // the two that stood are kept, not allocated over
    CHECK(four_bufs(b) == hipSuccess && g_allocs == allocs + 2);
  }
  CHECK(g_live == 0);
}

static void check_timer() {
  {
    KernelTimer t;
    CHECK(!t.armed() && t.ms == 0.0 && g_events == 0);
    CHECK(t.end(nullptr) != hipSuccess && t.collect() != hipSuccess && t.ms == 0.0);  // nothing to read before begin
    CHECK(t.begin(nullptr) == hipSuccess && t.armed() && g_events == 2);
    CHECK(t.end(nullptr) == hipSuccess && t.collect() == hipSuccess && t.ms == 1.5);
    CHECK(t.begin(nullptr) == hipSuccess && g_events == 2);  // the events are made once
    CHECK(t.end(nullptr) == hipSuccess && t.collect() == hipSuccess && t.ms == 3.0);
    t.clear();
    CHECK(t.ms == 0.0 && t.armed());
  }
  CHECK(g_events == 0);  // a destroyed timer releases both
  { KernelTimer never; }
  CHECK(g_events == 0);
}

int main() {
  check_reserve();
  check_pow2();
  check_failure();
  check_moves();
  check_partial_failure();
  check_timer();
  CHECK(g_live == 0 && g_events == 0);
  if (g_bad) return 1;
  printf("scratch ok: %d allocations, %d frees, %d event records\n", g_allocs, g_frees, g_records);
  return 0;
}
