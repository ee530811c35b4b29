// lm_loop_check — csrc/vg_lm_loop.h (the LM's host loop: ba_run / ba_resolve)
// on the host, stand-alone, against a scripted device: the device converges at
// a given iteration (or never), publishes k_ba_control's word per iteration,
// and its flags arrive on time, early or late. Built with ASan + UBSan by
// tests/test_lm_loop.py; no GPU, no HIP runtime.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined tools/lm_loop_check.cpp -o lm_loop_check && ./lm_loop_check
#include "../csrc/vg_lm_loop.h"

#include <cstdio>
#include <vector>

static int g_bad = 0, g_cases = 0, g_deferred = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      g_bad++;                                                      \
    }                                                               \
  } while (0)

// The scripted device: iteration j (0-based) leaves iters = j + 1 and done = 0
// until the run converges in iteration `conv` (1-based; 0: never), after which
// every queued iteration early-exits and republishes conv * 2 + 1.
struct Dev {
  int conv = 0;
  bool early = false;   // a read of iteration k's flag sees the word of the last iteration enqueued
  int launched = 0;     // iterations on the stream
  int reads = 0;        // flags read so far
  std::vector<int> log;  // one entry per launch: reads * 1000 + kind * 100 + the iteration's index (kind 1: the two-iteration graph)
  int word_after(int j) const {
    const int n = j + 1;
    return conv > 0 && n >= conv ? conv * 2 + 1 : n * 2;
  }
  void launch(int kind = 0) {
    log.push_back(reads * 1000 + kind * 100 + launched);
    launched += kind ? 2 : 1;
  }
  int read(int k) {  // the word the host finds once iteration k's flag is up
    CHECK(launched > k);  // else the host would wait for an iteration nobody enqueued
    reads++;
    return word_after(early && launched > k ? launched - 1 : k);
  }
};

struct Outcome {
  std::vector<int> log;
  int iters = 0, last_iters = 0, tail_at = 0;
  bool tail_ok = false;
  bool operator==(const Outcome& o) const {
    return log == o.log && iters == o.iters && last_iters == o.last_iters && tail_at == o.tail_at && tail_ok == o.tail_ok;
  }
};

// The loop of ba_run as it stood before vg_lm_loop.h, restated literally (the
// HIP calls replaced by the scripted device, no deferral): what the shared loop
// must reproduce.
static Outcome parent_loop(Dev dev, int ba_last_iters, int pre, bool graph2, bool spec_tail) {
  auto iteration = [&](int) { dev.launch(); };
  int enq = 1, done_iters = 0, tail_at = 0;  // iterations enqueued so far / ahead of the speculative tail
  if (pre > 0) {
    enq = pre;
    tail_at = pre;
  } else if (graph2) {
    dev.launch(1);
    enq = 2;
  } else {
    iteration(0);
  }
  for (int k = 0; k < 10; k++) {
    if (enq == k + 1 && enq < 10 && enq < ba_last_iters) iteration(enq++);  // one ahead
    if (spec_tail && !tail_at && enq >= ba_last_iters) tail_at = enq;
    const int bw = dev.read(k);
    done_iters = bw >> 1;
    if ((bw & 1) && done_iters <= k + 1) break;
    done_iters = k + 1;
    if (enq == k + 1 && enq < 10) iteration(enq++);  // not queued ahead: now
  }
  Outcome o;
  o.log = dev.log;
  o.tail_at = tail_at;
  o.tail_ok = tail_at > 0 && done_iters <= tail_at;
  o.iters = done_iters;
  o.last_iters = done_iters > 0 ? done_iters : 2;
  return o;
}

// ba_run's use of the shared loop, and ba_resolve's for a run deferred at its
// first opportunity (defer); poll: the resolve does not block, and every flag
// is "not yet" at its first poll
static Outcome shared_loop(Dev dev, int ba_last_iters, int pre, bool graph2, bool spec_tail, bool defer, bool poll) {
  vg::BaLoop L;
  vg::lm_loop_begin(L, 100, pre);
  auto launch = [&]() {
    dev.launch();
    return 0;
  };
  if (graph2) {
    dev.launch(1);
    L.enq = 2;
  } else if (pre == 0) {
    launch();
    L.enq = 1;
  }
  int r = vg::lm_loop_advance(
      L, ba_last_iters, launch,
      [&](int) -> int {
        if (spec_tail && vg::lm_tail_due(L, ba_last_iters)) L.tail_at = L.enq;
        return defer && L.tail_at > 0 ? vg::kLmPause : 0;
      },
      [&](int k, int* bw) {
        *bw = dev.read(k);
        return 0;
      });
  if (r == vg::kLmPause) {
    g_deferred++;
    L.active = true;
    vg::BaLoop saved = L;  // ctx->ba_loop
    int polled_k = -1, spins = 0;
    do {
      CHECK(saved.active && ++spins < 64);
      r = vg::lm_loop_advance(
          saved, ba_last_iters, launch, [](int) { return 0; },
          [&](int k, int* bw) -> int {
            if (poll && polled_k != k) {
              polled_k = k;
              return vg::kLmNotYet;
            }
            *bw = dev.read(k);
            return 0;
          });
    } while (r == vg::kLmNotYet);
    L = saved;
  }
  CHECK(r == vg::kLmEnd);
  const vg::LmOutcome e = vg::lm_loop_end(L);
  Outcome o;
  o.log = dev.log;
  o.iters = e.iters;
  o.tail_at = L.tail_at;
  o.tail_ok = e.tail_ok;
  o.last_iters = e.last_iters;
  return o;
}

int main() {
  for (int conv = 0; conv <= 10; conv++)  // 0: never converges
    for (int last = 1; last <= 10; last++)
      for (int pre = 0; pre <= 2; pre += 2)
        for (int two = 0; two < 2; two++)
          for (int spec = 0; spec < 2; spec++) {
            const bool graph2 = pre == 0 && two && last >= 2;  // ba_run's condition for the two-iteration graph
            if (two && !graph2) continue;
            Dev dev;
            dev.conv = conv;
            dev.launched = pre;
            Dev dev_early = dev;
            dev_early.early = true;
            g_cases++;
            const Outcome ref = parent_loop(dev, last, pre, graph2, spec);
            // the device's own count: conv iterations, or all ten
            CHECK(ref.iters == (conv > 0 ? conv : 10) && ref.last_iters == ref.iters);
            // (c) early flags change nothing in the parent's loop either: one reference serves
            CHECK(parent_loop(dev_early, last, pre, graph2, spec) == ref);
            for (int early = 0; early < 2; early++) {
              const Dev& d = early ? dev_early : dev;
              // (a) the shared loop equals the parent's, launch for launch
              CHECK(shared_loop(d, last, pre, graph2, spec, false, false) == ref);
              // (b) deferred and resolved, blocking or polling (late flags), and (c)
              const int before = g_deferred;
              CHECK(shared_loop(d, last, pre, graph2, spec, true, false) == ref);
              CHECK(shared_loop(d, last, pre, graph2, spec, true, true) == ref);
              CHECK((g_deferred - before == 2) == (ref.tail_at > 0));  // deferred wherever a tail was queued
            }
          }
  printf("lm loop: %d cases, %d deferred runs\n", g_cases, g_deferred);
  if (g_bad) return 1;
  printf("lm loop ok\n");
  return 0;
}
