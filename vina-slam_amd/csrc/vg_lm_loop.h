// vg_lm_loop.h — the host's part of the LM run: which iterations it enqueues
// and when it stops, as one rule over BaLoop. No HIP and no vg_ctx in here:
// the caller brings "launch one more iteration" and "the flag of iteration k"
// as callables (ba.hip's ba_run and ba_resolve; tools/lm_loop_check.cpp drives
// the same code against a scripted device).
//
// One iteration ahead: iteration k+1 is enqueued before the host waits for
// iteration k's flags, so the stream never drains; a converged LM leaves at
// most one early-exiting iteration behind (optimizers.cpp:449, at most 10).
// Except at the iteration count the previous LM run converged at: there the
// host waits first (a round trip, ~15 us) rather than queue an iteration
// that most likely early-exits (~35 us of dispatches). Results do not depend
// on it: the device-side flags decide.
#pragma once

namespace vg {

constexpr int kLmMaxIters = 10;

// An LM run's host loop state. A run whose outcome the host has not read yet
// (ctx->ba_loop, active) is continued by ba_resolve: the fused step returns
// once the LM iterations and the speculative margi tail are enqueued, and the
// next step enqueues its downsample, propagation and IEKF before it waits for
// that outcome
struct BaLoop {
  int seq0 = 0, enq = 0, tail_at = 0, k = 0;  // first iteration flag number, iterations enqueued, ahead of the tail, next k
  int done_iters = 0;                         // iterations the device ran, as far as the flags read so far tell
  bool active = false;
};

// what lm_loop_advance and its callables return besides 0; a callable's
// negative value (an error) ends the advance and is returned as it is
enum { kLmEnd = 1, kLmNotYet = 2, kLmPause = 3 };

// A run begins with `pre` iterations already on the stream and the gated margi
// tail behind them (the scan graph). With pre == 0 the caller enqueues the
// first one or two iterations itself and sets L.enq to that count before it
// advances the loop.
inline void lm_loop_begin(BaLoop& L, int seq0, int pre) {
  L = BaLoop{};
  L.seq0 = seq0;
  L.enq = L.tail_at = pre;
}

// The margi tail goes in right behind the iteration count the previous run
// converged at (steady state: 2 of 2), gated on the device: if the LM needs
// more, that copy runs as no-ops and the caller enqueues it again after the
// last iteration.
inline bool lm_tail_due(const BaLoop& L, int last_iters) { return !L.tail_at && L.enq >= last_iters; }

// Advance the run from iteration L.k until it ends (kLmEnd: lm_loop_end holds
// the outcome), a flag is not published yet (kLmNotYet) or the caller's hook
// stops it (its non-zero value). Calling it again after kLmNotYet or kLmPause
// continues where it stopped and launches nothing twice.
//   launch()        enqueue one more iteration (0, or an error)
//   before_wait(k)  the caller's work between the enqueue-ahead and the wait
//   flag(k, &word)  0 with ba_word once iteration k has published, kLmNotYet,
//                   or an error
// last_iters: the iteration count of the previous run (ba_last_iters).
template <class Launch, class Hook, class Flag>
int lm_loop_advance(BaLoop& L, int last_iters, Launch&& launch, Hook&& before_wait, Flag&& flag) {
  auto one_more = [&]() -> int {
    const int r = launch();
    if (r == 0) L.enq++;
    return r;
  };
  for (; L.k < kLmMaxIters; L.k++) {
    const int k = L.k;
    int r = 0, bw = 0;
    if (L.enq == k + 1 && L.enq < kLmMaxIters && L.enq < last_iters && (r = one_more()) != 0) return r;  // one ahead
    if ((r = before_wait(k)) != 0) return r;
    if ((r = flag(k, &bw)) != 0) return r;
    // The flags may already come from iteration k+1 (queued ahead, possibly
    // finished by now): decide on iteration k's outcome only — done at or
    // before it (the device stops counting once done) — so the number of
    // iterations enqueued never depends on timing (sharded mode: every
    // enqueue is an exchange, all ranks must enqueue alike)
    L.done_iters = bw >> 1;
    if ((bw & 1) && L.done_iters <= k + 1) break;
    L.done_iters = k + 1;
    if (L.enq == k + 1 && L.enq < kLmMaxIters && (r = one_more()) != 0) return r;  // not queued ahead: now
  }
  return kLmEnd;
}

struct LmOutcome {
  int iters;       // LM iterations executed
  bool tail_ok;    // the gate opened for the speculative tail's copy
  int last_iters;  // the next run's ba_last_iters
};
inline LmOutcome lm_loop_end(const BaLoop& L) {
  return {L.done_iters, L.tail_at > 0 && L.done_iters <= L.tail_at, L.done_iters > 0 ? L.done_iters : 2};
}

}  // namespace vg
