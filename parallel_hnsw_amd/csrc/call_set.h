// The scratch set of the filtered and exact calls, written once: filter_auto.hip, filter_dense.hip, filter_grouped.hip
// and filter_labeled.hip each derive their set from PhCallSet and keep only their own blocks on top of it
// (filter_ranged.hip uses the labels' set, list_scan.h).
//
// A set is kept with its owner (an index's PhCallPool per kind of call, or a labels handle's), one per call in flight.
// The rule all of this serves: nothing goes back to the pool while work that uses it may still be enqueued, whichever
// way a call ends.  `done` closes the last call that used the set; the next one's stream waits for it (block_ensure),
// and a block that must grow waits for it on the host before it is freed.  PhSetGuard is the one drain of every return
// path of a call: it records `done` on the call's stream, then hands the set back under the owner's mutex.
#pragma once
#include "phnsw_internal.h"

#define PH_TRY(x)          \
  do {                     \
    int rc__ = (x);        \
    if (rc__) return rc__; \
  } while (0)

struct PhCallSet {
  hipEvent_t done = nullptr;
  hipStream_t stream = nullptr;  // the host form's (host_call.h), made on first use
  hipStream_t last = nullptr;    // the stream of the last call that used the set; has_last: there was one
  bool has_last = false;
  bool in_use = false;  // this, last and has_last: under the owner's mutex

  int ready() {
    if (!done) PH_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    return 0;
  }
  // a block of the set at least `need` bytes large, behind the set's last user (after ready())
  int block_ensure(void **block, size_t *have, size_t need, hipStream_t on) {
    if (*have < need) {
      if (*block) {
        PH_HIP(hipEventSynchronize(done));  // the block goes back to the pool: nothing may still use it
        ph_pool_free(*block);
        *block = nullptr, *have = 0;
      }
      PH_HIP(ph_pool_alloc(block, need));
      *have = need;
    } else {
      PH_HIP(hipStreamWaitEvent(on, done, 0));
    }
    return 0;
  }
};

struct PhSetGuard {
  PhCallPool &pool;
  PhCallSet *set;
  hipStream_t stream;
  ~PhSetGuard() {
    if (set->done) hipEventRecord(set->done, stream);
    std::lock_guard<std::mutex> g(pool.mutex);
    set->last = stream, set->has_last = true;
    set->in_use = false;
  }
};

// The acquire of the index's pools: any set not in use, else a new one.  (The handles -- labels, attribute -- have a
// policy of their own, ph_handle_set_acquire in list_scan.h.)
template <class Set>
Set *ph_set_acquire(PhCallPool &pool) {
  std::lock_guard<std::mutex> g(pool.mutex);
  for (PhCallSet *s : pool.sets)
    if (!s->in_use) {
      s->in_use = true;
      return static_cast<Set *>(s);
    }
  Set *s = new Set();
  s->in_use = true;
  pool.sets.push_back(s);
  return s;
}

// The end of a pool, with its owner: every set waits for the call that used it last, loses event and stream, has its
// own blocks freed by `free_blocks(Set &)` and is deleted.
template <class Set, class F>
void ph_sets_free(PhCallPool &pool, F free_blocks) {
  for (PhCallSet *b : pool.sets) {
    Set *s = static_cast<Set *>(b);
    if (s->done) {
      hipEventSynchronize(s->done);
      hipEventDestroy(s->done);
    }
    free_blocks(*s);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
  }
  pool.sets.clear();
}

// ------------------------------------------------------------------ the steps' times of one call

// PHNSW_DENSE_TIMES=1 / PHNSW_GROUP_TIMES=1 (scripts/bench_filter_dense.py, bench_filter_grouped.py): the steps' times
// from events; the call then waits for its own work and prints its one line on stderr from what collect() sums.
struct StepTimes {
  bool on = false;
  hipStream_t stream = nullptr;
  struct Span { int step; hipEvent_t e0, e1; };
  std::vector<Span> spans;
  void begin(int step) {
    if (!on) return;
    Span s{step, nullptr, nullptr};
    if (hipEventCreate(&s.e0) != hipSuccess || hipEventCreate(&s.e1) != hipSuccess) {
      on = false;
      return;
    }
    hipEventRecord(s.e0, stream);
    spans.push_back(s);
  }
  void end() {
    if (on && !spans.empty()) hipEventRecord(spans.back().e1, stream);
  }
  // ms[step] = the sum of that step's spans, steps < `steps`; false: nothing was timed
  bool collect(float *ms, int steps) {
    if (spans.empty()) return false;
    for (int i = 0; i < steps; i++) ms[i] = 0.f;
    hipStreamSynchronize(stream);
    for (Span &s : spans) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, s.e0, s.e1) == hipSuccess) ms[s.step] += t;
      hipEventDestroy(s.e0);
      hipEventDestroy(s.e1);
    }
    spans.clear();
    return true;
  }
  ~StepTimes() {
    for (Span &s : spans) {
      if (s.e0) hipEventDestroy(s.e0);
      if (s.e1) hipEventDestroy(s.e1);
    }
  }
};
