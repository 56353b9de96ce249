// PhExactTopK (exact_topk.h) for a wave of a MULTI-WAVE workgroup: the same ascending list, the same rank merge, the
// same results, with the two __syncthreads() of insert replaced by what they are to a one-wave workgroup -- the
// workgroup-scope release / acquire fences around a barrier -- minus the s_barrier, which only the other waves would
// wait at.  A wave runs in lockstep, so once its own stores have completed (the fence's s_waitcnt) every lane sees
// them: lists in LDS or in global memory alike, the wave's CU being the one place both are served from.
// Beside the existing struct rather than a parameter of it, so that no kernel that has one compiles differently.
#pragma once
#include "exact_topk.h"

// what __syncthreads() is, without the barrier: for the lanes of ONE wave
__device__ __forceinline__ void ph_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct PhWaveTopK {
  uint64_t *cur, *nxt;  // [k] each
  uint64_t *sv;         // [64], this wave's own: a batch's survivors, ascending
  uint32_t len, k;      // wave-uniform

  // PhExactTopK::insert: one key per lane (KEY_NONE: none), whether the batch had a survivor.  Called by the whole
  // wave in uniform control flow; the other waves of the workgroup may be anywhere.
  __device__ __forceinline__ bool insert(uint64_t key, uint32_t lane) {
    const uint64_t kth = len == k ? cur[k - 1u] : KEY_NONE;
    const bool surv = key < kth;
    const uint64_t sm = __ballot(surv);
    if (!sm) return false;
    const uint32_t ns = (uint32_t)__popcll(sm);
    uint32_t rank = 0;
    for (uint64_t t = sm; t; t &= t - 1ull) rank += rl64(key, __ffsll((unsigned long long)t) - 1) < key ? 1u : 0u;
    const uint32_t below = ph_keys_lower_bound(cur, len, key);
    if (surv) {
      sv[rank] = key;  // rank < ns <= 64
      if (below + rank < k) nxt[below + rank] = key;
    }
    ph_wave_sync();
    for (uint32_t base = 0; base < len; base += 64u) {
      const uint32_t i = base + lane;
      const uint64_t e = i < len ? cur[i] : KEY_NONE;
      const uint32_t to = i + ph_keys_lower_bound(sv, ns, e);
      if (i < len && to < k) nxt[to] = e;
    }
    ph_wave_sync();
    uint64_t *t = cur;
    cur = nxt;
    nxt = t;
    len = min(k, len + ns);
    return true;
  }
};
