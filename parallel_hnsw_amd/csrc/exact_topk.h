// The running top-k of (distance, id) keys that the exact calls over an allow-list keep per wave, and the row they
// write from it: shared by the scan (filter_exact.hip) and the table path for a shared bitmap (filter_dense.hip).
// Device code; the keys are mkkey's (phnsw_device.h), distinct because the id is part of the key.
#pragma once
#include "phnsw_device.h"

// partition_point over an ascending key list in LDS; len is wave-uniform, every lane may call it
__device__ __forceinline__ uint32_t ph_keys_lower_bound(const uint64_t *keys, uint32_t len, uint64_t key) {
  if (len == 0) return 0;
  uint32_t base = 0, n = len;
  while (n > 1) {
    const uint32_t half = n >> 1;
    base = keys[base + half - 1] < key ? base + half : base;
    n -= half;
  }
  return base + (keys[base] < key ? 1u : 0u);
}

// The running top-k of one wave: an ascending list of at most k keys in LDS and a second list it is merged into.
struct PhExactTopK {
  uint64_t *cur, *nxt;  // [k] each
  uint64_t *sv;         // [64]: a batch's survivors, ascending
  uint32_t len, k;      // wave-uniform

  // One key per lane (KEY_NONE: none).  A batch is first tested against the current k-th key with one ballot -- once
  // the list is full most batches end there.  Survivors are rank-merged: a survivor lands at (entries of the list below
  // it) + (survivors below it), a list entry moves up by the survivors below it; whatever lands at or past k is dropped.
  // Returns whether the batch had a survivor.  Called by the whole wave in uniform control flow.
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
    __syncthreads();
    for (uint32_t base = 0; base < len; base += 64u) {
      const uint32_t i = base + lane;
      const uint64_t e = i < len ? cur[i] : KEY_NONE;
      const uint32_t to = i + ph_keys_lower_bound(sv, ns, e);
      if (i < len && to < k) nxt[to] = e;
    }
    __syncthreads();
    uint64_t *t = cur;
    cur = nxt;
    nxt = t;
    len = min(k, len + ns);
    return true;
  }
};

// row q of the result from an ascending key list; A: the kernel's argument block (k, out_ids, out_d, out_len, status)
template <class A>
__device__ __forceinline__ void ph_exact_write_row(const A &a, uint32_t q, const uint64_t *keys, uint32_t len,
                                                   bool bad_query, uint32_t lane) {
  for (uint32_t i = lane; i < a.k; i += 64u) {
    const uint64_t key = i < len ? keys[i] : KEY_NONE;
    a.out_ids[(uint64_t)q * a.k + i] = key == KEY_NONE ? PH_EMPTY32 : ((uint32_t)key & IDM);
    a.out_d[(uint64_t)q * a.k + i] = key == KEY_NONE ? PH_FMAX : unfkey((uint32_t)(key >> 32));
  }
  if (lane == 0) {
    a.out_len[q] = len;
    a.status[q] = bad_query ? ST_MISSING : ST_OK;  // a Stored query id at or past n (device form; the host form checks)
  }
}
