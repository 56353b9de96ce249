// The running top-k of (distance, id) keys that the exact calls over an allow-list keep per wave, what feeds it and what
// is written from it, and the block-level scan and sum of their list builders: everything the kernels of
// filter_exact.hip, filter_dense.hip, filter_grouped.hip, filter_labeled.hip and filter_ranged.hip have in common, written
// once.
// Device code; the keys are mkkey's (phnsw_device.h), distinct because the id is part of the key.
#pragma once
#include "phnsw_device.h"

// inclusive prefix sum over the wave's lanes
template <class T>
__device__ __forceinline__ T ph_wave_inclusive_sum(T v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const T t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// One round of a 1024-thread workgroup's scan: a shuffle scan per wave, the 16 waves' totals through LDS, the running
// base in every thread.  Returns the exclusive prefix of v over the threads, on top of `base`, and advances `base` by
// the round's total.  Called by the whole workgroup in uniform control flow; a __syncthreads() of the caller's stands
// between two rounds, which rewrite the totals.
template <class T>
__device__ __forceinline__ T ph_block_exclusive_scan(T v, T &base) {
  __shared__ T wave_total[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const T incl = ph_wave_inclusive_sum(v, lane);
  if (lane == 63u) wave_total[wave] = incl;
  __syncthreads();
  T before = base, all = 0;
  for (uint32_t i = 0; i < 16u; i++) {
    if (i < wave) before += wave_total[i];
    all += wave_total[i];
  }
  base += all;
  return before + incl - v;
}

// the sum of c over a 256-thread workgroup, in every thread; uniform control flow
__device__ __forceinline__ uint32_t ph_block_sum256(uint32_t c) {
  __shared__ uint32_t part[4];
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) c += __shfl_xor(c, sft);
  __syncthreads();  // part[] of the previous sum has been read
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

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

  // empty, over keys [2k + 64]
  __device__ __forceinline__ void init(uint64_t *keys, uint32_t k_) {
    cur = keys, nxt = keys + k_, sv = keys + 2u * k_, len = 0, k = k_;
  }

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

  // the list a previous launch stored (ph_exact_store_list) becomes the current one
  __device__ __forceinline__ void load(const uint64_t *list, uint32_t lane) {
    uint32_t have = 0;
    for (uint32_t i = lane; i < k; i += 64u) {
      const uint64_t key = list[i];
      cur[i] = key;
      have += key != KEY_NONE ? 1u : 0u;
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) have += __shfl_xor(have, sft);
    len = have;  // the padding is KEY_NONE and no key is (mkkey keeps bit 31 of the id word clear)
    __syncthreads();
  }

  // One row of a distance table, 64 entries at a time, coalesced: entry j is the distance to ids[j] (j < tn, inside the
  // row); the id `ex` is left out.
  __device__ __forceinline__ void insert_row(const float *row, const uint32_t *ids, uint32_t tn, uint32_t ex, uint32_t lane) {
    for (uint32_t b = 0; b < tn; b += 64u) {
      const uint32_t j = b + lane;
      const bool ok = j < tn;
      const uint32_t id = ok ? ids[j] : PH_EMPTY32;
      insert(ok && id != ex ? mkkey(row[j], id) : KEY_NONE, lane);
    }
  }
};

// An ascending [k] list, KEY_NONE padded (another slice's, another wave's), into `top`: fed 64 keys at a time and left at
// the first batch without a survivor -- whatever follows in it is larger still.  A statement, not a function: through
// any function (member or free, the length passed in or not, with or without a branch hint) the merge kernels compile
// to another block order, the k-th key's reload out of line, and the label-set merge measured slower for it; expanded
// in place they compile to the code they had with the loop written into each (profiles/exact_once/).
#define PH_EXACT_FEED(top, list_, k_, lane_)                                                  \
  do {                                                                                        \
    const uint64_t *const feed_list = (list_);                                                \
    for (uint32_t b = 0; b < (k_); b += 64u)                                                  \
      if (!(top).insert(b + (lane_) < (k_) ? feed_list[b + (lane_)] : KEY_NONE, (lane_))) break; \
  } while (0)

// an ascending key list as a [k] list padded with KEY_NONE
__device__ __forceinline__ void ph_exact_store_list(uint64_t *out, const uint64_t *keys, uint32_t len, uint32_t k, uint32_t lane) {
  for (uint32_t i = lane; i < k; i += 64u) out[i] = i < len ? keys[i] : KEY_NONE;
}

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

// What a scan or tile wave leaves of (position, slice): the row of query q if this is the only slice and the kernel is
// not a PAIRS instance, else its list in the scratch [positions][slices][k].  A: as above, with slices and scratch.
template <bool PAIRS, class A>
__device__ __forceinline__ void ph_exact_write_slice(const A &a, uint32_t q, uint32_t pos, uint32_t slice, const uint64_t *keys,
                                                     uint32_t len, bool bad_query, uint32_t lane) {
  if (!PAIRS && a.slices == 1u)
    ph_exact_write_row(a, q, keys, len, bad_query, lane);
  else
    ph_exact_store_list(a.scratch + ((uint64_t)pos * a.slices + slice) * a.k, keys, len, a.k, lane);
}
