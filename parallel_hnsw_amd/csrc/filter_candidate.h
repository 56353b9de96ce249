// Which VectorIds a filtered call may return: the one candidate test of the exact scan, of the candidate count
// (filter_exact.hip) and of the routed call's e_q (filter_auto.hip).  Device code.
//
//   v is a candidate (exclude aside) iff v < n, bit v of the bitmap is set and v is a vector of the bottom layer
#pragma once
#include "phnsw_device.h"

// VectorIds of the bottom layer lie below this: an identity layer holds 0 .. n_nodes - 1, any other layer's largest
// vector is its last node (nodes ascend), and vec2node has an entry for every id up to that one
__device__ __forceinline__ uint32_t ph_exact_id_limit(uint32_t n, uint32_t n_nodes, const uint32_t *nodes,
                                                      const uint32_t *vec2node) {
  if (n_nodes == 0) return 0u;
  return min(n, vec2node ? nodes[n_nodes - 1u] + 1u : n_nodes);
}

// word `widx` of a bitmap reduced to candidates: bits at or past the limit cleared, then the bits of vectors the
// bottom layer does not hold.  bitmap == nullptr: every bit set.
__device__ __forceinline__ uint32_t ph_exact_word(const uint32_t *bitmap, uint32_t widx, uint32_t nwords, uint32_t nlim,
                                                  const uint32_t *vec2node) {
  if (widx >= nwords) return 0u;
  const uint32_t first = widx * 32u;  // widx < nwords <= 2^26
  if (first >= nlim) return 0u;
  uint32_t w = bitmap ? bitmap[widx] : 0xFFFFFFFFu;
  if (nlim - first < 32u) w &= (1u << (nlim - first)) - 1u;
  if (vec2node)
    for (uint32_t t = w; t; t &= t - 1u) {
      const uint32_t b = (uint32_t)__ffs((int)t) - 1u;
      if (vec2node[first + b] == PH_EMPTY32) w &= ~(1u << b);  // first + b < nlim
    }
  return w;
}

// the same test for one id: bit v & 31 of ph_exact_word(bitmap, v >> 5, ..)
__device__ __forceinline__ bool ph_exact_is_candidate(const uint32_t *bitmap, uint32_t v, uint32_t nlim,
                                                      const uint32_t *vec2node) {
  if (v >= nlim) return false;  // nlim <= n: the word of v exists
  if (bitmap && !((bitmap[v >> 5] >> (v & 31u)) & 1u)) return false;
  return !vec2node || vec2node[v] != PH_EMPTY32;
}
