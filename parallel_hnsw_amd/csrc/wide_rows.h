// DistF32Wide<NV>: the distance policy of f32 rows of 1537 .. 4096 floats (NV = 8, 12, 16 float4 chunks per lane:
// ph_wide_chunk_count, phnsw_internal.h).
//
// DistRows keeps a whole candidate row in registers beside the query: U x NV float4 per lane, 256 VGPRs at NV = 16 and
// four rows in flight.  A lane's share of a distance is ONE fma chain over its chunks lane, lane + 64, ... in address
// order, sequential in the chunk index, so nothing asks for the row to be resident whole.  Here
//   * the query stays in registers (4 NV VGPRs), as in DistRows -- the prepare functions are DistRows' own;
//   * the U candidate rows of a round stream through in pieces of P chunks: two buffers of U x P float4, the loads of
//     piece p + 1 issued before the fmas of piece p, each row's accumulator carried from piece to piece;
//   * chain_piece continues a chain from a starting accumulator at a chunk offset with chain_partial's operations in
//     chain_partial's order, so the 64 partial sums are those one long chain_partial would give; they combine through
//     wave_sum4 and finalize_metric like every other distance -- the oracle's ORC_SUM_BLOCKED64 bits;
//   * chunks past nv4 (dim not a multiple of 256) load a clamped address and are dropped by a select, not a branch;
//     L2 runs the same chain on (q - x).
// The candidates of a hop are compacted as batch_distances compacts them (phnsw_device.h).
// profiles/wide_rows has the compiler's figures for the (P, U) shapes tried and the reason for the ones chosen.
#pragma once
#include <type_traits>

#include "phnsw_device.h"

// chunks K0 .. K0 + P - 1 of the chain chain_partial<NV> runs, continued from `a`
template <int NV, int P, int K0, bool EXACT, bool L2>
__device__ __forceinline__ float chain_piece(const float4 (&x)[P], const float4 (&q)[NV], uint32_t nv4, uint32_t lane, float a) {
#pragma unroll
  for (int k = 0; k < P; k++) {
    const float4 &qk = q[K0 + k];
    float t = a;
    if (L2) {
      float d0 = qk.x - x[k].x, d1 = qk.y - x[k].y, d2 = qk.z - x[k].z, d3 = qk.w - x[k].w;
      t = fmaf(d0, d0, t);
      t = fmaf(d1, d1, t);
      t = fmaf(d2, d2, t);
      t = fmaf(d3, d3, t);
    } else {
      t = fmaf(qk.x, x[k].x, t);
      t = fmaf(qk.y, x[k].y, t);
      t = fmaf(qk.z, x[k].z, t);
      t = fmaf(qk.w, x[k].w, t);
    }
    a = (EXACT || lane + 64u * (uint32_t)(K0 + k) < nv4) ? t : a;
  }
  return a;
}

// piece PI (chunks PI * P ..) of U rows into one buffer
template <int P, int U, int PI, bool EXACT>
__device__ __forceinline__ void wide_load_piece(const float4 *const (&row)[U], uint32_t nv4, uint32_t lane, float4 (&buf)[U][P]) {
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int k = 0; k < P; k++) {
      uint32_t c = lane + 64u * (uint32_t)(PI * P + k);
      if (!EXACT) c = c < nv4 ? c : nv4 - 1;
      buf[u][k] = row[u][c];
    }
}

// pieces PI, PI + 1, ... of the U chains: the next piece is requested into the other buffer before this one is used
template <int NV, int P, int U, int PI, bool EXACT, bool L2>
__device__ __forceinline__ void wide_pieces(const float4 *const (&row)[U], const float4 (&q)[NV], uint32_t nv4, uint32_t lane,
                                            float4 (&cur)[U][P], float4 (&nxt)[U][P], float (&acc)[U]) {
  // (the order is a request, not a guarantee: with one wave per SIMD allowed the scheduler moves later pieces' loads
  // forward as far as the register file lets it -- more rows' bytes in flight, no scratch; profiles/wide_rows)
  if constexpr (PI + 1 < NV / P) wide_load_piece<P, U, PI + 1, EXACT>(row, nv4, lane, nxt);
#pragma unroll
  for (int u = 0; u < U; u++) acc[u] = chain_piece<NV, P, PI * P, EXACT, L2>(cur[u], q, nv4, lane, acc[u]);
  if constexpr (PI + 1 < NV / P) wide_pieces<NV, P, U, PI + 1, EXACT, L2>(row, q, nv4, lane, nxt, cur, acc);
}

template <int NV, int P, int U, bool EXACT, bool L2>
__device__ __forceinline__ void wide_rows_partial_impl(const float4 *const (&row)[U], const float4 (&q)[NV], uint32_t nv4,
                                                       uint32_t lane, float (&acc)[U]) {
  static_assert(NV % P == 0, "a row is a whole number of pieces");
  float4 a[U][P], b[U][P];
  wide_load_piece<P, U, 0, EXACT>(row, nv4, lane, a);
#pragma unroll
  for (int u = 0; u < U; u++) acc[u] = 0.f;
  wide_pieces<NV, P, U, 0, EXACT, L2>(row, q, nv4, lane, a, b, acc);
}

template <int NV, int P, int U>
__device__ __forceinline__ void wide_rows_partial(const float4 *const (&row)[U], const float4 (&q)[NV], uint32_t nv4,
                                                  uint32_t lane, bool l2, float (&acc)[U]) {
  const bool exact = nv4 == 64u * NV;  // wave-uniform
  if (exact) {
    if (l2)
      wide_rows_partial_impl<NV, P, U, true, true>(row, q, nv4, lane, acc);
    else
      wide_rows_partial_impl<NV, P, U, true, false>(row, q, nv4, lane, acc);
  } else {
    if (l2)
      wide_rows_partial_impl<NV, P, U, false, true>(row, q, nv4, lane, acc);
    else
      wide_rows_partial_impl<NV, P, U, false, false>(row, q, nv4, lane, acc);
  }
}

// the (P, U) of a class: chunks per piece and rows in flight (profiles/wide_rows/README.md)
#ifndef PH_WIDE_P
#define PH_WIDE_P 4
#endif
#ifndef PH_WIDE_U
#define PH_WIDE_U 4
#endif

template <int NV, int P = PH_WIDE_P, int U = PH_WIDE_U>
struct DistF32Wide;
template <class D>
struct dist_is_wide : std::false_type {};
template <int NV, int P, int U>
struct dist_is_wide<DistF32Wide<NV, P, U>> : std::true_type {};

template <int NV, int P, int U>
struct DistF32Wide : DistRows<NV, U, RowF32> {
  static_assert(U % 4 == 0, "the rows of a round are summed four at a time (wave_sum4)");
  // distances of the query to the (up to 64) rows whose ids sit in the lanes flagged by `mask`; the result lands in
  // the lane that held the id (batch_distances' contract)
  __device__ __forceinline__ float batch(const PhDistArgs &d, uint64_t mask, uint32_t vid, uint32_t lane) const {
    float myd = 0.f;
    const uint32_t m = __popcll(mask);
    if (m == 0) return myd;
    const bool l2 = d.metric == PHNSW_METRIC_L2;
    // candidate number k (in lane order) leaves the byte offset of its row in lane k
    const bool cand = (mask >> lane) & 1ull;
    const uint32_t myrank = __popcll(mask & lanemask_lt(lane));
    const uint64_t off = (uint64_t)vid * (uint64_t)d.rows.stride;
    const int dst = (int)((cand ? myrank : 63u) << 2);  // non-candidates park in lane 63 (never read: m <= 63 there)
    uint32_t olo = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)off);
    uint32_t ohi = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)(off >> 32));
    if (m == 64) {  // every lane is a candidate: the permutation is the identity
      olo = (uint32_t)off;
      ohi = (uint32_t)(off >> 32);
    }
    for (uint32_t base = 0; base < m; base += U) {
      const float4 *r[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const uint32_t k = min(base + (uint32_t)u, m - 1u);  // short tail: the last row again (same value, unused)
        const uint64_t o = ((uint64_t)rl32(ohi, (int)k) << 32) | rl32(olo, (int)k);
        r[u] = (const float4 *)((const char *)d.rows.base + o);
      }
      float p[U];
      wide_rows_partial<NV, P, U>(r, this->qv, d.nv4, lane, l2, p);
      const uint32_t mine = myrank - base;  // < U when this is the lane's round
      // row u of a group of four ends in lanes {0, 32, 16, 48}[u] + 0..15 (wave_sum4)
#pragma unroll
      for (int g = 0; g < U; g += 4) {
        const float d4 = finalize_metric(wave_sum4(p[g], p[g + 1], p[g + 2], p[g + 3]), d.metric);
        const uint32_t u = (mine - g) & 3u;
        const uint32_t src = ((u & 1u) << 5) | ((u & 2u) << 3);  // 0, 32, 16, 48
        const float got = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)__float_as_uint(d4)));
        if (cand && mine >= (uint32_t)g && mine < (uint32_t)g + 4u) myd = got;
      }
    }
    return myd;
  }
};
