// Dense top layers: the LDS-staged queries x rows tile pass of the search path.
//
// Every query of Hnsw::search walks ALL layers (/root/reference/src/search.rs:113-137), and in
// the small ones at the top -- 4 / 48 / 578 nodes of a 1M-vector index with the default order 12
// (lib.rs:1883-1899) -- a queue of number_of_candidates >= 100 makes closest_nodes
// (lib.rs:175-248) evaluate nearly every node.  Reading those few hundred rows once per query
// is the one place on the traversal where a batch of queries meets the SAME candidate rows, so
// it is done as a tile pass instead of a gather:
//
//   ph_tiny_table_kernel   D[position][node] = compare_vec(query, Stored(node's vector)) for every
//                          query of the launch and every node of the largest small layer.  A
//                          256-thread block stages 8 rows in LDS (ds_write_b128) and its 4 waves
//                          hold 8 queries each in registers: one LDS read of a row feeds 8 fma
//                          chains.  The chain is chain_partial (phnsw_device.h) and the 64 partial
//                          sums are combined in the butterfly's order, so D holds exactly the bits
//                          the per-hop evaluation would produce.  64 results (8 queries x 8 rows)
//                          are reduced together: two registers are folded into one per step
//                          (lanes pick their half), 63 shuffles instead of 384.
//   ph_tiny_prep_kernel    neighbour rows of the small layers rewritten in the id space of the
//                          largest one ("table ids": layers are nested and their node lists are
//                          sorted, lib.rs:685 / search.rs:150-157, so NodeId order == table-id
//                          order and queue ties break identically), plus a membership mask.
//
//   ph_tiny_table_mfma_kernel  the same table on the matrix cores for dot-product metrics over rows of whole
//                          64-chunk groups (256 / 768 / 1536 floats): chains of v_mfma_f32_32x32x1_2b_f32, one
//                          fused multiply-add per K step, visited in the butterfly's own tree order -- the same
//                          bits again (see the comment above the kernel).
//
// search.hip then walks those layers with its visited set and its table row in LDS and never
// touches a vector row there.  Compute bound, not HBM: 2*dim flop per entry at the f32 vector or matrix rate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "phnsw_device.h"

struct PhTinyPrepArgs {
  PhLayerDev layers[PH_TINY_MAX_LAYERS];
  uint32_t T, tiny_n;
  uint32_t off[PH_TINY_MAX_LAYERS];
  uint32_t *nbr;
  uint32_t *member;  // [tiny_n + 1]
};

__global__ void ph_tiny_prep_kernel(PhTinyPrepArgs p) {
  const uint32_t l = blockIdx.y;
  const PhLayerDev L = p.layers[l], TL = p.layers[p.T - 1];
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n_nodes; i += gridDim.x * blockDim.x) {
    const uint32_t vid = L.nodes[i];
    const uint32_t t = TL.vec2node ? TL.vec2node[vid] : vid;
    if (t >= p.tiny_n) {  // a node of layer l that the table layer lacks: not nested, table unusable
      p.member[p.tiny_n] = 1u;
      continue;
    }
    atomicOr(&p.member[t], 1u << l);
    for (uint32_t k = 0; k < L.W; k++) {
      const uint32_t nb = L.neighbors[(uint64_t)i * L.W + k];
      uint32_t tn = PH_EMPTY32;
      if (nb < L.n_nodes) {
        const uint32_t v2 = L.nodes[nb];
        tn = TL.vec2node ? TL.vec2node[v2] : v2;
        if (tn >= p.tiny_n) {
          p.member[p.tiny_n] = 1u;
          tn = PH_EMPTY32;
        }
      }
      p.nbr[p.off[l] + (uint64_t)t * L.W + k] = tn;
    }
  }
}

struct PhTinyTableArgs {
  PhDistArgs dist;
  const float *queries;
  uint32_t ldq;
  const uint32_t *qids;
  const uint32_t *order;
  uint32_t npos;
  const uint32_t *tnodes;  // table id -> VectorId
  uint32_t tiny_n, stride;
  float *D;
  uint32_t rows_per_slice;  // multiple of 8
  uint32_t dbg;             // PHNSW_TINY_DBG (experiments): 1 = no table stores, 2 = stage only the first tile
};

// two registers folded into one: lanes whose bit `m` is clear keep A's butterfly step, the others
// B's -- the same two operands as v += shfl_xor(v, m) on each (f32 add is commutative, so which
// of the two comes first does not change the bits).  m = 32 / 16 are one v_permlane{32,16}_swap
// (gfx950) + one add; 8, 2, 1 one DPP move (row_ror:8, quad_perm); 4 two DPP moves with bank masks.
template <int M>
__device__ __forceinline__ float fold2(float A, float B, uint32_t lane) {
#ifdef PH_FOLD_GENERIC
  const bool hi = (lane & M) != 0;
  const float own = hi ? B : A, other = hi ? A : B;
  return own + __shfl_xor(other, M);
#else
  if constexpr (M == 32) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(A), __float_as_uint(B), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  } else if constexpr (M == 16) {
    auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(A), __float_as_uint(B), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
  } else {
    const bool hi = (lane & M) != 0;
    const float own = hi ? B : A, other = hi ? A : B;
    const int o = (int)__float_as_uint(other);
    int t;
    if constexpr (M == 8) {
      t = __builtin_amdgcn_update_dpp(0, o, 0x128, 0xF, 0xF, true);  // row_ror:8
    } else if constexpr (M == 4) {
      t = __builtin_amdgcn_update_dpp(o, o, 0x114, 0xF, 0xA, false);  // row_shr:4 into lanes 4-7, 12-15
      t = __builtin_amdgcn_update_dpp(t, o, 0x104, 0xF, 0x5, false);  // row_shl:4 into lanes 0-3, 8-11
    } else if constexpr (M == 2) {
      t = __builtin_amdgcn_update_dpp(0, o, 0x4E, 0xF, 0xF, true);  // quad_perm [2,3,0,1]
    } else {
      t = __builtin_amdgcn_update_dpp(0, o, 0xB1, 0xF, 0xF, true);  // quad_perm [1,0,3,2]
    }
    return own + __uint_as_float((uint32_t)t);
  }
#endif
}

template <int NV, int QT, bool EXACT, bool L2>
__device__ __forceinline__ void tiny_tile(const float4 *lds, const ph_f2 (&qv)[QT / 2][NV][4], uint32_t nv4, uint32_t lane,
                                          float &V) {
  float R[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    float4 x[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) x[k] = lds[(i * NV + k) * 64 + lane];
    float p[QT];
    ph_f2 pp[QT / 2];
    chain_partial2<NV, QT / 2, EXACT, L2>(x, qv, nv4, lane, pp);
#pragma unroll
    for (int j = 0; j < QT / 2; j++) {
      p[2 * j] = pp[j].x;
      p[2 * j + 1] = pp[j].y;
    }
    if constexpr (QT == 8) {
      float f0 = fold2<32>(p[0], p[1], lane), f1 = fold2<32>(p[2], p[3], lane);
      float f2 = fold2<32>(p[4], p[5], lane), f3 = fold2<32>(p[6], p[7], lane);
      float g0 = fold2<16>(f0, f1, lane), g1 = fold2<16>(f2, f3, lane);
      R[i] = fold2<8>(g0, g1, lane);
    } else {
      float f0 = fold2<32>(p[0], p[1], lane), f1 = fold2<32>(p[2], p[3], lane);
      R[i] = fold2<16>(f0, f1, lane);
    }
  }
  constexpr int M0 = QT == 8 ? 4 : 8;
  float h0 = fold2<M0>(R[0], R[1], lane), h1 = fold2<M0>(R[2], R[3], lane);
  float h2 = fold2<M0>(R[4], R[5], lane), h3 = fold2<M0>(R[6], R[7], lane);
  float e0 = fold2<M0 / 2>(h0, h1, lane), e1 = fold2<M0 / 2>(h2, h3, lane);
  V = fold2<M0 / 4>(e0, e1, lane);
  if constexpr (QT == 4) V += __shfl_xor(V, 1);
}

// R: how the stored rows are read (RowF32, or RowF16 / RowI8: the halves of an f16 store widened, the codes of an i8
// store dequantised, as they are staged, so the tile pass below sees the f32 operands it always saw)
template <int NV, int QT, class R = RowF32>
__global__ __launch_bounds__(256) void ph_tiny_table_kernel(PhTinyTableArgs a) {
  __shared__ float4 rows_lds[8 * NV * 64];
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const uint32_t nv4 = a.dist.nv4;
  const uint32_t p0 = (blockIdx.x * 4u + w) * QT;
  // queries in pairs: qv[j][k][e] = component e of chunk k of (query 2j, query 2j + 1)
  ph_f2 qv[QT / 2][NV][4];
#pragma unroll
  for (int j = 0; j < QT; j++) {
    const uint32_t p = p0 + j;
    const bool valid = p < a.npos;
    const uint32_t q = valid ? (a.order ? a.order[p] : p) : 0u;
    const float4 *src = nullptr;
    const typename R::chunk *srcs = nullptr;  // a stored query
    typename R::aux sax = typename R::aux();
    if (valid) {
      if (a.queries)
        src = (const float4 *)(a.queries + (uint64_t)q * a.ldq);
      else {
        srcs = R::row(a.dist.rows, a.qids[q]);
        sax = R::row_aux(srcs);
      }
    }
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const uint32_t c = lane + 64u * k;
      const float4 v = (valid && c < nv4) ? (src ? src[c] : R::widen(R::load(srcs, c), sax)) : make_float4(0.f, 0.f, 0.f, 0.f);
      qv[j / 2][k][0][j & 1] = v.x;
      qv[j / 2][k][1][j & 1] = v.y;
      qv[j / 2][k][2][j & 1] = v.z;
      qv[j / 2][k][3][j & 1] = v.w;
    }
  }
  const bool exact = nv4 == 64u * NV, l2 = a.dist.metric == PHNSW_METRIC_L2;
  const uint32_t r_begin = blockIdx.y * a.rows_per_slice;
  const uint32_t r_end = min(a.tiny_n, r_begin + a.rows_per_slice);
  for (uint32_t r0 = r_begin; r0 < r_end; r0 += 8) {
    __syncthreads();  // the previous tile has been consumed
    if (!(a.dbg & 2u) || r0 == r_begin)
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint32_t slot = 2u * w + u;
      const uint32_t rr = min(r0 + slot, a.tiny_n - 1u);
      const typename R::chunk *src = R::row(a.dist.rows, a.tnodes[rr]);
      const typename R::aux ax = R::row_aux(src);
#pragma unroll
      for (int k = 0; k < NV; k++) {
        uint32_t c = lane + 64u * k;
        c = c < nv4 ? c : nv4 - 1u;
        rows_lds[(slot * NV + k) * 64 + lane] = R::widen(R::load(src, c), ax);
      }
    }
    __syncthreads();
    float V;
    if (exact) {
      if (l2)
        tiny_tile<NV, QT, true, true>(rows_lds, qv, nv4, lane, V);
      else
        tiny_tile<NV, QT, true, false>(rows_lds, qv, nv4, lane, V);
    } else {
      if (l2)
        tiny_tile<NV, QT, false, true>(rows_lds, qv, nv4, lane, V);
      else
        tiny_tile<NV, QT, false, false>(rows_lds, qv, nv4, lane, V);
    }
    // lane -> (query j, row i) after the folds: the first log2(QT) levels chose the query, the next three the row
    uint32_t j, i;
    bool writer = true;
    if (QT == 8) {
      j = ((lane >> 5) & 1u) | (((lane >> 4) & 1u) << 1) | (((lane >> 3) & 1u) << 2);
      i = ((lane >> 2) & 1u) | (((lane >> 1) & 1u) << 1) | ((lane & 1u) << 2);
    } else {
      j = ((lane >> 5) & 1u) | (((lane >> 4) & 1u) << 1);
      i = ((lane >> 3) & 1u) | (((lane >> 2) & 1u) << 1) | (((lane >> 1) & 1u) << 2);
      writer = (lane & 1u) == 0u;
    }
    const uint32_t p = p0 + j, r = r0 + i;
    if (writer && p < a.npos && r < r_end && !(a.dbg & 1u)) a.D[(uint64_t)p * a.stride + r] = finalize_metric(V, a.dist.metric);
  }
}

// ------------------------------------------------------------------ the same table on the matrix cores
//
// D[position][node] is a GEMM, but its bits are fixed by the per-hop evaluation: lane l of a wave chains
// fma(x, q, acc) over the 4 components of float4 chunks l, l + 64, ... (chain_partial) and the 64 partial sums
// meet in the xor-butterfly's tree (32, 16, 8, 4, 2, 1).  v_mfma_f32_32x32x1_2b_f32 performs exactly one fused
// multiply-add per output element and K step (measured bit-identical to v_fma_f32 including denormals:
// scripts/micro/mfma_fma_exact.hip), so a chain of NV*4 such instructions over the columns of lane l builds
// p_l for 32 x 32 (position, node) pairs at once -- its two blocks take lanes l and l + 32, whose sum is the
// butterfly's first step.  The 32 sums s1[l] are visited in bit-reversed order, which is a depth-first walk of
// the butterfly's tree: finished subtrees are added as soon as both halves exist, five pending 32 x 32 tiles at
// most.  Operands are packed once per launch (ph_tiny_pack_kernel) so that what a leaf needs of 32 rows is one
// contiguous, lane-ordered run: [row tile][leaf t][chunk k][block b][row x] float4.
typedef float ph_f32x32 __attribute__((ext_vector_type(32)));

__host__ __device__ constexpr uint32_t ph_rev5(uint32_t t) {
  return ((t & 1u) << 4) | ((t & 2u) << 2) | (t & 4u) | ((t & 8u) >> 2) | ((t & 16u) >> 4);
}

struct PhTinyPackArgs {
  PhRows rows;  // stored rows: widened / dequantised here, the packed operand is f32 whatever their kind
  const float *queries;  // raw query rows, or nullptr: rows are stored vectors
  uint32_t ldq;
  const uint32_t *ids;    // row -> VectorId of a stored vector (when queries == nullptr)
  const uint32_t *order;  // nullable: row r reads entry order[r]
  uint32_t n, n_pad;      // rows, rows rounded up to the block tile (the rest is zero)
  uint32_t nv;            // float4 chunks per lane
  float4 *out;
};

template <class R>
__device__ __forceinline__ float4 tiny_pack_stored(const PhRows &rows, uint32_t vid, uint32_t c) {
  const typename R::chunk *src = R::row(rows, vid);
  return R::widen(R::load(src, c), R::row_aux(src));
}
// blockDim (32 rows, 8 chunks): a row's 8 chunks are one 128-byte read, a chunk's 32 rows one 512-byte write
__global__ void ph_tiny_pack_kernel(PhTinyPackArgs p) {
  const uint32_t r = blockIdx.x * 32u + threadIdx.x;
  const uint32_t c = blockIdx.y * 8u + threadIdx.y;  // < 64 * nv
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r < p.n) {
    const uint32_t e = p.order ? p.order[r] : r;
    if (p.queries) {
      v = ((const float4 *)(p.queries + (uint64_t)e * p.ldq))[c];
    } else {
      switch (p.rows.kind) {
        case PH_ROWS_F16: v = tiny_pack_stored<RowF16>(p.rows, p.ids[e], c); break;
        case PH_ROWS_I8: v = tiny_pack_stored<RowI8>(p.rows, p.ids[e], c); break;
        default: v = tiny_pack_stored<RowF32>(p.rows, p.ids[e], c); break;
      }
    }
  }
  const uint32_t t = ph_rev5(c & 31u), b = (c >> 5) & 1u, k = c >> 6;
  p.out[(((((uint64_t)(r >> 5) * 32u + t) * p.nv + k) * 2u + b) << 5) + (r & 31u)] = v;
}

struct PhTinyMfmaArgs {
  const float4 *pq, *pn;  // packed positions / nodes
  uint32_t npos, tiny_n, stride;
  uint32_t qtiles, ntiles;  // 64-row block tiles along each side
  int metric;
  float *D;
};

// 256 threads = 4 waves, block tile 64 positions x 64 nodes, wave w: positions half w & 1, nodes half w >> 1.
// G leaves of all four 32-row tiles are staged per step (double buffered: the next step's global loads are in
// flight while the matrix cores work on this one); wave w stages row tile w (0, 1: positions; 2, 3: nodes), G * NV
// wave-wide loads of 1 KiB per step.  The butterfly's tree is written as a compile-time recursion, so that the
// pending partial tiles are plain locals (five at most) and every index is a constant.
template <int NV, int G>
struct PhMfmaTile {
  static constexpr int TILE4 = G * NV * 64;  // float4 of one row tile in one step
  static constexpr int BUF4 = 4 * TILE4;
  static constexpr int NG = 32 / G;
  float4 *sm4;
  const float4 *mysrc;   // this wave's row tile in the packed operand, + lane
  const float4 *A0, *B0;  // this wave's operand tiles in LDS buffer 0, + lane
  float4 *mydst;          // where this wave parks its row tile in LDS buffer 0, + lane
  float4 stage[G * NV];

  __device__ __forceinline__ void fetch(int g) {
#pragma unroll
    for (int i = 0; i < G * NV; i++) stage[i] = mysrc[g * TILE4 + i * 64];
  }
  __device__ __forceinline__ void park(int buf) {
#pragma unroll
    for (int i = 0; i < G * NV; i++) mydst[buf * BUF4 + i * 64] = stage[i];
  }
  // s1 of leaf T: p_l + p_(l + 32) for l = ph_rev5(T), 32 x 32 pairs (16 registers per lane)
  template <int T>
  __device__ __forceinline__ void leaf(float (&out)[16]) {
    constexpr int g = T / G, tt = T % G;
    if (tt == 0 && g + 1 < NG) fetch(g + 1);
    ph_f32x32 acc;
#pragma unroll
    for (int v = 0; v < 32; v++) acc[v] = 0.f;
#pragma unroll
    for (int k = 0; k < NV; k++) {
      const float4 qa = A0[(g & 1) * BUF4 + (tt * NV + k) * 64];
      const float4 xb = B0[(g & 1) * BUF4 + (tt * NV + k) * 64];
      acc = __builtin_amdgcn_mfma_f32_32x32x1f32(qa.x, xb.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x1f32(qa.y, xb.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x1f32(qa.z, xb.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x1f32(qa.w, xb.w, acc, 0, 0, 0);
    }
#pragma unroll
    for (int v = 0; v < 16; v++) {
      out[v] = acc[v] + acc[v + 16];
      // pins the add here: instruction selection otherwise keeps all 32 leaves' accumulators (spilled) and adds at the end
      asm volatile("" : "+v"(out[v]));
    }
    if (tt == G - 1) {
      if (g + 1 < NG) park((g + 1) & 1);
      __syncthreads();
    }
  }
  // the subtree of 2^L leaves starting at leaf T0 (bit-reversed leaf order = the butterfly's pairing, deepest first)
  template <int L, int T0>
  __device__ __forceinline__ void subtree(float (&out)[16]) {
    if constexpr (L == 0) {
      leaf<T0>(out);
    } else {
      float lo[16], hi[16];
      subtree<L - 1, T0>(lo);
      subtree<L - 1, T0 + (1 << (L - 1))>(hi);
#pragma unroll
      for (int v = 0; v < 16; v++) {
        out[v] = lo[v] + hi[v];
        asm volatile("" : "+v"(out[v]));
      }
    }
  }
};

//
// G = 2 is the form of a launch that has the chip to itself.  G = 1 is the form that runs BESIDE the other workspace's
// search kernel (ph_tiny_prepare): half the LDS (24 KiB at NV = 3, the hole the search waves of a CU leave together,
// search.hip: vis_table_slots) and at most 128 registers, which is what two resident search waves of 192 leave of a
// SIMD's 512.  The staging depth changes neither the order of the leaves nor anything inside one, so both forms give
// the same bits.
template <int NV, int G>
__global__ __launch_bounds__(256, G == 1 ? 4 : 1) void ph_tiny_table_mfma_kernel(PhTinyMfmaArgs a) {
  extern __shared__ float4 sm4[];
  using Tile = PhMfmaTile<NV, G>;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  // XCD-aware tile order: blocks are dealt round-robin to the 8 XCDs, so the blocks one L2 sees are B % 8 == xcd;
  // each XCD walks its own 8 x 8 super-tiles (8 position tiles x 8 node tiles = 3 MiB of operands, inside its L2)
  const uint32_t B = blockIdx.x, xcd = B & 7u, slot = B >> 3;
  const uint32_t sq = (a.qtiles + 7u) / 8u;  // super-tiles along positions
  const uint32_t super = (slot >> 6) * 8u + xcd, within = slot & 63u;
  const uint32_t qt = (super % sq) * 8u + (within & 7u), nt = (super / sq) * 8u + (within >> 3);
  if (qt >= a.qtiles || nt >= a.ntiles) return;  // the whole block
  Tile t;
  t.sm4 = sm4;
  t.mysrc = (w < 2u ? a.pq + (uint64_t)(2u * qt + w) * (32u * NV * 64u)
                    : a.pn + (uint64_t)(2u * nt + (w - 2u)) * (32u * NV * 64u)) + lane;
  t.mydst = sm4 + w * Tile::TILE4 + lane;
  t.A0 = sm4 + (w & 1u) * Tile::TILE4 + lane;
  t.B0 = sm4 + (2u + (w >> 1)) * Tile::TILE4 + lane;
  t.fetch(0);
  t.park(0);
  __syncthreads();
  float V[16];
  t.template subtree<5, 0>(V);
  // 32x32 accumulator layout: register v of lane L holds row 8 * (v / 4) + 4 * (L / 32) + v % 4, column L % 32;
  // rows are the A operand's (positions), columns the B operand's (nodes): a register is two 128-byte row pieces
  const uint32_t r = (2u * nt + (w >> 1)) * 32u + (lane & 31u);
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const uint32_t p = (2u * qt + (w & 1u)) * 32u + 8u * (v / 4) + 4u * (lane >> 5) + (v & 3);
    if (p < a.npos && r < a.tiny_n) a.D[(uint64_t)p * a.stride + r] = finalize_metric(V[v], a.metric);
  }
}

// ------------------------------------------------------------------ the table of an i8q store: an int8 GEMM
//
// D[p][t] = ph_i8q_distance(sq[p], sr[t], idot, metric) with idot = sum_j cq[p][j] * cr[t][j] in int32.  An integer
// sum has the same bits in any order, so the table needs neither the packed operand layout nor the butterfly-order
// recursion of the f32 kernel above: the operands are plain row-major code matrices [rows_pad][K_pad] with one scale
// per row, K zero-padded to a whole staging step (zeros add nothing, so ragged dimensions and launches of a few
// queries take the same kernel), and the kernel is a textbook tiled GEMM on v_mfma_i32_32x32x32_i8.
//
// ph_tiny_quant_kernel makes an operand: one wave per row.  A raw query goes through the quantiser of the rows
// (ph_i8_scale / ph_i8_quant4, the functions DistI8Q::prepare_raw calls); a stored vector -- a stored query or a node
// of the table layer -- is its row's codes and scale copied as they are.
#define PH_I8T_KS 128u                 // code bytes of a row staged per step (four MFMAs deep)
#define PH_I8T_ROW (PH_I8T_KS + 16u)   // LDS bytes per staged row: the 16-byte pad spreads a 16-lane read over all banks
#define PH_I8T_LDS (2u * 64u * PH_I8T_ROW)  // 18 KiB: fits the hole a running search kernel leaves (24 KiB, search.hip)

struct PhTinyQuantArgs {
  PhRows rows;
  const float *queries;   // raw query rows, or nullptr: rows are stored vectors
  uint32_t ldq, nv4;      // nv4: float4 chunks (= code words) of a vector
  const uint32_t *ids;    // row -> VectorId of a stored vector (when queries == nullptr)
  const uint32_t *order;  // nullable: row r reads entry order[r]
  uint32_t n, n_pad;      // rows, rows rounded up to the block tile (the rest: codes 0, scale 0)
  uint32_t kw;            // K_pad / 4: code words per operand row
  uint32_t *codes;        // [n_pad][kw]
  float *scales;          // [n_pad]
};

__global__ __launch_bounds__(256) void ph_tiny_quant_kernel(PhTinyQuantArgs p) {
  const uint32_t lane = threadIdx.x & 63u, r = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (r >= p.n_pad) return;
  uint32_t *dst = p.codes + (uint64_t)r * p.kw;
  float scale = 0.f;
  if (r >= p.n) {
    for (uint32_t c = lane; c < p.kw; c += 64u) dst[c] = 0u;
  } else {
    const uint32_t e = p.order ? p.order[r] : r;
    if (p.queries) {
      const float4 *q = (const float4 *)(p.queries + (uint64_t)e * p.ldq);
      float m = 0.f;
      for (uint32_t c = lane; c < p.nv4; c += 64u) m = ph_maxabs4(m, q[c]);
      scale = ph_i8_scale(wave_max(m));
      for (uint32_t c = lane; c < p.kw; c += 64u) dst[c] = c < p.nv4 ? ph_i8_quant4(q[c], scale) : 0u;
    } else {
      const uint32_t *row = RowI8::row(p.rows, p.ids[e]);
      scale = RowI8::row_aux(row);
      for (uint32_t c = lane; c < p.kw; c += 64u) dst[c] = c < p.nv4 ? RowI8::load(row, c) : 0u;
    }
  }
  if (lane == 0) p.scales[r] = scale;
}

typedef int ph_i32x4 __attribute__((ext_vector_type(4)));
typedef int ph_i32x16 __attribute__((ext_vector_type(16)));

struct PhTinyI8Args {
  const ph_i32x4 *cq, *cn;  // code matrices of the positions / the nodes, [rows_pad][k16] runs of 16 codes
  const float *sq, *sn;    // their scales
  uint32_t npos, tiny_n, stride;
  uint32_t k16;            // K_pad / 16 (a multiple of PH_I8T_KS / 16)
  int metric;
  float *D;
};

// 256 threads = 4 waves, block tile 64 positions x 64 nodes, wave w: positions half w & 1, nodes half w >> 1 (as
// the f32 kernel).  Per step, PH_I8T_KS code bytes of the 64 + 64 rows are staged in LDS (the next step's global loads
// are in flight while the matrix cores work on this one) and every wave issues four MFMAs: lane l feeds row l % 32 with
// the 16 codes at byte 16 * (l / 32) of each 32-byte K slab -- whichever K positions the instruction assigns to a
// lane's 16 bytes, it assigns them alike on both operands, and the sum does not care.  One form: 18 KiB of LDS and 4
// blocks per CU, so it always fits beside a running search kernel and PHNSW_TABLE_BESIDE has nothing to choose.
__global__ __launch_bounds__(256, 4) void ph_tiny_table_i8_kernel(PhTinyI8Args a) {
  __shared__ ph_i32x4 sm[PH_I8T_LDS / 16u];
  constexpr uint32_t ROW16 = PH_I8T_ROW / 16u, KS16 = PH_I8T_KS / 16u;  // 16-byte runs per staged row / of it that are codes
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  const uint32_t qt = blockIdx.x, nt = blockIdx.y;
  // staging: thread t moves run t % 8 of rows t / 8 and t / 8 + 32, for both operands
  const uint32_t srow = tid / KS16, scol = tid % KS16;
  const ph_i32x4 *gq = a.cq + ((uint64_t)qt * 64u + srow) * a.k16 + scol;
  const ph_i32x4 *gn = a.cn + ((uint64_t)nt * 64u + srow) * a.k16 + scol;
  ph_i32x4 *lq = sm + srow * ROW16 + scol, *ln = sm + (64u + srow) * ROW16 + scol;
  const ph_i32x4 *A = sm + ((w & 1u) * 32u + (lane & 31u)) * ROW16 + (lane >> 5);
  const ph_i32x4 *B = sm + (64u + (w >> 1) * 32u + (lane & 31u)) * ROW16 + (lane >> 5);
  ph_i32x16 acc;
#pragma unroll
  for (int v = 0; v < 16; v++) acc[v] = 0;
  const uint64_t half = (uint64_t)32u * a.k16;  // 32 operand rows on
  ph_i32x4 q0 = gq[0], q1 = gq[half], n0 = gn[0], n1 = gn[half];
  const uint32_t steps = a.k16 / KS16;
  for (uint32_t s = 0; s < steps; s++) {
    __syncthreads();  // the previous step has been consumed
    lq[0] = q0;
    lq[32u * ROW16] = q1;
    ln[0] = n0;
    ln[32u * ROW16] = n1;
    __syncthreads();
    if (s + 1u < steps) {
      const uint32_t o = (s + 1u) * KS16;
      q0 = gq[o];
      q1 = gq[half + o];
      n0 = gn[o];
      n1 = gn[half + o];
    }
#pragma unroll
    for (uint32_t j = 0; j < KS16 / 2u; j++) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[2u * j], B[2u * j], acc, 0, 0, 0);
  }
  // 32x32 accumulator layout: register v of lane L holds row 8 * (v / 4) + 4 * (L / 32) + v % 4, column L % 32;
  // rows are the A operand's (positions), columns the B operand's (nodes)
  const uint32_t r = (2u * nt + (w >> 1)) * 32u + (lane & 31u);
  const float sr = a.sn[r];  // (padded to the tile)
#pragma unroll
  for (int v = 0; v < 16; v++) {
    const uint32_t p = (2u * qt + (w & 1u)) * 32u + 8u * (v / 4) + 4u * (lane >> 5) + (v & 3);
    if (p < a.npos && r < a.tiny_n) a.D[(uint64_t)p * a.stride + r] = ph_i8q_distance(a.sq[p], sr, acc[v], a.metric);
  }
}

// ------------------------------------------------------------------ host side

void ph_tiny_free(PhWorkspace &ws) {
  ws.tiny_prep_key = PhTinyPrepKey();
  ws.tiny_pack_key = PhTinyPackKey();
  if (ws.tiny_d) hipFree(ws.tiny_d);
  if (ws.tiny_nbr) hipFree(ws.tiny_nbr);
  if (ws.tiny_member) hipFree(ws.tiny_member);
  if (ws.tiny_pq) hipFree(ws.tiny_pq);
  if (ws.tiny_pn) hipFree(ws.tiny_pn);
  ws.tiny_pq = ws.tiny_pn = nullptr;
  ws.tiny_pq_bytes = ws.tiny_pn_bytes = 0;
  ws.tiny_d = nullptr;
  ws.tiny_nbr = ws.tiny_member = nullptr;
  ws.tiny_d_bytes = ws.tiny_nbr_bytes = ws.tiny_member_bytes = 0;
}

// rows the matrix-core table kernel takes: a dot-product metric over whole 64-chunk rows (256 / 768 / 1536 floats)
static bool tiny_mfma_shape(int metric, uint32_t ld) {
  return metric != PHNSW_METRIC_L2 && (ld == 256u || ld == 768u || ld == 1536u) && !getenv("PHNSW_TINY_VALU");
}

// PHNSW_TABLE_BESIDE = 0: the table pass never runs beside a search kernel (G = 2 always, no hole in the search
// kernel's LDS); 1: always the G = 1 form; auto (default): G = 1 when the index's other workspace has a launch in flight
static int table_beside_mode() {
  const char *e = getenv("PHNSW_TABLE_BESIDE");
  if (!e || !strcmp(e, "auto")) return 2;
  return atoi(e) > 0 ? 1 : 0;
}
static bool tiny_keep_off() { return getenv("PHNSW_NO_TINY_KEEP") != nullptr; }  // tests: prep and node pack every launch
static size_t tiny_mfma_lds(int nv, int g) { return (size_t)2 * 4 * g * nv * 64 * sizeof(float4); }

// an i8q store's table always comes from the int8 matrix-core kernel (PHNSW_TINY_VALU means nothing to it)
bool ph_tiny_matrix_cores(const phnsw_index *ix) {
  return ix->store->kind == PH_ROWS_I8Q || tiny_mfma_shape(ix->store->metric, ix->store->ld);
}

// Which leading layers run densely.  Measured at 1M x 768 (100 000 queries): the vector-unit tile pass costs
// 0.030 us per (query, node), the matrix-core one 0.016 us, a table lookup on the walk 0.08 us, a gathered
// evaluation 0.28-0.35 us; closest_nodes evaluates about 7 x number_of_candidates nodes of a layer it cannot
// exhaust.  A layer of n nodes is therefore worth a table when n * cost < 7 * ef * 0.2, i.e. n <= 48 * ef (80 * ef
// on the matrix cores) and <= PH_TINY_MAX_NODES: at ef 104 the 7 000-node layer of a 1M x 768 cosine index is
// tabulated on the matrix cores and stays on the per-hop path otherwise; at ef >= 150 (and in every build round,
// ef 300) it is tabulated either way.  PHNSW_TINY_MAX overrides.
uint32_t ph_tiny_layer_count(const phnsw_index *ix, uint32_t n_layers, uint32_t ef) {
  const bool off = getenv("PHNSW_NO_TINY") != nullptr;  // tests compare both paths
  if (off || (!ph_store_f32(ix->store) && !ph_store_converted(ix->store)) || !ph_chunk_count(ix->store->ld / 4)) return 0;
  const uint64_t per_ef = ph_tiny_matrix_cores(ix) ? 80ull : 48ull;
  uint64_t cap = std::min<uint64_t>(PH_TINY_MAX_NODES, per_ef * ef);
  if (const char *e = getenv("PHNSW_TINY_MAX"))
    if (atoi(e) > 0) cap = std::min<uint64_t>(PH_TINY_MAX_NODES, (uint64_t)atoi(e));
  uint32_t T = 0;
  while (T < n_layers && T < PH_TINY_MAX_LAYERS && ix->layers[T].n_nodes <= cap) T++;
  return T;
}

static uint32_t tiny_stride_of(uint32_t n) { return (n + 63u) / 64u * 64u; }

// the table of one launch is kept below 4 GiB (PHNSW_TINY_TABLE_BYTES overrides: tests, small devices); longer
// query lists run in chunks (api.hip)
uint64_t ph_tiny_max_positions(const phnsw_index *ix, uint32_t n_layers, uint32_t ef) {
  uint32_t T = ph_tiny_layer_count(ix, n_layers, ef);
  if (!T) return 0;
  uint64_t budget = 4ull << 30;
  if (const char *e = getenv("PHNSW_TINY_TABLE_BYTES"))
    if (atoll(e) > 0) budget = (uint64_t)atoll(e);
  return std::max<uint64_t>(64, budget / ((uint64_t)tiny_stride_of(ix->layers[T - 1].n_nodes) * 4u));
}

// what a search launch leaves free of a CU's LDS: one block of the G = 1 table kernel, when the launches of this index
// get their table from that kernel (per launch, on the matrix cores)
size_t ph_tiny_beside_lds(const phnsw_index *ix, const PhSearchArgs &a) {
  if (!a.tiny_layers || a.tiny_rows || !table_beside_mode()) return 0;
  if (ix->store->kind == PH_ROWS_I8Q) return PH_I8T_LDS;  // its one form
  const uint32_t nv4 = a.dist.nv4;
  if (!tiny_mfma_shape(ix->store->metric, nv4 * 4u)) return 0;
  return tiny_mfma_lds((int)(nv4 / 64u), 1);
}

size_t ph_tiny_lds_bytes(const PhSearchArgs &a) {
  if (!a.tiny_layers) return 0;
  return (a.tiny_n <= a.tiny_lds_nodes ? (size_t)a.tiny_stride * 4u : 0u) + (size_t)((a.tiny_n + 31u) / 32u + 1u) * 4u;
}

template <class T>
static hipError_t grow(T **p, size_t *have, size_t need) {
  if (*have >= need) return hipSuccess;
  if (*p) ph_timed_free(*p);
  *p = nullptr;
  *have = 0;
  hipError_t e = ph_timed_malloc((void **)p, need);
  if (e == hipSuccess) *have = need;
  return e;
}

static bool same_key(const PhTinyPrepKey &a, const PhTinyPrepKey &b) {
  if (!a.valid || !b.valid || a.nodes_epoch != b.nodes_epoch || a.T != b.T || a.tn != b.tn || a.vec2node != b.vec2node) return false;
  for (uint32_t l = 0; l < a.T; l++)
    if (a.nodes[l] != b.nodes[l] || a.nbrs[l] != b.nbrs[l] || a.n[l] != b.n[l] || a.W[l] != b.W[l] || a.links[l] != b.links[l])
      return false;
  return true;
}

// the neighbour rows of the dense layers rewritten in table ids + the membership mask.  The rows change between build
// rounds (links_epoch) and the lists with every promotion (nodes_epoch); between the searches of a finished index
// neither does, and the workspace keeps what the last launch made (the launches of a workspace are ordered by
// ph_search_begin, so the kept rows are complete before this launch's kernels read them)
static int tiny_prep_graph(const phnsw_index *ix, PhWorkspace &ws, PhSearchArgs &a, uint32_t T, uint32_t tn, hipStream_t stream,
                           bool *kept = nullptr) {
  if (kept) *kept = false;
  PhTinyPrepArgs p;
  memset(&p, 0, sizeof(p));
  p.T = T;
  p.tiny_n = tn;
  PhTinyPrepKey key;
  key.valid = !tiny_keep_off();
  key.nodes_epoch = ix->nodes_epoch;
  key.T = T;
  key.tn = tn;
  key.vec2node = a.layers[T - 1].vec2node;
  size_t nbr_words = 0;
  for (uint32_t l = 0; l < T; l++) {
    p.layers[l] = a.layers[l];
    p.off[l] = (uint32_t)nbr_words;
    a.tiny_off[l] = (uint32_t)nbr_words;
    nbr_words += (size_t)tn * a.layers[l].W;
    key.nodes[l] = a.layers[l].nodes;
    key.nbrs[l] = a.layers[l].neighbors;
    key.n[l] = a.layers[l].n_nodes;
    key.W[l] = a.layers[l].W;
    key.links[l] = ix->layers[l].links_epoch;
  }
  const uint32_t *nbr_was = ws.tiny_nbr, *member_was = ws.tiny_member;
  if (grow(&ws.tiny_nbr, &ws.tiny_nbr_bytes, nbr_words * 4u) != hipSuccess ||
      grow(&ws.tiny_member, &ws.tiny_member_bytes, (size_t)(PH_TINY_MAX_NODES + 1u) * 4u) != hipSuccess) {
    (void)hipGetLastError();
    ws.tiny_prep_key.valid = false;
    return 1;  // not an error: the launch walks every layer on the per-hop path
  }
  if (ws.tiny_nbr == nbr_was && ws.tiny_member == member_was && same_key(key, ws.tiny_prep_key)) {
    if (kept) *kept = true;
    return 0;
  }
  ws.tiny_prep_key = key;
  p.nbr = ws.tiny_nbr;
  p.member = ws.tiny_member;
  PH_HIP(hipMemsetAsync(ws.tiny_nbr, 0xFF, nbr_words * 4u, stream));
  PH_HIP(hipMemsetAsync(ws.tiny_member, 0, (size_t)(tn + 1u) * 4u, stream));
  hipLaunchKernelGGL(ph_tiny_prep_kernel, dim3((tn + 255u) / 256u, T), dim3(256), 0, stream, p);
  PH_HIP(hipGetLastError());
  return 0;
}

// the vector-unit tile pass over the rows of one kind
template <class R>
static void tiny_table_valu(int nv, dim3 grid, hipStream_t stream, const PhTinyTableArgs &t) {
  switch (nv) {
    case 1: hipLaunchKernelGGL((ph_tiny_table_kernel<1, 8, R>), grid, dim3(256), 0, stream, t); break;
    case 3: hipLaunchKernelGGL((ph_tiny_table_kernel<3, 8, R>), grid, dim3(256), 0, stream, t); break;
    default: hipLaunchKernelGGL((ph_tiny_table_kernel<6, 4, R>), grid, dim3(256), 0, stream, t); break;
  }
}

// the table of an i8q store: both operands as code matrices + scales (the node side kept under the pack key, like the
// packed f32 operand), then the int8 GEMM.  The buffers are the workspace's operand buffers, which an index over an i8q
// store uses for nothing else.
static int tiny_table_i8q(const phnsw_index *ix, PhWorkspace &ws, const PhDistArgs &dist, const float *queries, uint32_t ldq,
                          const uint32_t *qids, const uint32_t *order, uint32_t npos, const uint32_t *tnodes, uint32_t tn,
                          uint32_t stride, float *D, hipStream_t stream, bool *kept) {
  const uint32_t qtiles = (npos + 63u) / 64u, ntiles = (tn + 63u) / 64u;
  const uint32_t kpad = (dist.ld + PH_I8T_KS - 1u) / PH_I8T_KS * PH_I8T_KS;
  const size_t row_bytes = (size_t)kpad + 4u;  // codes, and the row's scale behind the code matrix
  const float4 *pn_was = ws.tiny_pn;
  if (grow(&ws.tiny_pq, &ws.tiny_pq_bytes, (size_t)qtiles * 64u * row_bytes) != hipSuccess ||
      grow(&ws.tiny_pn, &ws.tiny_pn_bytes, (size_t)ntiles * 64u * row_bytes) != hipSuccess) {
    (void)hipGetLastError();
    ws.tiny_pack_key.valid = false;
    return 1;
  }
  PhTinyPackKey key;
  key.valid = !tiny_keep_off();
  key.nodes_epoch = ix->nodes_epoch;
  key.vecs = dist.rows.base;
  key.tnodes = tnodes;
  key.ld = dist.ld;
  key.tn = tn;
  key.nv = kpad;
  const PhTinyPackKey &have = ws.tiny_pack_key;
  const bool pn_kept = ws.tiny_pn == pn_was && key.valid && have.valid && have.nodes_epoch == key.nodes_epoch &&
                       have.vecs == key.vecs && have.tnodes == key.tnodes && have.ld == key.ld && have.tn == key.tn &&
                       have.nv == key.nv;
  ws.tiny_pack_key = key;
  if (kept) *kept = pn_kept;
  PhTinyQuantArgs k;
  memset(&k, 0, sizeof(k));
  k.rows = dist.rows;
  k.nv4 = dist.nv4;
  k.kw = kpad / 4u;
  k.queries = queries;
  k.ldq = ldq;
  k.ids = qids;
  k.order = order;
  k.n = npos;
  k.n_pad = qtiles * 64u;
  k.codes = (uint32_t *)ws.tiny_pq;
  k.scales = (float *)((char *)ws.tiny_pq + (size_t)k.n_pad * kpad);
  hipLaunchKernelGGL(ph_tiny_quant_kernel, dim3(k.n_pad / 4u), dim3(256), 0, stream, k);
  PhTinyI8Args m;
  memset(&m, 0, sizeof(m));
  m.cq = (const ph_i32x4 *)k.codes;
  m.sq = k.scales;
  k.queries = nullptr;
  k.ids = tnodes;
  k.order = nullptr;
  k.n = tn;
  k.n_pad = ntiles * 64u;
  k.codes = (uint32_t *)ws.tiny_pn;
  k.scales = (float *)((char *)ws.tiny_pn + (size_t)k.n_pad * kpad);
  if (!pn_kept) hipLaunchKernelGGL(ph_tiny_quant_kernel, dim3(k.n_pad / 4u), dim3(256), 0, stream, k);
  PH_HIP(hipGetLastError());
  m.cn = (const ph_i32x4 *)k.codes;
  m.sn = k.scales;
  m.npos = npos;
  m.tiny_n = tn;
  m.stride = stride;
  m.k16 = kpad / 16u;
  m.metric = dist.metric;
  m.D = D;
  ws.tiny_table_g = 1;
  hipLaunchKernelGGL(ph_tiny_table_i8_kernel, dim3(qtiles, ntiles), dim3(256), 0, stream, m);
  PH_HIP(hipGetLastError());
  return 0;
}

// D[p][t] = compare_vec(query of position p, Stored(tnodes[t])) for npos positions (position p = query order[p], or p
// itself; raw queries or Stored ids), the per-hop path's bits: the matrix-core kernel where it applies, else the
// vector-unit tile pass.  returns 1 (no error set) when its operand buffers cannot be allocated.
// g: staging depth of the matrix-core kernel, 1 = the form that fits beside a running search kernel.  The packed node
// operand depends on the table layer's node list and the stored rows alone and is kept like the prepared graph.
static int tiny_table(const phnsw_index *ix, PhWorkspace &ws, const PhDistArgs &dist, const float *queries, uint32_t ldq,
                      const uint32_t *qids, const uint32_t *order, uint32_t npos, const uint32_t *tnodes, uint32_t tn,
                      uint32_t stride, float *D, hipStream_t stream, int g = 2, bool *kept = nullptr) {
  if (kept) *kept = false;
  ws.tiny_table_g = 0;
  PhTinyTableArgs t;
  memset(&t, 0, sizeof(t));
  t.dist = dist;
  t.queries = queries;
  t.ldq = ldq;
  t.qids = qids;
  t.order = order;
  t.npos = npos;
  t.tnodes = tnodes;
  t.tiny_n = tn;
  t.stride = stride;
  t.D = D;
  if (const char *e = getenv("PHNSW_TINY_DBG")) t.dbg = (uint32_t)atoi(e);
  const uint32_t nv4 = dist.nv4;
  const int nv = ph_chunk_count(nv4);  // 1, 3 or 6: ph_tiny_layer_count gives longer rows no dense layer
  if (dist.rows.kind == PH_ROWS_BITS) return ph_bits_unsupported(ix->store, "dense distance table");  // no row policy reads bit rows
  if (dist.rows.kind == PH_ROWS_I8Q) return tiny_table_i8q(ix, ws, dist, queries, ldq, qids, order, npos, tnodes, tn, stride, D, stream, kept);
  // dot-product metrics over whole 64-chunk rows go to the matrix cores (same bits, see above); the Euclidean
  // chain (fma(d, d, acc) of a difference) is not a product of the two operands and stays on the vector units, as
  // do ragged rows and launches of a handful of queries.  PHNSW_TINY_VALU=1 forces the vector kernel (tests).
  const bool mfma = tiny_mfma_shape(dist.metric, nv4 * 4u) && nv4 == 64u * (uint32_t)nv && npos >= 32u;
  if (mfma) {
    const uint32_t qtiles = (npos + 63u) / 64u, ntiles = (tn + 63u) / 64u;
    const size_t row_bytes = (size_t)nv * 64u * sizeof(float4);
    const float4 *pn_was = ws.tiny_pn;
    if (grow(&ws.tiny_pq, &ws.tiny_pq_bytes, (size_t)qtiles * 64u * row_bytes) != hipSuccess ||
        grow(&ws.tiny_pn, &ws.tiny_pn_bytes, (size_t)ntiles * 64u * row_bytes) != hipSuccess) {
      (void)hipGetLastError();
      ws.tiny_pack_key.valid = false;
      return 1;
    }
    PhTinyPackKey key;
    key.valid = !tiny_keep_off();
    key.nodes_epoch = ix->nodes_epoch;
    key.vecs = dist.rows.base;
    key.tnodes = tnodes;
    key.ld = dist.ld;
    key.tn = tn;
    key.nv = (uint32_t)nv;
    const PhTinyPackKey &have = ws.tiny_pack_key;
    const bool pn_kept = ws.tiny_pn == pn_was && key.valid && have.valid && have.nodes_epoch == key.nodes_epoch &&
                         have.vecs == key.vecs && have.tnodes == key.tnodes && have.ld == key.ld && have.tn == key.tn &&
                         have.nv == key.nv;
    ws.tiny_pack_key = key;
    if (kept) *kept = pn_kept;
    PhTinyPackArgs k;
    memset(&k, 0, sizeof(k));
    k.rows = dist.rows;
    k.nv = (uint32_t)nv;
    k.queries = queries;
    k.ldq = ldq;
    k.ids = qids;
    k.order = order;
    k.n = npos;
    k.n_pad = qtiles * 64u;
    k.out = ws.tiny_pq;
    hipLaunchKernelGGL(ph_tiny_pack_kernel, dim3(k.n_pad / 32u, 8u * (uint32_t)nv), dim3(32, 8), 0, stream, k);
    k.queries = nullptr;
    k.ids = tnodes;
    k.order = nullptr;
    k.n = tn;
    k.n_pad = ntiles * 64u;
    k.out = ws.tiny_pn;
    if (!pn_kept) hipLaunchKernelGGL(ph_tiny_pack_kernel, dim3(k.n_pad / 32u, 8u * (uint32_t)nv), dim3(32, 8), 0, stream, k);
    PH_HIP(hipGetLastError());
    PhTinyMfmaArgs m;
    memset(&m, 0, sizeof(m));
    m.pq = ws.tiny_pq;
    m.pn = ws.tiny_pn;
    m.npos = npos;
    m.tiny_n = tn;
    m.stride = stride;
    m.qtiles = qtiles;
    m.ntiles = ntiles;
    m.metric = dist.metric;
    m.D = D;
    const uint32_t supers = ((qtiles + 7u) / 8u) * ((ntiles + 7u) / 8u);
    const uint32_t blocks = (supers + 7u) / 8u * 8u * 64u;
    const size_t lds = tiny_mfma_lds(nv, g == 1 ? 1 : 2);
    ws.tiny_table_g = g == 1 ? 1 : 2;
    if (g != 1 && nv == 6)
      PH_HIP(hipFuncSetAttribute((const void *)ph_tiny_table_mfma_kernel<6, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
#define PH_MFMA(NV, G) hipLaunchKernelGGL((ph_tiny_table_mfma_kernel<NV, G>), dim3(blocks), dim3(256), lds, stream, m)
    if (g == 1) {
      switch (nv) {
        case 1: PH_MFMA(1, 1); break;
        case 3: PH_MFMA(3, 1); break;
        default: PH_MFMA(6, 1); break;
      }
    } else {
      switch (nv) {
        case 1: PH_MFMA(1, 2); break;
        case 3: PH_MFMA(3, 2); break;
        default: PH_MFMA(6, 2); break;
      }
    }
#undef PH_MFMA
  } else {
    const uint32_t qt = nv == 6 ? 4u : 8u;
    const uint32_t gx = (npos + 4u * qt - 1u) / (4u * qt);
    const uint32_t tiles = (tn + 7u) / 8u;
    uint32_t slices = std::min<uint32_t>(tiles, std::max<uint32_t>(1u, (2048u + gx - 1u) / gx));
    t.rows_per_slice = (tiles + slices - 1u) / slices * 8u;
    slices = (tn + t.rows_per_slice - 1u) / t.rows_per_slice;
    dim3 grid(gx, slices);
    switch (dist.rows.kind) {
      case PH_ROWS_F16: tiny_table_valu<RowF16>(nv, grid, stream, t); break;
      case PH_ROWS_I8: tiny_table_valu<RowI8>(nv, grid, stream, t); break;
      default: tiny_table_valu<RowF32>(nv, grid, stream, t); break;
    }
  }
  PH_HIP(hipGetLastError());
  return 0;
}

// the table of one (node chunk, position chunk) of the exact calls over shared allow-lists (ph_table_run,
// filter_dense.hip): positions [0, npos) of the given queries (raw rows, or Stored ids the caller has checked) -- position
// p is query order[p], or p itself without an order -- against the VectorIds tnodes[0 .. tn), rows of D tn rounded up to
// 64 floats apart, the G = 2 form.  `ws` is the caller's own: only its operand buffers and their key are used.  Returns
// what tiny_table returns.
int ph_tiny_table_chunk(const phnsw_index *ix, PhWorkspace &ws, const float *queries, uint32_t ldq, const uint32_t *qids,
                        const uint32_t *order, uint32_t npos, const uint32_t *tnodes, uint32_t tn, float *D, hipStream_t stream,
                        bool *kept) {
  return tiny_table(ix, ws, ph_dist_args(ix->store), queries, ldq, qids, order, npos, tnodes, tn, tiny_stride_of(tn), D, stream,
                    2, kept);
}

int ph_tiny_prepare(const phnsw_index *ix, PhWorkspace &ws, PhSearchArgs &a, uint32_t max_layers, hipStream_t stream) {
  a.tiny_layers = 0;
  a.tiny_rows = 0;
  if (a.knn_mode || a.layer_lo) return 0;
  uint32_t T = std::min(ph_tiny_layer_count(ix, a.n_layers, a.ef), max_layers);
  if (!T) return 0;
  const uint32_t tn = ix->layers[T - 1].n_nodes, stride = tiny_stride_of(tn), npos = a.nq;
  if ((uint64_t)npos > ph_tiny_max_positions(ix, a.n_layers, a.ef)) return 0;  // the caller chunks; never reached through api.hip
  // the table is an accelerator, never a requirement: when the device cannot spare it the launch simply walks
  // every layer on the per-hop path (same results)
  if (grow(&ws.tiny_d, &ws.tiny_d_bytes, std::max<size_t>((size_t)npos * stride * 4u, 1u << 20)) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  // The form of the table kernel: a caller that keeps two batches in flight (the index's two workspaces, a stream
  // each) finds the other workspace's search kernel running or queued when it launches -- its end event has not
  // come -- and this launch's table pass, which wants the matrix cores the search kernel leaves idle, takes the
  // form that fits on the CUs beside it.  A lone launch keeps the faster G = 2 form.  A query, never a wait.
  const int mode = table_beside_mode();
  bool beside = mode == 1;
  if (mode == 2) {
    const PhWorkspace &other = &ws == &ix->ws[0] ? ix->ws[1] : ix->ws[0];
    if ((&ws == &ix->ws[0] || &ws == &ix->ws[1]) && other.timed && other.ev1) {
      beside = hipEventQuery(other.ev1) == hipErrorNotReady;
      (void)hipGetLastError();
    }
  }
  bool prep_kept = false, pack_kept = false;
  int rc = tiny_prep_graph(ix, ws, a, T, tn, stream, &prep_kept);
  if (rc) return rc < 0 ? rc : 0;
  rc = tiny_table(ix, ws, a.dist, a.queries, a.ldq, a.qids, a.order, npos, a.layers[T - 1].nodes, tn, stride, ws.tiny_d, stream,
                  beside ? 1 : 2, &pack_kept);
  if (rc) return rc < 0 ? rc : 0;
  if (getenv("PHNSW_VERBOSE")) {
    if (ws.tiny_table_g)
      fprintf(stderr, "[phnsw] dense table: %u positions x %u nodes on the matrix cores, G = %d (%s), graph %s, node operand %s\n",
              npos, tn, ws.tiny_table_g, beside ? "beside the other workspace's launch" : "alone",
              prep_kept ? "kept" : "prepared", pack_kept ? "kept" : "packed");
    else
      fprintf(stderr, "[phnsw] dense table: %u positions x %u nodes on the vector units, graph %s\n", npos, tn,
              prep_kept ? "kept" : "prepared");
  }
  ws.tiny_last_npos = npos;
  ws.tiny_last_tn = tn;
  ws.tiny_last_stride = stride;
  a.tiny_layers = T;
  a.tiny_n = tn;
  a.tiny_lds_nodes = PH_TINY_LDS_NODES;
  a.tiny_stride = stride;
  a.tiny_d = ws.tiny_d;
  a.tiny_nbr = ws.tiny_nbr;
  a.tiny_member = ws.tiny_member;
  return 0;
}

// ------------------------------------------------------------------ the table order of a launch

// The table of a launch already holds every query's distance to every node of the table layer, so where a query
// will land there costs one pass over its row.  key[q] = the cell (pos, bruteforce.hip) most of its four nearest
// table nodes lie in, the nearest of them deciding a tie: on the headline data the nearest node alone names the cell
// a GEMM of the query against the anchors would in 0.43 of the queries, the four in 0.47 (profiles/cells/).  One wave
// per query; the nodes are ranked by (distance, table id) like everywhere, so the key is one value run after run.
__global__ __launch_bounds__(64) void ph_tiny_row_cell_kernel(const float *__restrict__ D, uint32_t stride, uint32_t tn,
                                                              uint32_t nq, const uint32_t *__restrict__ pos,
                                                              uint32_t *__restrict__ key) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const float *row = D + (uint64_t)q * stride;
    uint64_t top[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};  // the lane's own four nearest, ascending
    for (uint32_t t = lane; t < tn; t += 64) {
      uint64_t k = mkkey(row[t], t);
      if (k < top[3]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const uint64_t lo = k < top[j] ? k : top[j], hi = k < top[j] ? top[j] : k;
          top[j] = lo;
          k = hi;
        }
      }
    }
    uint32_t cell[4], n = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {  // the wave's four nearest: the least head, four times (keys are distinct)
      uint64_t m = top[0];
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        const uint64_t o = __shfl_xor(m, s);
        m = o < m ? o : m;
      }
      if (top[0] == m) top[0] = top[1], top[1] = top[2], top[2] = top[3], top[3] = KEY_NONE;
      const uint32_t t = (uint32_t)m & IDM;
      cell[r] = 0u;
      if (m != KEY_NONE && t < tn) cell[r] = pos[t], n = r + 1;  // (wave-uniform)
    }
    uint32_t best = 0, best_cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      uint32_t cnt = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) cnt += ((uint32_t)j < n && cell[j] == cell[i]) ? 1u : 0u;
      if ((uint32_t)i < n && cnt > best_cnt) best = cell[i], best_cnt = cnt;
    }
    if (lane == 0) key[q] = best;
  }
}

int ph_tiny_table_order(PhWorkspace &ws, PhSearchArgs &b, const uint32_t *pos, uint32_t bins, hipStream_t stream) {
  if (!b.tiny_layers || b.tiny_rows || !pos || !bins || ws.order_cap < b.nq) return 0;
  if (ws.ocell_cap < bins) {
    if (ws.ocell) PH_HIP(hipFree(ws.ocell));
    ws.ocell = nullptr, ws.ocell_cap = 0;
    PH_HIP(hipMalloc(&ws.ocell, ((size_t)bins + 1u) * 4u));
    ws.ocell_cap = bins;
  }
  hipLaunchKernelGGL(ph_tiny_row_cell_kernel, dim3(std::min<uint32_t>(b.nq, 1u << 16)), dim3(64), 0, stream, b.tiny_d,
                     b.tiny_stride, b.tiny_n, b.nq, pos, ws.okey);
  int rc = ph_cell_order_device(ws.okey, b.nq, bins, ws.ocell, ws.oorder, stream);
  if (rc) return rc;
  b.order = ws.oorder;
  b.table_by_query = 1u;
  return 0;
}

// ------------------------------------------------------------------ the build's kept table

void ph_build_table_free(phnsw_index *ix) {
  for (PhBuildTable &b : ix->bt)
    if (b.D) ph_timed_free(b.D);
  ix->bt.clear();
  for (auto &sp : ix->bt_spare) ph_timed_free(sp.first);
  ix->bt_spare.clear();
}
// the rows go, the slot (which layer it belongs to) stays; the buffer waits for the next table that fits
static void build_table_drop(phnsw_index *ix, PhBuildTable &b) {
  if (b.D) ix->bt_spare.emplace_back(b.D, b.cap);
  b.D = nullptr;
  b.bytes = b.cap = 0;
  b.lo = b.hi = b.lo_alloc = b.hi_alloc = 0;
}
// every table is void (a node list changed): the slots go, the buffers are kept for their successors
static void build_table_recycle(phnsw_index *ix) {
  for (PhBuildTable &b : ix->bt) build_table_drop(ix, b);
  ix->bt.clear();
}
// a buffer of at least `bytes`: the smallest spare that holds them without wasting more than half of itself, or a new
// allocation with a sixteenth of headroom (a promotion grows a layer by a few per cent)
static float *build_table_buffer(phnsw_index *ix, size_t bytes, size_t *cap) {
  int best = -1;
  for (size_t i = 0; i < ix->bt_spare.size(); i++)
    if (ix->bt_spare[i].second >= bytes && ix->bt_spare[i].second <= 2 * bytes &&
        (best < 0 || ix->bt_spare[i].second < ix->bt_spare[(size_t)best].second))
      best = (int)i;
  if (best >= 0) {
    float *p = ix->bt_spare[(size_t)best].first;
    *cap = ix->bt_spare[(size_t)best].second;
    ix->bt_spare.erase(ix->bt_spare.begin() + best);
    return p;
  }
  size_t mfree = 0, mtotal = 0;
  if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) return nullptr;
  size_t want = bytes + bytes / 16;
  if (want + (8ull << 30) > mfree) {  // the searches' own workspaces come first: give the spares back, then try the bare size
    for (auto &sp : ix->bt_spare) ph_timed_free(sp.first);
    ix->bt_spare.clear();
    if (hipMemGetInfo(&mfree, &mtotal) != hipSuccess) return nullptr;
    want = bytes;
  }
  if (want + (8ull << 30) > mfree || bytes > mtotal / 2) return nullptr;
  float *p = nullptr;
  if (ph_timed_malloc((void **)&p, want) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  *cap = want;
  return p;
}

// rows kept only for table layers of at least this many nodes (smaller tables cost less than the bookkeeping);
// PHNSW_BUILD_TABLE_MIN overrides (the tests keep every table), PHNSW_NO_BUILD_TABLE=1 switches the cache off
static uint32_t build_table_min() {
  if (const char *e = getenv("PHNSW_BUILD_TABLE_MIN"))
    if (atoi(e) > 0) return (uint32_t)atoi(e);
  return 1024u;
}

int ph_build_table_prepare(phnsw_index *ix, PhWorkspace &ws, PhSearchArgs &a, const PhRowHint &h, uint32_t T,
                           hipStream_t stream, bool *used) {
  *used = false;
  a.tiny_rows = 0;
  if (!ix->bt_enabled || !T || !a.qids || a.queries || a.knn_mode || a.layer_lo || getenv("PHNSW_NO_BUILD_TABLE")) return 0;
  const uint32_t tn = ix->layers[T - 1].n_nodes, stride = tiny_stride_of(tn);
  const uint32_t *tnodes = a.layers[T - 1].nodes;
  if (tn < build_table_min() || h.qn == 0) return 0;
  // one table per querying layer (an outer round of improve_neighbors_upto links every layer in turn); a changed node
  // list anywhere (epoch) voids them all
  if (!ix->bt.empty() && ix->bt[0].epoch != ix->nodes_epoch) build_table_recycle(ix);
  PhBuildTable *found = nullptr;
  for (PhBuildTable &b : ix->bt)
    if (b.qnodes == h.qnodes && b.qn == h.qn) found = &b;
  if (!found) {
    if (ix->bt.size() >= PH_MAX_LAYERS) return 0;
    ix->bt.emplace_back();
    found = &ix->bt.back();
    found->epoch = ix->nodes_epoch;
    found->qnodes = h.qnodes;
    found->qn = h.qn;
  }
  PhBuildTable &B = *found;
  const uint32_t need_lo = h.contiguous ? h.first : 0u, need_hi = h.contiguous ? h.first + h.count : h.qn;
  if (need_hi > h.qn || need_lo >= need_hi) return 0;
  const bool same = B.D && B.tnodes == tnodes && B.tn == tn && B.T == T;
  if (B.D && !same) build_table_drop(ix, B);
  if (!h.contiguous && !(B.D && B.lo <= need_lo && B.hi >= need_hi)) return 0;  // a sample: only from rows already there
  if (!B.D || need_lo < B.lo_alloc || need_hi > B.hi_alloc) {
    // (re)allocate for the requested range: the whole layer on one GPU, a rank's node range in a sharded build
    if (B.D && (need_lo > B.lo_alloc || need_hi < B.hi_alloc)) return 0;  // a second, different range: not worth juggling
    build_table_drop(ix, B);
    const size_t bytes = (size_t)(need_hi - need_lo) * stride * 4u;
    B.D = build_table_buffer(ix, bytes, &B.cap);
    if (!B.D) return 0;
    B.bytes = bytes;
    B.qnodes = h.qnodes;
    B.qn = h.qn;
    B.tnodes = tnodes;
    B.tn = tn;
    B.T = T;
    B.stride = stride;
    B.lo_alloc = need_lo;
    B.hi_alloc = need_hi;
    B.lo = B.hi = need_lo;
    B.epoch = ix->nodes_epoch;
  }
  // rows missing from [need_lo, need_hi): the valid rows are one interval; fill what lies outside it
  auto fill = [&](uint32_t lo, uint32_t hi) -> int {
    const uint32_t PIECE = 131072u;  // bounds the packed-operand buffer (400 MB at 768 floats)
    for (uint32_t at = lo; at < hi; at += PIECE) {
      const uint32_t cnt = std::min(PIECE, hi - at);
      int rc = tiny_table(ix, ws, a.dist, nullptr, 0, h.qnodes + at, nullptr, cnt, tnodes, tn, stride,
                          B.D + (size_t)(at - B.lo_alloc) * stride, stream);
      if (rc) return rc;
    }
    return 0;
  };
  int rc = 0;
  if (B.lo == B.hi) {
    rc = fill(need_lo, need_hi);
    if (!rc) B.lo = need_lo, B.hi = need_hi;
  } else {
    if (need_lo < B.lo) {
      rc = fill(need_lo, B.lo);
      if (!rc) B.lo = need_lo;
    }
    if (!rc && need_hi > B.hi) {
      rc = fill(B.hi, need_hi);
      if (!rc) B.hi = need_hi;
    }
  }
  if (rc) return rc < 0 ? rc : 0;
  rc = tiny_prep_graph(ix, ws, a, T, tn, stream);
  if (rc) return rc < 0 ? rc : 0;
  a.tiny_layers = T;
  a.tiny_n = tn;
  a.tiny_lds_nodes = PH_TINY_LDS_NODES;
  a.tiny_stride = stride;
  a.tiny_d = B.D;
  a.tiny_rows = 1;
  a.tiny_row_first = B.lo_alloc;
  a.tiny_row_map = h.vec2node;
  a.tiny_nbr = ws.tiny_nbr;
  a.tiny_member = ws.tiny_member;
  *used = true;
  return 0;
}
