// Converted row stores: the rows of an f32 store in a narrower format, searched through a row policy (RowF16 / RowI8,
// phnsw_device.h) by the kernels of the f32 store.
//
// The contract, whatever the format: a distance on a converted store is the f32 chain on the rows R::widen makes of
// it, so a search equals, bit for bit, the f32 search over the store phnsw_store_read returns.  A converted store
// serves searches and distance batches only (ph_search_only_unsupported names everything else).  Everything here but
// the two conversion kernels is written once over the policy.
//
// f16: every component rounded to IEEE binary16 (round to nearest even, ph_f32_to_f16_bits), [n][ld] halves in
// component order: a row starts on an 8-byte boundary and a lane's chunk of four components is one 8-byte load.
// Widening is exact.
//
// i8: every row quantised on its own, symmetrically --
//   scale  = maxabs(row) / 127.0f                      (IEEE f32 division)
//   code_j = (int8) clamp(rintf(x_j / scale), -127, 127) (IEEE f32 division, round half to even)
// with scale 0 (a row of zeros, or a maxabs so small that the quotient underflows to 0) giving codes 0 -- and kept as
// rows of 4 + ld bytes rounded up to a multiple of 16: the f32 scale, the ld code bytes in component order (padding
// components: code 0), padding.  A lane's chunk of four components is one 4-byte load; a component dequantises to
// scale * (float)code with one rounding (ph_i8_dequant).
//
// i8q: the rows of an i8 store, byte for byte (same kernel, same layout, same phnsw_i8_read and phnsw_store_read); what
// differs is the distance, which quantises the query with the rows' own quantiser and takes integer dot products
// (DistI8Q, phnsw_device.h).  Dot-product metrics only: the Euclidean distance would need the rows' norms.
//
// bits: one sign bit per component (bits_plan.h has the layout rules: bit j = the component is below zero, component j
// in bit j & 31 of word j >> 5, rows of 32 * NV bytes, padding bits 0).  NOT a converted store in the sense above: no
// row policy widens it in registers, a distance is a popcount (DistBits, phnsw_device.h), and only the plain walk, the
// distance batch and the re-ranked search serve it (ph_bits_unsupported names everything else).  phnsw_store_read
// returns its rows as +1 / -1, the values on which the f32 search gives the same distances, bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "phnsw_device.h"

// one thread per component of the padded row; a NaN or a magnitude that rounds to infinity raises the flag
__global__ void ph_f16_convert_kernel(const float *__restrict__ rows, uint32_t ld, uint32_t dim, uint64_t n,
                                      uint16_t *__restrict__ half, uint32_t stride, uint32_t *bad) {
  const uint64_t total = n * (uint64_t)stride;
  bool mine = false;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / stride;
    const uint32_t c = (uint32_t)(x - r * stride);
    uint16_t h = 0;
    if (c < dim) {
      h = ph_f32_to_f16_bits(rows[r * ld + c]);
      mine |= (h & 0x7C00u) == 0x7C00u;
    }
    half[x] = h;
  }
  if (mine) atomicOr(bad, 1u);
}

// one wave per row: max-abs reduction over the wave, then the row's scale and its codes, four to a word; a NaN or an
// infinite component raises the flag
__global__ void ph_i8_convert_kernel(const float *__restrict__ rows, uint32_t ld, uint32_t dim, uint64_t n,
                                     uint8_t *__restrict__ out, uint32_t stride, uint32_t *bad) {
  const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x / 64u;
  bool mine = false;
  for (uint64_t r = (uint64_t)blockIdx.x * wpb + threadIdx.x / 64u; r < n; r += (uint64_t)gridDim.x * wpb) {
    const float *src = rows + r * ld;
    float m = 0.f;
    for (uint32_t c = lane; c < dim; c += 64u) {
      const float x = src[c];
      mine |= (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u;
      m = fmaxf(m, fabsf(x));
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) m = fmaxf(m, __shfl_xor(m, sft));
    const float scale = ph_i8_scale(m);
    uint32_t *dst = (uint32_t *)(out + r * stride);
    if (lane == 0) dst[0] = __float_as_uint(scale);
    for (uint32_t w = 1u + lane; w < stride / 4u; w += 64u) {
      uint32_t word = 0;
#pragma unroll
      for (uint32_t e = 0; e < 4u; e++) {
        const uint32_t c = 4u * (w - 1u) + e;
        if (c < dim) word |= ((uint32_t)ph_i8_quant(src[c], scale) & 0xFFu) << (8u * e);
      }
      dst[w] = word;
    }
  }
  if (mine) atomicOr(bad, 1u);
}

// one wave per row: 64 components at a time (coalesced), their sign bits by one ballot = two words of the row; lane w
// keeps word w and the row's 8 NV words leave in one coalesced store (words past the row's components: 0).  A NaN or
// an infinite component raises the flag.  stride_words <= 48 < 64.
__global__ void ph_bits_convert_kernel(const float *__restrict__ rows, uint32_t ld, uint32_t dim, uint64_t n,
                                       uint32_t *__restrict__ out, uint32_t stride_words, uint32_t *bad) {
  const uint32_t lane = threadIdx.x & 63u, wpb = blockDim.x / 64u;
  bool mine = false;
  for (uint64_t r = (uint64_t)blockIdx.x * wpb + threadIdx.x / 64u; r < n; r += (uint64_t)gridDim.x * wpb) {
    const float *src = rows + r * ld;
    uint32_t word = 0u;
    for (uint32_t b = 0; 64u * b < dim; b++) {
      const uint32_t c = 64u * b + lane;
      uint32_t neg = 0u;
      if (c < dim) {
        const uint32_t u = __float_as_uint(src[c]);
        mine |= (u & 0x7F800000u) == 0x7F800000u;
        neg = ph_bits_sign_of(u);
      }
      const uint64_t m = __ballot(neg != 0u);
      if (lane == 2u * b) word = (uint32_t)m;
      if (lane == 2u * b + 1u) word = (uint32_t)(m >> 32);
    }
    if (lane < stride_words) out[r * stride_words + lane] = word;
  }
  if (mine) atomicOr(bad, 1u);
}

// rows [first, first + count) of a bits store as a dense [count][dim] array of +1.0f (bit 0) / -1.0f (bit 1)
__global__ void ph_bits_read_kernel(const uint32_t *__restrict__ words, uint32_t stride_words, uint32_t dim, uint64_t first,
                                    uint64_t count, float *__restrict__ out) {
  const uint64_t total = count * (uint64_t)dim;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / dim;
    const uint32_t j = (uint32_t)(x - r * dim);
    const uint32_t w = words[(first + r) * stride_words + ph_bits_word_of(j)];
    out[x] = ((w >> ph_bits_bit_of(j)) & 1u) ? -1.0f : 1.0f;
  }
}

// rows [first, first + count) converted into a dense [count][dim] f32 array: what the distance kernels see.  One
// thread per chunk of four components (a row holds whole chunks: ld is a multiple of 4), the last one cut at dim.
template <class R>
__global__ void ph_store_read_kernel(PhRows rows, uint32_t dim, uint64_t first, uint64_t count, float *__restrict__ out) {
  const uint32_t nc = (dim + 3u) / 4u;
  const uint64_t total = count * (uint64_t)nc;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / nc;
    const uint32_t c = (uint32_t)(x - r * nc);
    const typename R::chunk *row = R::row(rows, (uint32_t)(first + r));  // n < 2^31
    const float4 v = R::widen(R::load(row, c), R::row_aux(row));
    const float e[4] = {v.x, v.y, v.z, v.w};
    float *dst = out + r * dim + 4u * c;
    for (uint32_t j = 0; j < 4u && 4u * c + j < dim; j++) dst[j] = e[j];
  }
}

// the rows of `ids` converted into [cnt][ld] f32 rows: operands of the locality cells' GEMM (bruteforce.hip)
template <class R>
__global__ void ph_gather_rows_kernel(PhRows rows, uint32_t ld, const uint32_t *ids, uint32_t first, uint32_t cnt,
                                      float *__restrict__ out) {
  const uint32_t r = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (r >= cnt) return;
  const typename R::chunk *src = R::row(rows, ids ? ids[r] : first + r);
  const typename R::aux ax = R::row_aux(src);
  float4 *dst = (float4 *)(out + (uint64_t)r * ld);
  for (uint32_t j = lane; j < ld / 4; j += 64) dst[j] = R::widen(R::load(src, j), ax);
}

template <class R>
static int gather_rows(const phnsw_store *s, const uint32_t *ids_dev, uint32_t first, uint32_t cnt, float *out_dev) {
  hipLaunchKernelGGL(ph_gather_rows_kernel<R>, dim3((cnt + 3) / 4), dim3(256), 0, 0, ph_store_rows(s), s->ld, ids_dev, first,
                     cnt, out_dev);
  PH_HIP(hipGetLastError());
  return 0;
}
int ph_converted_gather_rows(const phnsw_store *s, const uint32_t *ids_dev, uint32_t first, uint32_t cnt, float *out_dev) {
  if (cnt == 0) return 0;
  if (int rc = ph_bits_unsupported(s, "locality cells")) return rc;  // (ph_layer_wants_cells is false for the kind)
  return s->kind == PH_ROWS_F16 ? gather_rows<RowF16>(s, ids_dev, first, cnt, out_dev)
                                : gather_rows<RowI8>(s, ids_dev, first, cnt, out_dev);
}

template <class R>
static int store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out) {
  const uint64_t PIECE = 65536;
  float *tmp = nullptr;
  PH_HIP(hipMalloc(&tmp, (size_t)std::min(PIECE, count) * s->dim * 4));
  int rc = 0;
  for (uint64_t at = 0; at < count && !rc; at += PIECE) {
    const uint64_t cnt = std::min(PIECE, count - at);
    const uint64_t total = cnt * s->dim;
    const uint64_t chunks = cnt * ((s->dim + 3u) / 4u);
    hipLaunchKernelGGL(ph_store_read_kernel<R>, dim3((uint32_t)std::min<uint64_t>((chunks + 255) / 256, 65536)), dim3(256), 0,
                       0, ph_store_rows(s), s->dim, first + at, cnt, tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out + at * s->dim, tmp, (size_t)total * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "converted store read", __FILE__, __LINE__);
  }
  hipFree(tmp);
  return rc;
}
static int bits_store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out) {
  const uint64_t PIECE = 65536;
  float *tmp = nullptr;
  PH_HIP(hipMalloc(&tmp, (size_t)std::min(PIECE, count) * s->dim * 4));
  int rc = 0;
  for (uint64_t at = 0; at < count && !rc; at += PIECE) {
    const uint64_t cnt = std::min(PIECE, count - at);
    const uint64_t total = cnt * s->dim;
    hipLaunchKernelGGL(ph_bits_read_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, 0,
                       (const uint32_t *)s->packed, s->packed_stride / 4u, s->dim, first + at, cnt, tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out + at * s->dim, tmp, (size_t)total * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "bits store read", __FILE__, __LINE__);
  }
  hipFree(tmp);
  return rc;
}
int ph_converted_store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out) {
  if (ph_store_bits(s)) return bits_store_read(s, first, count, out);
  return s->kind == PH_ROWS_F16 ? store_read<RowF16>(s, first, count, out) : store_read<RowI8>(s, first, count, out);
}

// `name`: the entry point, for its messages.  The allocation holds at least one row, so that an empty store has a
// pointer like any other.
static int create_converted(const char *name, const phnsw_store *full, int kind, phnsw_store **out) {
  if (!full || !out) {
    ph_set_error("%s: full and out must not be NULL", name);
    return PHNSW_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    ph_set_error("no HIP device available (libphnsw has no CPU fallback)");
    return PHNSW_E_NO_DEVICE;
  }
  if (!ph_store_f32(full)) {
    ph_set_error("%s: the source must be an f32 store", name);
    return PHNSW_E_INVALID;
  }
  if (kind == PH_ROWS_I8Q && full->metric == PHNSW_METRIC_L2) {
    ph_set_error("%s: the Euclidean metric is not supported on an i8q store (dot-product metrics only)", name);
    return PHNSW_E_UNSUPPORTED;
  }
  if (kind == PH_ROWS_BITS && !ph_chunk_count(full->ld / 4)) return ph_dim_unsupported(full->dim);
  PH_HIP(hipSetDevice(full->device));
  phnsw_store *s = new phnsw_store();
  s->device = full->device;
  s->kind = kind;
  s->n = full->n;
  s->dim = full->dim;
  s->ld = full->ld;
  s->packed_stride = kind == PH_ROWS_BITS  ? ph_bits_stride(ph_chunk_count(full->ld / 4))
                     : kind == PH_ROWS_F16 ? full->ld * 2u
                                           : ((4u + full->ld + 15u) & ~15u);
  s->metric = full->metric;
  s->rows = nullptr;
  uint32_t *bad = nullptr;
  uint32_t h_bad = 0;
  hipError_t e = hipMalloc(&s->packed, (size_t)std::max<uint64_t>(s->n, 1) * s->packed_stride);
  if (e == hipSuccess) e = hipMalloc(&bad, 4);
  if (e == hipSuccess) e = hipMemset(bad, 0, 4);
  if (e == hipSuccess && s->n) {
    if (kind == PH_ROWS_F16) {
      const uint64_t total = s->n * (uint64_t)s->ld;
      hipLaunchKernelGGL(ph_f16_convert_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 1u << 20)), dim3(256), 0,
                         0, full->rows, full->ld, full->dim, s->n, (uint16_t *)s->packed, s->ld, bad);
    } else if (kind == PH_ROWS_BITS) {
      hipLaunchKernelGGL(ph_bits_convert_kernel, dim3((uint32_t)std::min<uint64_t>((s->n + 3) / 4, 1u << 16)), dim3(256), 0, 0,
                         full->rows, full->ld, full->dim, s->n, (uint32_t *)s->packed, s->packed_stride / 4u, bad);
    } else {
      hipLaunchKernelGGL(ph_i8_convert_kernel, dim3((uint32_t)std::min<uint64_t>((s->n + 3) / 4, 1u << 16)), dim3(256), 0, 0,
                         full->rows, full->ld, full->dim, s->n, (uint8_t *)s->packed, s->packed_stride, bad);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&h_bad, bad, 4, hipMemcpyDeviceToHost);
  if (bad) hipFree(bad);
  int rc = 0;
  if (e != hipSuccess)
    rc = ph_hip_fail(e, kind == PH_ROWS_F16 ? "f16 store conversion" : (kind == PH_ROWS_BITS ? "bits store conversion" : "i8 store conversion"),
                     __FILE__, __LINE__);
  else if (h_bad) {
    if (kind == PH_ROWS_F16)
      ph_set_error("%s: a component is NaN or rounds to infinity in binary16 (|x| >= 65520)", name);
    else
      ph_set_error("%s: a component is NaN or infinite", name);
    rc = PHNSW_E_INVALID;
  }
  if (rc) {
    if (s->packed) hipFree(s->packed);
    delete s;
    return rc;
  }
  *out = s;
  return 0;
}

extern "C" int phnsw_store_create_f16(const phnsw_store *full, phnsw_store **out) try {
  return create_converted("phnsw_store_create_f16", full, PH_ROWS_F16, out);
} catch (...) { return ph_caught(); }
extern "C" int phnsw_store_create_i8(const phnsw_store *full, phnsw_store **out) try {
  return create_converted("phnsw_store_create_i8", full, PH_ROWS_I8, out);
} catch (...) { return ph_caught(); }
extern "C" int phnsw_store_create_i8q(const phnsw_store *full, phnsw_store **out) try {
  return create_converted("phnsw_store_create_i8q", full, PH_ROWS_I8Q, out);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_store_create_bits(const phnsw_store *full, phnsw_store **out) try {
  return create_converted("phnsw_store_create_bits", full, PH_ROWS_BITS, out);
} catch (...) { return ph_caught(); }

// the sign bits [n][ceil(dim / 32)]: the public layout, whatever the device stride
extern "C" int phnsw_bits_read(const phnsw_store *s, uint32_t *words) try {
  if (!s || !ph_store_bits(s) || !words) {
    ph_set_error("phnsw_bits_read: needs a bits store and the output");
    return PHNSW_E_INVALID;
  }
  if (s->n == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  const size_t width = (size_t)ph_bits_words(s->dim) * 4u;
  PH_HIP(hipMemcpy2D(words, width, s->packed, s->packed_stride, width, s->n, hipMemcpyDeviceToHost));
  return 0;
} catch (...) { return ph_caught(); }

// the stored codes [n][dim] and scales [n], as they lie in the rows
extern "C" int phnsw_i8_read(const phnsw_store *s, int8_t *codes, float *scales) try {
  if (!s || !ph_rows_i8_layout(s->kind) || !codes || !scales) {
    ph_set_error("phnsw_i8_read: needs an i8 or i8q store and both outputs");
    return PHNSW_E_INVALID;
  }
  if (s->n == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  const uint8_t *rows = (const uint8_t *)s->packed;
  PH_HIP(hipMemcpy2D(scales, 4, rows, s->packed_stride, 4, s->n, hipMemcpyDeviceToHost));
  PH_HIP(hipMemcpy2D(codes, s->dim, rows + 4, s->packed_stride, s->dim, s->n, hipMemcpyDeviceToHost));
  return 0;
} catch (...) { return ph_caught(); }
