// Int8 row store: the rows of an f32 store quantised per row, symmetrically --
//   scale  = maxabs(row) / 127.0f                      (IEEE f32 division)
//   code_j = (int8) clamp(rintf(x_j / scale), -127, 127) (IEEE f32 division, round half to even)
// with scale 0 (a row of zeros, or a maxabs so small that the quotient underflows to 0) giving codes 0 -- and kept as n
// rows of ldb bytes, ldb = 4 + ld rounded up to a multiple of 16: the f32 scale, the ld code bytes in component order
// (padding components: code 0), padding.  A lane's chunk of four components is one 4-byte load (DistI8 / RowI8,
// phnsw_device.h).
//
// The contract: a distance on this store is the f32 chain on the DEQUANTISED rows, scale * (float)code with one
// rounding (ph_i8_dequant), so a search equals, bit for bit, the f32 search over the store phnsw_store_read returns.
// The store serves searches and distance batches only (ph_search_only_unsupported names everything else).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "phnsw_device.h"

__device__ __forceinline__ int ph_i8_quant(float x, float scale) {
  if (scale == 0.f) return 0;
  const float t = rintf(__fdiv_rn(x, scale));
  return (int)fminf(fmaxf(t, -127.f), 127.f);
}

// one wave per row: max-abs reduction over the wave, then the row's scale and its codes, four to a word; a NaN or an
// infinite component raises the flag
__global__ void ph_i8_convert_kernel(const float *__restrict__ rows, uint32_t ld, uint32_t dim, uint64_t n,
                                     uint8_t *__restrict__ out, uint32_t ldb, uint32_t *bad) {
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
    const float scale = __fdiv_rn(m, 127.0f);
    uint32_t *dst = (uint32_t *)(out + r * ldb);
    if (lane == 0) dst[0] = __float_as_uint(scale);
    for (uint32_t w = 1u + lane; w < ldb / 4u; w += 64u) {
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

// rows [first, first + count) dequantised into a dense [count][dim] f32 array: what the distance kernels see
__global__ void ph_i8_dequant_kernel(const uint8_t *__restrict__ i8, uint32_t ldb, uint32_t dim, uint64_t first,
                                     uint64_t count, float *__restrict__ out) {
  const uint64_t total = count * (uint64_t)dim;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / dim;
    const uint32_t c = (uint32_t)(x - r * dim);
    const uint8_t *row = i8 + (first + r) * ldb;
    out[x] = ph_i8_dequant(*(const float *)row, (int)(int8_t)row[4u + c]);
  }
}

// the rows of `ids` dequantised into [cnt][ld] f32 rows: operands of the locality cells' GEMM (bruteforce.hip)
__global__ void ph_i8_gather_rows_kernel(const uint8_t *__restrict__ i8, uint32_t ldb, uint32_t ld, const uint32_t *ids,
                                         uint32_t first, uint32_t cnt, float *__restrict__ out) {
  const uint32_t r = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (r >= cnt) return;
  const uint64_t id = ids ? ids[r] : first + r;
  const RowI8::chunk *src = (const RowI8::chunk *)(i8 + id * ldb);
  const float scale = RowI8::row_aux(src);
  float4 *dst = (float4 *)(out + (uint64_t)r * ld);
  for (uint32_t j = lane; j < ld / 4; j += 64) dst[j] = RowI8::widen(RowI8::load(src, j), scale);
}

int ph_i8_gather_rows(const phnsw_store *s, const uint32_t *ids_dev, uint32_t first, uint32_t cnt, float *out_dev) {
  if (cnt == 0) return 0;
  hipLaunchKernelGGL(ph_i8_gather_rows_kernel, dim3((cnt + 3) / 4), dim3(256), 0, 0, s->i8, s->ldb, s->ld, ids_dev, first, cnt,
                     out_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

int ph_i8_store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out) {
  const uint64_t PIECE = 65536;
  float *tmp = nullptr;
  PH_HIP(hipMalloc(&tmp, (size_t)std::min(PIECE, count) * s->dim * 4));
  int rc = 0;
  for (uint64_t at = 0; at < count && !rc; at += PIECE) {
    const uint64_t cnt = std::min(PIECE, count - at);
    const uint64_t total = cnt * s->dim;
    hipLaunchKernelGGL(ph_i8_dequant_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, 0,
                       s->i8, s->ldb, s->dim, first + at, cnt, tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out + at * s->dim, tmp, (size_t)total * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "i8 store read", __FILE__, __LINE__);
  }
  hipFree(tmp);
  return rc;
}

extern "C" int phnsw_store_create_i8(const phnsw_store *full, phnsw_store **out) try {
  if (!full || !out) {
    ph_set_error("phnsw_store_create_i8: full and out must not be NULL");
    return PHNSW_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    ph_set_error("no HIP device available (libphnsw has no CPU fallback)");
    return PHNSW_E_NO_DEVICE;
  }
  if (!full->rows) {
    ph_set_error("phnsw_store_create_i8: the source must be an f32 store");
    return PHNSW_E_INVALID;
  }
  PH_HIP(hipSetDevice(full->device));
  phnsw_store *s = new phnsw_store();
  s->device = full->device;
  s->n = full->n;
  s->dim = full->dim;
  s->ld = full->ld;
  s->ldb = (4u + full->ld + 15u) & ~15u;
  s->metric = full->metric;
  s->rows = nullptr;
  uint32_t *bad = nullptr;
  uint32_t h_bad = 0;
  hipError_t e = hipMalloc(&s->i8, (size_t)std::max<uint64_t>(s->n, 1) * s->ldb);
  if (e == hipSuccess) e = hipMalloc(&bad, 4);
  if (e == hipSuccess) e = hipMemset(bad, 0, 4);
  if (e == hipSuccess && s->n) {
    hipLaunchKernelGGL(ph_i8_convert_kernel, dim3((uint32_t)std::min<uint64_t>((s->n + 3) / 4, 1u << 16)), dim3(256), 0, 0,
                       full->rows, full->ld, full->dim, s->n, s->i8, s->ldb, bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&h_bad, bad, 4, hipMemcpyDeviceToHost);
  if (bad) hipFree(bad);
  int rc = 0;
  if (e != hipSuccess)
    rc = ph_hip_fail(e, "i8 store conversion", __FILE__, __LINE__);
  else if (h_bad) {
    ph_set_error("phnsw_store_create_i8: a component is NaN or infinite");
    rc = PHNSW_E_INVALID;
  }
  if (rc) {
    if (s->i8) hipFree(s->i8);
    delete s;
    return rc;
  }
  *out = s;
  return 0;
} catch (...) { return ph_caught(); }

// the stored codes [n][dim] and scales [n], as they lie in the rows
extern "C" int phnsw_i8_read(const phnsw_store *s, int8_t *codes, float *scales) try {
  if (!s || !s->i8 || !codes || !scales) {
    ph_set_error("phnsw_i8_read: needs an i8 store and both outputs");
    return PHNSW_E_INVALID;
  }
  if (s->n == 0) return 0;
  PH_HIP(hipSetDevice(s->device));
  PH_HIP(hipMemcpy2D(scales, 4, s->i8, s->ldb, 4, s->n, hipMemcpyDeviceToHost));
  PH_HIP(hipMemcpy2D(codes, s->dim, s->i8 + 4, s->ldb, s->dim, s->n, hipMemcpyDeviceToHost));
  return 0;
} catch (...) { return ph_caught(); }
