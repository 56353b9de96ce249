// Half-precision row store: the rows of an f32 store rounded to IEEE binary16 (round to nearest even,
// ph_f32_to_f16_bits) and kept as [n][ldh] halves in component order, ldh == ld, so a row starts on an 8-byte
// boundary and a lane's chunk of four components is one 8-byte load (DistF16 / RowF16, phnsw_device.h).
//
// The contract: a distance on this store is the f32 chain on the WIDENED rows -- widening is exact -- so a search
// equals, bit for bit, the f32 search over the store phnsw_store_read returns.  The store serves searches and
// distance batches only (ph_search_only_unsupported names everything else).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "phnsw_device.h"

// one thread per component of the padded row; a NaN or a magnitude that rounds to infinity raises the flag
__global__ void ph_f16_convert_kernel(const float *__restrict__ rows, uint32_t ld, uint32_t dim, uint64_t n,
                                      uint16_t *__restrict__ half, uint32_t ldh, uint32_t *bad) {
  const uint64_t total = n * (uint64_t)ldh;
  bool mine = false;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / ldh;
    const uint32_t c = (uint32_t)(x - r * ldh);
    uint16_t h = 0;
    if (c < dim) {
      h = ph_f32_to_f16_bits(rows[r * ld + c]);
      mine |= (h & 0x7C00u) == 0x7C00u;
    }
    half[x] = h;
  }
  if (mine) atomicOr(bad, 1u);
}

// rows [first, first + count) widened into a dense [count][dim] f32 array: what the distance kernels see
__global__ void ph_f16_widen_kernel(const uint16_t *__restrict__ half, uint32_t ldh, uint32_t dim, uint64_t first,
                                    uint64_t count, float *__restrict__ out) {
  const uint64_t total = count * (uint64_t)dim;
  for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = x / dim;
    const uint32_t c = (uint32_t)(x - r * dim);
    out[x] = __half2float(__ushort_as_half(half[(first + r) * ldh + c]));
  }
}

// the rows of `ids` (stride apart) widened into [cnt][ld] f32 rows: operands of the locality cells' GEMM (bruteforce.hip)
__global__ void ph_f16_gather_rows_kernel(const uint16_t *__restrict__ half, uint32_t ld, const uint32_t *ids,
                                          uint32_t first, uint32_t cnt, float *__restrict__ out) {
  const uint32_t r = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (r >= cnt) return;
  const uint64_t id = ids ? ids[r] : first + r;
  const uint2 *src = (const uint2 *)(half + id * ld);
  float4 *dst = (float4 *)(out + (uint64_t)r * ld);
  for (uint32_t j = lane; j < ld / 4; j += 64) dst[j] = RowF16::widen(src[j]);
}

int ph_f16_gather_rows(const phnsw_store *s, const uint32_t *ids_dev, uint32_t first, uint32_t cnt, float *out_dev) {
  if (cnt == 0) return 0;
  hipLaunchKernelGGL(ph_f16_gather_rows_kernel, dim3((cnt + 3) / 4), dim3(256), 0, 0, s->half, s->ldh, ids_dev, first, cnt,
                     out_dev);
  PH_HIP(hipGetLastError());
  return 0;
}

int ph_f16_store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out) {
  const uint64_t PIECE = 65536;
  float *tmp = nullptr;
  PH_HIP(hipMalloc(&tmp, (size_t)std::min(PIECE, count) * s->dim * 4));
  int rc = 0;
  for (uint64_t at = 0; at < count && !rc; at += PIECE) {
    const uint64_t cnt = std::min(PIECE, count - at);
    const uint64_t total = cnt * s->dim;
    hipLaunchKernelGGL(ph_f16_widen_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 65536)), dim3(256), 0, 0,
                       s->half, s->ldh, s->dim, first + at, cnt, tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out + at * s->dim, tmp, (size_t)total * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = ph_hip_fail(e, "f16 store read", __FILE__, __LINE__);
  }
  hipFree(tmp);
  return rc;
}

extern "C" int phnsw_store_create_f16(const phnsw_store *full, phnsw_store **out) try {
  if (!full || !out) {
    ph_set_error("phnsw_store_create_f16: full and out must not be NULL");
    return PHNSW_E_INVALID;
  }
  if (!full->rows) {
    ph_set_error("phnsw_store_create_f16: the source must be an f32 store");
    return PHNSW_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    ph_set_error("no HIP device available (libphnsw has no CPU fallback)");
    return PHNSW_E_NO_DEVICE;
  }
  PH_HIP(hipSetDevice(full->device));
  phnsw_store *s = new phnsw_store();
  s->device = full->device;
  s->n = full->n;
  s->dim = full->dim;
  s->ld = full->ld;
  s->ldh = full->ld;
  s->metric = full->metric;
  s->rows = nullptr;
  uint32_t *bad = nullptr;
  uint32_t h_bad = 0;
  const uint64_t total = s->n * (uint64_t)s->ldh;
  hipError_t e = hipMalloc(&s->half, (size_t)total * 2);
  if (e == hipSuccess) e = hipMalloc(&bad, 4);
  if (e == hipSuccess) e = hipMemset(bad, 0, 4);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ph_f16_convert_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 1u << 20)), dim3(256), 0, 0,
                       full->rows, full->ld, full->dim, s->n, s->half, s->ldh, bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(&h_bad, bad, 4, hipMemcpyDeviceToHost);
  if (bad) hipFree(bad);
  int rc = 0;
  if (e != hipSuccess)
    rc = ph_hip_fail(e, "f16 store conversion", __FILE__, __LINE__);
  else if (h_bad) {
    ph_set_error("phnsw_store_create_f16: a component is NaN or rounds to infinity in binary16 (|x| >= 65520)");
    rc = PHNSW_E_INVALID;
  }
  if (rc) {
    if (s->half) hipFree(s->half);
    delete s;
    return rc;
  }
  *out = s;
  return 0;
} catch (...) { return ph_caught(); }
