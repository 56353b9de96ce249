// What the exact scans by a SET of labels share on the device -- the scan over posting lists (filter_labeled.hip) and
// the scan over spans of the (label, key) column (filter_label_ranged.hip): which query owns a pair of an untrusted CSR
// table (labelset_plan.h's claim), the marks of the subset form, and the test of a refused query.  (Kernels of the
// header: each unit launches its own copy.)
#pragma once
#include <hip/hip_runtime.h>

#include "labelset_plan.h"

// owner[nwant] is preset to PH_LABELSET_OWNER_NONE.  One thread per query claims the pairs of a sound range; the lowest
// query keeps a pair.
[[maybe_unused]] static __global__ __launch_bounds__(256) void ph_labelset_claim_kernel(const uint32_t *want_first, uint32_t nq,
                                                                                        uint32_t nwant, uint32_t *owner) {
  for (uint64_t q = (uint64_t)blockIdx.x * 256u + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * 256u) {
    const uint32_t b = want_first[q], e = want_first[q + 1u];
    if (!ph_labelset_range_ok(b, e, nwant)) continue;
    for (uint32_t i = b; i < e; i++)  // i < e <= nwant
      if (!ph_labelset_claim_goes_on(atomicMin(&owner[i], (uint32_t)q), (uint32_t)q)) break;
  }
}

// the subset form: sel [nq] is preset to 0; one thread per entry of the list marks its query
[[maybe_unused]] static __global__ __launch_bounds__(256) void ph_labelset_select_kernel(const uint32_t *list, uint32_t nlist,
                                                                                         uint32_t nq, uint32_t *sel) {
  for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < nlist; p += (uint64_t)gridDim.x * 256u)
    if (list[p] < nq) sel[list[p]] = 1u;
}

// whether query q owns every pair of a sound range [b, e): what makes its row; wave-uniform.  owner[] as the claim
// kernel left it.
__device__ __forceinline__ bool ph_labelset_owns_range(const uint32_t *owner, uint32_t nwant, uint32_t q, uint32_t b, uint32_t e,
                                                       uint32_t lane) {
  if (!ph_labelset_range_ok(b, e, nwant)) return false;
  for (uint32_t i0 = b; i0 < e; i0 += 64u) {  // i0 + lane cannot wrap: e <= nwant < 2^31
    const uint32_t i = i0 + lane;
    if (__ballot(i < e && owner[i] != q)) return false;
  }
  return true;
}
