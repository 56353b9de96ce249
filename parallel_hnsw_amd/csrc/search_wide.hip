// The search kernels of f32 rows of 1537 .. 4096 floats in a translation unit of their own, compiled beside the other
// search units (none of whose kernels changes), and the function that hands them to the launchers of search.hip.
//
// The walk is the plain search's, unchanged (ph_search_body); what differs is the distance policy: DistF32Wide<NV>
// (wide_rows.h) keeps the query in registers and streams the candidate rows of a hop through in pieces.  One
// throughput kernel per queue size and chunk class, run by batches of every size.  No dense tables
// (ph_tiny_layer_count is 0 for these rows), no LDS visited table (vis_lds_shape: the bitmap in HBM), no latency,
// instrumented or big-queue kernel, no filtered, collecting or radius twin: the family is absent from
// pick_kernel_family, so those instances do not exist and their calls keep refusing such a store.
#include "search_kernels.h"
#include "wide_rows.h"

ph_search_fn ph_pick_kernel_wide(int capc, int nv) {
#define PH_KW(C, N) \
  if (capc == C && nv == N) return (ph_search_fn)ph_search_kernel<C, DistF32Wide<N>, PH_FM_NONE>;
  PH_KW(2, 8) PH_KW(2, 12) PH_KW(2, 16)
  PH_KW(4, 8) PH_KW(4, 12) PH_KW(4, 16)
  PH_KW(8, 8) PH_KW(8, 12) PH_KW(8, 16)
  PH_KW(16, 8) PH_KW(16, 12) PH_KW(16, 16)
#undef PH_KW
  return nullptr;
}
