// The search kernels of a bits store (PH_ROWS_BITS: one sign bit per component, rowstore.hip) in a translation unit of
// their own, compiled beside the other search units, and the function that hands them to the launchers of search.hip.
//
// The walk is the plain search's, unchanged (ph_search_body); what differs is the distance policy: DistBits<NV>
// (phnsw_device.h) keeps the query's sign words wave-uniform and gives every candidate of a hop a lane of its own --
// 2 NV 16-byte loads, 8 NV XOR + popcount, one ph_bits_distance.  No dense tables (ph_tiny_layer_count is 0 for the
// kind: a popcount is cheaper than a table look-up), no split descent, no LDS visited table (the bitmap in HBM), no
// filtered, collecting or radius twin: the family is absent from pick_kernel_family, so those instances do not exist.
#include "search_kernels.h"

ph_search_fn ph_pick_kernel_bits(int capc, int nv) {
#define PH_KB(C, N) \
  if (capc == C && nv == N) return (ph_search_fn)ph_search_kernel<C, DistBits<N>, PH_FM_NONE>;
  PH_KB(2, 1) PH_KB(2, 3) PH_KB(2, 6)
  PH_KB(4, 1) PH_KB(4, 3) PH_KB(4, 6)
  PH_KB(8, 1) PH_KB(8, 3) PH_KB(8, 6)
  PH_KB(16, 1) PH_KB(16, 3) PH_KB(16, 6)
#undef PH_KB
  return nullptr;
}
