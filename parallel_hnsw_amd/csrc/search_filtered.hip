// The PH_FM_BITMAP instances of the search kernels (searches restricted to an allow-list of VectorIds) and the two functions
// that hand them to the launchers of search.hip: a translation unit of their own, compiled beside search.o.
#include "search_kernels.h"

ph_search_fn ph_pick_filtered_kernel(int family, int capc, int nv, int pqr_m, bool pq_global) {
  return pick_kernel_family<PH_FM_BITMAP>(family, capc, nv, pqr_m, pq_global);
}
ph_search_fn ph_pick_filtered_dense(int capc) { return pick_kernel_dense<PH_FM_BITMAP>(capc); }
