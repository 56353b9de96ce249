// The collecting twins of the search kernels over a label column (PH_FM_LABEL | PH_FM_COLLECT,
// phnsw_search_collect_labeled[_device]) and the function that hands them to the launchers of search.hip: a translation
// unit of their own, compiled beside the other search units.
#include "search_kernels.h"

ph_search_fn ph_pick_collect_labeled_kernel(int family, int capc, int nv, int pqr_m, bool pq_global) {
  return pick_kernel_family<PH_FM_LABEL | PH_FM_COLLECT>(family, capc, nv, pqr_m, pq_global);
}
