// The PH_FM_LABELSET_RANGE instances of the search kernels (searches restricted to the vectors that carry one of a set
// of labels per query and whose key in an attribute column lies inside a range per query) and the two functions that
// hand them to the launchers of search.hip: a translation unit of their own, like the seven other twins, so that the
// instances compile beside them.
#include "search_kernels.h"

ph_search_fn ph_pick_labelset_ranged_kernel(int family, int capc, int nv, int pqr_m, bool pq_global) {
  return pick_kernel_family<PH_FM_LABELSET_RANGE>(family, capc, nv, pqr_m, pq_global);
}
ph_search_fn ph_pick_labelset_ranged_dense(int capc) { return pick_kernel_dense<PH_FM_LABELSET_RANGE>(capc); }
