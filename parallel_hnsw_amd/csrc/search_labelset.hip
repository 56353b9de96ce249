// The PH_FM_LABELSET instances of the search kernels (searches restricted to the vectors that carry one of a SET of labels
// per query, read from a label column and a CSR table of wanted labels) and the two functions that hand them to the
// launchers of search.hip: a translation unit of their own, compiled beside search.o and search_labeled.o.
#include "search_kernels.h"

ph_search_fn ph_pick_labelset_kernel(int family, int capc, int nv, int pqr_m, bool pq_global) {
  return pick_kernel_family<PH_FM_LABELSET>(family, capc, nv, pqr_m, pq_global);
}
ph_search_fn ph_pick_labelset_dense(int capc) { return pick_kernel_dense<PH_FM_LABELSET>(capc); }
