// The radius search by graph walk (phnsw_search_batch_radius[_device]): the radius twins of the search kernels
// (PH_FM_RADIUS, search_kernels.h) in a translation unit of their own, compiled beside the other search units, the
// function that hands them to the launchers of search.hip, and the two entry points.
//
// The reference's own functions, composed: search_layers' descent over layers[0 .. L-1) (search.rs:93-140), the running
// candidates mapped to NodeIds of the bottom layer as closest_vectors maps them (lib.rs:258-266) into a queue of
// capacity number_of_candidates, then threshold_nn's loop (lib.rs:944-953) on that queue with threshold = radius[q], and
// the result read from the queue (lib.rs:954-959): the entries other than exclude[q], taken while d < radius[q].
//
// One launch per call, whatever the batch: a radius call takes no part in the split descent, the locality order or
// the dense top-layer tables (ph_search_device: out_stride and radius switch them off).  Those change where rows are
// read from and in which order queries run, never a result, so nothing a caller can see depends on the choice; what it
// costs a large batch is not measured.  The queues are the 1024-slot LDS queues: a query whose queue would pass 1024
// entries ends with status 6 and an empty row -- phnsw_search_exact_radius is the answer there.
#include "search_kernels.h"

#include "host_call.h"

template <template <int, int> class D>
static ph_search_fn pick_radius_rows(int nv) {
  switch (nv) {
    case 1: return (ph_search_fn)ph_search_kernel<16, D<1, 4>, PH_FM_RADIUS>;
    case 3: return (ph_search_fn)ph_search_kernel<16, D<3, 4>, PH_FM_RADIUS>;
    case 6: return (ph_search_fn)ph_search_kernel<16, D<6, 4>, PH_FM_RADIUS>;
  }
  return nullptr;
}

ph_search_fn ph_pick_radius_kernel(int family, int nv) {
  switch (family) {
    case PH_KF_ROWS_F32: return pick_radius_rows<DistF32>(nv);
    case PH_KF_ROWS_F16: return pick_radius_rows<DistF16>(nv);
    case PH_KF_ROWS_I8: return pick_radius_rows<DistI8>(nv);
    case PH_KF_ROWS_I8Q: return pick_radius_rows<DistI8Q>(nv);
    default: return nullptr;
  }
}

// what both entry points check first, in this order: the index and the search parameters (as phnsw_search_batch), max_out,
// the store
static int radius_walk_check(const phnsw_index *ix, const phnsw_search_params *sp, uint64_t max_out, const char *call) {
  if (ix) PH_TRY(ph_bits_unsupported(ix->store, call));  // a bits store has the plain walk alone
  PH_TRY(ph_check_sp(ix, sp));
  if (max_out < 1u || max_out > 1024u) {
    ph_set_error("%s: max_out must be 1..1024 (got %llu)", call, (unsigned long long)max_out);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  if (ph_store_pq(s) || ph_store_pq_shared(s)) {
    ph_set_error("%s: the radius walk runs over row vectors (f32, f16, i8, i8q), not over a %s store", call, ph_rows_name(s->kind));
    return PHNSW_E_UNSUPPORTED;
  }
  if (!ph_chunk_count(s->ld / 4)) return ph_dim_unsupported(s->dim);
  return 0;
}

extern "C" int phnsw_search_batch_radius_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                                const uint32_t *exclude_dev, const float *radius_dev, uint64_t max_out,
                                                uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) try {
  const char *const call = "phnsw_search_batch_radius_device";
  PH_TRY(radius_walk_check(ix, sp, max_out, call));
  if (nq == 0) return 0;
  if (!ph_device_queries_ok(ix, queries_dev, qids_dev, ldq) || !radius_dev || !out_ids_dev || !out_d_dev || !out_len_dev ||
      !status_dev || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (queries or qids, exactly one; radius; outputs; queries need ldq >= store ld, multiple "
                 "of 4, 16-byte base)", call);
    return PHNSW_E_INVALID;
  }
  PhSearchCall c = {};
  c.queries = queries_dev, c.ldq = ldq, c.qids = qids_dev, c.exclude = exclude_dev, c.nq = nq, c.sp = sp;
  c.out_ids = out_ids_dev, c.out_d = out_d_dev, c.out_len = out_len_dev, c.out_stats = out_stats_dev, c.status = status_dev;
  c.out_stride = (uint32_t)max_out, c.radius = radius_dev, c.stream = (hipStream_t)stream;
  PH_HIP(hipSetDevice(ix->store->device));
  return ph_search_device(ix, c);
} catch (...) { return ph_caught(); }

extern "C" int phnsw_search_batch_radius(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                         const phnsw_search_params *sp, const uint64_t *exclude, const float *radius,
                                         uint64_t max_out, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                         uint64_t *out_stats, uint32_t *out_status) try {
  const char *const call = "phnsw_search_batch_radius";
  PH_TRY(radius_walk_check(ix, sp, max_out, call));
  if (nq == 0) return 0;
  if ((!queries) == (!qids)) {
    ph_set_error("%s: pass queries or qids (exactly one)", call);
    return PHNSW_E_INVALID;
  }
  if (!radius || !out_ids || !out_d || !out_len || !out_status || nq > 0xFFFFFFFFull) {
    ph_set_error("%s: invalid argument (radius, out_ids, out_d, out_len, out_status)", call);
    return PHNSW_E_INVALID;
  }
  const phnsw_store *s = ix->store;
  PH_HIP(hipSetDevice(s->device));
  PH_TRY(ph_stored_ids_check(qids, nq, s->n, "search"));
  phnsw_index *mix = const_cast<phnsw_index *>(ix);
  // the scratch set of a radius call (filter_radius.hip's pool): only its stream and its event are used here
  PhCallSet *set = ph_radius_host_set(mix);
  PhHostCall h(mix->radii, set);
  // small's extra: the counters [nq][2], read back with len and status, then the radii [nq]
  PH_TRY(h.stage_in(s, queries, qids, exclude, nq, (size_t)nq * 3u, 2, (uint32_t)max_out, (uint32_t)max_out));
  uint32_t *const stats = h.extra();
  float *const rad = (float *)(h.extra() + 2u * nq);
  PH_HIP(hipMemcpyAsync(rad, radius, (size_t)nq * 4u, hipMemcpyHostToDevice, h.st));
  PhSearchCall c = {};
  h.fill(c);
  c.sp = sp, c.out_stats = stats, c.out_stride = (uint32_t)max_out, c.radius = rad;
  PH_TRY(ph_search_device(ix, c));
  PH_TRY(h.finish(out_ids, out_d, nullptr));
  for (uint64_t i = 0; i < nq; i++) {
    out_len[i] = h.len(i);  // every entry inside the radius: may exceed max_out
    out_status[i] = h.status(i);
    if (out_stats) out_stats[2 * i] = h.read_extra(0, 2 * i), out_stats[2 * i + 1] = h.read_extra(0, 2 * i + 1);
  }
  return 0;
} catch (...) { return ph_caught(); }
