/*
 * phnsw.h -- C ABI of the MI355X-native HNSW build + search engine.
 *
 * Drop-in boundary for ONE hot path of terminusdb-labs/parallel-hnsw (Rust): the per-hop
 * candidate distance batch and the greedy layer search / layer construction loops around
 * it.  The reference's seam is the generic, one-pair-per-call trait
 *     Comparator::{lookup, compare_raw, compare_vec}            src/lib.rs:53-74
 * which cannot feed a GPU, so this ABI sits one level up, under the method surface of
 *     Hnsw<C>::{generate, search, search_upto, improve_index, improve_neighbors,
 *               stochastic_recall, knn, threshold_nn}           src/lib.rs:585-1686
 * and batches beneath it.  A Rust shim implements `Comparator` for a
 * store handle and wraps `Hnsw` around an index handle.
 *
 * Conventions
 *  - every entry point returns 0 on success, a negative PHNSW_E_* otherwise, and never
 *    unwinds; phnsw_last_error() gives the message of the calling thread's last failure.
 *    (The reference panics: unwrap lib.rs:261, NaN types.rs:86, empty input lib.rs:683,837.)
 *  - ids are u64 at the boundary like the reference's usize VectorId/NodeId
 *    (src/types.rs:3-13); PHNSW_EMPTY == !0 is the empty-slot sentinel.
 *  - host pointers unless the name ends in _device; outputs are caller allocated; the
 *    library never frees caller memory and copies what it needs before returning.
 *  - search entry points are thread safe; build / improve entry points need exclusive
 *    access to their index (lib.rs: &self vs &mut self).
 *  - there is NO CPU fallback: every call fails with PHNSW_E_NO_DEVICE without a gfx950 GPU.
 */
#ifndef PHNSW_H
#define PHNSW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHNSW_EMPTY UINT64_MAX /* VectorId::MAX / NodeId::MAX  src/types.rs:8-13 */

enum {
  PHNSW_OK = 0,
  PHNSW_E_INVALID = -1,   /* bad argument (the reference would panic/assert) */
  PHNSW_E_NO_DEVICE = -2, /* no HIP device / wrong architecture */
  PHNSW_E_HIP = -3,       /* HIP runtime error, see phnsw_last_error */
  PHNSW_E_MISSING_NODE = -4, /* candidate vector absent from a lower layer (lib.rs:261 unwrap) */
  PHNSW_E_OVERFLOW = -5,  /* frontier workspace exhausted even after growth */
  PHNSW_E_NAN = -6,       /* NaN in input vectors (types.rs:86 would panic later) */
  PHNSW_E_UNSUPPORTED = -7,
  PHNSW_E_NOMEM = -8      /* host allocation failed (a C++ exception never crosses this ABI) */
};

/* the three Comparator::compare_raw implementations in the reference tree */
enum {
  PHNSW_METRIC_COSINE_HALF = 0,   /* (1 - dot)/2        BigComparator, src/bigvec.rs:47-53 */
  PHNSW_METRIC_ONE_MINUS_DOT = 1, /* 1 - dot            src/lib.rs:1985-1991 */
  PHNSW_METRIC_L2 = 2             /* sqrt(sum (a-b)^2)  src/lib.rs:2431-2437, src/pq.rs:499-505 */
};

/* SearchParameters  src/parameters.rs:3-18 (field for field) */
typedef struct {
  uint64_t number_of_candidates;
  uint64_t upper_layer_candidate_count;
  uint64_t probe_depth;
} phnsw_search_params;

/* OptimizationParameters  src/parameters.rs:20-40 */
typedef struct {
  float promotion_threshold;
  float neighborhood_threshold;
  float recall_proportion;
  float promotion_proportion;
  phnsw_search_params search;
} phnsw_optimization_params;

/* BuildParameters  src/parameters.rs:42-64, plus the two knobs that replace the
 * reference's non-determinism / unbounded loops */
typedef struct {
  uint64_t order;
  uint64_t zero_layer_neighborhood_size;
  uint64_t neighborhood_size;
  phnsw_optimization_params optimization;
  phnsw_search_params initial_partition_search;
  uint64_t seed;            /* replaces thread_rng() of lib.rs:832 */
  uint64_t max_link_rounds; /* 0 = loop until improvement < neighborhood_threshold (lib.rs:1527) */
  uint64_t promote;         /* 1 (default) = promote_at_layer as the reference (lib.rs:1575-1589); 0 = never */
} phnsw_build_params;

void phnsw_default_search_params(phnsw_search_params *sp);
void phnsw_default_build_params(phnsw_build_params *bp);

typedef struct phnsw_store phnsw_store; /* vector store + metric == a Comparator */
typedef struct phnsw_index phnsw_index; /* Hnsw<C> */

/* ProgressMonitor::update / keep_alive  src/progress.rs:12-16: called from the calling
 * thread between build phases; return non-zero to request an interrupt. */
typedef int (*phnsw_progress_cb)(void *user, const char *phase, uint64_t done, uint64_t total);

const char *phnsw_last_error(void);
int phnsw_device_count(void);

/* ---- store: replaces BigComparator{data: Arc<Vec<Vec<f32>>>}  src/bigvec.rs:38-57 ----
 * rows are copied into one flat HBM array [n][ld], ld = dim rounded up to 4 floats. */
int phnsw_store_create(const float *rows, uint64_t n, uint32_t dim, int metric, int device,
                       phnsw_store **out);
/* append rows to a store that owns its array (ids continue at the old n; *out_first_id = first
 * new VectorId).  The reference grows the Vec behind its comparator the same way before it
 * indexes new ids (src/bigvec.rs:38-44).  Not concurrent with searches/builds on this store. */
int phnsw_store_append(phnsw_store *s, const float *rows, uint64_t count, uint64_t *out_first_id);
/* adopt an existing device array (e.g. a torch tensor); caller keeps it alive */
int phnsw_store_create_device(const float *rows_dev, uint64_t n, uint32_t dim, uint32_t ld,
                              int metric, int device, phnsw_store **out);
/* synthetic rows with the distribution of random_normed_vec (src/bigvec.rs:59-65),
 * generated on the device: component j of vector i keyed (seed + first + i, j) */
int phnsw_store_create_synthetic(uint64_t first, uint64_t n, uint32_t dim, uint64_t seed,
                                 int normalize, int metric, int device, phnsw_store **out);
/* clustered synthetic rows (n_clusters unit centres + uniform noise of norm ~noise,
 * normalised): the benchmark dataset on which recall@10 >= 0.95 is reachable */
int phnsw_store_create_clustered(uint64_t first, uint64_t n, uint32_t dim, uint64_t seed,
                                 uint32_t n_clusters, float noise, int metric, int device,
                                 phnsw_store **out);
int phnsw_store_info(const phnsw_store *s, uint64_t *n, uint32_t *dim, uint32_t *ld, int *metric,
                     const float **rows_dev);
/* copy rows [first, first+count) back to the host, dim floats each */
int phnsw_store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out);
void phnsw_store_destroy(phnsw_store *s);

/* Comparator::compare_vec batched  src/lib.rs:69-73: out[i] = d(query, Stored(ids[i])).
 * query == NULL means AbstractVector::Stored(query_id). */
int phnsw_distance_batch(const phnsw_store *s, const float *query, uint64_t query_id,
                         const uint64_t *ids, uint64_t k, float *out);

/* ---- index ---- */
/* adopt a layer stack built elsewhere (e.g. by the Rust crate); layers top first like
 * Hnsw.layers (lib.rs:587); nodes sorted ascending; neighbor rows padded with PHNSW_EMPTY */
int phnsw_index_from_layers(phnsw_store *s, uint32_t layer_count, const uint64_t *node_counts,
                            const uint64_t *neighborhood_sizes, const uint64_t *const *nodes,
                            const uint64_t *const *neighbors, phnsw_index **out);
/* Hnsw::generate  src/lib.rs:825-893 */
int phnsw_build(phnsw_store *s, const uint64_t *vids, uint64_t n, const phnsw_build_params *bp,
                phnsw_progress_cb cb, void *user, phnsw_index **out);
/* Hnsw::generate_layer appended below the current stack  src/lib.rs:675-823 */
int phnsw_generate_layer(phnsw_index *ix, const uint64_t *vids, uint64_t n,
                         uint64_t neighborhood_size, const phnsw_build_params *bp);
/* link_layer_to_better_neighbors  src/lib.rs:1070-1154 ; *out_added = new edges */
int phnsw_link_layer(phnsw_index *ix, uint32_t layer_from_top, const phnsw_search_params *sp,
                     uint64_t link_count, uint64_t *out_added);
/* Hnsw::improve_index(bp, last_recall, progress)  src/lib.rs:1664-1686, promotion included
 * (bp->promote).  last_recall: NaN = None (the recall is estimated first, lib.rs:1671); a number is
 * taken as the current recall, exactly like Some(r) -- it only saves that first estimate, every
 * improve_index_at call below is made with None (lib.rs:1679). */
int phnsw_improve_index(phnsw_index *ix, const phnsw_build_params *bp, float last_recall,
                        phnsw_progress_cb cb, void *user, float *out_recall);
/* Hnsw::improve_neighbors_upto  src/lib.rs:1515-1544 ; last_recall NaN = None */
int phnsw_improve_neighbors_upto(phnsw_index *ix, uint32_t upto, const phnsw_build_params *bp,
                                 float last_recall, float *out_recall);
/* Hnsw::extend_layer  src/lib.rs:1039-1068: vids join the layer with empty neighbourhoods, NodeIds
 * are renumbered (generate_node_maps :1767-1812); inserting a vector twice is PHNSW_E_INVALID */
int phnsw_extend_layer(phnsw_index *ix, uint32_t layer_from_top, const uint64_t *vids, uint64_t n);
/* Hnsw::promote_at_layer  src/lib.rs:1273-1427 ; *out_promoted = the bool it returns */
int phnsw_promote_at_layer(phnsw_index *ix, uint32_t layer_from_top, const phnsw_build_params *bp,
                           int *out_promoted);
/* Hnsw::discover_unreachable_vectors  src/lib.rs:1002-1037 ; out sized node_count of the layer */
int phnsw_discover_unreachable(phnsw_index *ix, uint32_t layer_from_top, const phnsw_search_params *sp,
                               uint64_t *out_vecs, uint64_t *out_count);
/* Hnsw::stochastic_recall_at  src/lib.rs:1463-1499 */
int phnsw_stochastic_recall_at(phnsw_index *ix, uint32_t layer_from_top,
                               const phnsw_optimization_params *op, float *out_recall);
void phnsw_index_destroy(phnsw_index *ix);

uint32_t phnsw_index_layer_count(const phnsw_index *ix);
/* Layer{neighborhood_size, nodes, neighbors}  src/lib.rs:85-91 */
int phnsw_index_layer_info(const phnsw_index *ix, uint32_t layer_from_top, uint64_t *node_count,
                           uint64_t *neighborhood_size);
int phnsw_index_layer_read(const phnsw_index *ix, uint32_t layer_from_top, uint64_t *nodes,
                           uint64_t *neighbors);

/* Hnsw::search for a batch  src/lib.rs:663-665 -> src/search.rs:84-140.
 * queries: nq rows of dim floats (AbstractVector::Unstored).  exclude: NULL or nq ids
 * (PHNSW_EMPTY = None).  upto_layers: 0 = all (Hnsw::search_upto lib.rs:654-661).
 * Outputs: [nq][number_of_candidates] ids / distances sorted by (distance, id), padded with
 * PHNSW_EMPTY / f32::MAX; out_len[q] = valid entries; out_stats (nullable) [nq][2] =
 * {distance evaluations, hops}. */
int phnsw_search_batch(const phnsw_index *ix, const float *queries, uint64_t nq,
                       const phnsw_search_params *sp, uint32_t upto_layers,
                       const uint64_t *exclude, uint64_t *out_ids, float *out_d,
                       uint64_t *out_len, uint64_t *out_stats);
/* same for AbstractVector::Stored(qids[q]) */
int phnsw_search_batch_stored(const phnsw_index *ix, const uint64_t *qids, uint64_t nq,
                              const phnsw_search_params *sp, uint32_t upto_layers,
                              const uint64_t *exclude, uint64_t *out_ids, float *out_d,
                              uint64_t *out_len, uint64_t *out_stats);
/* the same keeping only the best k <= number_of_candidates results per query, out_* [nq][k]: the reference
 * returns the whole queue and its callers truncate (lib.rs:1118 takes neighborhood_size, a k-NN service takes k);
 * here the truncation happens on the device, before the transfer.  Exactly one of queries / qids is non-NULL. */
int phnsw_search_batch_topk(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                            const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude, uint64_t k,
                            uint64_t *out_ids, float *out_d, uint64_t *out_len);
/* Hnsw::search_instrumented  src/lib.rs:667-673: the results of phnsw_search_batch plus, per query, the second
 * value of search_layers_instrumented (src/search.rs:93-140): the index_sum of the last hop of the bottom layer's
 * closest_nodes that changed the best candidate (lib.rs:211-231); UINT64_MAX = usize::MAX.  f32 stores. */
int phnsw_search_instrumented(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                              const phnsw_search_params *sp, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                              uint64_t *out_index_distance);
/* zero-copy form: everything already resident in HBM, u32 ids (0xFFFFFFFF = empty),
 * queries [nq][ldq] with ldq a multiple of 4 and zero padding, launched on `stream`
 * (a hipStream_t, NULL = default) without synchronising.  out_stats_dev [nq][2] u32.
 * Returns after enqueueing; per-query status lands in status_dev[nq] (0 = ok). */
int phnsw_search_batch_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                              const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                              uint32_t upto_layers, const uint32_t *exclude_dev,
                              uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                              uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* ---- searches restricted to an allow-list of VectorIds: Layer::closest_vectors' `include` closure
 * (src/lib.rs:250-277) as a bitmap instead of the one instantiation `|v| Some(v) != exclude` (src/search.rs:128-134).
 * A layer's result keeps v iff v != exclude[q] and the bit of v is set; take(candidate_count) counts kept entries only.
 * It is a POST-filter on each layer's queue: the traversal is the unfiltered one, so a filter of density p leaves about
 * p * number_of_candidates results -- selective filters want a larger number_of_candidates, and below some density no
 * number_of_candidates is large enough: there phnsw_search_exact_filtered (below) scans the allowed rows instead.
 * The entry vector (layers[0].nodes[0]) enters the candidates before any filter runs (search.rs:102-111) and can be
 * returned although it is disallowed, exactly as it can be returned although excluded; PHNSW_FILTER_STRICT removes
 * disallowed ids from the final rows (lengths shrink, padding PHNSW_EMPTY / f32::MAX).
 * Every store kind phnsw_search_batch accepts (f32, f16, i8, i8q, PQ).  The re-ranked calls (phnsw_f16_ / phnsw_i8_ /
 * phnsw_i8q_search_batch[_device], phnsw_pq_search_batch*) take no filter. */
enum { PHNSW_FILTER_STRICT = 1 };
/* phnsw_search_batch_topk restricted to allowed VectorIds.  filter: bitmap words, bit v%32 of word v/32 set = allowed;
 * filter_stride_words 0 = one bitmap of ceil(n/32) words for all queries, else nq bitmaps that far apart (>= ceil(n/32)):
 * `filter` then holds nq * filter_stride_words words, the last bitmap a whole stride like the others (the host form
 * copies whole strides).  Bits at or past n are ignored.  filter NULL = the index's default filter
 * (phnsw_index_set_filter_device), else none.
 * k 0 = number_of_candidates (the shape of phnsw_search_batch): out_ids / out_d hold nq rows of k entries, of
 * number_of_candidates entries when k is 0.  out_stats nullable.  Exactly one of queries / qids. */
int phnsw_search_batch_filtered(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                const uint32_t *filter, uint32_t filter_stride_words, uint32_t flags, uint64_t k,
                                uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats);
/* phnsw_search_batch_device with the same filter, its words resident in HBM (rows of number_of_candidates entries) */
int phnsw_search_batch_filtered_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                       const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                       uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *filter_dev,
                                       uint32_t filter_stride_words, uint32_t flags, uint32_t *out_ids_dev,
                                       float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_stats_dev,
                                       uint32_t *status_dev, void *stream);
/* tombstones: a shared device bitmap of ceil(n/32) words, kept alive by the caller, becomes the filter of every
 * FILTERED call on this index that passes filter == NULL (NULL here clears it).  The other entry points never see it.
 * Not to be called while searches on the index are in flight. */
int phnsw_index_set_filter_device(phnsw_index *ix, const uint32_t *filter_dev);
/* ---- exact top-k over the allow-list: the call for SELECTIVE filters.  No traversal: the allowed rows are scanned, so
 * the recall is 1 and the cost is one distance per candidate -- cheaper than the graph walk when few rows are allowed,
 * and the only form that answers at all when density * number_of_candidates falls below k.
 * A VectorId v is a candidate of query q iff v < n, its bit is set in q's bitmap, v != exclude[q] and v is a vector of
 * the index's bottom layer (an index may cover only part of its store).  Bitmap layout, stride rule and the default
 * filter (filter NULL) as phnsw_search_batch_filtered; no filter at all = every vector of the index; bits at or past n
 * are ignored.  There is no entry-vector quirk: a disallowed id is never returned.
 * Result: the k candidates with the smallest (distance, id), ascending; out_len[q] = min(k, candidates of q); rows of k
 * entries padded with PHNSW_EMPTY / f32::MAX.  The distance of (q, v) has exactly the bits phnsw_distance_batch returns
 * for it on the same store; equal distances are ordered by id.
 * +inf (an L2 sum of squares past f32::MAX): a candidate at +inf is a candidate like any other and is returned, behind
 * every finite one and in id order among its like, with the distance bits 0x7F800000; it counts in out_len.  The padding
 * value f32::MAX therefore compares BELOW such entries: tell padding by out_len (or PHNSW_EMPTY), not by the distance.
 * The graph walk (phnsw_search_batch[_filtered]) never returns a candidate at +inf -- the reference's queue never holds
 * one -- so on such data this call and the walk differ by design; phnsw_search_exact_shared follows this call.
 * 1 <= k <= 1024, else PHNSW_E_INVALID.  nq == 0 is a
 * no-op.  Exactly one of queries / qids.  Every store kind phnsw_distance_batch accepts (f32, f16, i8, i8q, PQ); a
 * shared-codebook PQ store is PHNSW_E_UNSUPPORTED, and so is a PQ store whose lookup table plus the scan's own LDS
 * (16 * k + 8704 bytes) exceed a workgroup's 160 KiB.
 * Choosing between this call and phnsw_search_batch_filtered is the caller's job: phnsw_filter_count_device gives the
 * number of candidates to choose by.  Guidance (measured on 1M x 768 f32 rows, 10 000-query batches, k = 10;
 * profiles/filter_exact/README.md): the scan is the faster call below roughly 13 000 candidates per query with a shared
 * bitmap and about 10 000 with per-query bitmaps, and the only one that returns k results once density * 1024 < k.
 * phnsw_search_filtered_auto (below) makes this choice per query. */
int phnsw_search_exact_filtered(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                                const uint64_t *exclude, const uint32_t *filter, uint32_t filter_stride_words,
                                uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len);
/* zero-copy form: device pointers, u32 ids [nq][k] padded with 0xFFFFFFFF / f32::MAX, enqueued on `stream` without
 * synchronising; queries [nq][ldq] as for phnsw_search_batch_device.  status_dev[q]: 0 = ok, 4 = a Stored query id at
 * or past n (the row is then empty). */
int phnsw_search_exact_filtered_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                       const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                       const uint32_t *filter_dev, uint32_t filter_stride_words, uint64_t k,
                                       uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                       uint32_t *status_dev, void *stream);
/* the number of candidates of each of nbitmaps bitmaps (filter_stride_words apart; 0 = the one shared bitmap, counted
 * nbitmaps times): set bits below n whose vector is in the index, no exclude.  filter_dev NULL = the default filter,
 * else every vector of the index.  out_count_dev [nbitmaps] u32, device memory; enqueued on `stream`. */
int phnsw_filter_count_device(const phnsw_index *ix, const uint32_t *filter_dev, uint32_t filter_stride_words,
                              uint64_t nbitmaps, uint32_t *out_count_dev, void *stream);
/* ---- exact top-k for ONE allow-list shared by the whole batch, as a distance table.  With a shared bitmap (tombstones,
 * a category predicate, a tenant's bulk job) every query meets the same candidate rows: the call expands the bitmap to
 * the ascending list of its candidates and computes queries x candidates distance tables with the kernels of the dense
 * top layers (the f32 matrix cores for dot-product metrics at 256 / 768 / 1536 floats, the int8 matrix cores on an i8q
 * store, the vector-unit tile pass for L2, ragged dimensions and fewer than 32 queries; PHNSW_TINY_VALU=1 forces the
 * last), then selects the top k per query over the table.
 * Arguments: those of phnsw_search_exact_filtered[_device] without filter_stride_words -- `filter` is one bitmap of
 * ceil(n/32) words; NULL = the index's default filter (phnsw_index_set_filter_device), else every vector of the index.
 * Candidates: exactly those of phnsw_search_exact_filtered -- v < n, bit set, v != exclude[q], v a vector of the bottom
 * layer.  Result: the k candidates with the smallest (distance, id), ascending; out_len[q] = min(k, candidates of q);
 * rows of k entries padded with PHNSW_EMPTY / f32::MAX; 1 <= k <= 1024.
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for the same arguments with filter_stride_words 0; the distance has the bits of
 * phnsw_distance_batch.  The result does not depend on the chunk sizes below.
 * Checks, in this order: a null index or one without layers, then k outside 1..1024 (PHNSW_E_INVALID); then the store:
 * f32, f16, i8 and i8q stores with rows of at most 1536 floats, every metric the store kind has -- a PQ store of either
 * form and longer rows are PHNSW_E_UNSUPPORTED (phnsw_search_exact_filtered scans those); then nq == 0, a no-op; then
 * exactly one of queries / qids and the outputs (PHNSW_E_INVALID); the host form then refuses a Stored query id at or
 * past n as phnsw_search_exact_filtered does (PHNSW_E_INVALID).  phnsw_exact_shared_supported returns what the first
 * three checks return, without running anything.
 * Knobs (environment, read per call): PHNSW_DENSE_NODES, candidates per table (rounded up to a multiple of 64, default
 * 8192); PHNSW_DENSE_TABLE_BYTES, the bytes of one table (default 1 GiB, below 4 GiB), which bounds the queries per table.
 * Guidance (measured on 1M x 768 f32 rows, cosine, 10 000-query batches, k = 10, the three calls alternating in one
 * run; profiles/filter_dense/README.md): against phnsw_search_exact_filtered with the same shared bitmap this call was
 * the faster one in every cell, 6 x at 1 037 candidates rising to 18 x at 300 322, and no crossover was found (fewer
 * candidates were not measured).  Against the strict graph walk of phnsw_search_batch_filtered at the minimal
 * number_of_candidates (an APPROXIMATE result, recall@10 0.10-0.65) it was faster at 1 037, 9 988 and 20 043 candidates
 * (146 x, 22 x, 7 x) and SLOWER at 99 217 (18.3 ms against 13.2 ms) and 300 322 (55.0 ms against 8.7 ms): the crossover
 * lies between 20 000 and 99 000 candidates, and above it this call stands on its exact, bit-equal contract alone.
 * f16, i8 and i8q stores, L2 and ragged dimensions (the vector-unit pass), other k and batch sizes: not measured.
 * No other call routes here: phnsw_search_exact_filtered keeps scanning. */
int phnsw_exact_shared_supported(const phnsw_index *ix, uint64_t k);
int phnsw_search_exact_shared(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                              const uint64_t *exclude, const uint32_t *filter, uint64_t k, uint64_t *out_ids, float *out_d,
                              uint64_t *out_len);
/* device form: device pointers, u32 ids [nq][k] padded with 0xFFFFFFFF / f32::MAX; queries [nq][ldq] as for
 * phnsw_search_batch_device.  status_dev[q]: 0 = ok, 4 = a Stored query id at or past n (the row is then empty, the
 * other rows unaffected).  Unlike phnsw_search_exact_filtered_device this call SYNCHRONISES `stream`, once, to read the
 * candidate count back (the tables' shape depends on it); the tables and the selection are enqueued after that and the
 * call returns without waiting for them.  Thread safe like the other search calls: every call in flight has a scratch
 * set of its own. */
int phnsw_search_exact_shared_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                     const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                     const uint32_t *filter_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                     uint32_t *out_len_dev, uint32_t *status_dev, void *stream);
/* ---- exact RADIUS search: every candidate closer to a query than the query's radius, for a batch of queries and ONE
 * allow-list shared by the batch (near-duplicate detection, clustering joins, retrieval by threshold).  The candidates
 * and the distance tables are those of phnsw_search_exact_shared; in place of the top-k select a table is compacted by
 * threshold into a pool of (query, distance, id) records, which is sorted and unpacked after the last table.
 * Arguments: those of phnsw_search_exact_shared[_device] with `radius` [nq] f32 (one per query) and `cap`, the entries
 * out_ids / out_d hold, in place of k.
 * Candidates of q: exactly those of phnsw_search_exact_shared -- v < n, bit set (filter NULL = the index's default
 * filter, else every vector of the index), v != exclude[q], v a vector of the bottom layer.
 * A candidate is returned iff d(q, v) < radius[q] as an f32 comparison: strict, as the reference's threshold_nn takes
 * while distance < threshold (src/lib.rs:955-958).  A NaN, zero or negative radius matches nothing; a candidate at +inf
 * or NaN is never inside a radius, not even +inf.
 * Result (CSR): the rows of q are out_ids / out_d[out_first[q] .. out_first[q + 1]), ascending by (distance, id);
 * out_first has nq + 1 entries, out_first[0] == 0 and out_first[nq] == *out_total.  The distances carry the bits of
 * phnsw_distance_batch on the same store (a -0.0 comes back as +0.0, as from the exact top-k calls).
 * Size negotiation, as snprintf: out_first and *out_total are always complete and exact; out_ids / out_d are written
 * only if *out_total <= cap, and left untouched otherwise -- call again with cap >= *out_total.  cap == 0 with NULL
 * out_ids / out_d is the count-only form: no record is kept, sorted or written.  The return is PHNSW_OK in all three
 * cases.  cap <= 2^31 - 1 and nq <= 2^31 - 2, else PHNSW_E_INVALID.  The scratch of a call holds min(cap, nq x
 * candidates) records of 12 bytes twice over, so a cap far above the total costs device memory, not time.
 * The result does not depend on PHNSW_DENSE_NODES / PHNSW_DENSE_TABLE_BYTES (the knobs of phnsw_search_exact_shared,
 * which cut the tables here too), on the chunk plan or on how the waves are scheduled: the pool's order does, the
 * sorted order does not, because the keys of one query are distinct.
 * Checks, in this order (as phnsw_search_exact_shared, cap in k's place): a null index or one without layers, then cap
 * above 2^31 - 1 (PHNSW_E_INVALID); then the store: f32, f16, i8 and i8q stores with rows of at most 1536 floats, every
 * metric the store kind has -- a PQ store of either form and longer rows are PHNSW_E_UNSUPPORTED
 * (phnsw_exact_shared_supported(ix, 1) answers for this call too); then nq == 0: the empty result (the host form writes
 * out_first[0] = 0 and *out_total = 0 where the pointers are given; the device form enqueues nothing); then exactly one
 * of queries / qids, radius, out_first, out_total, the device form's status, out_ids / out_d unless cap == 0, nq
 * (PHNSW_E_INVALID); the host form then refuses a Stored query id at or past n as its siblings do (PHNSW_E_INVALID).
 * PHNSW_DENSE_TIMES=1 prints the steps' times of a call on stderr.
 * OUT OF SCOPE, so that nobody assumes otherwise: per-query bitmaps as the filter of a radius call (a row label or a
 * numeric range per query: phnsw_search_exact_radius_labeled / _ranged below); routing between a walk and this call; re-ranked (f16 / i8 / PQ first, f32 after) radius
 * calls -- a converted store is searched with its own distances, as by phnsw_search_exact_shared.
 * Guidance (measured on 1M x 768 f32 rows, cosine, 10 000-query batches, no filter, one radius for the batch, the calls
 * alternating in one run; profiles/radius/README.md): with 9.6 / 97.6 / 991.7 rows inside the radius per query on
 * average the call took 179.7 / 185.0 / 202.5 ms, against 177.3 ms of phnsw_search_exact_shared at k = 10 over the same
 * tables: 2.3, 8.0 and 25.2 ms for compaction, sort and unpack in place of that call's select.  The count-only form took
 * 176.0 / 179.8 / 185.9 ms.  Of a call's 150 ms of tables and 33 to 54 ms of compaction the sort is 0.2 to 1.1 ms.
 * f16, i8 and i8q stores, L2 and ragged dimensions (the vector-unit pass), a filter, per-query radii, other batch sizes,
 * the host form and a cap below the total (two calls): not measured. */
int phnsw_search_exact_radius(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                              const uint64_t *exclude, const uint32_t *filter, const float *radius, uint64_t cap,
                              uint64_t *out_first, uint64_t *out_ids, float *out_d, uint64_t *out_total);
/* device form: device pointers; u32 ids [cap], u64 out_first [nq + 1] and one u64 at out_total_dev; queries [nq][ldq]
 * as for phnsw_search_batch_device.  status_dev[q]: 0 = ok, 4 = a Stored query id at or past n (its segment is then
 * empty, the other segments unaffected).  The call SYNCHRONISES `stream` twice: once to read the candidate count back
 * (the tables' shape depends on it) and once, after the last table, to read the total (whether and how much to sort
 * depends on it); with cap == 0 only the first.  The sort and the unpack are enqueued after that and the call returns
 * without waiting for them.  Thread safe like the other exact calls: every call in flight has a scratch set of its
 * own. */
int phnsw_search_exact_radius_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                     const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                     const uint32_t *filter_dev, const float *radius_dev, uint64_t cap,
                                     uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                     uint32_t *status_dev, uint64_t *out_total_dev, void *stream);
/* ---- RADIUS search by graph walk: the approximate sibling of phnsw_search_exact_radius, for external queries with a
 * radius each.  The reference's own functions, composed: layers[0 .. L-1) are descended exactly as search_layers does
 * (search.rs:93-140: queue capacity number_of_candidates, upper_layer_candidate_count, probe_depth, include = v !=
 * exclude[q]); on the bottom layer the running candidates are mapped to NodeIds as closest_vectors maps them
 * (lib.rs:258-266) into a queue of capacity number_of_candidates, and that queue goes through threshold_nn's loop
 * (lib.rs:944-953) with threshold = radius[q]: last = 0, last_size = 0; while last < r and len > last_size: closest_nodes,
 * last = the queue's last distance, and the capacity doubles when last < r and the queue is full.
 * Result: the queue's entries with v != exclude[q], taken while d < radius[q], as VectorIds, ascending by (distance, id).
 * An excluded id is never returned (there is no entry-vector quirk: the row is read from the queue, not merged into the
 * running candidates).  out_len[q] is the number of such entries and MAY EXCEED max_out; the row holds the nearest
 * max_out of them, padded with PHNSW_EMPTY / f32::MAX; 1 <= max_out <= 1024.  A zero, negative or NaN radius makes no
 * bottom-layer call: the empty row, and the counters of the upper layers alone.
 * out_status[q]: 0 = ok; 4 = a candidate is not a node of the layer below, or (device form) a Stored query id at or past
 * n; 5 = the spill list overflowed; 6 = the queue would pass 1024 entries (the queues live in LDS): the row is empty
 * and out_len[q] is 0 -- phnsw_search_exact_radius answers such a query.  out_stats (nullable): [nq][2] = {distance
 * evaluations, hops}.  number_of_candidates <= 1024 as everywhere.
 * Every call runs as ONE launch: it takes no part in the split descent of large batches, the locality order or the
 * dense top-layer tables, none of which changes a result.  Stores: f32, f16, i8 and i8q rows of at most 1536 floats (a
 * converted store is searched with its own distances); a PQ store of either form is PHNSW_E_UNSUPPORTED.
 * Checks, in this order: the index and the search parameters as phnsw_search_batch; max_out outside 1..1024
 * (PHNSW_E_INVALID); the store; nq == 0, a no-op; exactly one of queries / qids, radius and the outputs
 * (PHNSW_E_INVALID); the host form then refuses a Stored query id at or past n.
 * OUT OF SCOPE: a filter on this call; the global-memory queue of phnsw_threshold_nn for external queries (status 6
 * instead); routing between this walk and the exact call on the device.
 * Guidance (1M x 768 f32 rows, 10 000 queries, max_out 1024, upper_layer_candidate_count = number_of_candidates / 4,
 * probe_depth 2; profiles/radius/README.md): at number_of_candidates 128 / 256 / 512 the walk took 10.3 / 13.5 / 19.7 ms
 * with about 10 rows inside the radius per query, 10.8 / 13.6 / 19.7 ms with about 98, and 20.9 / 20.0 / 21.1 ms with about
 * 992 -- 1.5 to 3.0 times the plain walk (phnsw_search_batch_device) at the same parameters -- and returned 0.81 / 0.91 /
 * 0.96, 0.74 / 0.84 / 0.91 and 0.40 / 0.42 / 0.44 of the exact in-radius rows; no query had status 6.  With
 * upper_layer_candidate_count equal to number_of_candidates the bottom-layer queue starts full and the loop ends after
 * one call (len cannot pass last_size): choose it smaller.  Other stores, metrics and batch sizes: not measured. */
int phnsw_search_batch_radius(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                              const phnsw_search_params *sp, const uint64_t *exclude, const float *radius,
                              uint64_t max_out, uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats,
                              uint32_t *out_status);
/* device form: device pointers, u32 ids [nq][max_out] padded with 0xFFFFFFFF / f32::MAX, u32 out_len and out_stats;
 * queries [nq][ldq] as for phnsw_search_batch_device; enqueued on `stream` without synchronising. */
int phnsw_search_batch_radius_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                     const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                     const uint32_t *exclude_dev, const float *radius_dev, uint64_t max_out,
                                     uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                     uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* ---- exact top-k for a TABLE of allow-lists with a selector per query, grouped by bitmap: a handful of distinct
 * bitmaps (tenants, ACL classes), each shared by many queries of the batch.  The call groups the batch by bitmap on the
 * device and runs every group as phnsw_search_exact_shared runs its batch -- the candidate list of the group's bitmap,
 * queries x candidates distance tables on the table kernels, a select per query -- with one stream synchronisation for
 * the whole call.  The caller neither replicates a bitmap per query (phnsw_search_exact_filtered's layout) nor splits
 * the batch by bitmap on the host (one phnsw_search_exact_shared call per bitmap).
 * Table: `filters` holds nfilters bitmaps, filter_stride_words apart; the stride is >= ceil(n/32) and REQUIRED (0 is
 * PHNSW_E_INVALID); bit layout as everywhere; bits at or past n, and the words between ceil(n/32) and the stride, are
 * ignored whatever they hold.  1 <= nfilters <= 0xFFFFFFFE.  filter_of[q] names the bitmap of query q, or is
 * PHNSW_FILTER_ALL: no bitmap, every vector of the index.  filters and filter_of must not be NULL; the index's default
 * filter (phnsw_index_set_filter_device) is NOT consulted: the caller passed a filter.
 * Candidates of q: exactly those of phnsw_search_exact_filtered when q's bitmap is filters[filter_of[q]] -- v < n, bit
 * set, v != exclude[q], v a vector of the bottom layer.
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for that query with that bitmap (hence also phnsw_search_exact_shared's row for a
 * group run alone); +inf, tie order by id and padding (PHNSW_EMPTY / f32::MAX) as there.  The result does not depend on
 * how the queries are spread over the bitmaps, on their order in the batch, or on any knob below.
 * Checks, in this order (as phnsw_search_exact_shared): a null index or one without layers, then k outside 1..1024
 * (PHNSW_E_INVALID); then the store: f32, f16, i8 and i8q stores with rows of at most 1536 floats, else
 * PHNSW_E_UNSUPPORTED (phnsw_exact_shared_supported answers for this call too); then nq == 0, a no-op; then exactly one
 * of queries / qids, the outputs, the table arguments above and nq <= 2^31 - 2 (PHNSW_E_INVALID).  The host form then
 * refuses, before any device work, a Stored query id at or past n and a selector that is neither below nfilters nor
 * PHNSW_FILTER_ALL (PHNSW_E_INVALID; the message names the query).
 * Knobs (environment, read per call): PHNSW_DENSE_NODES and PHNSW_DENSE_TABLE_BYTES as for phnsw_search_exact_shared,
 * applied per group; PHNSW_GROUP_LIST_BYTES, the bytes of candidate lists and per-word offsets built at a time
 * (default 256 MiB, at most 16 GiB): groups are taken in ascending bitmap order in rounds that fit it, a round always
 * taking at least one group, so the scratch never grows as nfilters x n beyond it.  PHNSW_GROUP_TIMES=1 prints the
 * steps' times of a call on stderr.
 * Guidance (measured on 1M x 768 f32 rows, cosine, 10 000-query batches spread evenly over the bitmaps, k = 10, the
 * variants alternating in one run; profiles/filter_grouped/README.md): against phnsw_search_exact_filtered with the
 * table replicated per query this call was 8.3 x, 4.1 x and 1.8 x faster at 1, 8 and 64 bitmaps of 10 000 candidates,
 * 3.7 x and 11.7 x at 8 bitmaps of 1 000 and 100 000 candidates, and FOUR TIMES SLOWER at 1000 bitmaps (groups of 10
 * queries: 166 ms against 42 ms) -- every group pays its own table and select launches, and groups below 32 queries run
 * on the vector units.  The crossover lies between 156 and 10 queries per group; below it the scan is the call.  Against
 * one phnsw_search_exact_shared call per bitmap over queries gathered on the host (gather and scatter not timed) it was
 * never slower and 1.2 x to 1.75 x faster from 8 bitmaps on.  Other store kinds, L2, ragged dimensions, other k, uneven
 * groups and the host form: not measured.  No other call routes here. */
enum { PHNSW_FILTER_ALL = 0xFFFFFFFFu }; /* filter_of[q]: no bitmap, every vector of the index */
int phnsw_search_exact_grouped(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                               const uint64_t *exclude, const uint32_t *filters, uint32_t filter_stride_words,
                               uint64_t nfilters, const uint32_t *filter_of, uint64_t k,
                               uint64_t *out_ids, float *out_d, uint64_t *out_len);
/* device form: device pointers, u32 ids [nq][k] padded with 0xFFFFFFFF / f32::MAX; queries [nq][ldq] as for
 * phnsw_search_batch_device.  status_dev[q]: 0 = ok; 4 = a Stored query id at or past n; 6 = a selector that is neither
 * below nfilters nor PHNSW_FILTER_ALL; 7 = the bitmap of q changed while the call read it (its candidate list no longer
 * had the counted length).  With 4, 6 and 7 the row is empty and out_len[q] is 0; every other query is unaffected, and
 * no bitmap word outside the table is ever read.  The host form reports 7 as PHNSW_E_INVALID.
 * The call SYNCHRONISES `stream` once: that read fetches the groups and the candidate count of every bitmap in use
 * together.  Everything after is enqueued and the call returns without waiting.  Selectors that change during that
 * read are PHNSW_E_INVALID.  Thread safe like the other exact calls: every call in flight has a scratch set of its own. */
int phnsw_search_exact_grouped_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                               const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                               const uint32_t *filters_dev, uint32_t filter_stride_words, uint64_t nfilters,
                               const uint32_t *filter_of_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                               uint32_t *out_len_dev, uint32_t *status_dev, void *stream);
/* ---- exact top-k by ROW LABEL, posting lists instead of bitmaps: the filter of a partition (a tenant, a collection,
 * an ACL class).  Every vector carries one u32 label and a query wants the rows of one label.  A phnsw_labels handle
 * turns the label column once into posting lists -- the ascending VectorIds of every label, CSR -- on the device; a
 * search derives nothing from a bitmap and reads nothing back.  A label column is 4 bytes per vector whatever the
 * number of labels (1000 bitmaps over 1M rows are 125 MB, 100 000 are 12.5 GB).
 * The handle also keeps the column itself on the device, label_of[n] -- the label of every listed vector, PHNSW_LABEL_NONE
 * for one that is not listed --, for the graph walk by label (phnsw_search_batch_labeled, below): 4 * n bytes more than the
 * posting lists.
 * Listed: vector v is listed under labels[v] iff v < n, labels[v] != PHNSW_LABEL_NONE and v is a vector of the index's
 * bottom layer (the candidate test of the other exact calls, without a bitmap).  Labels are arbitrary 32-bit values,
 * neither dense nor small.  n must equal the store's vector count, else PHNSW_E_INVALID.
 * The handle is a SNAPSHOT: it remembers the index, the store's n and the bottom layer's node count.  A search with a
 * handle made for another index, or after either count has changed, is PHNSW_E_INVALID ("the labels are stale"); make a
 * new handle.  The check cannot see more than that: an index destroyed and another created at the same address with the
 * same two counts but other vectors in its bottom layer passes it -- destroy the handle with its index.  Creation synchronises (the null stream, or `stream` of the device form, whose labels_dev is device
 * memory read before the call returns).  phnsw_labels_info: the n it was made for, the distinct labels that list a
 * vector, the listed vectors, the longest list; any output may be NULL.  phnsw_labels_count_device writes, per query,
 * the length of the list of want_dev[q], 0 for a label nobody carries and for PHNSW_LABEL_NONE: phnsw_filter_count_device's
 * figure for the equivalent bitmap; enqueued on `stream`.  phnsw_labels_destroy waits for the calls in flight that use
 * the handle; NULL is a no-op.  The handle does not own the index and must not outlive it in use.
 * Candidates of q: the listed vectors of label want[q], except exclude[q].  want[q] == PHNSW_LABEL_NONE, or a label
 * nobody carries, is no error: the row is empty, the length 0, the status 0.
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for that query with the bitmap {v : labels[v] == want[q]}: ascending (distance,
 * id), the distances with phnsw_distance_batch's bits, +inf and tie order as there, rows of k entries padded with
 * PHNSW_EMPTY / f32::MAX, 1 <= k <= 1024.  The result does not depend on how the batch is spread over the labels, on its
 * order, or on any knob below.
 * Checks, in this order: a null index or one without layers, then k outside 1..1024, then a null or stale `lb`
 * (PHNSW_E_INVALID); then the store: every kind phnsw_search_exact_filtered scans (f32, f16, i8, i8q, PQ), with its
 * limits -- a shared-codebook PQ store, rows above 1536 floats and a PQ table that does not fit beside the scan's LDS
 * are PHNSW_E_UNSUPPORTED; then nq == 0, a no-op; then exactly one of queries / qids, the outputs, `want` and
 * nq <= 2^31 - 2 (PHNSW_E_INVALID).  The host form then refuses a Stored query id at or past n (PHNSW_E_INVALID).
 * Every message names the call.
 * How: per query a binary search of its label; the batch sorted by label; on f32 / f16 / i8 row stores a wave then takes
 * a TILE of up to T queries of one label and reads every row of (a slice of) that label's list once for the whole tile;
 * i8q and PQ stores, and T = 1, scan the list per query.  Knobs (environment, read per call, none changes a result):
 * PHNSW_LABEL_TILE, 1 = the per-query scan only, N = a cap on T (default 16; T also shrinks with k and the row length
 * so that a CU holds four tile waves); PHNSW_LABEL_SLICES forces the number of slices a list is cut into.
 * Guidance (measured on 1M x 768 f32 rows, cosine, 10 000-query batches spread evenly over the labels, k = 10, the
 * variants alternating in one run; profiles/filter_labeled/README.md): against phnsw_search_exact_filtered with per-query
 * bitmaps this call was 1.4 x to 3.8 x faster in every cell (1, 8, 64 labels of 10 000 rows, 1000 labels of 1000 rows, 8
 * labels of 1000 and of 100 000 rows).  Against phnsw_search_exact_grouped it was SLOWER wherever groups are large --
 * 0.26 x and 0.36 x at 1 and 8 labels of 10 000 rows, 0.69 x and 0.29 x at 8 labels of 1000 and 100 000 rows -- and faster
 * at 64 labels (1.5 x) and at 1000 labels of 1000 rows (1.24 ms against 42.9 ms).  The tile path was 2.2 x to 3.6 x faster
 * than PHNSW_LABEL_TILE=1 except where a label has one query or a short list (0.94 x, 0.64 x).  Other store kinds, L2,
 * other k, uneven labels and the host form: not measured. */
typedef struct phnsw_labels phnsw_labels;
#define PHNSW_LABEL_NONE 0xFFFFFFFFu /* labels[v]: v is not listed; want[q]: an empty row */
int phnsw_labels_create(const phnsw_index *ix, const uint32_t *labels, uint64_t n, phnsw_labels **out); /* host labels [n] */
int phnsw_labels_create_device(const phnsw_index *ix, const uint32_t *labels_dev, uint64_t n, void *stream,
                               phnsw_labels **out);
int phnsw_labels_info(const phnsw_labels *lb, uint64_t *n, uint64_t *nlabels, uint64_t *listed, uint64_t *longest);
int phnsw_labels_count_device(const phnsw_labels *lb, const uint32_t *want_dev, uint64_t nq, uint32_t *out_count_dev,
                              void *stream);
void phnsw_labels_destroy(phnsw_labels *lb); /* waits for the calls in flight that use it */
int phnsw_search_exact_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                               uint64_t nq, const uint64_t *exclude, const uint32_t *want, uint64_t k, uint64_t *out_ids,
                               float *out_d, uint64_t *out_len);
/* device form: device pointers, u32 ids [nq][k] padded with 0xFFFFFFFF / f32::MAX; queries [nq][ldq] as for
 * phnsw_search_batch_device.  status_dev[q]: 0 = ok, 4 = a Stored query id at or past n (the row is then empty, the
 * other rows unaffected).  The call ENQUEUES AND RETURNS: it never synchronises `stream`; where a label's list lies and
 * how the batch falls into tiles stay on the device.  One exception to "returns at once": scratch is kept with the handle
 * and grows with the largest call; a call that needs MORE scratch than the set it was given holds waits on the host for
 * that set's previous call to finish before the old block goes back to the pool (calls of one size, or shrinking ones,
 * never wait).  Thread safe like the other exact calls: every call in flight has a scratch set of its own.  Calls on one
 * stream share one set; calls on different streams get sets of their own (four per handle before they share one behind
 * its event), so they may overlap.  The sets -- grouping arrays of 28 bytes per query, the sort's temporaries, nq x slices
 * x k keys -- stay with the handle until phnsw_labels_destroy. */
int phnsw_search_exact_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                      const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                      const uint32_t *want_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                      uint32_t *out_len_dev, uint32_t *status_dev, void *stream);
/* ---- exact top-k by a SET of row labels, `label IN (a, b, c)`: an ACL's groups, a few categories, a tenant plus the
 * shared collection, a time range as a few bucket labels.  One label per row makes the lists of distinct labels
 * disjoint, so a set is more slices of the same scan: a (query, wanted label) PAIR takes the place of a query in the
 * machinery of phnsw_search_exact_labeled, and a query that wants {a, b} shares the tile of label a with every other
 * query that wants a.  This is the EXACT scan; the graph walk by set is phnsw_search_batch_labelset and the routed call by
 * set phnsw_search_labelset_auto (both below, after their one-label forms).
 * The sets of a batch in CSR form: want_first[nq + 1] (u32, want_first[0] == 0, non-decreasing) and
 * want_values[nwant] (u32 labels), nwant == want_first[nq]; S_q = { want_values[i] : want_first[q] <= i < want_first[q+1] }.
 * Candidates of q: the vectors listed (as phnsw_labels_create lists) under any label of S_q, except exclude[q].  A label
 * that occurs twice in S_q counts once; PHNSW_LABEL_NONE and labels nobody carries contribute nothing; an empty set is no
 * error: the row is empty, the length 0, the status 0.
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for that query with the bitmap {v : v listed and labels[v] in S_q}: ascending
 * (distance, id) with phnsw_distance_batch's bits, +inf as there, equal distances by id ALSO where the tied rows come from
 * different lists, rows of k entries padded with PHNSW_EMPTY / f32::MAX, 1 <= k <= 1024.  Hence a batch of one-label
 * sets equals phnsw_search_exact_labeled's rows.  The result depends on none of: the order of labels inside a set, the
 * order of queries in the batch, how the sets overlap, any knob.
 * phnsw_labels_count_set_device: out_count[q] = the sum of the list lengths of the DISTINCT labels of S_q --
 * phnsw_filter_count_device's figure for the equivalent bitmap; a range the device form would refuse (below) counts 0;
 * enqueued on `stream`.  Its cost is quadratic in the length of a set (a wave per query tests distinctness in place).
 * Checks, in this order: those of phnsw_search_exact_labeled (index, k, null or stale `lb`, store kind and its limits);
 * then nq == 0, a no-op; then exactly one of queries / qids, the outputs, want_first, and want_values (NULL only when
 * nwant == 0); then nq and nwant <= 2^31 - 2 (PHNSW_E_INVALID).  The host form reads nwant from want_first[nq] and then
 * refuses, before any device work and naming the query, a Stored query id at or past n, want_first[0] != 0 and a
 * want_first that runs backwards (PHNSW_E_INVALID).  Staging as in the host form of phnsw_search_exact_labeled.
 * How: every query claims the pairs of its range; per pair a binary search of its label; the pairs sorted by label
 * (stable, so equal (label, query) pairs end up adjacent: the later ones are duplicates and are left out); the scan and
 * tile kernels of phnsw_search_exact_labeled over pairs, every pair writing its per-slice lists of k keys to scratch; then
 * a wave per query merges the lists of its pairs through the same running top-k.  Knobs: PHNSW_LABEL_TILE and
 * PHNSW_LABEL_SLICES with the meaning above; none changes a result.
 * Guidance (measured on 1M x 768 f32 rows, cosine, 10 000-query batches, k = 10, every query wanting `set size`
 * distinct labels drawn at random, the variants alternating in one run; profiles/labelset/README.md): against
 * phnsw_search_exact_filtered with the union as per-query bitmaps this call was faster in every cell -- 2.7 x, 3.0 x,
 * 3.6 x, 4.0 x and 4.5 x at sets of 1, 2, 4, 8 and 32 labels out of 1000 labels of 1000 rows (1.64 ms to 29.5 ms against
 * 4.41 ms to 132 ms), 4.7 x at sets of 4 out of 64 labels of 10 000 rows (34.0 ms against 161 ms).  At one label per set
 * it took 1.640 ms where phnsw_search_exact_labeled took 1.658 ms: the pairs and the merge that always runs cost less than
 * the run-to-run spread (0.005 to 0.013 ms).  Other store kinds, L2, other k, uneven or duplicated sets, labels of uneven
 * length, the host form and the count call: not measured. */
int phnsw_labels_count_set_device(const phnsw_labels *lb, const uint32_t *want_first_dev, const uint32_t *want_values_dev,
                                  uint64_t nq, uint64_t nwant, uint32_t *out_count_dev, void *stream);
int phnsw_search_exact_labelset(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                uint64_t nq, const uint64_t *exclude, const uint32_t *want_first, const uint32_t *want_values,
                                uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len);
/* device form: as phnsw_search_exact_labeled_device; it ENQUEUES AND RETURNS, never synchronises `stream` and reads
 * nothing back, which is why it takes nwant: nwant sizes the scratch.  It does not trust the offsets: a query whose
 * range is not inside [0, nwant] or runs backwards gets status_dev[q] = 8, an empty row and length 0; so does a query
 * whose range overlaps the range of a LOWER query (honest offsets never overlap; the lower query keeps the shared
 * pairs).  Every other query is unaffected, and nothing outside want_values[0 .. nwant) is ever read.  status 4 = a
 * Stored query id at or past n, as elsewhere (8 wins where both hold).  Scratch sets, stream rules, the growing call
 * that waits for its set's previous call and phnsw_labels_destroy as for phnsw_search_exact_labeled_device; a set holds
 * grouping arrays of 44 bytes per PAIR, the sort's temporaries and nwant x slices x k keys (at one slice too: a pair
 * never writes an output row itself). */
int phnsw_search_exact_labelset_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                       const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                       const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                       uint64_t k, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                       uint32_t *status_dev, void *stream);
/* ---- one filtered call that picks scan or graph walk per query, and rescans what the walk left short.  For batches
 * whose bitmaps differ widely (tenants, ACLs, tombstones plus a predicate): the caller neither counts nor splits.
 * Candidates: exactly those of phnsw_search_exact_filtered -- v < n, its bit set in q's bitmap, v != exclude[q], v a
 * vector of the index's bottom layer.  Bitmap layout, stride rule, the default filter (filter NULL) and "no filter at
 * all = every vector of the index" as there.  Exactly one of queries / qids; nq == 0 is a no-op.  Every store kind both
 * underlying calls accept (f32, f16, i8, i8q, PQ); what either refuses (a shared-codebook PQ store, a PQ table that
 * does not fit beside the scan's LDS) is refused here with the same code.  1 <= k <= sp->number_of_candidates (<= 1024),
 * else PHNSW_E_INVALID.  All layers are searched (there is no upto).
 * Rows: k entries, ascending by (distance, id), padded with PHNSW_EMPTY / f32::MAX.  out_len[q] == min(k, candidates of
 * q) for EVERY query, and an id that is not a candidate is never returned: not the disallowed entry vector, and not the
 * excluded one either (both can come back from phnsw_search_batch_filtered).
 * Route: let c_q be what phnsw_filter_count_device reports for q's bitmap, N the bottom layer's node count and
 * ef = sp->number_of_candidates.  Query q is SCANNED iff c_q <= scan_below or c_q * ef < k * N (the walk's post-filter
 * is then expected to keep fewer than k of its queue); otherwise it WALKS THE GRAPH.  A Stored query id at or past n
 * (device form) is scanned whatever its count, which reports it.
 * scan_below 0 = the library default, the measured crossover of profiles/filter_exact/README.md: 13 000 with a shared
 * bitmap, 10 000 with per-query bitmaps -- measured on 1M x 768 f32 rows, k = 10, batches of 10 000 queries; other store
 * kinds, dimensions and batch sizes are unmeasured, pass your own.  UINT64_MAX = always scan.  No value never scans:
 * the second rule and the fallback below always hold.
 * A scanned row is, bit for bit, the row phnsw_search_exact_filtered returns.  A graph row is the PHNSW_FILTER_STRICT
 * row of phnsw_search_batch_filtered with the same sp, with exclude[q] removed if present, cut to k.  If that leaves
 * fewer than min(k, c_q - e_q) entries (e_q = 1 iff exclude[q] is itself a candidate by bitmap and index membership),
 * or the walk overflowed its spill list, the query is scanned: its row is then the scan's and its route reads
 * PHNSW_ROUTE_GRAPH_THEN_SCAN.
 * +inf: the walk never returns a candidate at +inf (an L2 sum past f32::MAX) while the scan returns it behind every
 * finite one, in id order (see phnsw_search_exact_filtered; f32::MAX, the padding, compares below such entries).  A
 * graph-routed query whose FINITE candidates number fewer than min(k, c_q - e_q) is therefore always left short by the
 * walk and scanned: its route reads PHNSW_ROUTE_GRAPH_THEN_SCAN and its row ends in entries at +inf.  A query at +inf
 * from the entry vector is outside the walk's contract, here as in phnsw_search_batch.
 * A graph-routed row is an APPROXIMATE result: its recall is that of the walk at this sp (the README's cells show
 * 0.45-0.67 at the minimal number_of_candidates).  The guarantee of this call is completeness -- the full
 * min(k, candidates) entries, candidates only -- not recall; scanned rows are exact.
 * Cost: the call adds a count, a routing pass and up to two stream synchronisations to the method it picks; it has not
 * been timed against the two calls (profiles/filter_auto/README.md).  A caller whose whole batch sits on one side of the
 * crossover loses nothing by calling that method directly.
 * out_route: nullable; per query one of the three values.  Thread safe like the other search calls. */
enum { PHNSW_ROUTE_GRAPH = 0, PHNSW_ROUTE_SCAN = 1, PHNSW_ROUTE_GRAPH_THEN_SCAN = 2 };
int phnsw_search_filtered_auto(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                               const phnsw_search_params *sp, const uint64_t *exclude,
                               const uint32_t *filter, uint32_t filter_stride_words,
                               uint64_t k, uint64_t scan_below,
                               uint64_t *out_ids, float *out_d, uint64_t *out_len, uint32_t *out_route);
/* device form: device pointers, u32 ids [nq][k] padded with 0xFFFFFFFF / f32::MAX; queries [nq][ldq] as for
 * phnsw_search_batch_device.  status_dev[q] is 0, or what the underlying call reports for that query (4 = a Stored
 * query id at or past n, or a vector missing from a lower layer; the row is then empty).  Unlike the other _device
 * calls this one SYNCHRONISES `stream`, at most twice, to read list lengths back: after counting and routing, and --
 * only when some query walks the graph -- after the graph rows are finished and the short ones are known.  The scan is
 * enqueued after that; the call returns without waiting for it. */
int phnsw_search_filtered_auto_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq,
                                      const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                      const uint32_t *exclude_dev, const uint32_t *filter_dev,
                                      uint32_t filter_stride_words, uint64_t k, uint64_t scan_below,
                                      uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                      uint32_t *out_route_dev, uint32_t *status_dev, void *stream);
/* ---- the graph walk restricted by ROW LABEL: phnsw_search_batch_filtered without a bitmap per query.  The handle keeps
 * the label column it was made from on the device, label_of[n] -- the label of every listed vector, PHNSW_LABEL_NONE for
 * one that is not listed; this costs a handle 4 * n more bytes than its posting lists -- and the search kernels test
 * label_of[v] == want[q] where the bitmap form tests bit v: one 4-byte load per kept queue entry instead of one word.
 * A batch of nq queries sends nq labels, not nq bitmaps of ceil(n / 32) words.
 * Arguments as phnsw_search_batch_filtered[_device] with (lb, want) in place of (filter, filter_stride_words): sp,
 * upto_layers, exclude, flags (PHNSW_FILTER_STRICT or 0), k (host form; 0 = the whole queue), out_stats.
 * ROW EQUALITY: the rows, lengths, stats and statuses are those of phnsw_search_batch_filtered[_device] called with the
 * per-query bitmaps {v : v listed under want[q]}, bit for bit.  It is the same post-filter: a query gets about
 * number_of_candidates * (list length) / N results, not k of them -- phnsw_search_labeled_auto (below) completes rows.
 * The entry vector may appear although its label differs (and although it is not listed), unless flags has
 * PHNSW_FILTER_STRICT.  want[q] == PHNSW_LABEL_NONE, or a label nobody carries, gives the row an all-zero bitmap gives.
 * The default filter of phnsw_index_set_filter_device is NOT consulted, as in phnsw_search_exact_labeled.
 * Checks: index and sp as phnsw_search_batch; then a null or stale `lb`, refused exactly as phnsw_search_exact_labeled
 * refuses it (PHNSW_E_INVALID, "the labels are stale"); unknown flag bits; exactly one of queries / qids, the outputs and
 * `want` (PHNSW_E_INVALID); nq == 0 is a no-op.  Every store kind phnsw_search_batch_filtered walks.
 * The host form stages its arrays once per call (queries, ids, want: 4 bytes per query where the bitmap form uploads
 * ceil(n / 32) words per query) and runs on a stream of its own; a query whose frontier spill overflowed is re-run
 * with more room, as in phnsw_search_batch.  Timing against the bitmap call: profiles/labeled_walk/README.md. */
int phnsw_search_batch_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                               uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                               const uint32_t *want, uint32_t flags, uint64_t k, uint64_t *out_ids, float *out_d,
                               uint64_t *out_len, uint64_t *out_stats);
/* device form: device pointers, rows of number_of_candidates entries as phnsw_search_batch_filtered_device writes them,
 * status_dev as there.  ENQUEUED on `stream`; never synchronises.  want_dev [nq] is read by the kernels: keep it alive
 * and unchanged until the work on `stream` is done. */
int phnsw_search_batch_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                      const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                      uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                      uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                      uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* ---- one call by label that routes: phnsw_search_filtered_auto with (lb, want) for the bitmaps.  Same arguments
 * otherwise, same three routes, same promise: every row holds exactly min(k, c_q - e_q) entries and only candidates,
 * where c_q is the length of the list of want[q] (what phnsw_labels_count_device writes) and e_q is 1 iff exclude[q] is
 * listed under want[q].  The counts come from the posting lists -- no bitmap is made or counted --, the rule is the
 * one above (filter_route.h), the walk is the PHNSW_FILTER_STRICT walk of phnsw_search_batch_labeled, and a scanned
 * row is phnsw_search_exact_labeled's row bit for bit, routed and short queries in ONE scan launch.  Hence every row
 * equals the row of phnsw_search_filtered_auto with the per-query bitmaps {v : v listed under want[q]} and the same
 * scan_below.
 * scan_below 0 = the library default for labels (filter_route.h, PH_AUTO_SCAN_BELOW_LABELED): 20 000, the measured
 * crossover of phnsw_search_exact_labeled and the label walk (profiles/labeled_walk/README.md: at 20 000 rows per label the
 * scan took 17.8 ms against the walk's 22.0, at 25 000 rows 22.0 against 21.5) -- measured on 1M x 768 f32 rows, ef 256 /
 * probe_depth 8, k = 10, batches of 10 000 queries; other store kinds, dimensions, parameters and batch sizes are
 * unmeasured, pass your own.  UINT64_MAX = always scan.
 * Checks: those of phnsw_search_filtered_auto (sp, then 1 <= k <= number_of_candidates, then the store), then the handle
 * as phnsw_search_exact_labeled checks it, then the pointers.  The default filter is not consulted.  The device form
 * synchronises `stream` at most twice, like phnsw_search_filtered_auto_device. */
int phnsw_search_labeled_auto(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                              uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude, const uint32_t *want,
                              uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                              uint32_t *out_route);
int phnsw_search_labeled_auto_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                     const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                     const uint32_t *exclude_dev, const uint32_t *want_dev, uint64_t k, uint64_t scan_below,
                                     uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                     uint32_t *out_route_dev, uint32_t *status_dev, void *stream);
/* ---- the graph walk restricted by a SET of row labels, `label IN (a, b, c)`: phnsw_search_batch_labeled with a set per
 * query.  The sets of a batch in CSR form as phnsw_search_exact_labelset takes them: want_first[nq + 1], want_values[nwant],
 * S_q = { want_values[i] : want_first[q] <= i < want_first[q+1] }.  A batch sends 4 * (nq + 1) + 4 * nwant bytes, not nq
 * bitmaps of ceil(n / 32) words.
 * Candidates: vector v passes iff label_of[v] != PHNSW_LABEL_NONE (v is listed) and label_of[v] is a label of S_q.  A
 * label that occurs twice in S_q, PHNSW_LABEL_NONE in S_q and labels nobody carries need no handling under this test.
 * Arguments as phnsw_search_batch_labeled[_device] with (want_first, want_values) in place of want; the device form takes
 * nwant as well, as phnsw_search_exact_labelset_device does.
 * ROW EQUALITY: the rows, lengths, stats and statuses are those of phnsw_search_batch_filtered[_device] called with the
 * per-query bitmaps {v : v listed and labels[v] in S_q}, bit for bit: the same post-filter walk, the same entry-vector
 * quirk unless flags has PHNSW_FILTER_STRICT, k cuts the same way (host form; 0 = the whole queue).  An empty set, a set
 * of PHNSW_LABEL_NONE only, or a set of labels nobody carries gives the row an all-zero bitmap gives.  The default filter
 * of phnsw_index_set_filter_device is NOT consulted.  The result depends on none of: the order of labels inside a set,
 * duplicates, the order of the batch, how the sets overlap, any knob.  Hence a batch of one-label sets equals
 * phnsw_search_batch_labeled's rows, stats included.
 * Checks, in this order: index and sp as phnsw_search_batch; a null or stale `lb`, refused as phnsw_search_batch_labeled
 * refuses it; unknown flag bits; (host form) k past number_of_candidates; nq == 0, a no-op; exactly one of queries /
 * qids, the outputs, want_first, and want_values (NULL only when nwant == 0); nq and nwant <= 2^31 - 2 (PHNSW_E_INVALID).
 * The host form reads nwant from want_first[nq] and then refuses, before any device work and naming the query, a Stored
 * query id at or past n, want_first[0] != 0 and a want_first that runs backwards.  Every message names the call.
 * Cost of the membership test: per 64 tested ids one 4-byte load per lane and, per label of the set, one scalar load, one
 * compare and one OR -- LINEAR in the length of the set, no LDS, no sort and no preparation kernel; first and last are
 * read once per query.  The test runs over a layer's queue once per layer, not per evaluated row.  Sets of hundreds of
 * labels are legal and slow in proportion.
 * The host form stages its arrays once per call (queries, ids, the 4 * (nq + 1) + 4 * nwant bytes of the sets) and runs
 * on a stream of its own; a query whose frontier spill overflowed is re-run with more room, as in
 * phnsw_search_batch_labeled.
 * Guidance (measured on 1M x 768 f32 rows, cosine, ef 256 / probe_depth 8, strict, 10 000-query batches of distinct
 * labels drawn at random out of 1000 labels of 1000 rows, the variants alternating in one run;
 * profiles/labelset_walk/README.md): against phnsw_search_batch_filtered_device with the union as per-query bitmaps
 * already on the device the device form took 0.992, 0.993 and 0.998 of its time at sets of 1, 4 and 32 labels (26.4,
 * 25.5 and 20.9 ms; run-to-run spread of either up to 0.25 ms), and 0.54, 0.54 and 0.49 of it with the upload of what
 * describes the filter counted on both sides (1.25 GB of bitmaps against 80 KB to 1.3 MB of sets).  At one label per set
 * it took 26.36 ms where phnsw_search_batch_labeled_device took 26.39 ms: the difference is below the spread of the same
 * run (0.16 to 0.25 ms).  Against phnsw_search_exact_labelset_device at sets of 4: slower up to a union of 20 000 rows
 * (22.0 ms against 17.6), faster from 40 000 (20.3 against 34.2).  Not measured: the host form, sets longer than 32, other
 * store kinds, L2, the latency kernels (small batches), and whether the registers or the LDS decide the resident waves of
 * the 15 instances that report one wave per SIMD fewer than their label twins. */
int phnsw_search_batch_labelset(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                const uint32_t *want_first, const uint32_t *want_values, uint32_t flags, uint64_t k,
                                uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats);
/* device form: device pointers, rows of number_of_candidates entries as phnsw_search_batch_filtered_device writes them.
 * ENQUEUED on `stream`; never synchronises.  want_first_dev [nq + 1] and want_values_dev [nwant] are read by the kernels:
 * keep them alive and unchanged until the work on `stream` is done.  The offsets are not trusted: a query whose range is
 * not inside [0, nwant] or runs backwards does not walk -- status_dev[q] = 8 (phnsw_search_exact_labelset_device's
 * value), an empty row, length 0, stats 0 --, nothing outside want_values[0 .. nwant) is ever read, and every other
 * query is unaffected.  Status 8 is raised for these range faults ONLY: ranges that OVERLAP are harmless to a walk (every
 * query reads its own range) and are NOT detected here, unlike in phnsw_search_exact_labelset_device and
 * phnsw_search_labelset_auto_device.  Other statuses as phnsw_search_batch_labeled_device. */
int phnsw_search_batch_labelset_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                       const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                       uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                       const uint32_t *want_values_dev, uint64_t nwant, uint32_t flags,
                                       uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                       uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* ---- one call by a set of labels that routes: phnsw_search_labeled_auto with (want_first, want_values[, nwant]) in
 * place of want.  Same three routes, same out_route values, same promise: every row holds exactly min(k, c_q - e_q)
 * entries and only candidates, where c_q is what phnsw_labels_count_set_device writes (distinct labels, listed vectors)
 * and e_q is 1 iff exclude[q] is listed under a label of S_q.  The rule is the one above (filter_route.h), the walk is
 * the PHNSW_FILTER_STRICT walk of phnsw_search_batch_labelset over the graph list, and a scanned row is
 * phnsw_search_exact_labelset's row bit for bit, routed and short queries in ONE scan launch (the scan's subset form:
 * which query owns a pair is still decided over the whole batch).  Hence every row equals the row of
 * phnsw_search_filtered_auto with the per-query bitmaps {v : v listed and labels[v] in S_q} and the same scan_below.
 * scan_below 0 = the library default for sets (filter_route.h, PH_AUTO_SCAN_BELOW_LABELSET): 20 000 candidates of the
 * UNION, from the crossover of phnsw_search_exact_labelset and the walk by set at sets of 4 labels (at a union of 20 000
 * rows the scan took 17.6 ms against the walk's 22.0, at 40 000 rows 34.2 against 20.3; the lines cross near 25 000) --
 * measured on 1M x 768 f32 rows, ef 256 / probe_depth 8, k = 10, batches of 10 000 queries; other set sizes, store kinds,
 * dimensions and parameters are unmeasured, pass your own.  UINT64_MAX = always scan.
 * Checks: those of phnsw_search_labeled_auto (sp, then 1 <= k <= number_of_candidates, then the store, then the handle),
 * then the pointer and size checks of phnsw_search_batch_labelset; the host form refuses the same offsets and Stored
 * ids, naming the query.  The default filter is not consulted.
 * The device form reports status 8 exactly where phnsw_search_exact_labelset_device reports it for the same arrays,
 * whichever route the count would have chosen -- a range fault, or an overlap with a LOWER query: such a query is routed
 * to the scan, its row is empty and its route reads PHNSW_ROUTE_SCAN.  A Stored query id at or past n: status 4, scanned,
 * an empty row (8 wins where both hold).  It synchronises `stream` at most twice, like its siblings.  The routed call
 * itself has not been timed against the two calls it chooses between. */
int phnsw_search_labelset_auto(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                               uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude,
                               const uint32_t *want_first, const uint32_t *want_values, uint64_t k, uint64_t scan_below,
                               uint64_t *out_ids, float *out_d, uint64_t *out_len, uint32_t *out_route);
int phnsw_search_labelset_auto_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                      const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                      const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                      const uint32_t *want_values_dev, uint64_t nwant, uint64_t k, uint64_t scan_below,
                                      uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                      uint32_t *out_route_dev, uint32_t *status_dev, void *stream);
/* ---- search by a NUMERIC RANGE of a row attribute, `lo <= attribute <= hi`: a timestamp, a price, a version, a size.
 * Every vector carries one u32 key, compared as an unsigned integer; PHNSW_ATTR_NONE means the row carries no value.
 * A phnsw_attr handle sorts the listed rows ONCE by (key, id) on the device; every range is then one contiguous span of
 * that order, found with two binary searches, and its candidate count is upper - lower: no bitmap per query, no bucket
 * labels, no merge of lists.  The handle keeps skeys[listed] (ascending), ids[listed] (ascending within equal keys) and,
 * for the graph walk, attr_of[n] (the key of a listed row, PHNSW_ATTR_NONE elsewhere): TWELVE BYTES PER VECTOR.
 * Listed: v is listed iff v < n, keys[v] != PHNSW_ATTR_NONE and v is a vector of the index's bottom layer (the test of
 * phnsw_labels_create).  n must equal the store's vector count, else PHNSW_E_INVALID.
 * Ranges are INCLUSIVE on both ends.  hi == 0xFFFFFFFF is legal and means "no upper bound": rows without a value are in
 * no span.  lo > hi is the empty range, not an error: the row is empty, the length 0, the status 0.
 * VALUE TYPES: the ABI is u32 keys.  Other 32-bit types go through an order-preserving map, applied to the column and to
 * both bounds alike (phnsw.hpp: phnsw::attr_key; Python: attr_keys):
 *   u32   the value itself
 *   i32   x ^ 0x80000000
 *   f32   -0.0 is first made +0.0; then bits | 0x80000000 for a value that is not negative, ~bits for a negative one
 * NaN has no place in an order and must not be mapped; a u32 value of 0xFFFFFFFF -- and so an i32 value of INT32_MAX,
 * which maps onto it -- cannot be told from "no value" in a column (as a bound it is "no upper end", which is what it
 * means).  64-bit columns are out of scope.
 * The handle is a SNAPSHOT like phnsw_labels, with its rule and its wording: a null handle, one made for another index
 * or before the store's n or the bottom layer's node count changed is PHNSW_E_INVALID ("... are stale").  Creation
 * synchronises (the null stream, or `stream` of the device form, whose keys_dev is read before the call returns).
 * phnsw_attr_info: the n it was made for, the listed vectors, the smallest and the largest key (0xFFFFFFFF and 0 when
 * nothing is listed); any output may be NULL.  phnsw_attr_count_device writes, per query, the length of the span of
 * [lo_dev[q], hi_dev[q]], 0 when lo > hi: phnsw_filter_count_device's figure for the equivalent bitmap; it is enqueued
 * on `stream` and never synchronises.  phnsw_attr_destroy waits for the calls in flight that use the handle; NULL is a
 * no-op.  The handle does not own the index and must not outlive it in use. */
typedef struct phnsw_attr phnsw_attr;
#define PHNSW_ATTR_NONE 0xFFFFFFFFu /* keys[v]: v carries no value */
int phnsw_attr_create(const phnsw_index *ix, const uint32_t *keys, uint64_t n, phnsw_attr **out); /* host keys [n] */
int phnsw_attr_create_device(const phnsw_index *ix, const uint32_t *keys_dev, uint64_t n, void *stream, phnsw_attr **out);
int phnsw_attr_info(const phnsw_attr *at, uint64_t *n, uint64_t *listed, uint32_t *key_min, uint32_t *key_max);
int phnsw_attr_count_device(const phnsw_attr *at, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq,
                            uint32_t *out_count_dev, void *stream);
void phnsw_attr_destroy(phnsw_attr *at); /* waits for the calls in flight that use it */
/* exact top-k over a range: phnsw_search_exact_labeled with (at, lo, hi) in place of (lb, want); lo and hi are u32 [nq].
 * Candidates of q: the listed vectors with lo[q] <= key <= hi[q], except exclude[q].
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for that query with the bitmap {v : v listed, lo[q] <= keys[v] <= hi[q]}: ascending
 * (distance, id) with phnsw_distance_batch's bits, +inf and tie order as there, rows of k entries padded with
 * PHNSW_EMPTY / f32::MAX, 1 <= k <= 1024.  The ids of a span are NOT ascending; the keys of the running top-k are
 * (distance, id), distinct, so the k smallest are one set in one order however the span is ordered or cut.  The result
 * does not depend on the batch's order or on the knob below.
 * Checks: those of phnsw_search_exact_labeled in its order, with `at` for `lb` and lo / hi for want.
 * How: per query the span; the batch sorted by span start, so that waves resident together read neighbouring rows; one
 * wave64 per (query, slice of its span), the scan loop of phnsw_search_exact_labeled's per-query path, over every store
 * kind that call scans.  There is NO tile path: overlapping spans are not the lists of one label.  Knob (environment,
 * read per call, changes no result): PHNSW_RANGE_SLICES forces the number of slices a span is cut into.
 * Guidance: NOT MEASURED (scripts/bench_ranged.py, profiles/ranged/README.md).  The per-query path of the label scan
 * measured 2.2 x to 3.6 x slower than its tile path; expect this call near phnsw_search_exact_labeled under
 * PHNSW_LABEL_TILE=1 for spans as long as the lists. */
int phnsw_search_exact_ranged(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                              uint64_t nq, const uint64_t *exclude, const uint32_t *lo, const uint32_t *hi, uint64_t k,
                              uint64_t *out_ids, float *out_d, uint64_t *out_len);
/* device form, as phnsw_search_exact_labeled_device: ENQUEUES AND RETURNS, never synchronises; status_dev[q] = 4 for a
 * Stored query id at or past n (an empty row, the others unaffected).  Scratch sets -- 28 bytes per query, the sort's
 * temporaries, nq x slices x k keys -- live with the handle under that call's policy until phnsw_attr_destroy. */
int phnsw_search_exact_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                     const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                     const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev,
                                     float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream);
/* ---- exact RADIUS search by ROW LABEL and by NUMERIC RANGE: phnsw_search_exact_radius with a filter PER QUERY -- every
 * row of this query's tenant, or newer than this query's cut-off, closer than this query's radius.  Arguments: those of
 * phnsw_search_exact_radius[_device] with the handle and want [nq] (or lo / hi [nq]) in the bitmap's place, as in
 * phnsw_search_exact_labeled / phnsw_search_exact_ranged.
 * Candidates of q: the listed vectors of label want[q], or the listed vectors with lo[q] <= key <= hi[q], except
 * exclude[q].  want[q] == PHNSW_LABEL_NONE, a label nobody carries and lo > hi give an empty segment with status 0, not
 * an error.
 * Inside the radius: d(q, v) < radius[q] as an f32 comparison, strict.  A NaN, zero or negative radius matches nothing,
 * and the rows of such a query are not read at all; a candidate at +inf or NaN is never inside a radius.
 * Result and size negotiation: exactly those of phnsw_search_exact_radius -- out_first [nq + 1] and *out_total always
 * complete and exact, segments ascending by (distance, id), phnsw_distance_batch's bits (a -0.0 comes back as +0.0),
 * out_ids / out_d written only if the total is at most cap, cap == 0 with NULL arrays the count-only form,
 * cap <= 2^31 - 1 and nq <= 2^31 - 2.
 * EQUALITY: for every query the segment equals, in ids, distance bits and count, the segment phnsw_search_exact_radius
 * returns for that query with the bitmap {v : labels[v] == want[q]} (or {v : v listed, lo[q] <= keys[v] <= hi[q]}), on
 * the stores that call accepts; its leading min(1024, count) entries equal the row of phnsw_search_exact_labeled /
 * phnsw_search_exact_ranged at k = 1024, cut at d < radius[q].  The result depends neither on the batch's order nor on
 * the slice count: the pool's order depends on scheduling, the sorted order does not (the keys of one query are distinct).
 * Stores: every kind the list scans accept -- f32, f16, i8, i8q and per-sub-space PQ, rows of at most 1536 floats --, one
 * kind more than phnsw_search_exact_radius: the distances are dist.batch's, not a table's.
 * Checks, in this order: a null index or one without layers; cap above 2^31 - 1 (PHNSW_E_INVALID); a null or stale
 * handle, refused as by phnsw_search_exact_labeled / _ranged (PHNSW_E_INVALID); the store as those calls check it at
 * k = 1 (a shared-codebook PQ store and longer rows: PHNSW_E_UNSUPPORTED); nq == 0: the host form writes the empty result,
 * the device form enqueues nothing; the pointers and nq (PHNSW_E_INVALID); the host form's Stored ids at or past n.
 * How: a lookup kernel writes the list (start, length) of every query; the batch is sorted by list start; ONE scan
 * kernel, one wave64 per (query, slice of its list) in slice-major order, takes 64 ids at a time into dist.batch, tests
 * ok && id != exclude && d < radius, stages the hits as (key, query) records in a per-wave LDS buffer and flushes it with
 * one 64-bit atomic add on the pool's cursor per flush -- every row is read once; records at or past the pool's capacity
 * are dropped but counted.  The tail (exclusive sum, the total's read-back, two stable radix passes, the unpack) is
 * phnsw_search_exact_radius's own code.  The pool holds min(cap, nq x the longest list of the handle) records and lives,
 * with the rest of a call's scratch, in the handle's scratch sets until phnsw_labels_destroy / phnsw_attr_destroy.
 * Knobs (environment, read per call, change no result): PHNSW_LABEL_SLICES / PHNSW_RANGE_SLICES force the slice count;
 * PHNSW_DENSE_TIMES=1 prints the times of scan and scan + sort on stderr.
 * NOT BUILT: a form for phnsw_label_attr, sets of labels, a tile path (queries of one label sharing a row read), a walk,
 * routing.
 * Guidance (measured on 1M x 768 f32 rows, cosine, 10 000-query batches, one radius for the batch, the calls alternating
 * in one run; scripts/list_radius_profile.py, profiles/radius_list/README.md): the call costs what the per-query top-k
 * scan over the same lists costs at k = 10 (phnsw_search_exact_labeled under PHNSW_LABEL_TILE=1,
 * phnsw_search_exact_ranged), which reads the same rows, plus the sort and unpack.  By label, lists of 100 000 / 10 000 /
 * 1000 rows: 320.1 / 31.4 / 4.07 ms with about 10 rows inside the radius per query, 319.5 / 31.6 / 4.36 ms with about 100
 * and 318.4 / 32.5 / 5.09 ms with about 1000, against 318.4 / 31.4 / 3.90, 319.9 / 31.8 / 3.95 and 317.2 / 31.6 / 3.93 ms of
 * the top-k scan; the scan kernel alone takes the top-k scan's time, the sort and unpack 0.2 / 0.4 / 1.2 ms at totals of
 * 10^5 / 10^6 / 10^7 records.  By range, windows of the same lengths: 390.8 / 42.0 / 4.41, 390.5 / 42.3 / 4.67 and 391.2 /
 * 43.1 / 5.44 ms (the top-k scan by range: 389.3 / 41.8 / 4.28 at 10 rows inside).  Counting only saves the sort and the
 * unpack: 3.90 against 5.09 ms at lists of 1000 rows all inside the radius.  Against phnsw_search_exact_radius called once
 * per distinct label with its bitmap (warmed, the same rounds) this call LOSES at few long lists -- 8 labels of 100 000
 * rows: 318 to 320 against 29 to 34 ms, eight matrix-core tables against 10 000 waves reading 100 000 rows each --, is level
 * at 64 labels of 10 000 rows (31.4 to 32.5 against 24.9 to 31.0 ms) and wins at 1000 labels of 1000 rows (4.1 to 5.1
 * against 180 to 217 ms, about 40 to 1): with a handful of tenants keep calling the table call per tenant.  f16, i8, i8q
 * and PQ stores, L2 and ragged dimensions, per-query radii, batches
 * small enough for slices, exclude, the host forms and a cap below the total: not measured. */
int phnsw_search_exact_radius_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                      uint64_t nq, const uint64_t *exclude, const uint32_t *want, const float *radius,
                                      uint64_t cap, uint64_t *out_first, uint64_t *out_ids, float *out_d, uint64_t *out_total);
/* device forms: device pointers as for phnsw_search_exact_radius_device; status_dev[q] = 4 for a Stored query id at or
 * past n (an empty segment, the others unaffected).  The call synchronises `stream` ONCE, to read the total, when
 * cap > 0; with cap == 0 it never synchronises.  No candidate count is read back. */
int phnsw_search_exact_radius_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev, uint32_t ldq,
                                             const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                             const uint32_t *want_dev, const float *radius_dev, uint64_t cap,
                                             uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                             uint32_t *status_dev, uint64_t *out_total_dev, void *stream);
int phnsw_search_exact_radius_ranged(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                                     uint64_t nq, const uint64_t *exclude, const uint32_t *lo, const uint32_t *hi,
                                     const float *radius, uint64_t cap, uint64_t *out_first, uint64_t *out_ids, float *out_d,
                                     uint64_t *out_total);
int phnsw_search_exact_radius_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                            const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                            const uint32_t *lo_dev, const uint32_t *hi_dev, const float *radius_dev, uint64_t cap,
                                            uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                            uint32_t *status_dev, uint64_t *out_total_dev, void *stream);
/* the graph walk by range: phnsw_search_batch_labeled with (at, lo, hi) in place of (lb, want) -- the search kernels'
 * range mode over attr_of, one 4-byte load and two compares per tested id.
 * ROW EQUALITY: rows, lengths, stats and statuses are those of phnsw_search_batch_filtered[_device] called with the
 * per-query bitmaps {v : v listed, lo[q] <= keys[v] <= hi[q]}, bit for bit, the entry-vector quirk and
 * PHNSW_FILTER_STRICT included.  The index's default filter is not consulted.  Every store kind
 * phnsw_search_batch_filtered walks is accepted.  Not measured against it (profiles/ranged/README.md). */
int phnsw_search_batch_ranged(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                              uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                              const uint32_t *lo, const uint32_t *hi, uint32_t flags, uint64_t k, uint64_t *out_ids,
                              float *out_d, uint64_t *out_len, uint64_t *out_stats);
/* device form: ENQUEUED on `stream`, never synchronises.  lo_dev and hi_dev [nq] are read by the kernels: keep them alive
 * and unchanged until the work on `stream` is done. */
int phnsw_search_batch_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                     const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                     uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *lo_dev,
                                     const uint32_t *hi_dev, uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev,
                                     uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* one call by range that routes: phnsw_search_labeled_auto with (at, lo, hi).  Same three routes, rule and promise: every
 * row holds exactly min(k, c_q - e_q) entries and only candidates; c_q is the span's length (no bitmap is made or
 * counted), e_q is 1 iff exclude[q] < n and its key is inside the range.  The walk is the STRICT range walk; scanned rows
 * and graph rows left short go through ONE launch of the exact scan above.  Hence every row equals the row of
 * phnsw_search_filtered_auto with the per-query bitmaps and the same scan_below.  The device form synchronises `stream`
 * at most twice.  scan_below 0 = the library default for ranges (filter_route.h, PH_AUTO_SCAN_BELOW_RANGED): 20 000,
 * UNMEASURED -- it is the one-label figure, and the range scan has no tile path, so the true crossover is expected
 * below it; pass your own.  UINT64_MAX = always scan. */
int phnsw_search_ranged_auto(const phnsw_index *ix, const phnsw_attr *at, const float *queries, const uint64_t *qids,
                             uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude, const uint32_t *lo,
                             const uint32_t *hi, uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d,
                             uint64_t *out_len, uint32_t *out_route);
int phnsw_search_ranged_auto_device(const phnsw_index *ix, const phnsw_attr *at, const float *queries_dev, uint32_t ldq,
                                    const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                    const uint32_t *exclude_dev, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k,
                                    uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                    uint32_t *out_route_dev, uint32_t *status_dev, void *stream);
/* ---- search by a ROW LABEL AND A NUMERIC RANGE, `label == want AND lo <= attribute <= hi`: this tenant's rows of the
 * last week.  Every vector carries one u32 label (PHNSW_LABEL_NONE: none) and one u32 key (PHNSW_ATTR_NONE: no value);
 * the value types and the key map are those of phnsw_attr above.
 * A phnsw_label_attr handle sorts the listed rows ONCE on the device by the 64-bit composite (label << 32) | key, then
 * by id; every (label, range) pair is then one contiguous SPAN of that order,
 *   [lower_bound(want << 32 | lo), upper_bound(want << 32 | hi)),
 * found with two binary searches: no bitmap per query, no merge of a posting list with a span, no bucket labels.  The
 * handle keeps spairs[listed] (u64, ascending), ids[listed] (ascending within equal composites) and, for the graph walk,
 * pair_of[n] (the composite of a listed row, UINT64_MAX elsewhere): TWENTY BYTES PER VECTOR (8 + 4 + 8).
 * Listed: v is listed iff v < n, labels[v] != PHNSW_LABEL_NONE, keys[v] != PHNSW_ATTR_NONE and v is a vector of the
 * index's bottom layer.  A row with a label but no value, or a value but no label, is not listed.  n must equal the
 * store's vector count, else PHNSW_E_INVALID.
 * The span is EMPTY -- the row empty, the length 0, the status 0, no error -- when want == PHNSW_LABEL_NONE, when
 * lo > hi, or when nobody carries the label.  Ranges are inclusive on both ends; hi == 0xFFFFFFFF means "no upper end
 * within this label": no listed row has that key, so the span ends at the first row of the next label.
 * The handle is a SNAPSHOT like phnsw_attr, with its rule and its wording; creation synchronises.
 * phnsw_label_attr_info: the n it was made for, the listed vectors, the number of distinct labels that list a row and
 * the most rows listed under one label; any output may be NULL.  phnsw_label_attr_count_device writes, per query, the
 * length of its span: phnsw_filter_count_device's figure for the equivalent bitmap; enqueued on `stream`, never
 * synchronises.  phnsw_label_attr_destroy waits for the calls in flight that use the handle; NULL is a no-op.
 * A SET of labels with one range is built on the same handle (phnsw_search_exact_labelset_ranged and its siblings,
 * below).  NOT BUILT: a different range per label of a set, 64-bit keys, a tile path for the scan, a collecting twin of
 * the walk. */
typedef struct phnsw_label_attr phnsw_label_attr;
int phnsw_label_attr_create(const phnsw_index *ix, const uint32_t *labels, const uint32_t *keys, uint64_t n,
                            phnsw_label_attr **out); /* host labels [n], keys [n] */
int phnsw_label_attr_create_device(const phnsw_index *ix, const uint32_t *labels_dev, const uint32_t *keys_dev, uint64_t n,
                                   void *stream, phnsw_label_attr **out);
int phnsw_label_attr_info(const phnsw_label_attr *h, uint64_t *n, uint64_t *listed, uint64_t *nlabels, uint64_t *longest);
int phnsw_label_attr_count_device(const phnsw_label_attr *h, const uint32_t *want_dev, const uint32_t *lo_dev,
                                  const uint32_t *hi_dev, uint64_t nq, uint32_t *out_count_dev, void *stream);
void phnsw_label_attr_destroy(phnsw_label_attr *h); /* waits for the calls in flight that use it */
/* exact top-k over a label and a range: phnsw_search_exact_ranged with (h, want, lo, hi) in place of (at, lo, hi); want,
 * lo and hi are u32 [nq].  Candidates of q: the listed vectors with labels[v] == want[q] and lo[q] <= keys[v] <= hi[q],
 * except exclude[q].
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for that query with the bitmap
 * {v : v listed, labels[v] == want[q], lo[q] <= keys[v] <= hi[q]}; +inf, tie order by id, padding and 1 <= k <= 1024 as
 * there.  The result does not depend on the batch's order or on the knob below.
 * Checks: those of phnsw_search_exact_ranged in its order, with `h` for `at` and want / lo / hi for lo / hi.
 * How: the kernel sequence of phnsw_search_exact_ranged over every store kind that call scans; no tile path.  Knob
 * (environment, read per call, changes no result): PHNSW_LABEL_RANGE_SLICES forces the number of slices a span is cut
 * into.
 * Guidance: NOT MEASURED (scripts/bench_label_ranged.py, profiles/label_ranged/README.md).  The scan runs the loop of
 * phnsw_search_exact_ranged over spans found in u64 instead of u32 words; expect that call's times. */
int phnsw_search_exact_label_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                    const uint64_t *qids, uint64_t nq, const uint64_t *exclude, const uint32_t *want,
                                    const uint32_t *lo, const uint32_t *hi, uint64_t k, uint64_t *out_ids, float *out_d,
                                    uint64_t *out_len);
/* device form: ENQUEUES AND RETURNS, never synchronises; status_dev[q] = 4 for a Stored query id at or past n (an empty
 * row, the others unaffected).  Scratch sets live with the handle until phnsw_label_attr_destroy. */
int phnsw_search_exact_label_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                           uint32_t ldq, const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                           const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                           uint64_t k, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                           uint32_t *status_dev, void *stream);
/* the graph walk by label and range: phnsw_search_batch_ranged with (h, want, lo, hi) -- the search kernels' label-range
 * mode over pair_of, one 8-byte load per tested id, compared word by word with the query's three words.
 * ROW EQUALITY: rows, lengths, stats and statuses are those of phnsw_search_batch_filtered[_device] called with the
 * per-query bitmaps above, bit for bit, the entry-vector quirk and PHNSW_FILTER_STRICT included.  The index's default
 * filter is not consulted.  Every store kind phnsw_search_batch_filtered walks is accepted.  Not measured against it
 * (profiles/label_ranged/README.md). */
int phnsw_search_batch_label_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                    const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers,
                                    const uint64_t *exclude, const uint32_t *want, const uint32_t *lo, const uint32_t *hi,
                                    uint32_t flags, uint64_t k, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                    uint64_t *out_stats);
/* device form: ENQUEUED on `stream`, never synchronises.  want_dev, lo_dev and hi_dev [nq] are read by the kernels: keep
 * them alive and unchanged until the work on `stream` is done. */
int phnsw_search_batch_label_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                           uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                           const phnsw_search_params *sp, uint32_t upto_layers, const uint32_t *exclude_dev,
                                           const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                           uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                           uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* one call by label and range that routes: phnsw_search_ranged_auto with (h, want, lo, hi).  Same three routes, rule and
 * promise: every row holds exactly min(k, c_q - e_q) entries and only candidates; c_q is the span's length, e_q is 1 iff
 * exclude[q] < n and it is listed under want[q] with its key inside the range.  The walk is the STRICT walk above;
 * scanned rows and graph rows left short go through ONE launch of the exact scan above.  Hence every row equals the row
 * of phnsw_search_filtered_auto with the per-query bitmaps and the same scan_below.  The device form synchronises
 * `stream` at most twice.  scan_below 0 = the library default (filter_route.h, PH_AUTO_SCAN_BELOW_LABEL_RANGED): the
 * ranged figure, 20 000, UNMEASURED; pass your own.  UINT64_MAX = always scan. */
int phnsw_search_label_ranged_auto(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                   const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude,
                                   const uint32_t *want, const uint32_t *lo, const uint32_t *hi, uint64_t k,
                                   uint64_t scan_below, uint64_t *out_ids, float *out_d, uint64_t *out_len,
                                   uint32_t *out_route);
int phnsw_search_label_ranged_auto_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                          uint32_t ldq, const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                          const uint32_t *exclude_dev, const uint32_t *want_dev, const uint32_t *lo_dev,
                                          const uint32_t *hi_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                          float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                          uint32_t *status_dev, void *stream);
/* ---- search by a SET OF ROW LABELS AND A NUMERIC RANGE, `label IN (a, b, c) AND lo <= attribute <= hi`: the rows of my
 * ACL groups from the last week.  Seven calls over the phnsw_label_attr handle above; no new handle, and the handle's
 * layout does not change.  The sets of a batch are in CSR form exactly as phnsw_search_exact_labelset takes them:
 * want_first[nq + 1] (u32, want_first[0] == 0, non-decreasing) and want_values[nwant] (u32 labels), nwant ==
 * want_first[nq]; S_q = { want_values[i] : want_first[q] <= i < want_first[q+1] }; the device forms also take nwant.
 * lo[nq] and hi[nq] are u32 keys, inclusive, ONE range per query, shared by every label of that query's set.
 * Candidates of q, the same in all seven: v is a candidate iff v is listed by the handle, labels[v] is in S_q,
 * lo[q] <= keys[v] <= hi[q] and v != exclude[q].  A label that occurs twice in S_q counts once; PHNSW_LABEL_NONE in a set
 * and a label nobody carries contribute nothing; an empty set, or lo > hi, is no error: the row is empty, the length 0,
 * the status 0; hi == 0xFFFFFFFF means "no upper end within each label".
 * phnsw_label_attr_count_set_device: out_count[q] = the sum of the span lengths of the DISTINCT labels of S_q --
 * phnsw_filter_count_device's figure for the equivalent bitmap -- and 0 for a query the exact device form below would
 * refuse (status 8); enqueued on `stream`, never synchronises.  Its cost is quadratic in the length of a set (a wave per
 * query tests distinctness in place).  Checks, in this order: null `h`; nq == 0 returns 0; null want_first, lo, hi or
 * output, null want_values with nwant > 0; nq and nwant below 2^31 - 1 (PHNSW_E_INVALID). */
int phnsw_label_attr_count_set_device(const phnsw_label_attr *h, const uint32_t *want_first_dev,
                                      const uint32_t *want_values_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                      uint64_t nq, uint64_t nwant, uint32_t *out_count_dev, void *stream);
/* exact top-k over a set of labels and a range.
 * EQUALITY: the row of every query equals, in ids, distance bits, length and status, the row
 * phnsw_search_exact_filtered returns for that query with the bitmap
 * {v : v listed, labels[v] in S_q, lo[q] <= keys[v] <= hi[q]}: ascending (distance, id), equal distances by id ALSO where
 * the tied rows come from different spans; +inf, padding and 1 <= k <= 1024 as there.  Hence a batch of one-label sets
 * equals phnsw_search_exact_label_ranged's rows.  The result depends on none of: the order of labels inside a set, the
 * order of queries in the batch, the knob below.
 * Checks, in this order: those of phnsw_search_exact_label_ranged (index, k, null or stale `h`, store kind and its
 * limits); nq == 0 returns 0; queries or qids, exactly one; outputs, want_first, lo, hi, nq < 2^31 - 1; then those of
 * phnsw_search_exact_labelset: want_values unless want_first[nq] is 0 and want_first[nq] < 2^31 - 1; a Stored id at or
 * past n, naming the query; want_first[0] != 0 or offsets that run backwards, naming the query (all PHNSW_E_INVALID).
 * How: every query claims the pairs (query, wanted label) of its range, as phnsw_search_exact_labelset does; per pair
 * the span of (its label, its query's range), two binary searches; the pairs sorted by span start (stable); a position
 * that has the query and the non-empty span of the position before it is a duplicate and scans nothing
 * (labelset_range_plan.h has the argument why that finds every repeated label); one wave64 per (pair, slice of its
 * span) through the scan loop of phnsw_search_exact_label_ranged, every store kind it scans, every pair writing its
 * per-slice lists of k keys to scratch; then a wave per query merges the lists of its pairs through the same running
 * top-k.  The slice count comes from the longest label's run; nothing is read back; no tile path.  Knob (environment,
 * read per call, changes no result): PHNSW_LABELSET_RANGE_SLICES forces the number of slices a span is cut into.
 * Guidance (the run described at phnsw_search_labelset_ranged_auto below): against phnsw_search_exact_filtered with the
 * equivalent per-query bitmaps already on the device this call took 6.61 ms against 6.62 at sets of 1, 25.4 against 25.6
 * at sets of 4 and 149 against 200 at sets of 32 (a tenth of each label: 1 538, 6 152 and 49 216 candidates); with the
 * upload counted -- 160 KB to 1.4 MB against 1.25 GB -- 0.23, 0.54 and 0.67 of it.  Its time grows with the candidates
 * (no tile path): 20.8 ms at 5 000 candidates of a set of 4, 77.7 at 20 000, 195 at 60 000. */
int phnsw_search_exact_labelset_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                       const uint64_t *qids, uint64_t nq, const uint64_t *exclude, const uint32_t *want_first,
                                       const uint32_t *want_values, const uint32_t *lo, const uint32_t *hi, uint64_t k,
                                       uint64_t *out_ids, float *out_d, uint64_t *out_len);
/* device form: ENQUEUES AND RETURNS, never synchronises; scratch sets live with the handle.  The offsets are NOT trusted:
 * status_dev[q] = 8 for a query whose range [want_first[q], want_first[q+1]) is not inside [0, nwant], runs backwards,
 * or overlaps the range of a LOWER query; such a query gets an empty row, every other query is unaffected, and nothing
 * outside want_values[0 .. nwant) is ever read.  status_dev[q] = 4 for a Stored query id at or past n (an empty row);
 * status 8 wins where both hold. */
int phnsw_search_exact_labelset_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                              uint32_t ldq, const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                              const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                              const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev,
                                              float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream);
/* the graph walk by a set of labels and a range: phnsw_search_batch_labelset with (h, want_first, want_values, lo, hi)
 * -- the search kernels' set-range mode over pair_of: one 8-byte load per tested id, the loop of the set mode over the
 * wave-uniform set values against the label word, two compares of the key word (ph_pairset_holds, filter_route.h).
 * ROW EQUALITY: rows, lengths, stats and statuses are those of phnsw_search_batch_filtered[_device] called with the
 * per-query bitmaps above, bit for bit, the entry-vector quirk and PHNSW_FILTER_STRICT included.  k cuts as in
 * phnsw_search_batch_labelset (host form; 0 = the whole queue).  The index's default filter is not consulted.  Every
 * store kind phnsw_search_batch_filtered walks is accepted.  The host form checks the offsets and the Stored ids as
 * the exact host form does.  Measured (the run described at phnsw_search_labelset_ranged_auto below): the device form
 * took 0.997 to 1.008 of the bitmap walk's kernel time at sets of 1, 4 and 32 labels (24.2, 23.1 and 18.4 ms) and 0.46
 * to 0.52 of it with the upload counted. */
int phnsw_search_batch_labelset_ranged(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                       const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers,
                                       const uint64_t *exclude, const uint32_t *want_first, const uint32_t *want_values,
                                       const uint32_t *lo, const uint32_t *hi, uint32_t flags, uint64_t k, uint64_t *out_ids,
                                       float *out_d, uint64_t *out_len, uint64_t *out_stats);
/* device form: ENQUEUED on `stream`, never synchronises.  want_first_dev, want_values_dev, lo_dev and hi_dev are read by
 * the kernels: keep them alive and unchanged until the work on `stream` is done.  A query whose range is not inside
 * [0, nwant] or runs backwards does not walk -- status_dev[q] = 8, an empty row, length 0, stats 0 --, nothing outside
 * want_values[0 .. nwant) is ever read, and every other query is unaffected.  Status 8 is raised for these range faults
 * ONLY: ranges that OVERLAP are harmless to a walk and are NOT detected here, as in phnsw_search_batch_labelset_device. */
int phnsw_search_batch_labelset_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                              uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                              const phnsw_search_params *sp, uint32_t upto_layers, const uint32_t *exclude_dev,
                                              const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                              const uint32_t *lo_dev, const uint32_t *hi_dev, uint32_t flags,
                                              uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                              uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* one call by a set of labels and a range that routes: phnsw_search_labelset_auto with the handle and (lo, hi).  Same
 * three routes, out_route values, rule and promise: every row holds exactly min(k, c_q - e_q) entries and only
 * candidates; c_q is what phnsw_label_attr_count_set_device writes, e_q is 1 iff exclude[q] passes the walk's predicate.
 * The walk is the STRICT walk above over the graph list; scanned rows and graph rows left short go through ONE launch
 * of the exact scan's subset form, whose claim still runs over the whole batch.  Hence every row equals the row of
 * phnsw_search_filtered_auto with the per-query bitmaps and the same scan_below.  Status 8 is reported where
 * phnsw_search_exact_labelset_ranged_device reports it, whatever the route; such a query reads PHNSW_ROUTE_SCAN.  The
 * device form synchronises `stream` at most twice.  scan_below 0 = the library default (filter_route.h,
 * PH_AUTO_SCAN_BELOW_LABELSET_RANGED): 5 000 candidates of the union, the last measured count at which the scan still
 * won.  UINT64_MAX = always scan.
 * Guidance (measured on 1M x 768 f32 rows, cosine, ef 256 / probe_depth 8, 10 000-query batches, k = 10, 64 labels of
 * about 15 600 rows, the variants alternating in one run, run-to-run spread under 1 % unless said;
 * profiles/labelset_ranged/README.md): sets of 4 labels, scan against walk by candidates of the union -- 20.8 ms against
 * 23.6 at 5 000, 40.2 against 22.3 at 10 000, 77.7 against 20.5 at 20 000, 195 against 17.8 at 60 000: the lines cross
 * between 5 000 and 10 000.  With a range that keeps a tenth of each label the routed call took 6.72 ms at sets of 1
 * (all scanned), 25.5 ms at sets of 4 (all scanned; the walk alone took 23.1 and returned 6.1 rows per query) and
 * 18.4 ms at sets of 32 (all walked), 0.96 to 0.99 of phnsw_search_filtered_auto over bitmaps on the device and 0.23 to
 * 0.53 of it with the upload of the filter's description counted.  Other store kinds, other k, uneven or duplicated
 * sets and the host forms: not measured. */
int phnsw_search_labelset_ranged_auto(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries,
                                      const uint64_t *qids, uint64_t nq, const phnsw_search_params *sp, const uint64_t *exclude,
                                      const uint32_t *want_first, const uint32_t *want_values, const uint32_t *lo,
                                      const uint32_t *hi, uint64_t k, uint64_t scan_below, uint64_t *out_ids, float *out_d,
                                      uint64_t *out_len, uint32_t *out_route);
int phnsw_search_labelset_ranged_auto_device(const phnsw_index *ix, const phnsw_label_attr *h, const float *queries_dev,
                                             uint32_t ldq, const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                             const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                             const uint32_t *want_values_dev, uint64_t nwant, const uint32_t *lo_dev,
                                             const uint32_t *hi_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                             float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                             uint32_t *status_dev, void *stream);
/* ---- the COLLECTING search: the graph walk that remembers the best ALLOWED rows it evaluates.  The filtered walks above
 * are post-filters: they keep the best number_of_candidates rows, allowed or not, and filter that queue when the layer
 * ends, so a filter of density p leaves about p * number_of_candidates results although the walk evaluated several
 * times as many rows.  A collecting search of query q with result size k (1 <= k <= 64) IS the plain search
 * phnsw_search_batch with the same sp, upto_layers and exclude -- split descents included --, and only the walk of the
 * LAST LAYER IT RUNS is extended:
 *  - beside the layer's queue there is a second queue `kept`, a PriorityQueue of capacity k ordered by (distance, id)
 *    like every queue here;
 *  - a node with vector v QUALIFIES iff v passes the filter (bit v of the query's bitmap; or
 *    label_of[v] == want[q] && want[q] != PHNSW_LABEL_NONE), v != exclude[q], and its distance is <= f32::MAX (the walk
 *    never returns +inf, and neither does this);
 *  - `kept` is seeded with the qualifying entries of the queue the layer starts with (the running candidates).  There is
 *    no entry-vector quirk: a row that does not qualify is never returned;
 *  - at every hop the qualifying members of that hop's evaluated batch are merged into `kept` -- the batch the layer's
 *    queue is merged with, including the members that are too far away for that queue;
 *  - without flags NOTHING ELSE changes: the traversal, the visited sets, the per-query evaluation and hop counters are
 *    the plain search's, bit for bit, so out_stats equals phnsw_search_batch's for any filter;
 *  - with PHNSW_COLLECT_EXTEND a hop additionally "did something" when it changed `kept`.  This is the only change to the
 *    walk: probe_depth then counts the hops that improve NEITHER queue, so hops that find better allowed rows no longer
 *    use up the budget.  probe_depth idle hops IN ALL (the budget is never refilled) still end the walk, however many
 *    allowed rows lie further out and however few `kept` holds: the flag does not make the walk exhaust its
 *    frontier, and a row shorter than k does not mean that fewer than k allowed rows are reachable;
 *  - upper layers run exactly as in the plain search, unfiltered apart from exclude: a selective filter cannot starve
 *    the descent.
 * Result row: the entries of `kept`, ascending by (distance, id); out_len[q] = its length; rows of k entries padded with
 * PHNSW_EMPTY / f32::MAX; the distance has the bits the walk computed, which are phnsw_distance_batch's for that store
 * (a -0.0 comes back as +0.0, as from the exact calls); out_stats as phnsw_search_batch (evaluations, hops).
 * Consequences: with every row allowed, no exclude and k <= number_of_candidates the row is the first k entries of
 * phnsw_search_batch's row, with or without the flag.  With any filter the row holds the first k of the ALLOWED entries
 * of phnsw_search_batch's row (same sp, upto_layers, exclude) -- the strict post-filter of the plain search -- or better
 * ones: every allowed entry of that row is in `kept` or behind its tail.  The same holds against the
 * PHNSW_FILTER_STRICT row of phnsw_search_batch_filtered ONLY where the two descents coincide (one layer walked:
 * upto_layers 1 or a one-layer index): that call filters the queue of every layer, descends from other candidates below
 * the top layer and may return rows this walk never evaluates, as this walk may return rows that one never does.  It is
 * an APPROXIMATE result: it holds only rows the walk evaluated.
 * Arguments as phnsw_search_batch_filtered[_device] / phnsw_search_batch_labeled[_device]; flags: PHNSW_COLLECT_EXTEND
 * or 0; k follows the flags in the device forms too, whose rows hold k entries.  `filter` NULL = the index's default
 * filter (phnsw_index_set_filter_device), else every row is allowed.  The label forms do not consult the default filter.
 * Checks, in this order: index and sp as phnsw_search_batch; unknown flag bits; k == 0 or k > 64; a stride below the
 * words of one bitmap; (label forms) a null or stale `lb`; all PHNSW_E_INVALID.  Then nq == 0, a no-op.  Then exactly
 * one of queries / qids and the other pointers (PHNSW_E_INVALID).  Every store kind the filtered walk accepts.
 * The host forms stage like phnsw_search_batch_filtered (per-query bitmaps travel with their chunk, u64 ids out, a query
 * whose frontier spill overflowed is re-run with 8x the room, else PHNSW_E_OVERFLOW).  The device forms are ENQUEUED on
 * `stream` and never synchronise it, with two exceptions that allocate and therefore wait for the device: the first call
 * without any filter on an index makes that index's all-ones bitmap, once; and a call that descends in several launches
 * (phnsw_search_batch_device's split descent of large batches) parks its running candidates in rows of
 * number_of_candidates entries kept with the index's workspace, which grow -- free and allocate -- when a call needs more
 * than any before it (calls of one size, or smaller ones, never wait): status_dev per query as phnsw_search_batch_device, u32 ids padded with 0xFFFFFFFF, rows of k.
 * want_dev and the handle's column are read by the kernels: keep both alive until the work on `stream` is done.
 * Cost and yield: profiles/collect/README.md.  The routed calls (phnsw_search_filtered_auto, phnsw_search_labeled_auto)
 * do not use this walk. */
enum { PHNSW_COLLECT_EXTEND = 1 };
int phnsw_search_collect(const phnsw_index *ix, const float *queries, const uint64_t *qids, uint64_t nq,
                         const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                         const uint32_t *filter, uint32_t filter_stride_words, uint32_t flags, uint64_t k,
                         uint64_t *out_ids, float *out_d, uint64_t *out_len, uint64_t *out_stats);
int phnsw_search_collect_device(const phnsw_index *ix, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers,
                                const uint32_t *exclude_dev, const uint32_t *filter_dev, uint32_t filter_stride_words,
                                uint32_t flags, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
int phnsw_search_collect_labeled(const phnsw_index *ix, const phnsw_labels *lb, const float *queries, const uint64_t *qids,
                                 uint64_t nq, const phnsw_search_params *sp, uint32_t upto_layers, const uint64_t *exclude,
                                 const uint32_t *want, uint32_t flags, uint64_t k, uint64_t *out_ids, float *out_d,
                                 uint64_t *out_len, uint64_t *out_stats);
int phnsw_search_collect_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const float *queries_dev,
                                        uint32_t ldq, const uint32_t *qids_dev, uint64_t nq, const phnsw_search_params *sp,
                                        uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                        uint32_t flags, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                        uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);
/* Throughput callers keep TWO batches in flight: phnsw_search_batch_device calls issued alternately on two streams
 * overlap (an index holds two search workspaces) -- if the two streams sit on different hardware queues.  HIP maps a
 * process's streams onto a few of them (GPU_MAX_HW_QUEUES, 4 by default) and two streams that share one run in issue
 * order.  This makes a non-blocking stream that was SEEN to run beside `other_stream` (a hipStream_t; NULL = the
 * default stream): a kernel spinning for a millisecond on `other_stream`, an empty one on the candidate, up to six
 * candidates.  *out_stream is a hipStream_t the caller destroys with hipStreamDestroy. */
int phnsw_stream_create_beside(int device, void *other_stream, void **out_stream);
/* timing of the last phnsw_search_batch_device launch on this index measured with HIP
 * events on its stream: kernel milliseconds */
/* running totals of distance evaluations and hops over every search launched on the index since
 * its creation (build rounds included; the reference's SearchStats per query, search.rs:93-99,
 * summed): the build's algorithmic bytes are n_dist * row bytes + n_hops * neighbour-row bytes */
int phnsw_index_counters(const phnsw_index *ix, uint64_t *n_dist, uint64_t *n_hops);
int phnsw_last_search_kernel_ms(const phnsw_index *ix, float *ms);
/* the same descent dispatch by dispatch (measurement only): entry 0 = the dense-top-layer tile pass
 * (csrc/tiny.hip; layers 0..0), then one entry per launch of the search kernel: layers
 * [layer_lo, layer_hi), milliseconds, distance evaluations and hops.  *count = entries available;
 * at most cap are written; any output array may be NULL.  A query list longer than the dense table holds
 * (4 GiB by default: ~145 000 queries at 1M x 768) runs in chunks; times and counters then describe the LAST chunk. */
int phnsw_last_search_dispatches(const phnsw_index *ix, uint32_t cap, uint32_t *count, float *ms,
                                 uint64_t *n_dist, uint64_t *n_hops, uint32_t *layer_lo,
                                 uint32_t *layer_hi);
/* per entry of phnsw_last_search_dispatches: how many of the launch's distance evaluations were served by the
 * dense tables (measurement only); n_dist - n_table are gathered rows, the bytes an HBM roofline counts */
int phnsw_last_search_table_evals(const phnsw_index *ix, uint32_t cap, uint32_t *count, uint64_t *n_table);
/* how a search with this number_of_candidates treats the leading layers (measurement only): *layers =
 * how many of them are walked through the dense distance table (csrc/tiny.hip), *nodes = nodes of
 * the largest of them (the table's width), *matrix_cores = 1 when the table is built by the MFMA
 * kernel (dot-product metric, rows of 256 / 768 / 1536 floats), 0 for the vector-unit kernel. */
int phnsw_dense_top_layers(const phnsw_index *ix, uint64_t number_of_candidates, uint32_t *layers,
                           uint64_t *nodes, uint32_t *matrix_cores);

/* ---- phase API: the per-round pieces of phnsw_generate_layer / phnsw_link_layer /
 * phnsw_stochastic_recall_at over a NODE RANGE, device buffers, u32 ids (0xFFFFFFFF empty).
 * A multi-GPU driver (parallel_hnsw_amd/sharded.py) gives every rank a replica of store and
 * graph, lets rank r run the searches of its node range, all-gathers the per-node results
 * over RCCL and lets every rank apply them -- replicas stay bit-identical.  The
 * single-GPU entry points above are these phases over the whole range. ---- */
int phnsw_index_create(phnsw_store *s, const phnsw_build_params *bp, phnsw_index **out); /* no layers yet */
/* the id shuffle of phnsw_build (lib.rs:832-833) and its layer sizes, top first
 * (calculate_partitions lib.rs:1883-1899) */
int phnsw_build_plan(const uint64_t *vids, uint64_t n, const phnsw_build_params *bp,
                     uint64_t *shuffled, uint64_t *layer_sizes, uint32_t max_layers,
                     uint32_t *layer_count);
/* generate_layer: begin (sort, id maps; *needs_phases = 0 when the layer is already complete:
 * first layer of a stack) -> init_search(range) -> seed(range) -> finish */
int phnsw_layer_begin(phnsw_index *ix, const uint64_t *vids, uint64_t n, uint64_t neighborhood_size,
                      const phnsw_build_params *bp, int *needs_phases);
/* the same for a sharded driver: the cells of the new layer's locality schedule (a GEMM of its vectors against the
 * store's anchors -- a scheduling hint, never part of a result, but the one costly step of begin) are left out when
 * *needs_cells comes back 1: every rank computes a node range (cells_device), the ranges are all-gathered, every
 * rank installs the whole array (set_cells_device) */
int phnsw_layer_begin_sharded(phnsw_index *ix, const uint64_t *vids, uint64_t n, uint64_t neighborhood_size,
                              const phnsw_build_params *bp, int *needs_phases, int *needs_cells);
int phnsw_layer_cells_device(phnsw_index *ix, uint64_t first, uint64_t count, uint32_t *out_pos);
int phnsw_layer_set_cells_device(phnsw_index *ix, const uint32_t *pos);
/* out_* : [count][K] NodeIds of the new layer / distances, [count] lengths;
 * K = initial_partition_search.number_of_candidates  (search.rs:32-71) */
int phnsw_layer_init_search_device(phnsw_index *ix, const phnsw_build_params *bp, uint64_t first,
                                   uint64_t count, uint32_t *out_ids, float *out_d, uint32_t *out_len);
/* init_* : the FULL [n][K] lists; out_rows : [count][W]  (lib.rs:711-787) */
int phnsw_layer_seed_device(phnsw_index *ix, const phnsw_build_params *bp, const uint32_t *init_ids,
                            const float *init_d, const uint32_t *init_len, uint64_t first,
                            uint64_t count, uint32_t *out_rows, float *out_rows_d);
/* rows : the FULL [n][W] seeded rows; bidirectional pass + push  (lib.rs:789-822) */
int phnsw_layer_finish_device(phnsw_index *ix, const uint32_t *rows, const float *rows_d);
/* link round: searches of nodes [first, first+count) -> best link_count results as
 * VectorIds [count][link_count]  (lib.rs:1107-1117) */
int phnsw_link_search_device(phnsw_index *ix, uint32_t layer_from_top, const phnsw_search_params *sp,
                             uint64_t link_count, uint64_t first, uint64_t count, uint32_t *out_ids,
                             float *out_d, uint32_t *out_len);
/* ... and the row updates from the FULL [n][link_count] results  (lib.rs:1118-1147) */
int phnsw_link_apply_device(phnsw_index *ix, uint32_t layer_from_top, uint64_t link_count,
                            const uint32_t *ids, const float *d, const uint32_t *len,
                            uint64_t *out_added);
/* promote_at_layer in two phases: the self-hit flags (match_within_epsilon) of nodes
 * [first, first+count) -> all-gather -> the promotion from the FULL [node_count] flags */
int phnsw_discover_hits_device(phnsw_index *ix, uint32_t layer_from_top, const phnsw_search_params *sp,
                               uint64_t first, uint64_t count, uint32_t *out_hit);
int phnsw_promote_at_layer_hits_device(phnsw_index *ix, uint32_t layer_from_top,
                                       const phnsw_build_params *bp, const uint32_t *hit,
                                       int *out_promoted);
/* self-hits among sample[first, first+count) of stochastic_recall_at; *out_selection = sample size */
int phnsw_recall_hits(phnsw_index *ix, uint32_t layer_from_top, const phnsw_optimization_params *op,
                      uint64_t first, uint64_t count, uint64_t *out_hits, uint64_t *out_selection);

/* ---- sharded build: Hnsw::generate / improve_index with every per-node phase split over the GPUs
 * of one node (BASELINE config 4).  One process per GPU; every rank holds a replica of
 * store and graph; within a round nodes are independent (the searches of lib.rs:1107-1117 read a
 * snapshot), so rank r runs the phase for the node range [r*chunk, (r+1)*chunk), the per-node results
 * (u32 ids + f32 distances) are all-gathered, and every rank applies ALL of them (K5): replicas stay
 * bit-identical and the graph equals phnsw_build's.  Control flow = lib.rs:825-893, 1515-1686.
 *
 * phnsw_comm is the collective seam: a host supplies its own transport (MPI, a torch.distributed
 * group, ...) as two callbacks, or takes the built-in RCCL one (phnsw_comm_rccl_create: ncclAllGather
 * over xGMI on a stream of the library's, no torch).
 *   all_gather: every rank contributes `bytes` at `send`; `recv` receives world*bytes in rank order.
 *     host_buffers == 0: device pointers; the call ENQUEUES on `stream` (a hipStream_t) and may return
 *     before the transfer is done -- the library overlaps it with the next piece's searches and
 *     synchronises the stream itself.  host_buffers == 1: host pointers (the library stages through
 *     pinned memory), stream is NULL, the call returns when recv is complete.
 *   all_reduce_sum: element-wise sum of `count` host u64 over the ranks, in place.
 *   emulate != 0 with all_gather == NULL: ONE process plays all `world` ranks in turn on its GPU (every
 *     range is computed here, in rank order, with the same split, packing and reassembly): what the
 *     one-GPU tests and the scaling model of bench.py use; phnsw_sharded_stats separates rank `rank`'s
 *     time from the others'. */
typedef int (*phnsw_all_gather_fn)(void *ctx, const void *send, void *recv, uint64_t bytes, void *stream);
typedef int (*phnsw_all_reduce_sum_fn)(void *ctx, uint64_t *values, uint32_t count);
typedef struct phnsw_comm {
  uint32_t rank, world;
  uint32_t host_buffers;
  uint32_t emulate;
  void *ctx;
  phnsw_all_gather_fn all_gather;
  phnsw_all_reduce_sum_fn all_reduce_sum;
} phnsw_comm;

/* where a sharded build spent its time (seconds on the calling rank) and what it moved */
typedef struct phnsw_sharded_stats {
  double seconds_total;
  double seconds_sharded;    /* this rank's share of the per-node phases (searches, seeding) */
  double seconds_replicated; /* phases every rank repeats (row merges K5, layer bookkeeping, promotion) */
  double seconds_comm;       /* host time inside collectives, their waits and the reassembly copies */
  double seconds_others;     /* emulate: the other ranks' shares, computed here in turn */
  uint64_t all_gather_bytes; /* received, summed over calls */
  uint64_t all_gather_calls;
  uint64_t all_reduce_calls;
  uint64_t phases;           /* sharded phases run */
  uint64_t phases_whole;     /* work lists too short to split (every rank ran them whole, no collective) */
  /* this rank's seconds by phase: the sharded ones 0 layer_init_search, 1 layer_seed, 2 link_search, 3 recall_hits,
   * 4 discover_hits; the replicated ones 5 plan, 6 layer_begin, 7 layer_finish, 8 link_apply, 9 promote_from_hits */
  double seconds_by_phase[10];
} phnsw_sharded_stats;

/* Hnsw::generate (lib.rs:825-893) over the ranks of `comm`; comm == NULL or world == 1 is phnsw_build.
 * Every rank must call it with the same store contents, vids and bp.  stats nullable. */
int phnsw_build_sharded(phnsw_store *s, const uint64_t *vids, uint64_t n, const phnsw_build_params *bp,
                        const phnsw_comm *comm, phnsw_progress_cb cb, void *user, phnsw_index **out,
                        phnsw_sharded_stats *stats);
/* Hnsw::improve_index (lib.rs:1664-1686) on an existing, replicated index */
int phnsw_improve_index_sharded(phnsw_index *ix, const phnsw_build_params *bp, float last_recall,
                                const phnsw_comm *comm, float *out_recall, phnsw_sharded_stats *stats);
/* work lists shorter than shard_min run whole on every rank (default 4096); a rank's share is cut into
 * `subchunks` pieces of at least sub_min items whose all-gathers overlap the next piece (defaults 4, 65536).
 * 0 keeps a value.  Process-wide; for tests and tuning. */
int phnsw_sharded_tuning(uint64_t shard_min, uint32_t subchunks, uint64_t sub_min);

/* the built-in transport: RCCL (librccl is loaded on first use; PHNSW_RCCL_LIB overrides its path).
 * Rank 0 makes the 128-byte id, the host hands it to the other ranks by any means, every rank creates
 * its communicator on its own device.  The returned phnsw_comm has host_buffers == 0. */
int phnsw_comm_rccl_unique_id(uint8_t *out_id128);
int phnsw_comm_rccl_create(const uint8_t *id128, uint32_t rank, uint32_t world, int device, phnsw_comm **out);
void phnsw_comm_destroy(phnsw_comm *c);
/* checks a communicator end to end before a build is trusted to it: every rank contributes a known pattern of
 * `bytes` bytes, verifies all world blocks of the all-gather, then the all-reduce.  Collective: every rank calls it. */
int phnsw_comm_selftest(const phnsw_comm *comm, uint64_t bytes);
/* what a collective costs: `iters` all-gathers of `bytes` per rank back to back -- *host_us = host time per call to
 * enqueue it, *total_us = wall time per call until the last has landed.  Collective; device-buffer transports. */
int phnsw_comm_benchmark(const phnsw_comm *comm, uint64_t bytes, uint32_t iters, double *host_us, double *total_us);

/* The phase engine behind the sharded driver.  phnsw_build_sharded runs the driver over libphnsw's own
 * GPU phases (the phase API above); this entry runs the SAME driver over an engine given as callbacks,
 * which is how the CPU tests drive it under gloo with the oracle's phases (tests/test_sharded_gloo.py).
 * ids / lengths / hit flags are id_bytes wide (4 or 8), distances f32; host_buffers: alloc returns host
 * memory (then comm->host_buffers must be 1 too). */
typedef struct phnsw_shard_engine {
  void *ctx;
  uint32_t id_bytes;
  uint32_t host_buffers;
  void *(*alloc)(void *ctx, uint64_t bytes);
  void (*release)(void *ctx, void *p);
  int (*copy2d)(void *ctx, void *dst, uint64_t dpitch, const void *src, uint64_t spitch, uint64_t width,
                uint64_t height);
  int (*plan)(void *ctx, const uint64_t *vids, uint64_t n, uint64_t *shuffled, uint64_t *layer_sizes,
              uint32_t max_layers, uint32_t *layer_count);
  int (*layer_begin)(void *ctx, const uint64_t *vids, uint64_t n, uint64_t W, int *needs_phases, uint32_t *K);
  int (*layer_init_search)(void *ctx, uint64_t first, uint64_t count, void *ids, float *d, void *len);
  int (*layer_seed)(void *ctx, const void *init_ids, const float *init_d, const void *init_len, uint64_t first,
                    uint64_t count, void *rows, float *rows_d);
  int (*layer_finish)(void *ctx, const void *rows, const float *rows_d);
  uint32_t (*layer_count)(void *ctx);
  uint64_t (*layer_nodes)(void *ctx, uint32_t layer_from_top);
  int (*link_search)(void *ctx, uint32_t layer_from_top, const phnsw_search_params *sp, uint64_t link_count,
                     uint64_t first, uint64_t count, void *ids, float *d, void *len);
  int (*link_apply)(void *ctx, uint32_t layer_from_top, uint64_t link_count, const void *ids, const float *d,
                    const void *len, uint64_t *added);
  int (*recall_hits)(void *ctx, uint32_t layer_from_top, const phnsw_optimization_params *op, uint64_t first,
                     uint64_t count, uint64_t *hits, uint64_t *selection);
  int (*discover_hits)(void *ctx, uint32_t layer_from_top, const phnsw_search_params *sp, uint64_t first,
                       uint64_t count, void *hit);
  int (*promote_from_hits)(void *ctx, uint32_t layer_from_top, const void *hit, int *promoted);
  /* optional (NULL: layer_begin does it all): when layer_begin sets *needs_phases to 3 instead of 1 the driver
   * shards layer_cells (u32 per node) like any phase and hands the whole array to layer_set_cells */
  int (*layer_cells)(void *ctx, uint64_t first, uint64_t count, void *pos);
  int (*layer_set_cells)(void *ctx, const void *pos);
} phnsw_shard_engine;
int phnsw_build_sharded_engine(const phnsw_shard_engine *e, const uint64_t *vids, uint64_t n,
                               const phnsw_build_params *bp, const phnsw_comm *comm, phnsw_sharded_stats *stats);

/* ---- product quantisation (reference src/pq.rs; BASELINE config 5) ----
 * A PQ store holds u8 code rows [n][m] over per-sub-space codebooks [m][ksub][dim/m]
 * (random_centroids pq.rs:261-285 per sub-space; Quantizer::quantize pq.rs:61-71 as the exact
 * nearest centroid).  It is a phnsw_store: phnsw_build / phnsw_search_batch / phnsw_link_layer
 * ... run on it with quantised distances (a per-query lookup table in LDS; a Stored query is its
 * reconstruction, so code-vs-code distances are symmetric).  m % 4 == 0, dim % m == 0,
 * ksub <= 256, m*ksub*4 bytes must fit the LDS. */
int phnsw_store_create_pq(phnsw_store *full, uint32_t m, uint32_t ksub, uint64_t seed, phnsw_store **out);
/* the same with k-means codebooks (the reference's own k-means is dead code,
 * pq.rs:215-259): kmeans_iters Lloyd iterations from the random_centroids start, trained on the first
 * min(n, sample) vectors of the seeded shuffle (sample 0 = all); kmeans_iters 0 == phnsw_store_create_pq */
int phnsw_store_create_pq_kmeans(phnsw_store *full, uint32_t m, uint32_t ksub, uint64_t seed,
                                 uint32_t kmeans_iters, uint64_t sample, phnsw_store **out);
/* The reference's own quantizer shape (src/pq.rs:19-27, 61-81, 261-364): ONE codebook of n_centroids <= 65535
 * centroid sub-vectors of dsub floats shared by every sub-space (random_centroids: the sub-vectors of selected
 * vectors, sorted, de-duplicated, shuffled, truncated), u16 codes, quantize = the best result of an HNSW search
 * (quantized_search) over the centroids (built with centroid_bp, centroid_metric).  A stored vector IS its
 * reconstruction and distances apply the store's metric to reconstructions (the quantised comparators of
 * pq.rs:585-599), so the store is searched with phnsw_search_batch* / phnsw_pq_search_batch like any other.
 * Build the Hnsw over the quantised vectors on phnsw_pq_shared_reconstruct_store (same distance bits) and
 * adopt it with phnsw_index_from_layers.  dim % dsub == 0, dsub % 4 == 0. */
int phnsw_store_create_pq_shared(phnsw_store *full, uint32_t dsub, uint32_t n_centroids, uint64_t seed,
                                 const phnsw_build_params *centroid_bp, const phnsw_search_params *quantized_search,
                                 int centroid_metric, phnsw_store **out);
/* Both constructors with Quantizer::quantize split over the ranks of `comm` (PQ encode shards by
 * vector range, pq.rs:326-333): codebooks / the centroid index are computed identically on every rank, rank r
 * encodes vectors [r*chunk, (r+1)*chunk), the code rows are all-gathered (n x m code bytes, resp. n x m x 2).
 * comm == NULL is the single-GPU call.  Every rank passes the same store contents and parameters. */
int phnsw_store_create_pq_sharded(phnsw_store *full, uint32_t m, uint32_t ksub, uint64_t seed, uint32_t kmeans_iters,
                                  uint64_t sample, const phnsw_comm *comm, phnsw_store **out);
int phnsw_store_create_pq_shared_sharded(phnsw_store *full, uint32_t dsub, uint32_t n_centroids, uint64_t seed,
                                         const phnsw_build_params *centroid_bp,
                                         const phnsw_search_params *quantized_search, int centroid_metric,
                                         const phnsw_comm *comm, phnsw_store **out);
int phnsw_pq_shared_read(const phnsw_store *s, uint16_t *codes, float *codebook);
int phnsw_pq_shared_reconstruct_store(const phnsw_store *s, phnsw_store **out);
int phnsw_pq_info(const phnsw_store *s, uint32_t *m, uint32_t *ksub, uint32_t *dsub);
/* storage of the per-query lookup table: 0 = f32 (reference arithmetic), 1 = IEEE half entries,
 * 2 = 8-bit entries with a per-query scale (integer sums; fewest L2 requests per hop).  Modes 1
 * and 2 change the quantised distances.  Mode 1 must be set before building an index over the
 * store.  Mode 2 scales by the query's own table, so d(a,b) != d(b,a): it is for SEARCHING a graph
 * built in mode 0 or 1 (build entry points refuse it with PHNSW_E_UNSUPPORTED). */
int phnsw_pq_set_table_mode(phnsw_store *s, int mode);
int phnsw_pq_set_table_f16(phnsw_store *s, int on); /* = set_table_mode(s, on ? 1 : 0) */
int phnsw_pq_read(const phnsw_store *s, uint8_t *codes, float *codebook);
/* Quantizer::quantize / ::reconstruct  src/pq.rs:61-81 for n host vectors [n][dim] <-> codes [n][m] */
int phnsw_pq_quantize(const phnsw_store *s, const float *rows, uint64_t n, uint8_t *out_codes);
int phnsw_pq_reconstruct(const phnsw_store *s, const uint8_t *codes, uint64_t n, float *out_rows);
/* QuantizedHnsw::search  pq.rs:346-364 for a batch: search the index over the PQ store, re-rank
 * every result with the full-precision store, sort by (distance, id).  quantize_query != 0
 * quantises the query first like the reference (pq.rs:351-352); 0 = asymmetric (raw query
 * against codes).  Outputs as phnsw_search_batch. */
int phnsw_pq_search_batch(const phnsw_index *ix, const phnsw_store *full, const float *queries, uint64_t nq,
                          const phnsw_search_params *sp, int quantize_query, uint64_t *out_ids,
                          float *out_d, uint64_t *out_len, uint64_t *out_stats);

/* zero-copy form (asymmetric queries): search + re-rank kernels enqueued on `stream`, u32 ids */
int phnsw_pq_search_batch_device(const phnsw_index *ix, const phnsw_store *full, const float *queries_dev,
                                 uint32_t ldq, uint64_t nq, const phnsw_search_params *sp,
                                 uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                 uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);

/* ---- half-precision row store (rowstore.hip) ----
 * The rows of the f32 store `full`, rounded to IEEE binary16 (round to nearest even) by a device kernel: half the
 * bytes per stored vector and per gathered candidate.  n, dim, metric and device are those of `full`; a component
 * that is NaN or rounds to infinity in binary16 is PHNSW_E_INVALID.  A distance on the store widens the halves to f32
 * (exact) and runs the f32 store's arithmetic, so every result equals, bit for bit, the f32 search over the widened
 * rows -- which phnsw_store_read returns (phnsw_store_info reports rows_dev NULL).  The store is SEARCH-ONLY:
 * phnsw_distance_batch, phnsw_index_from_layers (adopt a graph built over the f32 store), phnsw_search_batch,
 * _stored, _topk, _device, phnsw_index_layer_*, the phnsw_last_search_* / phnsw_dense_top_layers queries and the
 * destroy calls work on it and on an index over it; every other entry point returns PHNSW_E_UNSUPPORTED. */
int phnsw_store_create_f16(const phnsw_store *full, phnsw_store **out);
/* search the index over the f16 store with `sp`, recompute the distance of every returned id against the f32 store
 * `full` (the bits of phnsw_distance_batch on it), sort by (distance, id), keep the best k <= number_of_candidates.
 * out_ids / out_d are [nq][k], out_len[q] = min(results of query q, k). */
int phnsw_f16_search_batch(const phnsw_index *ix, const phnsw_store *full, const float *queries, uint64_t nq,
                           const phnsw_search_params *sp, uint64_t k, uint64_t *out_ids, float *out_d,
                           uint64_t *out_len);
/* zero-copy form: search, re-rank and cut enqueued on `stream`, u32 ids; rows keep the search's stride
 * (number_of_candidates entries per query), the first out_len[q] <= k are live, the rest empty */
int phnsw_f16_search_batch_device(const phnsw_index *ix, const phnsw_store *full, const float *queries_dev,
                                  uint32_t ldq, uint64_t nq, const phnsw_search_params *sp, uint64_t k,
                                  uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                  uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);

/* ---- int8 row store (rowstore.hip) ----
 * The rows of the f32 store `full`, scalar-quantised per row and symmetrically by a device kernel:
 *   scale = maxabs(row) / 127.0f,  code_j = (int8) clamp(rintf(x_j / scale), -127, 127)   (IEEE f32 divisions),
 * a scale of 0 (a row of zeros, or a maxabs whose quotient underflows) gives codes 0.  A stored row is its f32 scale
 * and its code bytes: a quarter of the bytes per stored vector and per gathered candidate.  n, dim, metric and device
 * are those of `full`; a NaN or infinite component is PHNSW_E_INVALID, and so is a source that is not an f32 store.
 * A distance on the store dequantises (scale * (float)code, one f32 multiply) and runs the f32 store's arithmetic, so
 * every result equals, bit for bit, the f32 search over the dequantised rows -- which phnsw_store_read returns
 * (phnsw_store_info reports rows_dev NULL).  The store is SEARCH-ONLY with the supported list of the f16 store:
 * phnsw_distance_batch, phnsw_index_from_layers, phnsw_search_batch, _stored, _topk, _device, phnsw_index_layer_*,
 * the phnsw_last_search_* / phnsw_dense_top_layers queries and the destroy calls; every other entry point returns
 * PHNSW_E_UNSUPPORTED. */
int phnsw_store_create_i8(const phnsw_store *full, phnsw_store **out);
/* the stored codes [n][dim] and scales [n] of an i8 (or i8q) store */
int phnsw_i8_read(const phnsw_store *s, int8_t *codes, float *scales);
/* phnsw_f16_search_batch / _device over an index on an i8 store: search, recompute every returned id on `full`,
 * sort by (distance, id), keep the best k <= number_of_candidates; same outputs */
int phnsw_i8_search_batch(const phnsw_index *ix, const phnsw_store *full, const float *queries, uint64_t nq,
                          const phnsw_search_params *sp, uint64_t k, uint64_t *out_ids, float *out_d,
                          uint64_t *out_len);
int phnsw_i8_search_batch_device(const phnsw_index *ix, const phnsw_store *full, const float *queries_dev,
                                 uint32_t ldq, uint64_t nq, const phnsw_search_params *sp, uint64_t k,
                                 uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                 uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);

/* ---- int8 row store searched symmetrically: int8 query, integer dot products (rowstore.hip) ----
 * The rows are exactly those of phnsw_store_create_i8 (same quantiser, same layout; phnsw_i8_read and phnsw_store_read
 * return the same values).  A distance quantises the query too -- a raw query with the rows' own quantiser
 *   sq = maxabs(query) / 127.0f,  cq_j = clamp(rintf(q_j / sq), -127, 127)   (sq == 0: codes 0),
 * a Stored query as its row's codes and scale, never requantised -- and is
 *   dot = (sq * sr) * (float)idot,  idot = sum_j cq_j * cr_j  in int32 (exact),
 * two IEEE f32 multiplies in that order and a round-to-nearest-even conversion, put through the metric like any dot
 * product (tests/i8q_reference.py restates it in numpy).  A non-finite raw query is outside the contract.  The two
 * dot-product metrics only: an L2 `full` is PHNSW_E_UNSUPPORTED (the Euclidean distance would need the rows' norms).
 * A source that is not an f32 store, or a NaN or infinite component, is PHNSW_E_INVALID.  SEARCH-ONLY, with the
 * supported list of the i8 store; every other entry point returns PHNSW_E_UNSUPPORTED. */
int phnsw_store_create_i8q(const phnsw_store *full, phnsw_store **out);
/* phnsw_i8_search_batch / _device over an index on an i8q store (the i8 calls refuse an i8q index and the other way
 * round): search, recompute every returned id on `full`, sort by (distance, id), keep the best k; same outputs */
int phnsw_i8q_search_batch(const phnsw_index *ix, const phnsw_store *full, const float *queries, uint64_t nq,
                           const phnsw_search_params *sp, uint64_t k, uint64_t *out_ids, float *out_d,
                           uint64_t *out_len);
int phnsw_i8q_search_batch_device(const phnsw_index *ix, const phnsw_store *full, const float *queries_dev,
                                  uint32_t ldq, uint64_t nq, const phnsw_search_params *sp, uint64_t k,
                                  uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                  uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);

/* ---- 1-bit sign row store: Hamming distances, f32 re-rank (rowstore.hip) ----
 * The rows of the f32 store `full` reduced to one bit per component by a device kernel: bit j of a row is
 * rows[i][j] < 0.0f (+0, -0 and every non-negative value give 0); components past dim (padding) are bit 0 in every row
 * and in every query.  96 bytes per stored 768-component vector instead of 3 072.  n, dim, ld, metric and device are
 * those of `full` (phnsw_store_info; rows_dev NULL); all three metrics are accepted.  A source that is not an f32 store,
 * or a NaN or infinite component, is PHNSW_E_INVALID; a row longer than 1536 floats is PHNSW_E_UNSUPPORTED.
 * phnsw_store_read returns a row as +1.0f (bit 0) / -1.0f (bit 1), [count][dim].
 * A distance is taken from h = popcount(row XOR query) over the row's words:
 *   dot-product metrics: r = (float)(dim - 2 h);   Euclidean: r = (float)(4 h);   then the metric's own last step.
 * A raw query is reduced to its sign bits by the rows' rule (q[j] < 0), a Stored query is its row as it is.  That is
 * exactly the f32 search over the rows phnsw_store_read returns with the query where(q < 0, -1, +1): every partial sum
 * is an integer below 2^24, so the f32 arithmetic reaches it in any summation order (tests/bits_reference.py restates
 * it in numpy).  The distances of the plain calls are therefore in SIGN-VECTOR UNITS (COSINE_HALF runs from 1/2 down
 * to (1 - dim) / 2, ONE_MINUS_DOT from 1 + dim to 1 - dim, L2 from 0 to 2 sqrt(dim)); a distance takes at most dim + 1
 * values, ties are the normal case and the id decides, as everywhere.  phnsw_bits_search_batch[_device] return TRUE
 * f32 distances: they recompute every candidate on `full`.
 * Served: phnsw_distance_batch, phnsw_index_from_layers (adopt a graph built over the f32 store), phnsw_search_batch,
 * _stored, _topk, _device (no dense tables, no split descent: every layer per hop), phnsw_index_layer_*, the
 * phnsw_last_search_* queries, the destroy calls and the re-ranked pair below.  EVERY other entry point -- every filtered,
 * labelled, ranged, collecting and radius walk, every exact scan and table, phnsw_bruteforce_topk, build / link / improve
 * / promote / extend, phnsw_store_append, serialisation, the PQ constructors, knn / threshold_nn / search_instrumented --
 * returns PHNSW_E_UNSUPPORTED on the host, before any launch, with a message that names the call and "bits". */
int phnsw_store_create_bits(const phnsw_store *full, phnsw_store **out);
/* the sign bits [n][ceil(dim / 32)] of a bits store: component j is bit j & 31 of word j >> 5 (the public layout,
 * whatever the stride of the rows on the device) */
int phnsw_bits_read(const phnsw_store *s, uint32_t *words);
/* phnsw_i8q_search_batch / _device over an index on a bits store: walk with `sp` (Hamming distances), recompute all
 * number_of_candidates returned ids on `full` (true f32 distances, the bits of phnsw_distance_batch on it), sort by
 * (distance, id), keep the best k <= number_of_candidates; same outputs */
int phnsw_bits_search_batch(const phnsw_index *ix, const phnsw_store *full, const float *queries, uint64_t nq,
                            const phnsw_search_params *sp, uint64_t k, uint64_t *out_ids, float *out_d,
                            uint64_t *out_len);
int phnsw_bits_search_batch_device(const phnsw_index *ix, const phnsw_store *full, const float *queries_dev,
                                   uint32_t ldq, uint64_t nq, const phnsw_search_params *sp, uint64_t k,
                                   uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                   uint32_t *out_stats_dev, uint32_t *status_dev, void *stream);

/* ---- on-disk interchange with the Rust crate: serialize_hnsw / deserialize_hnsw
 * (src/serialize.rs:33-209): <dir>/meta (JSON HNSWMeta), <dir>/comparator/ (this library's
 * store; a crate user substitutes their own Serializable comparator), layer.meta.N (JSON),
 * layer.nodes.N / layer.neighbors.N (raw native-endian u64, !0 = empty), N from the bottom.
 * Deserialising needs the store the index was built over (the crate's C::Params role); a
 * missing comparator entry is "Index not found" (serialize.rs:144-146). ---- */
int phnsw_index_serialize(const phnsw_index *ix, const char *path);
int phnsw_index_deserialize(phnsw_store *s, const char *path, phnsw_index **out);
int phnsw_index_build_params(const phnsw_index *ix, phnsw_build_params *bp);

/* Hnsw::knn  src/lib.rs:905-928 : bottom layer, out [node_count][k] */
int phnsw_knn(const phnsw_index *ix, uint64_t k, uint64_t probe_depth, uint64_t *out_ids,
              float *out_d, uint64_t *out_len);

/* ---- exact k nearest neighbours by brute force: the ground truth for recall@k (the reference
 * only measures self-recall, lib.rs:1485-1496).  A true GEMM (queries x base rows) on the f32
 * MFMA units, exact f32 with a k-ordered fma chain per score; dot-product metrics, k <= 16.
 * Results sorted by (distance, id). ---- */
int phnsw_bruteforce_topk(const phnsw_store *s, const float *queries, uint64_t nq, uint32_t k,
                          uint64_t *out_ids, float *out_d);
int phnsw_bruteforce_topk_device(const phnsw_store *s, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                 uint32_t k, uint32_t *out_ids_dev, float *out_d_dev, void *stream);
float phnsw_bruteforce_last_gemm_ms(void); /* MFMA GEMM time of this thread's last pass */

/* Hnsw::threshold_nn  src/lib.rs:930-962 : bottom layer; out [node_count][max_out], entries
 * with distance < threshold, self removed.  The queue doubles without bound like the reference's
 * (resize_capacity, lib.rs:949-951): in LDS up to 1024 entries, in global memory beyond. */
int phnsw_threshold_nn(const phnsw_index *ix, float threshold, uint64_t probe_depth,
                       uint64_t initial_search_depth, uint64_t max_out, uint64_t *out_ids,
                       float *out_d, uint64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif
