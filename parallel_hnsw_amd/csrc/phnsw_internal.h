// Internal declarations of libphnsw (gfx950 only).  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/phnsw.h"

#define PH_EMPTY32 0xFFFFFFFFu
#define PH_FMAX 3.4028234663852886e38f
#define PH_MAX_LAYERS 24
#define PH_WAVE 64
#define PH_MAX_DISPATCH 24
#define PH_DENSE_SPLIT_MIN 2048u  // batches from this size on walk their dense top layers in a launch of its own  // search launches of one descent (<= PH_MAX_LAYERS)
#define PH_TINY_MAX_NODES 8192u      // largest layer evaluated densely (tiny.hip)
#define PH_TINY_LDS_NODES 1024u      // up to here a query's table row is staged in LDS
#define PH_TINY_MAX_LAYERS 8

void ph_set_error(const char *fmt, ...);
// every extern "C" entry point is a function-try-block ending in `catch (...) { return ph_caught(); }`:
// nothing unwinds across the ABI (phnsw.h), a C++ exception becomes a status + message
int ph_caught() noexcept;
int ph_hip_fail(hipError_t e, const char *what, const char *file, int line);
#define PH_HIP(x)                                                       \
  do {                                                                  \
    hipError_t e__ = (x);                                               \
    if (e__ != hipSuccess) return ph_hip_fail(e__, #x, __FILE__, __LINE__); \
  } while (0)

// ---- device view of one layer (Layer<C>, src/lib.rs:85-91) ----
// node ids and vector ids are u32 on the device (n <= 2^31 - 1); the u64 <-> u32
// conversion and the !0 sentinel mapping happen at the ABI boundary.
struct PhLayerDev {
  uint32_t n_nodes;
  uint32_t W;                 // neighborhood_size
  const uint32_t *nodes;      // [n_nodes] NodeId -> VectorId, ascending
  const uint32_t *neighbors;  // [n_nodes * W], trailing PH_EMPTY32
  const uint32_t *vec2node;   // [store n] VectorId -> NodeId or PH_EMPTY32; nullptr = identity
};

struct PhLayerHost {
  uint32_t n_nodes = 0, W = 0;
  uint32_t *nodes = nullptr;
  uint32_t *neighbors = nullptr;
  float *nbr_dist = nullptr;  // [n_nodes * W] distance of each occupant to the row owner (build only)
  uint64_t links_epoch = 0;   // bumped whenever rows of `neighbors` are rewritten in place (build.hip: apply_proposals)
  uint32_t *vec2node = nullptr;
  bool identity = false;
  uint32_t *recall_q = nullptr;  // cached stochastic_recall_at sample (build.hip), recall_n entries
  uint32_t recall_n = 0;
  // locality schedule: pos[node] = the node's coarse cell (chain rank of its nearest anchor,
  // anchors = a strided sample of the store; bruteforce.hip); ord = argsort(pos[ord_first .. +ord_count)), cached
  uint32_t *pos = nullptr;
  uint32_t *ord = nullptr;
  uint32_t ord_first = 0, ord_count = 0;
};

// How a store keeps its vectors.  The three row kinds are searched by the same kernels through a row policy
// (RowF32 / RowF16 / RowI8, phnsw_device.h); f16, i8 and i8q are the converted, search-only stores of rowstore.hip.
enum PhRowKind : int {
  PH_ROWS_F32 = 0,    // [n][ld] f32
  PH_ROWS_F16,        // [n][ld] IEEE binary16 in component order: rows start on 8-byte boundaries
  PH_ROWS_I8,         // n rows of 4 + ld bytes rounded up to a multiple of 16: the f32 scale, then ld int8 codes
  PH_ROWS_PQ,         // u8 codes over per-sub-space codebooks (pq.hip)
  PH_ROWS_PQ_SHARED,  // u16 codes over one shared codebook (pq.hip)
  PH_ROWS_I8Q,        // the bytes of PH_ROWS_I8; a distance quantises the query too and takes integer dot products (DistI8Q)
  PH_ROWS_BITS,       // n rows of 32 * ph_chunk_count(ld / 4) bytes: one sign bit per component (bits_plan.h, DistBits)
};
static inline bool ph_rows_converted(int kind) { return kind == PH_ROWS_F16 || kind == PH_ROWS_I8 || kind == PH_ROWS_I8Q; }
// the 1-bit sign store is NOT one of the converted kinds: it has no f32 view of a row in registers, so the dense tables,
// the split descent, the cells and the filtered / exact kernels written over a row policy do not serve it
static inline bool ph_rows_bits(int kind) { return kind == PH_ROWS_BITS; }
static inline bool ph_rows_i8_layout(int kind) { return kind == PH_ROWS_I8 || kind == PH_ROWS_I8Q; }  // scale + int8 codes
static inline const char *ph_rows_name(int kind) {
  static const char *const names[] = {"f32", "f16", "i8", "product-quantised", "shared-codebook product-quantised", "i8q", "bits"};
  return names[kind];
}
// float4 chunks a lane holds of a row of nv4 float4s: the three shapes the row kernels are instantiated for (0: none;
// a launch switches on this value, one case per instance)
static inline int ph_chunk_count(uint32_t nv4) { return nv4 <= 64 ? 1 : (nv4 <= 192 ? 3 : (nv4 <= 384 ? 6 : 0)); }
int ph_dim_unsupported(uint32_t dim);  // sets "dim unsupported (max 1536)", returns PHNSW_E_UNSUPPORTED (misc.hip)
// where the rows of a row kind are: one base pointer, one stride in bytes
struct PhRows {
  const void *base;  // nullptr for a PQ store
  uint32_t stride;   // bytes from one row to the next
  int kind;          // PhRowKind
};

// what a distance evaluation needs: the rows of an f32, f16 or i8 store, or -- for a product-quantised store --
// code rows + per-subspace codebooks (pq.hip)
struct PhDistArgs {
  PhRows rows;
  uint32_t ld, nv4;  // components per row (padded), float4 chunks per row
  int metric;
  const uint8_t *codes;   // [n][m] u8 codes (PQ store)
  const uint16_t *codes16;  // [n][m] u16 codes over ONE shared codebook [ksub][dsub] (the reference's shape, pq.rs:19-27)
  const float *codebook;  // [m][ksub][dsub]
  uint32_t m, ksub, dsub;  // (a bit store, which has no code rows, keeps the rows' dim in m: ph_bits_distance needs it)
  uint32_t table_f16;  // 1: the per-query table holds IEEE half values (2 bytes per entry)
};

struct phnsw_store {
  int device = 0;
  int kind = PH_ROWS_F32;  // PhRowKind: what the store is, whatever its size (an empty store has no allocation to test)
  float *rows = nullptr;   // [n][ld] flat, HBM: the f32 rows, nullptr for every other kind
  // product-quantised store (phnsw_store_create_pq): rows == nullptr, dim/ld describe the
  // full vectors a query has
  uint8_t *codes = nullptr;
  uint16_t *codes16 = nullptr;  // shared-codebook PQ store (pq.hip): codes [n][pq_m], codebook [pq_ksub][pq_dsub]
  phnsw_store *centroid_store = nullptr;  // ... its centroids as a store of their own and the HNSW over them
  phnsw_index *centroid_index = nullptr;  //     (HnswQuantizer, pq.rs:29-81)
  phnsw_search_params quantized_search = {0, 0, 0};
  float *codebook = nullptr;
  uint32_t pq_m = 0, pq_ksub = 0, pq_dsub = 0;
  uint32_t pq_table_f16 = 0;
  // converted store (phnsw_store_create_f16 / _i8 / _i8q, rowstore.hip): rows == nullptr, packed = n rows of
  // packed_stride bytes in the layout of its kind; a distance widens / dequantises them to f32 and runs the f32 chain
  // (i8q: integer dot products of the codes, DistI8Q).  Search-only: see ph_search_only_unsupported.
  void *packed = nullptr;
  uint32_t packed_stride = 0;
  // coarse cells of the locality schedule (bruteforce.hip): anchor rows + their chain ranks
  float *anchors = nullptr;
  uint32_t *anchor_rank = nullptr;
  uint32_t n_anchors = 0;
  bool cells_raw = false;  // PHNSW_CELLS=raw when the anchors were made: the cells of before (A/B comparison)
  bool owns_rows = true;
  uint64_t n = 0;
  uint32_t dim = 0, ld = 0;
  int metric = 0;
  int refcount = 1;
};

// identity of the inputs of ph_tiny_prep_kernel (the dense layers' node lists and neighbour rows) and of the node-side
// ph_tiny_pack_kernel (the table layer's node list and the stored rows): pointers, sizes and the epochs that say
// whether what they point at has been rewritten
struct PhTinyPrepKey {
  bool valid = false;
  uint64_t nodes_epoch = 0;
  uint32_t T = 0, tn = 0;
  const void *nodes[PH_TINY_MAX_LAYERS] = {}, *nbrs[PH_TINY_MAX_LAYERS] = {}, *vec2node = nullptr;
  uint32_t n[PH_TINY_MAX_LAYERS] = {}, W[PH_TINY_MAX_LAYERS] = {};
  uint64_t links[PH_TINY_MAX_LAYERS] = {};
};
struct PhTinyPackKey {
  bool valid = false;
  uint64_t nodes_epoch = 0;
  const void *vecs = nullptr, *tnodes = nullptr;  // vecs: the base pointer of the stored rows (PhRows::base)
  uint32_t ld = 0, tn = 0, nv = 0;
};

struct PhWorkspace {
  // per resident-wave search state: visited bitmap + overflow (frontier spill) list
  uint32_t *visited = nullptr;
  uint64_t visited_words = 0;  // per slot
  uint2 *ovf = nullptr;
  uint32_t ovf_cap = 0;  // entries per slot
  uint32_t n_slots = 0;
  uint32_t *counter = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t evc = nullptr;  // start of the last chunk of the descent (== ev0 when the list ran in one piece)
  bool timed = false;
  void *pq_tables = nullptr;  // n_slots x table bytes (PQ stores)
  size_t pq_tables_bytes = 0;
  // two-launch descents: per-query locality keys, their argsort, radix-sort scratch
  uint32_t *okey = nullptr, *okey_sorted = nullptr, *oiota = nullptr, *oorder = nullptr;
  void *sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  uint32_t order_cap = 0;
  uint32_t *ocell = nullptr;  // table order (api.hip): queries per cell, then where a cell's queries start, [ocell_cap + 1]
  uint32_t ocell_cap = 0;
  // dense top layers (tiny.hip): distance table [positions][stride], neighbour rows in table ids,
  // per-node layer membership (+ one flag word)
  float *tiny_d = nullptr;
  size_t tiny_d_bytes = 0;
  uint32_t *tiny_nbr = nullptr;
  size_t tiny_nbr_bytes = 0;
  uint32_t *tiny_member = nullptr;
  size_t tiny_member_bytes = 0;
  float4 *tiny_pq = nullptr, *tiny_pn = nullptr;  // matrix-core operands: packed positions / nodes (tiny.hip)
  size_t tiny_pq_bytes = 0, tiny_pn_bytes = 0;
  // what tiny_nbr / tiny_member and tiny_pn were made from: a launch whose key matches skips the kernels (tiny.hip)
  PhTinyPrepKey tiny_prep_key;
  PhTinyPackKey tiny_pack_key;
  int tiny_table_g = 0;  // staging depth of the last matrix-core table kernel on this workspace (0: none ran)
  uint32_t tiny_last_npos = 0, tiny_last_tn = 0, tiny_last_stride = 0;  // shape of the last per-launch table in tiny_d
  uint2 *dense_ovf = nullptr;  // spill lists of the dense-only launch: [its resident waves][table nodes]
  size_t dense_ovf_bytes = 0;
  uint32_t *ovf_s = nullptr;  // search_instrumented: index sums of the spilled entries, [n_slots][ovf_cap]
  size_t ovf_s_cap = 0;
  // a collecting search in a split descent: its output rows hold collect_k entries, so the running candidates are
  // parked here between the launches, [nq][ef]
  uint32_t *park_ids = nullptr;
  float *park_d = nullptr;
  size_t park_ids_bytes = 0, park_d_bytes = 0;
  // per-dispatch bookkeeping of the last descent (phnsw_last_search_dispatches): evd[0] closes the
  // dense-top-layer kernels, evd[1 + i] search launch i; dtotals[i] = {distance evaluations, hops}
  hipEvent_t evd[PH_MAX_DISPATCH + 1] = {};
  unsigned long long *dtotals = nullptr;  // device [PH_MAX_DISPATCH][2], then [PH_MAX_DISPATCH] table-served evaluations
  uint32_t n_dispatch = 0;
  uint32_t n_chunks = 0;  // chunks of the last descent (a query list longer than the dense table holds): the per-dispatch
                          // figures then describe the LAST chunk, times and counters alike
  int cus = 0;            // compute units of the workspace's device
  uint32_t d_lo[PH_MAX_DISPATCH] = {}, d_hi[PH_MAX_DISPATCH] = {};
  bool d_tiny = false;
};

// The dense distance table of the BUILD's searches, kept across rounds (tiny.hip).  A link round, a recall estimate and
// discover_unreachable all search with Stored(node of layer X) queries, and the distance of such a node to the nodes
// of the table layer does not change between rounds: row r = node r of layer X, computed once, reused until a node
// list changes (epoch).  17 % of a 1M build's GPU time was recomputing it every round.
struct PhBuildTable {
  float *D = nullptr;       // rows [lo_alloc, hi_alloc) x stride
  size_t bytes = 0;         // ... in use; `cap` allocated
  size_t cap = 0;
  const uint32_t *qnodes = nullptr, *tnodes = nullptr;  // identity of layer X and of the table layer
  uint32_t qn = 0, tn = 0, T = 0, stride = 0;
  uint32_t lo_alloc = 0, hi_alloc = 0, lo = 0, hi = 0;  // allocated rows; valid rows [lo, hi)
  uint64_t epoch = 0;
};
// which layer the Stored queries of a build search are nodes of (build.hip -> ph_search_device)
struct PhRowHint {
  const uint32_t *qnodes;    // device: node list of layer X
  uint32_t qn;
  const uint32_t *vec2node;  // device: VectorId -> NodeId of layer X, nullptr = identity
  uint32_t first, count;     // contiguous: the queries are nodes [first, first + count) of X
  bool contiguous;           // false: any nodes of X (a recall sample)
};

// the allow-list of a filtered search as ph_search_device takes it (device words; PhSearchArgs::filter*)
// ... or its label form: label_of != nullptr, the column [n] of a phnsw_labels handle (PHNSW_LABEL_NONE where a vector
// is not listed) and want [nq], the label each query wants; words is then unused, flags mean the same
// ... or its set form: label_of and set_first != nullptr, set_first [nq + 1] offsets into set_values [set_nwant] (the
// labels each query wants, untrusted: PhSearchArgs::set_first); want is then unused
struct PhFilter {
  const uint32_t *words;
  uint32_t stride, flags;
  const uint32_t *label_of, *want;
  const uint32_t *set_first, *set_values;
  uint32_t set_nwant;
  // ... or its range form: attr_of != nullptr, the column [n] of a phnsw_attr handle (PHNSW_ATTR_NONE where a vector is
  // not listed), range_lo and range_hi [nq], the inclusive bounds of each query; nothing of the forms above goes with it
  const uint32_t *attr_of, *range_lo, *range_hi;
  // ... or its label-range form: pair_of != nullptr, the column [n] of a phnsw_label_attr handle (the composite
  // (label << 32) | key of a listed vector, UINT64_MAX elsewhere), pair_want, pair_lo and pair_hi [nq], the label and
  // the inclusive bounds of each query; nothing of the forms above goes with it
  // ... or the set form of that: pair_of and set_first != nullptr -- the set table above in place of pair_want, which is
  // then unused, and pair_lo, pair_hi [nq], ONE range per query shared by the labels of its set; label_of stays nullptr
  const uint64_t *pair_of;
  const uint32_t *pair_want, *pair_lo, *pair_hi;
};

// per-slice results of an exact scan that was cut into slices (filter_exact.hip): [nq][slices][k] keys from
// ph_pool_alloc, kept with the index.  Two of them, used alternately like the search workspaces, so that scans on two
// streams may overlap; `done` closes the last launch that used one, and the next user's stream waits for it.
struct PhExactScratch {
  uint64_t *keys = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;
};

// resident waves of the one-wave kernels an index or a labels handle has launched, per (kernel, dynamic LDS size):
// ph_resident_waves (filter_exact.hip), under a mutex of the owner
struct PhResidentMemo {
  struct Entry {
    const void *fn;
    size_t lds;
    uint64_t waves;
  };
  std::vector<Entry> known;
  int cus = 0;  // compute units of the device, 0 = not asked yet
};

// call_set.h: the scratch sets of one kind of filtered or exact call, one set per call in flight, handed out under mutex
struct PhCallSet;
struct PhCallPool {
  std::mutex mutex;
  std::vector<PhCallSet *> sets;
};
struct PhPendingLayer;
struct PhHostStage;  // hostpath.hip: persistent staging of the host-pointer search entry points
struct phnsw_index {
  std::vector<PhHostStage *> stages;  // handed out under stage_mutex, one per concurrent host-pointer call
  std::mutex stage_mutex;
  std::vector<PhBuildTable> bt;  // one per layer whose nodes query; build entry points only (exclusive access to the index)
  // buffers of dropped tables, reused by the next table that fits: a build re-makes its tables whenever a promotion
  // changes a node list, and device allocation is host work whose cost varies with what else the host is doing
  std::vector<std::pair<float *, size_t>> bt_spare;
  bool bt_enabled = false;    // set for the duration of a build / improve_index call: nothing else may keep 29 GB
  uint64_t nodes_epoch = 0;   // bumped whenever a layer's node list is created, replaced or dropped
  PhPendingLayer *pending = nullptr;  // layer under construction (phase API, build.hip)
  phnsw_store *store = nullptr;
  std::vector<PhLayerHost> layers;  // top first (src/lib.rs:587)
  phnsw_build_params bp;
  std::mutex ws_mutex;
  // two workspaces, used alternately: launches on different streams may overlap (the tail of
  // one batch with the head of the next); a third launch waits for the first
  PhWorkspace ws[2];
  uint32_t ws_next = 0, ws_last = 0;
  float last_kernel_ms = 0.f;
  unsigned long long *totals = nullptr;  // device [2]: distance evaluations, hops of every launch on this index
  const uint32_t *dbg_order = nullptr;  // experiment hook
  const uint32_t *default_filter = nullptr;  // phnsw_index_set_filter_device: the caller's shared bitmap, filtered calls only
  uint32_t *all_ones = nullptr;  // a bitmap that allows every vector of the store, for collecting calls without a filter
  uint64_t all_ones_words = 0;   // (made on first use under ws_mutex, remade when the store has grown)
  uint64_t dbg_order_n = 0;
  std::mutex exact_mutex;  // filter_exact.hip
  PhExactScratch exact[2];
  uint32_t exact_next = 0;
  PhResidentMemo exact_resident;  // under exact_mutex
  PhCallPool autos;     // filter_auto.hip: PhAutoSet, the scratch of one routed filtered search
  PhCallPool denses;    // filter_dense.hip: PhDenseSet, of one exact search for a shared allow-list
  PhCallPool groupeds;  // filter_grouped.hip: PhGroupedSet, of one exact search over a table of allow-lists
  PhCallPool radii;     // filter_radius.hip: PhRadiusSet, of one exact radius search
};

// ---- kernel argument block for the batched greedy search ----
struct PhSearchArgs {
  PhDistArgs dist;
  const float *queries;  // [nq][ldq] or nullptr
  uint32_t ldq;
  const uint32_t *qids;     // or nullptr
  const uint32_t *exclude;  // or nullptr
  // allow-list of closest_vectors' `include` (lib.rs:250-277): bit v & 31 of word v >> 5 set = VectorId v may be
  // returned; nullptr = no filter.  filter_stride: words from one query's bitmap to the next, 0 = one bitmap for the
  // whole launch.  filter_flags: PHNSW_FILTER_STRICT also drops disallowed ids from the final output row (search.hip)
  const uint32_t *filter;
  uint32_t filter_stride, filter_flags;
  uint32_t nq;
  uint32_t n_layers;
  PhLayerDev layers[PH_MAX_LAYERS];
  uint32_t ef, upper, probe_depth;
  uint32_t *out_ids;
  float *out_d;
  uint32_t *out_len;
  uint32_t *out_stats;  // [nq][2] or nullptr
  uint32_t *status;     // [nq]
  uint32_t *visited;
  uint64_t visited_words;
  uint2 *ovf;
  uint32_t ovf_cap;
  uint32_t *counter;
  // 1 = Hnsw::knn (lib.rs:905-928): bottom layer only, query = node, seed (node, 0.0);
  // 2 = Hnsw::threshold_nn (lib.rs:930-962): the same, repeated with a doubling queue
  uint32_t knn_mode;
  float threshold;
  uint32_t first_node;  // knn modes: queries are nodes first_node .. first_node + nq
  uint32_t cap_max;     // threshold_nn: largest queue capacity the launch must support (0 = ef)
  // threshold_nn beyond the LDS queues (ph_search_kernel_big): an explicit node list and, per resident wave, a
  // queue of cap_max (id, distance) slots in global memory
  const uint32_t *knn_nodes;
  uint32_t *big_q;
  // dense layers: a query's table row is staged in LDS when the table layer has at most this many nodes
  // (PH_TINY_LDS_NODES; the one-wave-per-SIMD kernels of small batches raise it to what a CU's LDS holds)
  uint32_t tiny_lds_nodes;
  float hit_eps;        // out_hit: > 0 selects match_within_epsilon (search.rs:173-187)
  uint32_t out_stride;  // entries written per query (0 = ef); link rounds keep only the top M
  unsigned long long *totals;   // nullable: [2] running sums of distance evaluations / hops (all launches)
  unsigned long long *launch_totals;  // nullable: [2] the same for this launch alone
  unsigned long long *launch_tab;     // nullable: of this launch's evaluations, those the dense tables served
  void *pq_tables;              // PQ store: per-wave lookup-table slots in global memory (DistPQG)
  uint32_t pq_table_bytes;      // bytes per slot
  uint32_t layer_lo, layer_hi;  // layers of this launch (0, 0 = all); see search.hip
  uint32_t *out_key;            // nullable: locality key of each query after layer_hi - 1
  const uint32_t *key_pos;      // nullable: pos[] of layer layer_hi - 1
  // A split descent walks its dense top layers in a launch of its own (ph_search_kernel_dense: no row registers, so
  // twice the resident waves): dense_only marks that launch (layers [0, tiny_layers), spill lists of dense_ovf_cap
  // entries in dense_ovf); after_dense = T marks the launch that follows it.  Whether the table was usable (layers
  // nested) is only known on the device (dense_flag[0] == 0): if not, the dense launch does nothing and the
  // follow-up starts from layer 0 on the per-hop path.
  uint32_t dense_only, after_dense;
  const uint32_t *dense_flag;
  uint2 *dense_ovf;
  uint32_t dense_ovf_cap;
#ifdef PH_CELL_PROBE
  // experiment: how far, in cell-chain ranks, the bottom layer's evaluations stray from where the query landed
  const uint32_t *probe_pos;
  unsigned long long *probe_out;  // [12]: evaluations within 0,1,2,4,...,256 ranks; [10] all; [11] queries
#endif
#ifdef PH_VISITED_PROBE
  // experiment: ids visited per gathered layer walk, in buckets of 64 ([0, 64) upper layers, [64, 128) the
  // bottom layer; the last bucket holds everything above); [128 + k]: walks that passed the LDS table's load limit
  unsigned long long *vprobe_out;
#endif
  // visited set of the gathered layers in LDS (search.hip): a table of vis_slots NodeIds at word vis_off of the
  // dynamic LDS, at most vis_limit of them live (the rest of the layer then runs on the bitmap); 0 slots = bitmap
  uint32_t vis_slots, vis_limit, vis_off;
  const uint32_t *order;  // nullable: processing order (a permutation of 0..nq-1), see search.hip
  uint32_t seg;           // order != nullptr: positions per XCD segment
  uint32_t *out_hit;    // nullable: 1 when a Stored query found itself (stochastic_recall lib.rs:1492)
  uint32_t *out_index;  // nullable: Hnsw::search_instrumented's index_distance per query (selects the INSTR kernels)
  uint32_t *ovf_s;      // ... and the index sums of the spilled entries, parallel to ovf
  // dense top layers (tiny.hip): layers [0, tiny_layers) of this launch hold <= PH_TINY_MAX_NODES
  // nodes; the distance of every query to every node of layer tiny_layers - 1 sits in tiny_d
  // (same bits as the per-hop evaluation), the traversal of those layers runs in the id space
  // of that layer ("table ids") with its visited set in LDS (and its table row, when small)
  uint32_t tiny_layers, tiny_n, tiny_stride;
  const float *tiny_d;          // [launch positions][tiny_stride]
  const uint32_t *tiny_nbr;     // layer l: [tiny_n][W_l] at tiny_off[l], table ids, PH_EMPTY32 padded
  const uint32_t *tiny_member;  // [tiny_n] bit l = node of layer l; [tiny_n] != 0: layers not nested, table off
  // tiny_rows != 0: tiny_d is the build's kept table -- the row of a Stored query is its NodeId in layer X
  // (tiny_row_map: VectorId -> NodeId, nullptr = identity) minus tiny_row_first, not its launch position
  uint32_t tiny_rows, tiny_row_first;
  const uint32_t *tiny_row_map;
  uint32_t tiny_off[PH_TINY_MAX_LAYERS];
  // the filter by row label (search_labeled.hip): label_of [n], the label of every listed vector and PHNSW_LABEL_NONE
  // elsewhere; label_want [nq], what each query wants.  nullptr = not a label launch.  filter_flags as for the bitmap.
  // (At the end: the argument offsets of every other kernel stay what they were.)
  const uint32_t *label_of, *label_want;
  // the collecting walk (phnsw_search_collect*, search_collect.hip): collect_k != 0 selects the PH_FM_COLLECT twins for
  // the LAST launch of a descent, which writes rows of collect_k entries to collect_ids / collect_d (and their lengths to
  // out_len); out_ids / out_d are then only where a split descent parked its candidates.  collect_flags:
  // PHNSW_COLLECT_EXTEND.  (At the end, like the label pair.)
  uint32_t collect_k, collect_flags;
  uint32_t *collect_ids;
  float *collect_d;
  // table_by_query != 0: the per-launch table was made in natural order and `order` only afterwards (api.hip: the
  // table order), so a query's row is q, not its position.  (At the end, like the pairs above.)
  uint32_t table_by_query;
  // the filter by a SET of row labels (search_labelset.hip): set_first [nq + 1] offsets into set_values [set_nwant], the
  // labels query q wants = set_values[set_first[q] .. set_first[q + 1]); label_of is the column as above.  nullptr = not
  // a set launch; never with a bitmap or with label_want.  The offsets are absolute and NOT trusted: a query whose range
  // is not inside [0, set_nwant] or runs backwards does not walk (status 8).  (At the end, like the pairs above.)
  const uint32_t *set_first, *set_values;
  uint32_t set_nwant;
  // the filter by a numeric range of a row attribute (search_ranged.hip): attr_of [n], the key of every listed vector and
  // PHNSW_ATTR_NONE elsewhere; range_lo / range_hi [nq], the inclusive bounds of query q.  nullptr = not a range launch;
  // never with a bitmap, a label or a set, and never collecting.  (At the end, like the pairs above.)
  const uint32_t *attr_of, *range_lo, *range_hi;
  // the filter by a label and a numeric range (search_label_ranged.hip): pair_of [n], the composite (label << 32) | key
  // of every listed vector and UINT64_MAX elsewhere; pair_want / pair_lo / pair_hi [nq], the label and the inclusive
  // bounds of query q.  nullptr = not a label-range launch; never with a bitmap, a label, a set or a range, and never
  // collecting.  (At the end, like the pairs above.)  With set_first beside pair_of the launch is one by a SET of labels
  // and a range (search_labelset_ranged.hip): the set table above instead of pair_want (nullptr), label_of nullptr.
  const uint64_t *pair_of;
  const uint32_t *pair_want, *pair_lo, *pair_hi;
  // the radius search by graph walk (search_radius.hip): radius [nq], the threshold of each query's loop on the last
  // layer; nullptr = not a radius launch.  Selects the PH_FM_RADIUS twins: one launch over every layer, rows of
  // out_stride entries read from the last layer's queue, cap_max 1024.  Never with a filter, a knn mode or collecting.
  // (At the end, like the pairs above.)
  const float *radius;
};

uint32_t ph_default_ovf_cap(uint32_t ef);
// scratch allocator of the build path (misc.hip): hipMalloc / hipFree cost ~0.1 ms and a device
// sync each, a build issues thousands of them; freed blocks are kept by size class and handed
// out again (everything on the path runs on the null stream, so reuse is stream ordered)
hipError_t ph_timed_malloc(void **p, size_t bytes);  // hipMalloc / hipFree with their wall time accounted (misc.hip)
hipError_t ph_timed_free(void *p);
#ifndef PH_RAW_ALLOC  // every device allocation of the library goes through the accounted forms
#define hipMalloc(p, n) ph_timed_malloc((void **)(p), (n))
#define hipFree(p) ph_timed_free((void *)(p))
#endif
// a knob of the environment as a number, 0 when unset; read per call: the tests switch them
static inline long long env_ll(const char *name) {
  const char *e = getenv(name);
  return e ? atoll(e) : 0;
}
// the grid of a kernel whose 256-thread blocks stride over `items`
static inline uint32_t grid1(uint64_t items) {
  const uint64_t blocks = (items + 255u) / 256u;
  return (uint32_t)(blocks < (1u << 16) ? blocks : (1u << 16));
}
int ph_stream_beside(hipStream_t other, hipStream_t *io);  // a non-blocking stream on another hardware queue than `other` (misc.hip)
hipError_t ph_pool_alloc(void **p, size_t bytes);
void ph_pool_free(void *p);
void ph_pool_trim(void);  // give everything cached back to the driver
void ph_layer_free(PhLayerHost &l);
void ph_pending_free(phnsw_index *ix);
void ph_host_stages_free(phnsw_index *ix);  // hostpath.hip
int ph_layer_upload(phnsw_index *ix, const uint32_t *nodes, const uint32_t *neighbors, uint32_t n, uint32_t W,
                    PhLayerHost *out);
// The request of one device search (ph_search_device).  All pointers are device memory owned by the caller; the
// value-initialised struct means "absent" for every optional field, so a call site names only what it uses.
struct PhSearchCall {
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids) or a knn mode
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  const phnsw_search_params *sp;
  uint32_t upto;    // layers searched, 0 = all
  PhFilter filter;  // words == nullptr and label_of == nullptr: none
  uint32_t *out_ids;  // [nq][out_stride ? out_stride : number_of_candidates]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  uint32_t *out_stats;         // [nq][2] or nullptr
  uint32_t ovf_cap;            // spill-list entries per resident wave, 0 = ph_default_ovf_cap
  hipStream_t stream;
  // the rest as PhSearchArgs describes it; out_stride: threshold_nn's largest queue capacity as well
  uint32_t knn_mode, first_node, out_stride;
  float threshold, hit_eps;
  uint32_t *out_hit, *out_index;  // [nq] or nullptr
  const uint32_t *order;
  const PhRowHint *hint;  // a build's searches: the kept table (tiny.hip)
  // the collecting search (phnsw_search_collect*): collect_k = 1..64 results per query, and out_ids / out_d are then
  // rows of collect_k entries; `filter` is what the last layer's walk collects by (never STRICT: the descent itself is
  // the plain search's).  collect_flags: PHNSW_COLLECT_EXTEND
  uint32_t collect_k, collect_flags;
  // the radius search by graph walk: radius [nq] (device), rows of out_stride = max_out entries read from the last
  // layer's queue; out_len counts every entry inside the radius.  One launch, no dense tables, no filter
  const float *radius;
};
int ph_search_device(const phnsw_index *ix, const PhSearchCall &c);
// argument checks the search entry points share (api.hip): index and parameters; the device forms' pointers (`call`
// names the entry point in the message); a filtered call's flags and stride, *f = the triple a launch gets
int ph_check_sp(const phnsw_index *ix, const phnsw_search_params *sp);
int ph_filter_check(const phnsw_index *ix, const uint32_t *filter, uint32_t stride, uint32_t flags, const char *call,
                    PhFilter *f);
// the filter of a collecting call by bitmap: the caller's, else the index's default filter, else a bitmap of all ones
// kept with the index (the collecting kernels exist over a bitmap and over a label column; api.hip)
int ph_collect_filter(const phnsw_index *ix, PhFilter *f, bool *on_device);
// what the collecting entry points check first, in this order: index and parameters, the flags, k in 1..64, the stride
int ph_collect_check(const phnsw_index *ix, const phnsw_search_params *sp, uint32_t stride, uint32_t flags, uint64_t k,
                     const char *call);
#define PH_COLLECT_KMAX 64u
// The request of one host-pointer search (ph_search_host, hostpath.hip): host arrays, ids as u64.
struct PhHostSearch {
  const float *queries;            // [nq][dim] or nullptr
  const uint64_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  const phnsw_search_params *sp;
  uint32_t upto, knn_mode;
  uint64_t out_k;  // results kept per query, 0 = the whole queue (number_of_candidates entries)
  uint64_t *out_ids;  // [nq][k]
  float *out_d;
  uint64_t *out_len;
  uint64_t *out_stats, *out_index;  // [nq][2], [nq] or nullptr
  PhFilter filter;                  // host words; words == nullptr: none
  bool filter_on_device;            // filter.words is a shared bitmap in device memory (phnsw_index_set_filter_device)
  bool exact;  // the exact scan over the allow-list instead of the graph search (ph_exact_device): sp unused, out_k = k >= 1
  // the collecting search: out_k = k = 1..64, rows of k entries.  Its label form: filter.label_of = the handle's column
  // (device), filter.want = HOST labels [nq], staged with their chunk
  bool collect;
  uint32_t collect_flags;
};
int ph_search_host(const phnsw_index *ix, const PhHostSearch &h);
// The request of one exact top-k scan over an allow-list (ph_exact_device, filter_exact.hip).  Device pointers of the
// caller, enqueued on `stream`; rows of k entries, PH_EMPTY32 / PH_FMAX padded.
struct PhExactCall {
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids)
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  PhFilter filter;  // words == nullptr: every vector of the index
  uint32_t k;       // 1..PH_EXACT_KMAX
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  hipStream_t stream;
  // nullable: the scan covers queries list[0 .. nq) only (device words; filter_auto.hip).  nq is then the list's length;
  // queries, qids, exclude, per-query bitmaps and every output stay addressed by the query index the list holds
  const uint32_t *list;
};
int ph_exact_device(const phnsw_index *ix, const PhExactCall &c);
// what ph_exact_device would refuse for this store and k (the row length, a PQ table beside the scan's LDS): 0 or the code
int ph_exact_supported(const phnsw_index *ix, uint32_t k);
// the bottom layer as the candidate test takes it (filter_candidate.h): *vec2node == nullptr for an identity layer
void ph_exact_bottom_layer(const phnsw_index *ix, uint32_t *n_nodes, const uint32_t **nodes, const uint32_t **vec2node);
int ph_filter_count(const phnsw_index *ix, const PhFilter &f, uint64_t nbitmaps, uint32_t *out_count_dev, hipStream_t stream);
void ph_exact_free(phnsw_index *ix);
// launch preparation of a one-wave kernel: the dynamic-LDS attribute above 48 KiB, and the waves of it the device holds
// at once, asked once per (kernel, LDS) and kept in `memo` under `mutex` (filter_exact.hip)
int ph_resident_waves(PhResidentMemo &memo, std::mutex &mutex, int device, const void *fn, size_t lds, uint64_t *waves);
// what the device forms of the filtered calls ask of their queries: raw rows or Stored ids, exactly one; raw rows at
// least a store row long, a multiple of 4 floats, on a 16-byte base
static inline bool ph_device_queries_ok(const phnsw_index *ix, const float *queries_dev, const uint32_t *qids_dev, uint32_t ldq) {
  return ((!queries_dev) != (!qids_dev)) &&
         !(queries_dev && (ldq < ix->store->ld || (ldq % 4) || ((uintptr_t)queries_dev % 16)));
}
// The table of the exact calls over shared allow-lists, then its select (filter_dense.hip): one run of positions against
// one ascending candidate list, node chunks x position chunks (dense_plan.h).
struct StepTimes;  // call_set.h
struct PhTableRun {
  const float *queries;  // [..][ldq] or nullptr: Stored queries
  uint32_t ldq;
  const uint32_t *qids;     // Stored ids the caller has checked (below n), or nullptr
  const uint32_t *order;    // position p is query order[p]; nullptr: query first + p
  uint64_t first, npos;     // the run
  const uint32_t *list;     // [cand] ascending VectorIds; cand == 0: the select alone, over no table
  uint64_t cand;
  uint32_t nodes_knob;      // ph_dense_nodes_knob / ph_dense_bytes_knob
  uint64_t bytes_knob;
  const uint32_t *exclude;  // [nq] or nullptr
  const uint32_t *refuse;   // [nq] or nullptr: 0, or the status of a query that gets the empty row
  const uint32_t *changed;  // nullptr, or the word of the run's group: nonzero = every row empty, PH_GROUP_ST_CHANGED
  uint64_t *keys;           // [nq][k] key scratch
  float *D;                 // the table block, plan.table_floats
  uint32_t k;
  uint32_t *out_ids;  // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  hipStream_t stream;
  StepTimes *times;
  int step_table, step_select;
  const char *verbose_prefix;  // what PHNSW_VERBOSE's line says after "[phnsw] " and before "node chunk"
  const char *call;            // the call's name in the error text
};
int ph_table_run(const phnsw_index *ix, PhWorkspace &ws, const PhTableRun &r);
// The request of one routed filtered search (ph_auto_device, filter_auto.hip): per query the exact scan or the graph
// walk, and the scan again for whatever the walk left short.  Device pointers of the caller; rows of k entries.
struct PhAutoCall {
  const float *queries;  // [nq][ldq], or nullptr: Stored queries (qids)
  uint32_t ldq;
  const uint32_t *qids, *exclude;  // [nq] or nullptr
  uint64_t nq;
  const phnsw_search_params *sp;
  PhFilter filter;  // words == nullptr: every vector of the index
  // the label form (phnsw_search_labeled_auto): candidates = the listed vectors of want[q]; filter is then unused
  const phnsw_labels *labels;
  const uint32_t *want;  // [nq]
  // the set form (phnsw_search_labelset_auto): labels with want_first [nq + 1] and want_values [nwant] instead of want;
  // candidates = the listed vectors of the labels of the query's range.  The offsets are not trusted
  const uint32_t *want_first, *want_values;
  uint64_t nwant;
  // the range form (phnsw_search_ranged_auto): candidates = the listed vectors with range_lo[q] <= key <= range_hi[q];
  // filter and labels are then unused
  const phnsw_attr *attr;
  const uint32_t *range_lo, *range_hi;  // [nq]
  // the label-range form (phnsw_search_label_ranged_auto): candidates = the listed vectors with label pair_want[q] and
  // pair_lo[q] <= key <= pair_hi[q]; filter, labels and attr are then unused
  // ... and its set form (phnsw_search_labelset_ranged_auto): label_attr with want_first, want_values and nwant (above)
  // in place of pair_want (nullptr); labels stays nullptr
  const phnsw_label_attr *label_attr;
  const uint32_t *pair_want, *pair_lo, *pair_hi;  // [nq]
  uint32_t k;
  uint64_t scan_below;  // 0 = the library default, UINT64_MAX = always scan (filter_route.h)
  uint32_t *out_ids;    // [nq][k]
  float *out_d;
  uint32_t *out_len, *status;  // [nq]
  uint32_t *out_route;         // [nq] or nullptr
  hipStream_t stream;
};
int ph_auto_device(const phnsw_index *ix, const PhAutoCall &c);
// The request of one exact top-k scan over posting lists (ph_labeled_device, filter_labeled.hip).  Device pointers of
// the caller, enqueued on `stream`; rows of k entries, PH_EMPTY32 / PH_FMAX padded.
struct PhLabeledCall {
  const float *queries;
  uint32_t ldq;
  const uint32_t *qids, *exclude, *want;
  uint64_t nq;
  uint32_t k;
  uint32_t *out_ids;
  float *out_d;
  uint32_t *out_len, *status;
  hipStream_t stream;
  // nullable: the subset form, as PhExactCall::list -- the scan covers queries list[0 .. nq) only (device words); nq is
  // the list's length; queries, qids, exclude, want and every output stay addressed by the query index the list holds
  const uint32_t *list;
};
int ph_labeled_device(const phnsw_index *ix, const phnsw_labels *lb, const PhLabeledCall &c);
// The request of one scan by label sets (ph_labelset_device, filter_labeled.hip): c without `want`, the sets in CSR form
// (device words, untrusted), nwant pairs.  c.list as above: the scan covers the queries of the list, but which query
// owns a pair -- and so which queries get status 8 -- is decided over the whole batch of batch_nq queries (c.nq is the
// list's length with a list, else batch_nq)
struct PhLabelsetCall {
  PhLabeledCall c;
  const uint32_t *want_first, *want_values;
  uint64_t nwant, batch_nq;
};
int ph_labelset_device(const phnsw_index *ix, const phnsw_labels *lb, const PhLabelsetCall &sc);
// out_count_dev[q] = the candidates of query q's set as phnsw_labels_count_set_device counts them, and 0 for a query the
// scan by set refuses (a range that is not sound, or a pair that a lower query holds); owner_scratch [nwant] words
int ph_labels_count_set(const phnsw_labels *lb, const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nq,
                        uint64_t nwant, uint32_t *out_count_dev, uint32_t *owner_scratch, hipStream_t stream);
// a null handle, one made for another index or before the index changed: PHNSW_E_INVALID ("the labels are stale")
int ph_labels_fresh(const phnsw_index *ix, const phnsw_labels *lb, const char *call);
// the index, k, handle and store checks of phnsw_search_exact_labeled, in its order
int ph_labeled_check(const phnsw_index *ix, const phnsw_labels *lb, uint64_t k, const char *call);
// label_of [n] of a handle: the label of every listed vector, PHNSW_LABEL_NONE elsewhere (device words)
const uint32_t *ph_labels_column(const phnsw_labels *lb);
// out_count_dev[q] = the length of the list of want_dev[q] (phnsw_labels_count_device without its checks)
int ph_labels_count(const phnsw_labels *lb, const uint32_t *want_dev, uint64_t nq, uint32_t *out_count_dev, hipStream_t stream);
// The request of one exact top-k scan over the spans of a sorted attribute column (ph_ranged_device, filter_ranged.hip):
// PhLabeledCall with the bounds lo, hi [nq] in place of want; list as there
struct PhRangedCall {
  const float *queries;
  uint32_t ldq;
  const uint32_t *qids, *exclude, *lo, *hi;
  uint64_t nq;
  uint32_t k;
  uint32_t *out_ids;
  float *out_d;
  uint32_t *out_len, *status;
  hipStream_t stream;
  const uint32_t *list;
};
int ph_ranged_device(const phnsw_index *ix, const phnsw_attr *at, const PhRangedCall &c);
// a null handle, one made for another index or before the index changed: PHNSW_E_INVALID, ph_labels_fresh's wording
int ph_attr_fresh(const phnsw_index *ix, const phnsw_attr *at, const char *call);
// ph_labeled_check for an attribute handle: the same checks in the same order
int ph_ranged_check(const phnsw_index *ix, const phnsw_attr *at, uint64_t k, const char *call);
// attr_of [n] of a handle: the key of every listed vector, PHNSW_ATTR_NONE elsewhere (device words)
const uint32_t *ph_attr_column(const phnsw_attr *at);
// out_count_dev[q] = the length of the span of [lo_dev[q], hi_dev[q]] (phnsw_attr_count_device without its checks)
int ph_attr_count(const phnsw_attr *at, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq, uint32_t *out_count_dev,
                  hipStream_t stream);
// What the exact radius search over lists (filter_list_radius.hip) reads of a handle -- a read-only view of its device
// arrays (PhListArrays: what the kernels get), and what the launcher needs beside them; the structs stay private to
// filter_labeled.hip and filter_ranged.hip.  A label handle fills values / first (nlabels), an attribute handle skeys (its
// `listed` entries); both fill ids, and `longest`, the longest list a query of the handle can have (the longest posting
// list; every listed row).  A later handle kind is a view of its own plus a lookup kernel.
struct PhListArrays {
  const uint32_t *values, *first;  // [nlabels] ascending, [nlabels + 1]; nullptr: not a label handle
  uint32_t nlabels;
  const uint32_t *skeys;  // [listed] ascending; nullptr: not an attribute handle
  uint32_t listed;
  const uint32_t *ids;  // the lists' ids: a list is ids + at, len
};
struct PhListView {
  PhListArrays dev;
  uint64_t longest;
  PhCallPool *pool;  // where the scratch sets live: PhLabeledSet (list_scan.h)
  PhResidentMemo *resident;  // under pool->mutex
};
PhListView ph_labels_view(const phnsw_labels *lb);  // filter_labeled.hip
PhListView ph_attr_view(const phnsw_attr *at);      // filter_ranged.hip
// The request of one exact top-k scan over the spans of a column sorted by (label, key) (ph_label_ranged_device,
// filter_label_ranged.hip): PhRangedCall with the wanted label beside the bounds; list as there
struct PhLabelRangedCall {
  const float *queries;
  uint32_t ldq;
  const uint32_t *qids, *exclude, *want, *lo, *hi;
  uint64_t nq;
  uint32_t k;
  uint32_t *out_ids;
  float *out_d;
  uint32_t *out_len, *status;
  hipStream_t stream;
  const uint32_t *list;
};
int ph_label_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const PhLabelRangedCall &c);
// a null handle, one made for another index or before the index changed: PHNSW_E_INVALID, ph_labels_fresh's wording
int ph_label_attr_fresh(const phnsw_index *ix, const phnsw_label_attr *h, const char *call);
// ph_ranged_check for a label-attribute handle: the same checks in the same order
int ph_label_ranged_check(const phnsw_index *ix, const phnsw_label_attr *h, uint64_t k, const char *call);
// pair_of [n] of a handle: the composite of every listed vector, UINT64_MAX elsewhere (device words)
const uint64_t *ph_label_attr_column(const phnsw_label_attr *h);
// out_count_dev[q] = the length of the span of (want_dev[q], [lo_dev[q], hi_dev[q]]) (phnsw_label_attr_count_device
// without its checks)
int ph_label_attr_count(const phnsw_label_attr *h, const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                        uint64_t nq, uint32_t *out_count_dev, hipStream_t stream);
// The request of one scan by label sets and a range (ph_labelset_ranged_device, filter_label_ranged.hip): c without
// `want` -- c.lo and c.hi [batch_nq] are the one range of each query --, the sets in CSR form (device words, untrusted),
// nwant pairs.  c.list, c.nq and batch_nq as in PhLabelsetCall: the claim runs over the whole batch
struct PhLabelsetRangedCall {
  PhLabelRangedCall c;
  const uint32_t *want_first, *want_values;
  uint64_t nwant, batch_nq;
};
int ph_labelset_ranged_device(const phnsw_index *ix, const phnsw_label_attr *h, const PhLabelsetRangedCall &sc);
// out_count_dev[q] = the candidates of query q as phnsw_label_attr_count_set_device counts them, and 0 for a query the
// scan refuses (a range that is not sound, or a pair that a lower query holds); owner_scratch [nwant] words
int ph_label_attr_count_set(const phnsw_label_attr *h, const uint32_t *want_first_dev, const uint32_t *want_values_dev,
                            const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq, uint64_t nwant, uint32_t *out_count_dev,
                            uint32_t *owner_scratch, hipStream_t stream);
void ph_auto_free(phnsw_index *ix);
void ph_dense_free(phnsw_index *ix);  // filter_dense.hip
// the checks the table calls make before they look at another argument: index, k, store kind and row length
int ph_dense_check(const phnsw_index *ix, uint64_t k, const char *call);  // filter_dense.hip
// The candidate list of ONE bitmap as the table calls take it (filter_dense.hip): ph_filter_count's count in head[0],
// the ascending VectorId list and its length in head[1], and -- with Stored queries -- safe [nq] (ids at or past n
// replaced by 0) and refuse [nq] (0, or status 4 for such an id).  Enqueued on `stream` into `pre`, which the caller
// holds: ph_dense_pre_words(words of the store, ph_dense_list_cap(ix), nq) words (dense_plan.h).
struct PhDenseList {
  uint32_t *head, *list, *safe, *refuse;
};
uint32_t ph_dense_list_cap(const phnsw_index *ix);  // the ids a list can hold at most
int ph_dense_list_enqueue(const phnsw_index *ix, const uint32_t *filter, const uint32_t *qids, uint64_t nq, uint32_t *pre,
                          StepTimes *times, int step_count, int step_list, hipStream_t stream, PhDenseList *out);
void ph_grouped_free(phnsw_index *ix);  // filter_grouped.hip
void ph_radius_free(phnsw_index *ix);   // filter_radius.hip
// a scratch set of the index's `radii` pool for a host call that needs only its stream and event (search_radius.hip)
PhCallSet *ph_radius_host_set(phnsw_index *ix);
// the argument checks the exact entry points share (api.hip): index with layers, 1 <= k <= 1024, a store kind the
// distance batch accepts
int ph_exact_check(const phnsw_index *ix, uint64_t k, const char *call);
// locality schedule helpers (group.hip / api.hip)
#define PH_ORDER_MIN 16384u  // shorter query lists run in natural order
#define PH_POS_MIN 256u     // smaller layers carry no cells (their node id is the key)
#define PH_TABLE_ORDER_MIN 2048u  // a plain launch with a dense table and at least this many queries walks in cell order
// a layer whose vector rows do not fit one XCD's L2 (4 MiB) gets a launch of its own in a split
// descent, its queries sorted by the cell they arrive in (PHNSW_SPLIT_BYTES overrides: tuning knob)
#define PH_SPLIT_BYTES (4ull << 20)
static inline bool ph_layer_own_launch(uint64_t n_nodes, uint32_t row_bytes) {
  const char *e = getenv("PHNSW_SPLIT_BYTES");  // read per call: the tests switch it
  const uint64_t limit = (e && atoll(e) > 0) ? (uint64_t)atoll(e) : (uint64_t)PH_SPLIT_BYTES;
  return n_nodes * (uint64_t)row_bytes > limit;
}
int ph_layer_anchor_pos(const phnsw_store *s, PhLayerHost &L);  // bruteforce.hip
bool ph_layer_wants_cells(const phnsw_store *s, uint32_t n_nodes);
int ph_layer_cells_range(const phnsw_store *s, const PhLayerHost &L, uint32_t first, uint32_t count, uint32_t *out_pos);
void ph_store_anchors_free(phnsw_store *s);
int ph_order_by_keys_device(const uint32_t *keys, uint32_t n, uint32_t *order_out, hipStream_t st);
int ph_layer_range_order(PhLayerHost &L, uint32_t first, uint32_t count, const uint32_t **out);
// stable counting sort (group.hip): order_out [n] = the indices 0 .. n-1 by ascending key, equal keys in index order.
// Keys are taken as min(key, bins - 1); start [bins + 1] is scratch.  Async on `st`, no host synchronisation.
int ph_cell_order_device(const uint32_t *keys, uint32_t n, uint32_t bins, uint32_t *start, uint32_t *order_out, hipStream_t st);
// the table order of a launch (tiny.hip): key of query q = pos[arg-min of row q of the natural-order table], the
// counting sort of the queries by it into ws.oorder; points b.order at it and sets b.table_by_query
int ph_tiny_table_order(PhWorkspace &ws, PhSearchArgs &b, const uint32_t *pos, uint32_t bins, hipStream_t stream);

// a search-only row store (f16, i8 or i8q): searched like the f32 store, its rows converted to f32 where a GEMM or a host reads them
static inline bool ph_store_converted(const phnsw_store *s) { return ph_rows_converted(s->kind); }
// the other kinds.  `rows` / `codes` / `codes16` are non-null exactly on an f32 / PQ / shared-codebook PQ store (every
// creator allocates n > 0 rows); a pointer is still what a hipFree or an ownership rule asks
static inline bool ph_store_f32(const phnsw_store *s) { return s->kind == PH_ROWS_F32; }
static inline bool ph_store_bits(const phnsw_store *s) { return ph_rows_bits(s->kind); }  // the 1-bit sign store (rowstore.hip)
static inline bool ph_store_pq(const phnsw_store *s) { return s->kind == PH_ROWS_PQ; }
static inline bool ph_store_pq_shared(const phnsw_store *s) { return s->kind == PH_ROWS_PQ_SHARED; }
// converted stores (rowstore.hip): rows of `ids_dev` (nullptr: rows first .. first + cnt) widened / dequantised into
// [cnt][ld] f32 rows; a range of the store converted into a dense host array
int ph_converted_gather_rows(const phnsw_store *s, const uint32_t *ids_dev, uint32_t first, uint32_t cnt, float *out_dev);
int ph_converted_store_read(const phnsw_store *s, uint64_t first, uint64_t count, float *out);

// dense top layers (tiny.hip): decides how many leading layers of the launch described by `a` run
// against a distance table, fills a.tiny_* and enqueues the table kernels for launch positions
// [0, npos) (position p = query order[p], or p itself) on `stream`.  a.tiny_layers = 0 when unused.
int ph_tiny_prepare(const phnsw_index *ix, PhWorkspace &ws, PhSearchArgs &a, uint32_t max_layers, hipStream_t stream);
// the build's kept table: rows for the hinted queries are made available (computed where missing) and the launch is
// pointed at them; *used = false when the table cannot serve this launch (then ph_tiny_prepare does, per launch)
int ph_build_table_prepare(phnsw_index *ix, PhWorkspace &ws, PhSearchArgs &a, const PhRowHint &h, uint32_t T,
                           hipStream_t stream, bool *used);
void ph_build_table_free(phnsw_index *ix);
size_t ph_tiny_lds_bytes(const PhSearchArgs &a);
bool ph_tiny_matrix_cores(const phnsw_index *ix);  // the table of this index's store is built by the MFMA kernel
uint32_t ph_tiny_layer_count(const phnsw_index *ix, uint32_t n_layers, uint32_t ef);  // leading layers a launch may run densely
uint64_t ph_tiny_max_positions(const phnsw_index *ix, uint32_t n_layers, uint32_t ef);  // 0 = no dense layers for this launch shape
void ph_tiny_free(PhWorkspace &ws);
// one table call of the exact searches over shared allow-lists (ph_table_run) on a workspace of its own: D[p][t] for
// positions [0, npos) -- position p is query order[p], or p itself without an order -- and the VectorIds tnodes[0 .. tn),
// stride = tn rounded up to 64
int ph_tiny_table_chunk(const phnsw_index *ix, PhWorkspace &ws, const float *queries, uint32_t ldq, const uint32_t *qids,
                        const uint32_t *order, uint32_t npos, const uint32_t *tnodes, uint32_t tn, float *D, hipStream_t stream,
                        bool *kept);

// launchers (search.hip)
int ph_search_begin(PhWorkspace &ws, hipStream_t stream);
int ph_search_launch(const phnsw_index *ix, PhWorkspace &ws, PhSearchArgs &a, hipStream_t stream, bool mark_end = true);
// threshold_nn's global-memory queues: `a` complete (visited / ovf / counter / big_q are the caller's, `grid` slots each)
int ph_search_launch_big(const phnsw_index *ix, PhSearchArgs &a, uint32_t grid, hipStream_t stream);
int ph_workspace_order_ensure(PhWorkspace &ws, uint32_t nq);                          // group.hip
int ph_workspace_order_sort(PhWorkspace &ws, uint32_t nq, hipStream_t stream);        // group.hip
void ph_workspace_order_free(PhWorkspace &ws);                                        // group.hip
#define PH_TWO_LAUNCH_MIN 32768u  // batches at least this large descend in two launches
int ph_workspace_ensure(const phnsw_index *ix, PhWorkspace &ws, uint32_t ef, uint32_t ovf_cap);
void ph_workspace_free(PhWorkspace &ws);
size_t ph_tiny_beside_lds(const phnsw_index *ix, const PhSearchArgs &a);  // LDS of one table block that runs beside a search (0: none)
static inline PhRows ph_store_rows(const phnsw_store *s) {
  PhRows r;
  const bool packed = ph_store_converted(s) || ph_store_bits(s);
  r.base = packed ? (const void *)s->packed : (const void *)s->rows;
  r.stride = packed ? s->packed_stride : s->ld * 4u;
  r.kind = s->kind;
  return r;
}
static inline PhDistArgs ph_dist_args(const phnsw_store *s) {
  PhDistArgs d;
  d.rows = ph_store_rows(s);
  d.ld = s->ld;
  d.nv4 = s->ld / 4;
  d.metric = s->metric;
  d.codes = s->codes;
  d.codes16 = s->codes16;
  d.codebook = s->codebook;
  d.m = ph_store_bits(s) ? s->dim : s->pq_m;
  d.ksub = s->pq_ksub;
  d.dsub = s->pq_dsub;
  d.table_f16 = s->pq_table_f16;
  return d;
}
// bytes of one stored row as the search gathers it
static inline uint32_t ph_row_bytes(const phnsw_store *s) { return ph_store_rows(s).stride; }
// an f16, i8, i8q or bits store serves searches only: every other entry point refuses it by name
static inline int ph_search_only_unsupported(const phnsw_store *s, const char *call) {
  if (!s || !(ph_store_converted(s) || ph_store_bits(s))) return 0;
  ph_set_error("%s: not supported on an %s store or an index over one (search-only; use the f32 store)", call,
               ph_rows_name(s->kind));
  return PHNSW_E_UNSUPPORTED;
}
// a bits store serves the plain walk, the distance batch and the re-ranked search alone: every filtered, labelled,
// ranged, collecting or radius walk, every exact scan and every table refuses it by name, on the host, before a launch
// (their kernels read rows through an f32 / f16 / i8 row policy: a 96-byte bit row is none of those)
static inline int ph_bits_unsupported(const phnsw_store *s, const char *call) {
  if (!s || !ph_store_bits(s)) return 0;
  ph_set_error("%s: not supported on a bits store or an index over one (plain search, distance batch and re-ranked "
               "search only; use the f32 store)", call);
  return PHNSW_E_UNSUPPORTED;
}
// the batched search keeps PQ tables in global memory unless PHNSW_PQ_TABLE=lds
static inline bool ph_pq_global_tables() {
  const char *e = getenv("PHNSW_PQ_TABLE");
  return !(e && e[0] == 'l');
}
static inline size_t ph_pq_lds_bytes(const phnsw_store *s) {
  return ph_store_pq(s) ? (size_t)s->pq_m * s->pq_ksub * (s->pq_table_f16 == 2 ? 1 : (s->pq_table_f16 ? 2 : 4)) : 0;
}

// sharded.hip: rank r's share of n items, and a synchronous all-gather of device blocks over any transport
void ph_comm_range(const phnsw_comm *comm, uint32_t r, uint64_t n, uint64_t *chunk, uint64_t *first, uint64_t *count);
int ph_comm_all_gather_device(const phnsw_comm *comm, const void *send_dev, void *recv_dev, uint64_t bytes);

// misc kernels (misc.hip)
int ph_synth_rows(float *rows_dev, uint64_t first, uint64_t count, uint32_t dim, uint32_t ld,
                  uint64_t seed, int normalize, hipStream_t s);
int ph_synth_clustered_rows(float *rows_dev, uint64_t first, uint64_t count, uint32_t dim, uint32_t ld, uint64_t seed,
                            uint32_t n_clusters, float noise, hipStream_t s);
// q_dev == nullptr: the query is Stored(query_id)
int ph_distance_batch(const phnsw_store *st, const float *q_dev, uint32_t query_id, const uint32_t *ids_dev,
                      uint32_t k, float *out_dev, hipStream_t s);
int ph_fill_u32(uint32_t *p, uint32_t v, uint64_t n, hipStream_t s);
// rows of `ef` results -> the leading k of each of the n rows as u64 ids (PH_EMPTY32 -> PHNSW_EMPTY) + distances,
// [n][k] (ph_take_kernel, hostpath.hip)
int ph_take_launch(const uint32_t *ids, const float *d, uint32_t ef, uint32_t k, uint64_t n, uint64_t *ids64, float *dk,
                   hipStream_t s);
int ph_scatter_vec2node(const uint32_t *nodes, uint32_t n, uint32_t *vec2node, hipStream_t s);
int ph_count_nan(const float *rows, uint64_t n_floats, uint32_t *out_count_dev, hipStream_t s);

// deterministic generators shared by definition with the oracle (host + device)
__host__ __device__ inline uint64_t ph_mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ULL;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBULL;
  x ^= x >> 31;
  return x;
}
__host__ __device__ inline uint64_t ph_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((__uint128_t)a * b) >> 64);
#endif
}
__host__ __device__ inline uint64_t ph_feistel_perm(uint64_t i, uint64_t domain, uint64_t key) {
  if (domain <= 1) return 0;
  uint32_t bits = 0;
  while (((uint64_t)1 << bits) < domain) bits++;
  uint32_t h = (bits + 1) / 2;
  if (h == 0) h = 1;
  uint64_t mask = ((uint64_t)1 << h) - 1;
  uint64_t x = i;
  do {
    uint64_t L = x >> h, R = x & mask;
    for (uint32_t r = 0; r < 4; r++) {
      uint64_t f = ph_mix64(R + key * 0x9E3779B97F4A7C15ULL + r * 0xC2B2AE3D27D4EB4FULL) & mask;
      uint64_t nl = R;
      R = L ^ f;
      L = nl;
    }
    x = (L << h) | R;
  } while (x >= domain);
  return x;
}
void ph_shuffle_u64(uint64_t *v, uint64_t n, uint64_t seed);
