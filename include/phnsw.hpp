// phnsw.hpp -- C++ mirror of the reference crate's public surface over the C ABI (phnsw.h).
//
// Names, argument meaning and result ordering follow terminusdb-labs/parallel-hnsw so that
// code (and tests) written against the crate read the same:
//
//   Hnsw::generate(c, vs, bp)                 src/lib.rs:825-830
//   hnsw.search(AbstractVector, sp)           src/lib.rs:663-665  -> Vec<(VectorId, f32)>, (d, id) order
//   hnsw.search_upto(v, sp, upto)             src/lib.rs:654-661
//   hnsw.improve_index(bp) / improve_neighbors / stochastic_recall   src/lib.rs:1501-1513, 1664-1686
//   hnsw.knn(k, probe_depth) / threshold_nn(threshold, probe_depth, initial_search_depth)   :905-962
//   hnsw.layer_count() / entry_vector() / get_layer(i)                src/lib.rs:591-650
//   SearchParameters / BuildParameters with the defaults of src/parameters.rs
//   AbstractVector::Stored(id) / Unstored(&v)                         src/types.rs:40-43
//   QuantizedHnsw::new(centroids, comparator, bp) / search            src/pq.rs:287-364
//
// Where the crate panics (unwrap / assert), these wrappers throw phnsw::Error.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "phnsw.h"

namespace phnsw {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  if (rc != 0) throw Error(rc, phnsw_last_error());
}

using VectorId = uint64_t;  // types.rs:3-4
using NodeId = uint64_t;    // types.rs:5-6
constexpr uint64_t EMPTY = PHNSW_EMPTY;

struct SearchParameters : phnsw_search_params {  // parameters.rs:3-18
  SearchParameters() { phnsw_default_search_params(this); }
  SearchParameters(uint64_t candidates, uint64_t upper, uint64_t probe) {
    number_of_candidates = candidates;
    upper_layer_candidate_count = upper;
    probe_depth = probe;
  }
  SearchParameters(const phnsw_search_params &p) : phnsw_search_params(p) {}  // e.g. bp.optimization.search
};
struct BuildParameters : phnsw_build_params {  // parameters.rs:42-64
  BuildParameters() { phnsw_default_build_params(this); }
};

// AbstractVector<'a, T>  types.rs:40-43
struct AbstractVector {
  bool stored;
  VectorId id;
  const float *vec;
  static AbstractVector Stored(VectorId v) { return {true, v, nullptr}; }
  static AbstractVector Unstored(const float *v) { return {false, 0, v}; }
  static AbstractVector Unstored(const std::vector<float> &v) { return {false, 0, v.data()}; }
};

enum Metric { CosineHalf = PHNSW_METRIC_COSINE_HALF, OneMinusDot = PHNSW_METRIC_ONE_MINUS_DOT, L2 = PHNSW_METRIC_L2 };

// the Comparator of the GPU path: vectors + metric (BigComparator bigvec.rs:38-57)
class Comparator {
 public:
  Comparator(const float *rows, uint64_t n, uint32_t dim, Metric metric = CosineHalf, int device = 0) : dim_(dim), n_(n) {
    check(phnsw_store_create(rows, n, dim, metric, device, &s_));
  }
  explicit Comparator(phnsw_store *adopt) : s_(adopt) {
    check(phnsw_store_info(s_, &n_, &dim_, nullptr, nullptr, nullptr));
  }
  Comparator(const Comparator &) = delete;
  Comparator &operator=(const Comparator &) = delete;
  ~Comparator() { phnsw_store_destroy(s_); }
  // compare_vec for a list of stored vectors in one launch  lib.rs:69-73
  std::vector<float> compare_vec(const AbstractVector &v, const std::vector<VectorId> &ids) const {
    std::vector<float> out(ids.size());
    check(phnsw_distance_batch(s_, v.stored ? nullptr : v.vec, v.id, ids.data(), ids.size(), out.data()));
    return out;
  }
  // more vectors behind the same comparator; returns the first new VectorId
  VectorId append(const float *rows, uint64_t count) {
    uint64_t first = 0;
    check(phnsw_store_append(s_, rows, count, &first));
    n_ += count;
    return first;
  }
  // exact k nearest (ground truth for recall@k)
  std::vector<std::vector<std::pair<VectorId, float>>> bruteforce(const std::vector<float> &queries, uint32_t k) const {
    uint64_t nq = queries.size() / dim_;
    std::vector<uint64_t> ids(nq * k);
    std::vector<float> d(nq * k);
    check(phnsw_bruteforce_topk(s_, queries.data(), nq, k, ids.data(), d.data()));
    std::vector<std::vector<std::pair<VectorId, float>>> r(nq);
    for (uint64_t q = 0; q < nq; q++)
      for (uint32_t j = 0; j < k; j++)
        if (ids[q * k + j] != EMPTY) r[q].push_back({ids[q * k + j], d[q * k + j]});
    return r;
  }
  // the same vectors as IEEE half rows (phnsw_store_create_f16): search-only -- adopt a graph built over this
  // comparator with Hnsw::from_layers(half, layers) and re-rank with Hnsw::search_many_reranked(*this, ...)
  phnsw_store *make_f16() const {
    phnsw_store *h = nullptr;
    check(phnsw_store_create_f16(s_, &h));
    return h;  // wrap it: Comparator half(full.make_f16());
  }
  // the same vectors as int8 rows with one f32 scale per row (phnsw_store_create_i8): search-only as well; re-rank
  // with Hnsw::search_many_reranked_i8(*this, ...)
  phnsw_store *make_i8() const {
    phnsw_store *h = nullptr;
    check(phnsw_store_create_i8(s_, &h));
    return h;  // wrap it: Comparator q8(full.make_i8());
  }
  // the rows of make_i8, searched with an int8 query and integer dot products (phnsw_store_create_i8q): dot-product
  // metrics only; re-rank with Hnsw::search_many_reranked_i8q(*this, ...)
  phnsw_store *make_i8q() const {
    phnsw_store *h = nullptr;
    check(phnsw_store_create_i8q(s_, &h));
    return h;  // wrap it: Comparator q8q(full.make_i8q());
  }
  // the same vectors as one sign bit per component (phnsw_store_create_bits): Hamming distances in sign-vector units,
  // plain searches only; re-rank with Hnsw::search_many_reranked_bits(*this, ...) for true f32 distances
  phnsw_store *make_bits() const {
    phnsw_store *h = nullptr;
    check(phnsw_store_create_bits(s_, &h));
    return h;  // wrap it: Comparator qb(full.make_bits());
  }
  // the sign bits [n][ceil(dim / 32)] of a comparator made by make_bits (phnsw_bits_read)
  void read_bits(std::vector<uint32_t> &words) const {
    words.resize(n_ * ((dim_ + 31u) / 32u));
    check(phnsw_bits_read(s_, words.data()));
  }
  // codes [n][dim] and scales [n] of a comparator made by make_i8 or make_i8q (phnsw_i8_read)
  void read_i8(std::vector<int8_t> &codes, std::vector<float> &scales) const {
    codes.resize(n_ * dim_);
    scales.resize(n_);
    check(phnsw_i8_read(s_, codes.data(), scales.data()));
  }
  uint32_t dim() const { return dim_; }
  uint64_t len() const { return n_; }
  phnsw_store *handle() const { return s_; }

 private:
  phnsw_store *s_ = nullptr;
  uint32_t dim_ = 0;
  uint64_t n_ = 0;
};

// Layer { neighborhood_size, nodes, neighbors }  lib.rs:85-91 (host copy)
struct Layer {
  uint64_t neighborhood_size = 0;
  std::vector<VectorId> nodes;
  std::vector<NodeId> neighbors;
  uint64_t node_count() const { return nodes.size(); }
  VectorId get_vector(NodeId n) const { return nodes[n]; }
  std::vector<NodeId> get_neighbors(NodeId n) const {  // trailing sentinels trimmed  lib.rs:114-148
    std::vector<NodeId> r;
    for (uint64_t k = 0; k < neighborhood_size; k++) {
      NodeId x = neighbors[n * neighborhood_size + k];
      if (x == EMPTY) break;
      r.push_back(x);
    }
    return r;
  }
};

using SearchResult = std::vector<std::pair<VectorId, float>>;

class Labels;
class Attribute;
class LabeledAttribute;

class Hnsw {
 public:
  BuildParameters build_parameters;

  // Hnsw::generate(c, vs, bp, progress)  lib.rs:825-893
  static Hnsw generate(const Comparator &c, const std::vector<VectorId> &vs, const BuildParameters &bp = BuildParameters()) {
    phnsw_index *ix = nullptr;
    check(phnsw_build(c.handle(), vs.data(), vs.size(), &bp, nullptr, nullptr, &ix));
    return Hnsw(ix, &c, bp);
  }
  // Hnsw::generate with every per-node phase split over the ranks of `comm` (BASELINE config 4: one process per
  // GPU; phnsw_comm_rccl_create for the built-in RCCL transport, or two callbacks of the host's own)
  static Hnsw generate_sharded(const Comparator &c, const std::vector<VectorId> &vs, const BuildParameters &bp,
                               const phnsw_comm &comm, phnsw_sharded_stats *stats = nullptr) {
    phnsw_index *ix = nullptr;
    check(phnsw_build_sharded(c.handle(), vs.data(), vs.size(), &bp, &comm, nullptr, nullptr, &ix, stats));
    return Hnsw(ix, &c, bp);
  }
  // adopt layers built elsewhere (top first), e.g. deserialised by the crate
  static Hnsw from_layers(const Comparator &c, const std::vector<Layer> &layers) {
    std::vector<uint64_t> counts, widths;
    std::vector<const uint64_t *> pn, pb;
    for (auto &l : layers) {
      counts.push_back(l.nodes.size());
      widths.push_back(l.neighborhood_size);
      pn.push_back(l.nodes.data());
      pb.push_back(l.neighbors.data());
    }
    phnsw_index *ix = nullptr;
    check(phnsw_index_from_layers(c.handle(), (uint32_t)layers.size(), counts.data(), widths.data(), pn.data(), pb.data(), &ix));
    return Hnsw(ix, &c, BuildParameters());
  }
  static Hnsw deserialize(const std::string &path, const Comparator &c) {  // lib.rs:1693-1698
    phnsw_index *ix = nullptr;
    check(phnsw_index_deserialize(c.handle(), path.c_str(), &ix));
    BuildParameters bp;
    check(phnsw_index_build_params(ix, &bp));
    return Hnsw(ix, &c, bp);
  }
  void serialize(const std::string &path) const { check(phnsw_index_serialize(ix_, path.c_str())); }

  Hnsw(Hnsw &&o) noexcept : build_parameters(o.build_parameters), ix_(o.ix_), c_(o.c_) { o.ix_ = nullptr; }
  Hnsw(const Hnsw &) = delete;
  ~Hnsw() {
    if (ix_) phnsw_index_destroy(ix_);
  }

  // Hnsw::search(v, sp)  lib.rs:663-665
  SearchResult search(const AbstractVector &v, const SearchParameters &sp = SearchParameters()) const {
    return search_upto(v, sp, 0);
  }
  // Hnsw::search_upto(v, sp, upto_layer_from_top)  lib.rs:654-661 (0 = all layers)
  SearchResult search_upto(const AbstractVector &v, const SearchParameters &sp, uint32_t upto) const {
    return search_many({v}, sp, upto)[0];
  }
  // an index over an f16 comparator: search, recompute the results' distances on the f32 comparator `full`, sort by
  // (distance, id), keep the best k  (phnsw_f16_search_batch); queries = nq * dim floats
  std::vector<SearchResult> search_many_reranked(const Comparator &full, const std::vector<float> &queries,
                                                 const SearchParameters &sp, uint64_t k) const {
    const uint64_t nq = queries.size() / c_->dim();
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_f16_search_batch(ix_, full.handle(), queries.data(), nq, &sp, k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // the same over an i8 comparator (phnsw_i8_search_batch)
  std::vector<SearchResult> search_many_reranked_i8(const Comparator &full, const std::vector<float> &queries,
                                                    const SearchParameters &sp, uint64_t k) const {
    const uint64_t nq = queries.size() / c_->dim();
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_i8_search_batch(ix_, full.handle(), queries.data(), nq, &sp, k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // zero-copy form: device pointers of the caller, enqueued on `stream` (phnsw_i8_search_batch_device)
  void search_reranked_i8_device(const Comparator &full, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                 const SearchParameters &sp, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                 uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_i8_search_batch_device(ix_, full.handle(), queries_dev, ldq, nq, &sp, k, out_ids_dev, out_d_dev, out_len_dev,
                                       out_stats_dev, status_dev, stream));
  }
  // the same two over an i8q comparator (phnsw_i8q_search_batch / _device)
  std::vector<SearchResult> search_many_reranked_i8q(const Comparator &full, const std::vector<float> &queries,
                                                     const SearchParameters &sp, uint64_t k) const {
    const uint64_t nq = queries.size() / c_->dim();
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_i8q_search_batch(ix_, full.handle(), queries.data(), nq, &sp, k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  void search_reranked_i8q_device(const Comparator &full, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                  const SearchParameters &sp, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                  uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_i8q_search_batch_device(ix_, full.handle(), queries_dev, ldq, nq, &sp, k, out_ids_dev, out_d_dev, out_len_dev,
                                        out_stats_dev, status_dev, stream));
  }
  // the same two over a bits comparator (phnsw_bits_search_batch / _device): the walk runs on Hamming distances, the
  // returned distances are true f32 distances on `full`
  std::vector<SearchResult> search_many_reranked_bits(const Comparator &full, const std::vector<float> &queries,
                                                      const SearchParameters &sp, uint64_t k) const {
    const uint64_t nq = queries.size() / c_->dim();
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_bits_search_batch(ix_, full.handle(), queries.data(), nq, &sp, k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  void search_reranked_bits_device(const Comparator &full, const float *queries_dev, uint32_t ldq, uint64_t nq,
                                   const SearchParameters &sp, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                   uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_bits_search_batch_device(ix_, full.handle(), queries_dev, ldq, nq, &sp, k, out_ids_dev, out_d_dev, out_len_dev,
                                         out_stats_dev, status_dev, stream));
  }
  // the batched form every GPU caller should use
  std::vector<SearchResult> search_many(const std::vector<AbstractVector> &vs, const SearchParameters &sp,
                                        uint32_t upto = 0) const {
    const uint64_t nq = vs.size(), ef = sp.number_of_candidates;
    std::vector<uint64_t> ids(nq * ef), len(nq);
    std::vector<float> d(nq * ef);
    bool stored = !vs.empty() && vs[0].stored;
    if (stored) {
      std::vector<uint64_t> q(nq);
      for (uint64_t i = 0; i < nq; i++) q[i] = vs[i].id;
      check(phnsw_search_batch_stored(ix_, q.data(), nq, &sp, upto, nullptr, ids.data(), d.data(), len.data(), nullptr));
    } else {
      std::vector<float> q(nq * c_->dim());
      for (uint64_t i = 0; i < nq; i++) std::copy(vs[i].vec, vs[i].vec + c_->dim(), q.begin() + i * c_->dim());
      check(phnsw_search_batch(ix_, q.data(), nq, &sp, upto, nullptr, ids.data(), d.data(), len.data(), nullptr));
    }
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * ef + j], d[i * ef + j]});
    return out;
  }
  // raw queries, the best k results of each: the truncation of lib.rs:1118 done before the transfer
  std::vector<SearchResult> search_many_topk(const std::vector<const float *> &queries, const SearchParameters &sp,
                                             uint64_t k) const {
    const uint64_t nq = queries.size(), dim = c_->dim();
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_search_batch_topk(ix_, q.data(), nullptr, nq, &sp, 0, nullptr, k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // search_many_topk restricted to an allow bitmap over VectorIds (bit v % 32 of word v / 32 set = v may be returned):
  // Layer::closest_vectors' `include` (lib.rs:250-277).  stride_words 0 = one bitmap for all queries, else one per
  // query that far apart; an empty `allow` = the default of set_filter_device.  A post-filter on each layer's queue:
  // expect about density * number_of_candidates results.  strict also removes a disallowed entry vector.  k 0 = all
  // number_of_candidates entries of a row.  Throws on k > number_of_candidates and on an `allow` shorter than its
  // bitmaps: ceil(n / 32) words shared, nq * stride_words words per query
  std::vector<SearchResult> search_many_filtered(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                 uint64_t k, const std::vector<uint32_t> &allow, uint32_t stride_words = 0,
                                                 bool strict = false) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (k == 0) k = sp.number_of_candidates;  // the C call's "whole row"; the buffers below are sized by it
    if (k > sp.number_of_candidates) throw Error(PHNSW_E_INVALID, "search_many_filtered: k exceeds number_of_candidates");
    if (!allow.empty() && (stride_words ? stride_words < words || allow.size() < nq * stride_words : allow.size() < words))
      throw Error(PHNSW_E_INVALID, "search_many_filtered: allow is shorter than its bitmaps (ceil(n / 32) words shared, "
                                   "nq * stride_words per query, stride_words >= ceil(n / 32))");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_search_batch_filtered(ix_, q.data(), nullptr, nq, &sp, 0, nullptr, allow.empty() ? nullptr : allow.data(),
                                      stride_words, strict ? PHNSW_FILTER_STRICT : 0u, k, ids.data(), d.data(), len.data(),
                                      nullptr));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // zero-copy form (phnsw_search_batch_filtered_device): device pointers of the caller, enqueued on `stream`
  void search_filtered_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                              const SearchParameters &sp, uint32_t upto, const uint32_t *exclude_dev, const uint32_t *filter_dev,
                              uint32_t stride_words, bool strict, uint32_t *out_ids_dev, float *out_d_dev,
                              uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_search_batch_filtered_device(ix_, queries_dev, ldq, qids_dev, nq, &sp, upto, exclude_dev, filter_dev,
                                             stride_words, strict ? PHNSW_FILTER_STRICT : 0u, out_ids_dev, out_d_dev,
                                             out_len_dev, out_stats_dev, status_dev, stream));
  }
  // the collecting search (phnsw_search_collect): search_many_topk whose walk of the last layer also keeps the best k
  // ALLOWED rows it evaluates and returns those, where search_many_filtered filters the queue afterwards.  `allow` and
  // stride_words as for search_many_filtered (empty = the default of set_filter_device, else every row).  extend: a hop
  // that improved the kept rows counts as one that did something (PHNSW_COLLECT_EXTEND).  1 <= k <= 64; k may exceed
  // number_of_candidates.  Throws on an `allow` shorter than its bitmaps
  std::vector<SearchResult> search_many_collect(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                uint64_t k, const std::vector<uint32_t> &allow, uint32_t stride_words = 0,
                                                bool extend = false) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (k == 0 || k > 64) throw Error(PHNSW_E_INVALID, "search_many_collect: k must be 1..64");
    if (!allow.empty() && (stride_words ? stride_words < words || allow.size() < nq * stride_words : allow.size() < words))
      throw Error(PHNSW_E_INVALID, "search_many_collect: allow is shorter than its bitmaps (ceil(n / 32) words shared, "
                                   "nq * stride_words per query, stride_words >= ceil(n / 32))");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_search_collect(ix_, q.data(), nullptr, nq, &sp, 0, nullptr, allow.empty() ? nullptr : allow.data(),
                               stride_words, extend ? PHNSW_COLLECT_EXTEND : 0u, k, ids.data(), d.data(), len.data(), nullptr));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // zero-copy form (phnsw_search_collect_device): rows of k u32 ids; enqueued on `stream`, never synchronises it
  void search_collect_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                             const SearchParameters &sp, uint32_t upto, const uint32_t *exclude_dev, const uint32_t *filter_dev,
                             uint32_t stride_words, bool extend, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                             uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_search_collect_device(ix_, queries_dev, ldq, qids_dev, nq, &sp, upto, exclude_dev, filter_dev, stride_words,
                                      extend ? PHNSW_COLLECT_EXTEND : 0u, k, out_ids_dev, out_d_dev, out_len_dev,
                                      out_stats_dev, status_dev, stream));
  }
  // the exact k nearest among the allowed VectorIds (phnsw_search_exact_filtered): a scan of the allow-list instead of
  // the graph walk, recall 1 -- the call for selective filters.  `allow` as for search_many_filtered (empty = the default
  // of set_filter_device, else every vector of the index).  Only vectors of the index are candidates; a disallowed id is
  // never returned; results ascend by (distance, id).  Throws unless 1 <= k <= 1024 and on a short `allow`
  std::vector<SearchResult> search_many_exact_filtered(const std::vector<const float *> &queries, uint64_t k,
                                                       const std::vector<uint32_t> &allow, uint32_t stride_words = 0) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_filtered: k must be 1..1024");
    if (!allow.empty() && (stride_words ? stride_words < words || allow.size() < nq * stride_words : allow.size() < words))
      throw Error(PHNSW_E_INVALID, "search_many_exact_filtered: allow is shorter than its bitmaps (ceil(n / 32) words "
                                   "shared, nq * stride_words per query, stride_words >= ceil(n / 32))");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_search_exact_filtered(ix_, q.data(), nullptr, nq, nullptr, allow.empty() ? nullptr : allow.data(),
                                      stride_words, k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // zero-copy form (phnsw_search_exact_filtered_device): u32 ids [nq][k], enqueued on `stream`
  void search_exact_filtered_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                    const uint32_t *exclude_dev, const uint32_t *filter_dev, uint32_t stride_words, uint64_t k,
                                    uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev,
                                    void *stream) const {
    check(phnsw_search_exact_filtered_device(ix_, queries_dev, ldq, qids_dev, nq, exclude_dev, filter_dev, stride_words, k,
                                             out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
  }
  // search_many_exact_filtered for ONE bitmap shared by all queries, computed as a queries x candidates distance table
  // (phnsw_search_exact_shared): the same results, bit for bit.  `allow`: ceil(n / 32) words, empty = the default of
  // set_filter_device, else every vector of the index.  f32, f16, i8 and i8q stores with rows up to 1536 floats
  std::vector<SearchResult> search_many_exact_shared(const std::vector<const float *> &queries, uint64_t k,
                                                     const std::vector<uint32_t> &allow) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_shared: k must be 1..1024");
    if (!allow.empty() && allow.size() < words)
      throw Error(PHNSW_E_INVALID, "search_many_exact_shared: allow is shorter than one bitmap (ceil(n / 32) words)");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_search_exact_shared(ix_, q.data(), nullptr, nq, nullptr, allow.empty() ? nullptr : allow.data(), k, ids.data(),
                                    d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // zero-copy form (phnsw_search_exact_shared_device): u32 ids [nq][k]; synchronises `stream` once
  void search_exact_shared_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                  const uint32_t *exclude_dev, const uint32_t *filter_dev, uint64_t k, uint32_t *out_ids_dev,
                                  float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_search_exact_shared_device(ix_, queries_dev, ldq, qids_dev, nq, exclude_dev, filter_dev, k, out_ids_dev,
                                           out_d_dev, out_len_dev, status_dev, stream));
  }
  // Exact radius search (phnsw_search_exact_radius): for every query the candidates with d < radius[i] (an f32
  // comparison, strict; a NaN, zero or negative radius matches nothing), ascending by (distance, id).  Candidates, `allow`
  // and stores as for search_many_exact_shared, whose distance tables this computes.  Calls the library once with room
  // for 64 results per query and, when more are inside the radii, once more with exactly that room
  std::vector<SearchResult> search_many_exact_radius(const std::vector<const float *> &queries, const std::vector<float> &radius,
                                                     const std::vector<uint32_t> &allow) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (radius.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_exact_radius: one radius per query");
    if (!allow.empty() && allow.size() < words)
      throw Error(PHNSW_E_INVALID, "search_many_exact_radius: allow is shorter than one bitmap (ceil(n / 32) words)");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> first(nq + 1), ids(std::max<uint64_t>(nq * 64, 1));
    std::vector<float> d(ids.size());
    uint64_t total = 0;
    for (int round = 0; round < 2; round++) {
      check(phnsw_search_exact_radius(ix_, q.data(), nullptr, nq, nullptr, allow.empty() ? nullptr : allow.data(), radius.data(),
                                      ids.size(), first.data(), ids.data(), d.data(), &total));
      if (total <= ids.size()) break;
      ids.resize(total), d.resize(total);
    }
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = first[i]; j < first[i + 1]; j++) out[i].push_back({ids[j], d[j]});
    return out;
  }
  // zero-copy form (phnsw_search_exact_radius_device): u32 ids [cap], u64 first [nq + 1], one u64 total; synchronises
  // `stream` twice (once with cap == 0)
  void search_exact_radius_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                  const uint32_t *exclude_dev, const uint32_t *filter_dev, const float *radius_dev, uint64_t cap,
                                  uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *status_dev,
                                  uint64_t *out_total_dev, void *stream) const {
    check(phnsw_search_exact_radius_device(ix_, queries_dev, ldq, qids_dev, nq, exclude_dev, filter_dev, radius_dev, cap,
                                           out_first_dev, out_ids_dev, out_d_dev, status_dev, out_total_dev, stream));
  }
  // Radius search by graph walk (phnsw_search_batch_radius): the plain descent, then threshold_nn's doubling-queue loop
  // on the bottom layer against radius[i]; approximate.  Per query the nearest max_out (1..1024) of the entries inside
  // the radius; `found` (nullable) gets how many were inside it, which may exceed max_out, and `status` (nullable) the
  // status words -- 6: the queue would pass 1024 entries, an empty row; search_many_exact_radius answers such a query
  std::vector<SearchResult> search_many_radius(const std::vector<const float *> &queries, const std::vector<float> &radius,
                                               const SearchParameters &sp, uint64_t max_out, std::vector<uint64_t> *found = nullptr,
                                               std::vector<uint32_t> *status = nullptr) const {
    const uint64_t nq = queries.size(), dim = c_->dim();
    if (radius.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_radius: one radius per query");
    if (max_out == 0 || max_out > 1024) throw Error(PHNSW_E_INVALID, "search_many_radius: max_out must be 1..1024");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * max_out), len(nq);
    std::vector<float> d(nq * max_out);
    std::vector<uint32_t> st(nq);
    check(phnsw_search_batch_radius(ix_, q.data(), nullptr, nq, &sp, nullptr, radius.data(), max_out, ids.data(), d.data(),
                                    len.data(), nullptr, st.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < std::min(len[i], max_out); j++) out[i].push_back({ids[i * max_out + j], d[i * max_out + j]});
    if (found) *found = len;
    if (status) *status = st;
    return out;
  }
  // zero-copy form (phnsw_search_batch_radius_device): u32 ids [nq][max_out]; enqueued on `stream`
  void search_radius_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                            const SearchParameters &sp, const uint32_t *exclude_dev, const float *radius_dev, uint64_t max_out,
                            uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_stats_dev,
                            uint32_t *status_dev, void *stream) const {
    check(phnsw_search_batch_radius_device(ix_, queries_dev, ldq, qids_dev, nq, &sp, exclude_dev, radius_dev, max_out,
                                           out_ids_dev, out_d_dev, out_len_dev, out_stats_dev, status_dev, stream));
  }
  // search_many_exact_filtered for a TABLE of bitmaps and a selector per query (phnsw_search_exact_grouped): query i may
  // return the vectors of bitmap allow_of[i] (PHNSW_FILTER_ALL: every vector of the index).  The batch is grouped by
  // bitmap on the device and every group runs as search_many_exact_shared runs its batch: the same results, bit for
  // bit.  `allows`: nfilters bitmaps stride_words apart, stride_words >= ceil(n / 32).  Throws on a bad k, table or
  // selector before the library is called
  std::vector<SearchResult> search_many_exact_grouped(const std::vector<const float *> &queries, uint64_t k,
                                                      const std::vector<uint32_t> &allows, uint32_t stride_words,
                                                      const std::vector<uint32_t> &allow_of) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_grouped: k must be 1..1024");
    if (stride_words == 0 || stride_words < words || allows.size() < stride_words || allows.size() % stride_words)
      throw Error(PHNSW_E_INVALID, "search_many_exact_grouped: allows holds whole bitmaps stride_words apart, at least one, "
                                   "stride_words >= ceil(n / 32)");
    const uint64_t nfilters = allows.size() / stride_words;
    if (allow_of.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_exact_grouped: one selector per query");
    for (uint32_t f : allow_of)
      if (f != PHNSW_FILTER_ALL && f >= nfilters)
        throw Error(PHNSW_E_INVALID, "search_many_exact_grouped: a selector outside the table");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    check(phnsw_search_exact_grouped(ix_, q.data(), nullptr, nq, nullptr, allows.data(), stride_words, nfilters, allow_of.data(),
                                     k, ids.data(), d.data(), len.data()));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // zero-copy form (phnsw_search_exact_grouped_device): u32 ids [nq][k]; synchronises `stream` once
  void search_exact_grouped_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                   const uint32_t *exclude_dev, const uint32_t *filters_dev, uint32_t stride_words,
                                   uint64_t nfilters, const uint32_t *filter_of_dev, uint64_t k, uint32_t *out_ids_dev,
                                   float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream) const {
    check(phnsw_search_exact_grouped_device(ix_, queries_dev, ldq, qids_dev, nq, exclude_dev, filters_dev, stride_words, nfilters,
                                            filter_of_dev, k, out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
  }
  // search_many_exact_filtered by row label (phnsw_search_exact_labeled): query i may return the vectors `labels` lists
  // under want[i]; PHNSW_LABEL_NONE or a label nobody carries gives an empty result.  The same results, bit for bit, as
  // the bitmaps {v : label of v == want[i]} give, from posting lists.  Throws on a bad k and on want.size() != queries
  // before the library is called, and on a handle made for another index (defined below, after Labels)
  inline std::vector<SearchResult> search_many_exact_labeled(const std::vector<const float *> &queries, uint64_t k,
                                                             const Labels &labels, const std::vector<uint32_t> &want) const;
  // zero-copy form (phnsw_search_exact_labeled_device): u32 ids [nq][k]; enqueued on `stream`, never synchronises it
  inline void search_exact_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                          uint64_t nq, const uint32_t *exclude_dev, const uint32_t *want_dev, uint64_t k,
                                          uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev,
                                          void *stream) const;
  // search_many_exact_labeled for a SET of labels per query (phnsw_search_exact_labelset): query i may return the vectors
  // `labels` lists under any label of want[i]; an empty set, PHNSW_LABEL_NONE and labels nobody carries give nothing, a
  // label twice counts once.  The same results, bit for bit, as the bitmaps {v : label of v in want[i]} give.  The exact
  // scan; search_many_labelset walks the graph by set, search_many_labelset_auto routes.  Throws on a bad k and on want.size() != queries before the library is called
  inline std::vector<SearchResult> search_many_exact_labelset(const std::vector<const float *> &queries, uint64_t k,
                                                              const Labels &labels,
                                                              const std::vector<std::vector<uint32_t>> &want) const;
  // zero-copy form (phnsw_search_exact_labelset_device): the sets in CSR form, want_first_dev [nq + 1] and want_values_dev
  // [nwant]; status 8 = a range of want_first_dev that is not sound; enqueued on `stream`, never synchronises it
  inline void search_exact_labelset_device(const Labels &labels, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                           uint64_t nq, const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                           const uint32_t *want_values_dev, uint64_t nwant, uint64_t k, uint32_t *out_ids_dev,
                                           float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream) const;
  // search_many_labeled for a SET of labels per query (phnsw_search_batch_labelset): the graph walk of query i restricted to
  // the vectors `labels` lists under any label of want[i] -- the results search_many_filtered gives with the equivalent
  // bitmaps, bit for bit.  A post-filter; strict also removes an entry vector whose label is not wanted.  k = 0: the whole
  // queue.  The membership test is linear in the length of a set.  Throws on want.size() != queries and k >
  // number_of_candidates before the library is called
  inline std::vector<SearchResult> search_many_labelset(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                        const Labels &labels, const std::vector<std::vector<uint32_t>> &want,
                                                        bool strict = false, uint64_t k = 0) const;
  // zero-copy form (phnsw_search_batch_labelset_device): the sets in CSR form; status 8 = a range of want_first_dev that is
  // not sound (that query does not walk); enqueued on `stream`, never synchronises it
  inline void search_batch_labelset_device(const Labels &labels, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                           uint64_t nq, const SearchParameters &sp, uint32_t upto_layers,
                                           const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                           const uint32_t *want_values_dev, uint64_t nwant, uint32_t flags,
                                           uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                           uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const;
  // search_many_labeled_auto for a SET of labels per query (phnsw_search_labelset_auto): per query the scan by set or the
  // strict walk by set, the scan again for short rows; every result holds min(k, candidates) entries, listed vectors of the
  // labels of want[i] only.  scan_below 0 = the library's threshold for sets (20 000 rows of the union, phnsw.h),
  // UINT64_MAX = always scan.  Throws unless 1 <= k <= number_of_candidates and want.size() == queries
  inline std::vector<SearchResult> search_many_labelset_auto(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                             uint64_t k, const Labels &labels,
                                                             const std::vector<std::vector<uint32_t>> &want,
                                                             uint64_t scan_below = 0, std::vector<uint32_t> *routes = nullptr) const;
  // device form (phnsw_search_labelset_auto_device): u32 ids [nq][k]; synchronises `stream` up to twice (phnsw.h)
  inline void search_labelset_auto_device(const Labels &labels, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                          uint64_t nq, const SearchParameters &sp, const uint32_t *exclude_dev,
                                          const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                          uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev,
                                          uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev, void *stream) const;
  // search_many_filtered by row label (phnsw_search_batch_labeled): the graph walk of query i restricted to the vectors
  // `labels` lists under want[i], read from the handle's label column instead of a bitmap per query -- the results
  // search_many_filtered gives with the equivalent bitmaps, bit for bit.  A post-filter: about number_of_candidates *
  // list length / N results; strict also removes an entry vector whose label differs.  k = 0: the whole queue.  Throws on
  // want.size() != queries and k > number_of_candidates before the library is called (defined below, after Labels)
  inline std::vector<SearchResult> search_many_labeled(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                       const Labels &labels, const std::vector<uint32_t> &want,
                                                       bool strict = false, uint64_t k = 0) const;
  // zero-copy form (phnsw_search_batch_labeled_device): rows of number_of_candidates u32 ids; enqueued on `stream`,
  // never synchronises it
  inline void search_batch_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                          uint64_t nq, const SearchParameters &sp, uint32_t upto_layers,
                                          const uint32_t *exclude_dev, const uint32_t *want_dev, uint32_t flags,
                                          uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                          uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const;
  // search_many_collect by row label (phnsw_search_collect_labeled): the rows search_many_collect gives with the
  // equivalent per-query bitmaps, bit for bit, read from the handle's label column
  inline std::vector<SearchResult> search_many_collect_labeled(const std::vector<const float *> &queries,
                                                               const SearchParameters &sp, uint64_t k, const Labels &labels,
                                                               const std::vector<uint32_t> &want, bool extend = false) const;
  // zero-copy form (phnsw_search_collect_labeled_device): rows of k u32 ids; enqueued on `stream`, never synchronises it
  inline void search_collect_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                            const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                            uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                            bool extend, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                            uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev,
                                            void *stream) const;
  // search_many_filtered_auto by row label (phnsw_search_labeled_auto): per query the posting-list scan or the strict
  // walk by label, the scan again for short rows; every result holds min(k, list length) entries, listed vectors of
  // want[i] only.  scan_below 0 = the library's threshold for labels (20 000, phnsw.h), UINT64_MAX = always scan.
  // Throws unless 1 <= k <= number_of_candidates and want.size() == queries
  inline std::vector<SearchResult> search_many_labeled_auto(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                            uint64_t k, const Labels &labels, const std::vector<uint32_t> &want,
                                                            uint64_t scan_below = 0, std::vector<uint32_t> *routes = nullptr) const;
  // device form (phnsw_search_labeled_auto_device): u32 ids [nq][k]; synchronises `stream` up to twice (phnsw.h)
  inline void search_labeled_auto_device(const Labels &labels, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                         uint64_t nq, const SearchParameters &sp, const uint32_t *exclude_dev,
                                         const uint32_t *want_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                         float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev,
                                         void *stream) const;
  // search_many_exact_filtered by a numeric range (phnsw_search_exact_ranged): query i may return the vectors `attr` lists
  // with lo[i] <= key <= hi[i], both ends inclusive, u32 KEYS (attr_key maps i32 and f32 bounds); lo > hi = nothing
  inline std::vector<SearchResult> search_many_exact_ranged(const std::vector<const float *> &queries, uint64_t k,
                                                            const Attribute &attr, const std::vector<uint32_t> &lo,
                                                            const std::vector<uint32_t> &hi) const;
  // zero-copy form (phnsw_search_exact_ranged_device): u32 ids [nq][k]; enqueued on `stream`, never synchronises it
  inline void search_exact_ranged_device(const Attribute &attr, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                         uint64_t nq, const uint32_t *exclude_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                         uint64_t k, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                         uint32_t *status_dev, void *stream) const;
  // search_many_exact_radius with a filter PER QUERY (phnsw_search_exact_radius_labeled / _ranged): for query i the
  // vectors `labels` lists under want[i] -- or `attr` lists with lo[i] <= key <= hi[i] -- with d < radius[i], ascending by
  // (distance, id); the segments of search_many_exact_radius over the equivalent bitmap, bit for bit.  Two library calls
  // at the most, as there
  inline std::vector<SearchResult> search_many_exact_radius_labeled(const std::vector<const float *> &queries,
                                                                    const std::vector<float> &radius, const Labels &labels,
                                                                    const std::vector<uint32_t> &want) const;
  inline std::vector<SearchResult> search_many_exact_radius_ranged(const std::vector<const float *> &queries,
                                                                   const std::vector<float> &radius, const Attribute &attr,
                                                                   const std::vector<uint32_t> &lo,
                                                                   const std::vector<uint32_t> &hi) const;
  // zero-copy forms (phnsw_search_exact_radius_labeled_device / _ranged_device): as search_exact_radius_device;
  // synchronise `stream` once when cap > 0, never with cap == 0
  inline void search_exact_radius_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                                 const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                 const uint32_t *want_dev, const float *radius_dev, uint64_t cap,
                                                 uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                                 uint32_t *status_dev, uint64_t *out_total_dev, void *stream) const;
  inline void search_exact_radius_ranged_device(const Attribute &attr, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                const uint32_t *lo_dev, const uint32_t *hi_dev, const float *radius_dev,
                                                uint64_t cap, uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                                uint32_t *status_dev, uint64_t *out_total_dev, void *stream) const;
  // search_many_filtered by a numeric range (phnsw_search_batch_ranged): the graph walk restricted to the range; k 0 =
  // all number_of_candidates entries of a row
  inline std::vector<SearchResult> search_many_ranged(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                      uint64_t k, const Attribute &attr, const std::vector<uint32_t> &lo,
                                                      const std::vector<uint32_t> &hi, bool strict = false) const;
  // zero-copy form (phnsw_search_batch_ranged_device): lo_dev / hi_dev stay alive until the work on `stream` is done
  inline void search_batch_ranged_device(const Attribute &attr, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                         uint64_t nq, const SearchParameters &sp, uint32_t upto_layers,
                                         const uint32_t *exclude_dev, const uint32_t *lo_dev, const uint32_t *hi_dev, bool strict,
                                         uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_stats_dev,
                                         uint32_t *status_dev, void *stream) const;
  // search_many_filtered_auto by a numeric range (phnsw_search_ranged_auto): per query the span scan or the strict range
  // walk, the scan again for short rows.  scan_below 0 = the library's threshold for ranges (20 000, UNMEASURED: phnsw.h)
  inline std::vector<SearchResult> search_many_ranged_auto(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                           uint64_t k, const Attribute &attr, const std::vector<uint32_t> &lo,
                                                           const std::vector<uint32_t> &hi, uint64_t scan_below = 0,
                                                           std::vector<uint32_t> *routes = nullptr) const;
  // device form (phnsw_search_ranged_auto_device): u32 ids [nq][k]; synchronises `stream` up to twice (phnsw.h)
  inline void search_ranged_auto_device(const Attribute &attr, const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev,
                                        uint64_t nq, const SearchParameters &sp, const uint32_t *exclude_dev,
                                        const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k, uint64_t scan_below,
                                        uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                        uint32_t *status_dev, void *stream) const;
  // search_many_exact_filtered by a label and a numeric range (phnsw_search_exact_label_ranged): query i may return the
  // vectors `attr` lists under want[i] with lo[i] <= key <= hi[i], both ends inclusive, u32 KEYS (attr_key); want
  // LabeledAttribute::NONE, lo > hi or a label nobody carries = nothing
  inline std::vector<SearchResult> search_many_exact_label_ranged(const std::vector<const float *> &queries, uint64_t k,
                                                                  const LabeledAttribute &attr, const std::vector<uint32_t> &want,
                                                                  const std::vector<uint32_t> &lo,
                                                                  const std::vector<uint32_t> &hi) const;
  // zero-copy form (phnsw_search_exact_label_ranged_device): u32 ids [nq][k]; enqueued on `stream`, never synchronises it
  inline void search_exact_label_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                               const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                               const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k,
                                               uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev,
                                               void *stream) const;
  // search_many_filtered by a label and a numeric range (phnsw_search_batch_label_ranged): the graph walk restricted to
  // the pair; k 0 = all number_of_candidates entries of a row
  inline std::vector<SearchResult> search_many_label_ranged(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                            uint64_t k, const LabeledAttribute &attr,
                                                            const std::vector<uint32_t> &want, const std::vector<uint32_t> &lo,
                                                            const std::vector<uint32_t> &hi, bool strict = false) const;
  // zero-copy form (phnsw_search_batch_label_ranged_device): want_dev / lo_dev / hi_dev stay alive until the work on
  // `stream` is done
  inline void search_batch_label_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                               const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                               uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                               const uint32_t *lo_dev, const uint32_t *hi_dev, bool strict, uint32_t *out_ids_dev,
                                               float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_stats_dev,
                                               uint32_t *status_dev, void *stream) const;
  // search_many_filtered_auto by a label and a numeric range (phnsw_search_label_ranged_auto): per query the span scan or
  // the strict walk, the scan again for short rows.  scan_below 0 = the library's threshold (20 000, UNMEASURED: phnsw.h)
  inline std::vector<SearchResult> search_many_label_ranged_auto(const std::vector<const float *> &queries,
                                                                 const SearchParameters &sp, uint64_t k,
                                                                 const LabeledAttribute &attr, const std::vector<uint32_t> &want,
                                                                 const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi,
                                                                 uint64_t scan_below = 0,
                                                                 std::vector<uint32_t> *routes = nullptr) const;
  // device form (phnsw_search_label_ranged_auto_device): u32 ids [nq][k]; synchronises `stream` up to twice (phnsw.h)
  inline void search_label_ranged_auto_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                              const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                              const uint32_t *exclude_dev, const uint32_t *want_dev, const uint32_t *lo_dev,
                                              const uint32_t *hi_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                              float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                              uint32_t *status_dev, void *stream) const;
  // search_many_exact_label_ranged for a SET of labels per query (phnsw_search_exact_labelset_ranged): query i may return
  // the vectors `attr` lists under any label of want[i] with lo[i] <= key <= hi[i], ONE range per query shared by its
  // labels.  A label twice counts once; LabeledAttribute::NONE, a label nobody carries, an empty set and lo > hi = nothing
  inline std::vector<SearchResult> search_many_exact_labelset_ranged(const std::vector<const float *> &queries, uint64_t k,
                                                                     const LabeledAttribute &attr,
                                                                     const std::vector<std::vector<uint32_t>> &want,
                                                                     const std::vector<uint32_t> &lo,
                                                                     const std::vector<uint32_t> &hi) const;
  // zero-copy form (phnsw_search_exact_labelset_ranged_device): the sets in CSR form, want_first_dev [nq + 1] and
  // want_values_dev [nwant]; status 8 = a range of want_first_dev that is not sound or overlaps a lower query's, 4 = a
  // Stored id at or past n (empty rows).  Enqueued on `stream`, never synchronises it
  inline void search_exact_labelset_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                  const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                  const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                                  const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev,
                                                  float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev,
                                                  void *stream) const;
  // search_many_label_ranged for a SET of labels per query (phnsw_search_batch_labelset_ranged): the graph walk restricted
  // to the sets and the ranges; k 0 = all number_of_candidates entries of a row
  inline std::vector<SearchResult> search_many_labelset_ranged(const std::vector<const float *> &queries,
                                                               const SearchParameters &sp, uint64_t k,
                                                               const LabeledAttribute &attr,
                                                               const std::vector<std::vector<uint32_t>> &want,
                                                               const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi,
                                                               bool strict = false) const;
  // zero-copy form (phnsw_search_batch_labelset_ranged_device): the table and the bounds stay alive until the work on
  // `stream` is done; status 8 = a range of want_first_dev that is not inside [0, nwant] or runs backwards
  inline void search_batch_labelset_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                  const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                  uint32_t upto_layers, const uint32_t *exclude_dev,
                                                  const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                                  const uint32_t *lo_dev, const uint32_t *hi_dev, bool strict,
                                                  uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                  uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const;
  // search_many_label_ranged_auto for a SET of labels per query (phnsw_search_labelset_ranged_auto): per query the span
  // scan or the strict walk, the scan again for short rows.  scan_below 0 = the library's threshold (5 000: phnsw.h)
  inline std::vector<SearchResult> search_many_labelset_ranged_auto(const std::vector<const float *> &queries,
                                                                    const SearchParameters &sp, uint64_t k,
                                                                    const LabeledAttribute &attr,
                                                                    const std::vector<std::vector<uint32_t>> &want,
                                                                    const std::vector<uint32_t> &lo,
                                                                    const std::vector<uint32_t> &hi, uint64_t scan_below = 0,
                                                                    std::vector<uint32_t> *routes = nullptr) const;
  // device form (phnsw_search_labelset_ranged_auto_device): u32 ids [nq][k]; synchronises `stream` up to twice (phnsw.h)
  inline void search_labelset_ranged_auto_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                 const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                 const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                                 const uint32_t *want_values_dev, uint64_t nwant, const uint32_t *lo_dev,
                                                 const uint32_t *hi_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                                 float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                                 uint32_t *status_dev, void *stream) const;
  // 0, or the code search_many_exact_shared would refuse this index and k with (phnsw_exact_shared_supported)
  int exact_shared_supported(uint64_t k) const { return phnsw_exact_shared_supported(ix_, k); }
  // candidates of each of nbitmaps device bitmaps (phnsw_filter_count_device): what to choose the search call by
  void filter_count_device(const uint32_t *filter_dev, uint32_t stride_words, uint64_t nbitmaps, uint32_t *out_count_dev,
                           void *stream) const {
    check(phnsw_filter_count_device(ix_, filter_dev, stride_words, nbitmaps, out_count_dev, stream));
  }
  // one filtered call that picks the scan or the graph walk per query and rescans what the walk left short
  // (phnsw_search_filtered_auto): every result holds min(k, candidates) entries, candidates only.  `allow` as for
  // search_many_filtered (empty = the default of set_filter_device, else every vector of the index); scan_below 0 = the
  // library's threshold, UINT64_MAX = always scan.  A graph-routed result is approximate (phnsw.h); routes, when given,
  // receives one PHNSW_ROUTE_* per query.  Throws unless 1 <= k <= number_of_candidates and on a short `allow`
  std::vector<SearchResult> search_many_filtered_auto(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                      uint64_t k, const std::vector<uint32_t> &allow, uint32_t stride_words = 0,
                                                      uint64_t scan_below = 0, std::vector<uint32_t> *routes = nullptr) const {
    const uint64_t nq = queries.size(), dim = c_->dim(), words = (c_->len() + 31) / 32;
    if (k == 0 || k > sp.number_of_candidates)
      throw Error(PHNSW_E_INVALID, "search_many_filtered_auto: k must be 1..number_of_candidates");
    if (!allow.empty() && (stride_words ? stride_words < words || allow.size() < nq * stride_words : allow.size() < words))
      throw Error(PHNSW_E_INVALID, "search_many_filtered_auto: allow is shorter than its bitmaps (ceil(n / 32) words "
                                   "shared, nq * stride_words per query, stride_words >= ceil(n / 32))");
    std::vector<float> q(nq * dim);
    for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
    std::vector<uint64_t> ids(nq * k), len(nq);
    std::vector<float> d(nq * k);
    if (routes) routes->assign(nq, 0u);
    check(phnsw_search_filtered_auto(ix_, q.data(), nullptr, nq, &sp, nullptr, allow.empty() ? nullptr : allow.data(),
                                     stride_words, k, scan_below, ids.data(), d.data(), len.data(),
                                     routes ? routes->data() : nullptr));
    std::vector<SearchResult> out(nq);
    for (uint64_t i = 0; i < nq; i++)
      for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
    return out;
  }
  // device form (phnsw_search_filtered_auto_device): u32 ids [nq][k]; synchronises `stream` up to twice (phnsw.h)
  void search_filtered_auto_device(const float *queries_dev, uint32_t ldq, const uint32_t *qids_dev, uint64_t nq,
                                   const SearchParameters &sp, const uint32_t *exclude_dev, const uint32_t *filter_dev,
                                   uint32_t stride_words, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                   float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev, uint32_t *status_dev,
                                   void *stream) const {
    check(phnsw_search_filtered_auto_device(ix_, queries_dev, ldq, qids_dev, nq, &sp, exclude_dev, filter_dev, stride_words, k,
                                            scan_below, out_ids_dev, out_d_dev, out_len_dev, out_route_dev, status_dev, stream));
  }
  // tombstones (phnsw_index_set_filter_device): the default bitmap of the filtered calls; nullptr clears it
  void set_filter_device(const uint32_t *filter_dev) { check(phnsw_index_set_filter_device(ix_, filter_dev)); }
  // Hnsw::search_instrumented(v, sp) -> (results, index_distance)  lib.rs:667-673
  std::pair<SearchResult, uint64_t> search_instrumented(const AbstractVector &v, const SearchParameters &sp) const {
    const uint64_t ef = sp.number_of_candidates;
    std::vector<uint64_t> ids(ef);
    std::vector<float> d(ef);
    uint64_t len = 0, index = 0;
    check(phnsw_search_instrumented(ix_, v.stored ? nullptr : v.vec, v.stored ? &v.id : nullptr, 1, &sp, ids.data(), d.data(),
                                    &len, &index));
    SearchResult r;
    for (uint64_t j = 0; j < len; j++) r.push_back({ids[j], d[j]});
    return {r, index};
  }
  // improve_index(bp, last_recall: Option<f32>, progress)  lib.rs:1664-1686; NaN = None
  float improve_index(const BuildParameters &bp, float last_recall = __builtin_nanf("")) {
    float r = 0;
    check(phnsw_improve_index(ix_, &bp, last_recall, nullptr, nullptr, &r));
    return r;
  }
  float improve_neighbors(const BuildParameters &bp) {  // lib.rs:1507-1513
    float r = 0;
    check(phnsw_improve_neighbors_upto(ix_, layer_count(), &bp, __builtin_nanf(""), &r));
    return r;
  }
  float stochastic_recall(const phnsw_optimization_params &op) {  // lib.rs:1501-1505
    float r = 0;
    check(phnsw_stochastic_recall_at(ix_, layer_count() - 1, &op, &r));
    return r;
  }
  bool promote_at_layer(uint32_t layer_from_top, const BuildParameters &bp) {  // lib.rs:1273-1427
    int p = 0;
    check(phnsw_promote_at_layer(ix_, layer_from_top, &bp, &p));
    return p != 0;
  }
  void extend_layer(uint32_t layer_from_top, const std::vector<VectorId> &vecs) {  // lib.rs:1039-1068
    check(phnsw_extend_layer(ix_, layer_from_top, vecs.data(), vecs.size()));
  }
  // distance evaluations / hops of every search launched on this index (SearchStats summed)
  std::pair<uint64_t, uint64_t> counters() const {
    uint64_t a = 0, b = 0;
    check(phnsw_index_counters(ix_, &a, &b));
    return {a, b};
  }
  // Hnsw::knn(k, probe_depth)  lib.rs:905-928
  std::vector<std::pair<VectorId, SearchResult>> knn(uint64_t k, uint64_t probe_depth) const {
    Layer bottom = get_layer(0);
    uint64_t n = bottom.node_count();
    std::vector<uint64_t> ids(n * k), len(n);
    std::vector<float> d(n * k);
    check(phnsw_knn(ix_, k, probe_depth, ids.data(), d.data(), len.data()));
    return pack(bottom, ids, d, len, k);
  }
  // Hnsw::threshold_nn(threshold, probe_depth, initial_search_depth)  lib.rs:930-962
  std::vector<std::pair<VectorId, SearchResult>> threshold_nn(float threshold, uint64_t probe_depth,
                                                              uint64_t initial_search_depth, uint64_t max_out = 64) const {
    Layer bottom = get_layer(0);
    uint64_t n = bottom.node_count();
    std::vector<uint64_t> ids(n * max_out), len(n);
    std::vector<float> d(n * max_out);
    check(phnsw_threshold_nn(ix_, threshold, probe_depth, initial_search_depth, max_out, ids.data(), d.data(), len.data()));
    return pack(bottom, ids, d, len, max_out);
  }
  uint32_t layer_count() const { return phnsw_index_layer_count(ix_); }  // lib.rs:643-645
  // get_layer(i): counted from the BOTTOM  lib.rs:604-606
  Layer get_layer(uint32_t i) const { return get_layer_from_top(layer_count() - i - 1); }
  Layer get_layer_from_top(uint32_t i) const {  // lib.rs:617-624
    Layer l;
    uint64_t n = 0;
    check(phnsw_index_layer_info(ix_, i, &n, &l.neighborhood_size));
    l.nodes.resize(n);
    l.neighbors.resize(n * l.neighborhood_size);
    check(phnsw_index_layer_read(ix_, i, l.nodes.data(), l.neighbors.data()));
    return l;
  }
  VectorId entry_vector() const { return get_layer_from_top(0).nodes[0]; }  // lib.rs:638-641
  uint64_t vector_count() const {                                           // lib.rs:592-594
    uint64_t n = 0;
    check(phnsw_index_layer_info(ix_, layer_count() - 1, &n, nullptr));
    return n;
  }
  phnsw_index *handle() const { return ix_; }

 private:
  Hnsw(phnsw_index *ix, const Comparator *c, const BuildParameters &bp) : build_parameters(bp), ix_(ix), c_(c) {}
  static std::vector<std::pair<VectorId, SearchResult>> pack(const Layer &bottom, const std::vector<uint64_t> &ids,
                                                             const std::vector<float> &d, const std::vector<uint64_t> &len,
                                                             uint64_t stride) {
    std::vector<std::pair<VectorId, SearchResult>> out;
    for (uint64_t i = 0; i < bottom.node_count(); i++) {
      SearchResult r;
      for (uint64_t j = 0; j < len[i]; j++) r.push_back({ids[i * stride + j], d[i * stride + j]});
      out.push_back({bottom.nodes[i], r});
    }
    return out;
  }
  phnsw_index *ix_ = nullptr;
  const Comparator *c_ = nullptr;
};

// phnsw_labels: one u32 label per vector of the index's store, turned once into posting lists on the device.  A snapshot:
// after the store or the index has changed a search refuses it as stale.  The Hnsw must outlive its use
class Labels {
 public:
  static constexpr uint32_t NONE = PHNSW_LABEL_NONE;  // a vector that is not listed; a wanted label with an empty result
  Labels(const Hnsw &hnsw, const std::vector<uint32_t> &labels) {
    check(phnsw_labels_create(hnsw.handle(), labels.data(), labels.size(), &lb_));
  }
  // labels_dev: u32 [store n] in device memory, read on `stream`, which is synchronised
  Labels(const Hnsw &hnsw, const uint32_t *labels_dev, uint64_t n, void *stream) {
    check(phnsw_labels_create_device(hnsw.handle(), labels_dev, n, stream, &lb_));
  }
  Labels(const Labels &) = delete;
  Labels &operator=(const Labels &) = delete;
  Labels(Labels &&o) noexcept : lb_(o.lb_) { o.lb_ = nullptr; }
  ~Labels() { phnsw_labels_destroy(lb_); }
  uint64_t label_count() const { return info(1); }
  uint64_t listed() const { return info(2); }
  uint64_t longest() const { return info(3); }
  void count_device(const uint32_t *want_dev, uint64_t nq, uint32_t *out_count_dev, void *stream) const {
    check(phnsw_labels_count_device(lb_, want_dev, nq, out_count_dev, stream));
  }
  // per query the summed list lengths of the distinct labels of its set (CSR, as search_exact_labelset_device)
  void count_set_device(const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nq, uint64_t nwant,
                        uint32_t *out_count_dev, void *stream) const {
    check(phnsw_labels_count_set_device(lb_, want_first_dev, want_values_dev, nq, nwant, out_count_dev, stream));
  }
  phnsw_labels *handle() const { return lb_; }

 private:
  uint64_t info(int which) const {
    uint64_t v[4] = {0, 0, 0, 0};
    check(phnsw_labels_info(lb_, &v[0], &v[1], &v[2], &v[3]));
    return v[which];
  }
  phnsw_labels *lb_ = nullptr;
};

inline std::vector<SearchResult> Hnsw::search_many_exact_labeled(const std::vector<const float *> &queries, uint64_t k,
                                                                 const Labels &labels, const std::vector<uint32_t> &want) const {
  const uint64_t nq = queries.size(), dim = c_->dim();
  if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_labeled: k must be 1..1024");
  if (want.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_exact_labeled: one wanted label per query");
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * k), len(nq);
  std::vector<float> d(nq * k);
  check(phnsw_search_exact_labeled(ix_, labels.handle(), q.data(), nullptr, nq, nullptr, want.data(), k, ids.data(), d.data(),
                                   len.data()));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
  return out;
}
inline void Hnsw::search_exact_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                              const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                              const uint32_t *want_dev, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                              uint32_t *out_len_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_exact_labeled_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, want_dev, k,
                                          out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
}

// the sets of a batch in CSR form, as the calls by set take them; `call` opens the message of what it throws
inline void pack_label_sets(const std::vector<std::vector<uint32_t>> &want, uint64_t nq, const char *call,
                            std::vector<uint32_t> *first, std::vector<uint32_t> *values) {
  if (want.size() != nq) throw Error(PHNSW_E_INVALID, std::string(call) + ": one set of wanted labels per query");
  first->assign(nq + 1, 0);
  values->clear();
  for (uint64_t i = 0; i < nq; i++) {
    values->insert(values->end(), want[i].begin(), want[i].end());
    if (values->size() > 0x7FFFFFFEull) throw Error(PHNSW_E_INVALID, std::string(call) + ": too many wanted labels");
    (*first)[i + 1] = (uint32_t)values->size();
  }
}

inline std::vector<SearchResult> Hnsw::search_many_exact_labelset(const std::vector<const float *> &queries, uint64_t k,
                                                                  const Labels &labels,
                                                                  const std::vector<std::vector<uint32_t>> &want) const {
  const uint64_t nq = queries.size(), dim = c_->dim();
  if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_labelset: k must be 1..1024");
  std::vector<uint32_t> first, values;
  pack_label_sets(want, nq, "search_many_exact_labelset", &first, &values);
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * k), len(nq);
  std::vector<float> d(nq * k);
  check(phnsw_search_exact_labelset(ix_, labels.handle(), q.data(), nullptr, nq, nullptr, first.data(), values.data(), k,
                                    ids.data(), d.data(), len.data()));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
  return out;
}
inline void Hnsw::search_exact_labelset_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                               const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                               const uint32_t *want_first_dev, const uint32_t *want_values_dev, uint64_t nwant,
                                               uint64_t k, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                               uint32_t *status_dev, void *stream) const {
  check(phnsw_search_exact_labelset_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, want_first_dev,
                                           want_values_dev, nwant, k, out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
}

inline std::vector<SearchResult> Hnsw::search_many_labelset(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                            const Labels &labels, const std::vector<std::vector<uint32_t>> &want,
                                                            bool strict, uint64_t k) const {
  const uint64_t nq = queries.size(), dim = c_->dim(), ef = sp.number_of_candidates;
  if (k > ef) throw Error(PHNSW_E_INVALID, "search_many_labelset: k must be 0 or 1..number_of_candidates");
  std::vector<uint32_t> first, values;
  pack_label_sets(want, nq, "search_many_labelset", &first, &values);
  const uint64_t w = k ? k : ef;
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * w), len(nq);
  std::vector<float> d(nq * w);
  check(phnsw_search_batch_labelset(ix_, labels.handle(), q.data(), nullptr, nq, &sp, 0, nullptr, first.data(), values.data(),
                                    strict ? PHNSW_FILTER_STRICT : 0u, k, ids.data(), d.data(), len.data(), nullptr));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * w + j], d[i * w + j]});
  return out;
}
inline void Hnsw::search_batch_labelset_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                               const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                               uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                               const uint32_t *want_values_dev, uint64_t nwant, uint32_t flags,
                                               uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                               uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_batch_labelset_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, &sp, upto_layers, exclude_dev,
                                           want_first_dev, want_values_dev, nwant, flags, out_ids_dev, out_d_dev, out_len_dev,
                                           out_stats_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_labelset_auto(const std::vector<const float *> &queries,
                                                                 const SearchParameters &sp, uint64_t k, const Labels &labels,
                                                                 const std::vector<std::vector<uint32_t>> &want,
                                                                 uint64_t scan_below, std::vector<uint32_t> *routes) const {
  const uint64_t nq = queries.size(), dim = c_->dim();
  if (k == 0 || k > sp.number_of_candidates)
    throw Error(PHNSW_E_INVALID, "search_many_labelset_auto: k must be 1..number_of_candidates");
  std::vector<uint32_t> first, values;
  pack_label_sets(want, nq, "search_many_labelset_auto", &first, &values);
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * k), len(nq);
  std::vector<float> d(nq * k);
  if (routes) routes->assign(nq, 0u);
  check(phnsw_search_labelset_auto(ix_, labels.handle(), q.data(), nullptr, nq, &sp, nullptr, first.data(), values.data(), k,
                                   scan_below, ids.data(), d.data(), len.data(), routes ? routes->data() : nullptr));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
  return out;
}
inline void Hnsw::search_labelset_auto_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                              const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                              const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                              const uint32_t *want_values_dev, uint64_t nwant, uint64_t k, uint64_t scan_below,
                                              uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                              uint32_t *out_route_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_labelset_auto_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, &sp, exclude_dev, want_first_dev,
                                          want_values_dev, nwant, k, scan_below, out_ids_dev, out_d_dev, out_len_dev,
                                          out_route_dev, status_dev, stream));
}

inline std::vector<SearchResult> Hnsw::search_many_labeled(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                           const Labels &labels, const std::vector<uint32_t> &want, bool strict,
                                                           uint64_t k) const {
  const uint64_t nq = queries.size(), dim = c_->dim(), ef = sp.number_of_candidates;
  if (k > ef) throw Error(PHNSW_E_INVALID, "search_many_labeled: k must be 0 or 1..number_of_candidates");
  if (want.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_labeled: one wanted label per query");
  const uint64_t w = k ? k : ef;
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * w), len(nq);
  std::vector<float> d(nq * w);
  check(phnsw_search_batch_labeled(ix_, labels.handle(), q.data(), nullptr, nq, &sp, 0, nullptr, want.data(),
                                   strict ? PHNSW_FILTER_STRICT : 0u, k, ids.data(), d.data(), len.data(), nullptr));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * w + j], d[i * w + j]});
  return out;
}
inline void Hnsw::search_batch_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                              const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                              uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                              uint32_t flags, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                              uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_batch_labeled_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, &sp, upto_layers, exclude_dev,
                                          want_dev, flags, out_ids_dev, out_d_dev, out_len_dev, out_stats_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_collect_labeled(const std::vector<const float *> &queries,
                                                                   const SearchParameters &sp, uint64_t k,
                                                                   const Labels &labels, const std::vector<uint32_t> &want,
                                                                   bool extend) const {
  const uint64_t nq = queries.size(), dim = c_->dim();
  if (k == 0 || k > 64) throw Error(PHNSW_E_INVALID, "search_many_collect_labeled: k must be 1..64");
  if (want.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_collect_labeled: one wanted label per query");
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * k), len(nq);
  std::vector<float> d(nq * k);
  check(phnsw_search_collect_labeled(ix_, labels.handle(), q.data(), nullptr, nq, &sp, 0, nullptr, want.data(),
                                     extend ? PHNSW_COLLECT_EXTEND : 0u, k, ids.data(), d.data(), len.data(), nullptr));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
  return out;
}
inline void Hnsw::search_collect_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                                const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                                bool extend, uint64_t k, uint32_t *out_ids_dev, float *out_d_dev,
                                                uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev,
                                                void *stream) const {
  check(phnsw_search_collect_labeled_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, &sp, upto_layers, exclude_dev,
                                            want_dev, extend ? PHNSW_COLLECT_EXTEND : 0u, k, out_ids_dev, out_d_dev,
                                            out_len_dev, out_stats_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_labeled_auto(const std::vector<const float *> &queries,
                                                                const SearchParameters &sp, uint64_t k, const Labels &labels,
                                                                const std::vector<uint32_t> &want, uint64_t scan_below,
                                                                std::vector<uint32_t> *routes) const {
  const uint64_t nq = queries.size(), dim = c_->dim();
  if (k == 0 || k > sp.number_of_candidates)
    throw Error(PHNSW_E_INVALID, "search_many_labeled_auto: k must be 1..number_of_candidates");
  if (want.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_labeled_auto: one wanted label per query");
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * k), len(nq);
  std::vector<float> d(nq * k);
  if (routes) routes->assign(nq, 0u);
  check(phnsw_search_labeled_auto(ix_, labels.handle(), q.data(), nullptr, nq, &sp, nullptr, want.data(), k, scan_below,
                                  ids.data(), d.data(), len.data(), routes ? routes->data() : nullptr));
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * k + j], d[i * k + j]});
  return out;
}
inline void Hnsw::search_labeled_auto_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                             const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                             const uint32_t *exclude_dev, const uint32_t *want_dev, uint64_t k,
                                             uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                             uint32_t *out_route_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_labeled_auto_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, &sp, exclude_dev, want_dev, k,
                                         scan_below, out_ids_dev, out_d_dev, out_len_dev, out_route_dev, status_dev, stream));
}

// The order-preserving maps onto the u32 keys of an Attribute (phnsw.h, "VALUE TYPES"): the unsigned order of the keys is
// the order of the values.  Apply the same map to the column and to both bounds.  NaN has no place in an order: do not
// map it.  A u32 0xFFFFFFFF and an i32 INT32_MAX are Attribute::NONE in a column, "no upper end" as a bound.
inline uint32_t attr_key(uint32_t x) { return x; }
inline uint32_t attr_key(int32_t x) { return (uint32_t)x ^ 0x80000000u; }
inline uint32_t attr_key(float x) {
  if (x == 0.0f) x = 0.0f;  // -0.0 -> +0.0
  uint32_t bits;
  std::memcpy(&bits, &x, 4);
  return (bits >> 31) ? ~bits : (bits | 0x80000000u);
}

// phnsw_attr: one u32 key per vector of the index's store, sorted once by (key, id) on the device (12 bytes per vector).
// A snapshot like Labels.  The Hnsw must outlive its use
class Attribute {
 public:
  static constexpr uint32_t NONE = PHNSW_ATTR_NONE;  // a row without a value
  Attribute(const Hnsw &hnsw, const std::vector<uint32_t> &keys) {
    check(phnsw_attr_create(hnsw.handle(), keys.data(), keys.size(), &at_));
  }
  // keys_dev: u32 [store n] in device memory, read on `stream`, which is synchronised
  Attribute(const Hnsw &hnsw, const uint32_t *keys_dev, uint64_t n, void *stream) {
    check(phnsw_attr_create_device(hnsw.handle(), keys_dev, n, stream, &at_));
  }
  Attribute(const Attribute &) = delete;
  Attribute &operator=(const Attribute &) = delete;
  Attribute(Attribute &&o) noexcept : at_(o.at_) { o.at_ = nullptr; }
  ~Attribute() { phnsw_attr_destroy(at_); }
  uint64_t listed() const {
    uint64_t v = 0;
    check(phnsw_attr_info(at_, nullptr, &v, nullptr, nullptr));
    return v;
  }
  // the smallest and the largest key (0xFFFFFFFF and 0 when nothing is listed)
  std::pair<uint32_t, uint32_t> key_range() const {
    uint32_t a = 0, b = 0;
    check(phnsw_attr_info(at_, nullptr, nullptr, &a, &b));
    return {a, b};
  }
  void count_device(const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq, uint32_t *out_count_dev, void *stream) const {
    check(phnsw_attr_count_device(at_, lo_dev, hi_dev, nq, out_count_dev, stream));
  }
  phnsw_attr *handle() const { return at_; }

 private:
  phnsw_attr *at_ = nullptr;
};

namespace detail {
// the host forms by range: queries copied to one block, rows of `row` entries cut to their lengths
template <class F>
inline std::vector<SearchResult> ranged_rows(const std::vector<const float *> &queries, uint64_t dim, uint64_t row,
                                             const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi, const char *call,
                                             F run) {
  const uint64_t nq = queries.size();
  if (lo.size() != nq || hi.size() != nq) throw Error(PHNSW_E_INVALID, std::string(call) + ": one lo and one hi per query");
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> ids(nq * row), len(nq);
  std::vector<float> d(nq * row);
  run(q.data(), nq, ids.data(), d.data(), len.data());
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = 0; j < len[i]; j++) out[i].push_back({ids[i * row + j], d[i * row + j]});
  return out;
}
}  // namespace detail

inline std::vector<SearchResult> Hnsw::search_many_exact_ranged(const std::vector<const float *> &queries, uint64_t k,
                                                                const Attribute &attr, const std::vector<uint32_t> &lo,
                                                                const std::vector<uint32_t> &hi) const {
  if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_ranged: k must be 1..1024");
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_exact_ranged",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_exact_ranged(ix_, attr.handle(), q, nullptr, nq, nullptr, lo.data(), hi.data(), k,
                                                               ids, d, len));
                             });
}
inline void Hnsw::search_exact_ranged_device(const Attribute &attr, const float *queries_dev, uint32_t ldq,
                                             const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                             const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k, uint32_t *out_ids_dev,
                                             float *out_d_dev, uint32_t *out_len_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_exact_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, lo_dev, hi_dev, k,
                                         out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
}
namespace detail {
// the two calls of a radius search by list: room for 64 results per query, then exactly the total;
// run(queries [nq][dim], room, first, ids, d, &total)
template <class Run>
std::vector<SearchResult> radius_segments(const std::vector<const float *> &queries, uint64_t dim, const std::vector<float> &radius,
                                          const char *who, Run run) {
  const uint64_t nq = queries.size();
  if (radius.size() != nq) throw Error(PHNSW_E_INVALID, std::string(who) + ": one radius per query");
  std::vector<float> q(nq * dim);
  for (uint64_t i = 0; i < nq; i++) std::copy(queries[i], queries[i] + dim, q.begin() + i * dim);
  std::vector<uint64_t> first(nq + 1), ids(std::max<uint64_t>(nq * 64, 1));
  std::vector<float> d(ids.size());
  uint64_t total = 0;
  for (int round = 0; round < 2; round++) {
    run(q.data(), (uint64_t)ids.size(), first.data(), ids.data(), d.data(), &total);
    if (total <= ids.size()) break;
    ids.resize(total), d.resize(total);
  }
  std::vector<SearchResult> out(nq);
  for (uint64_t i = 0; i < nq; i++)
    for (uint64_t j = first[i]; j < first[i + 1]; j++) out[i].push_back({ids[j], d[j]});
  return out;
}
}  // namespace detail
inline std::vector<SearchResult> Hnsw::search_many_exact_radius_labeled(const std::vector<const float *> &queries,
                                                                        const std::vector<float> &radius, const Labels &labels,
                                                                        const std::vector<uint32_t> &want) const {
  const uint64_t nq = queries.size();
  if (want.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_exact_radius_labeled: one wanted label per query");
  return detail::radius_segments(queries, c_->dim(), radius, "search_many_exact_radius_labeled",
                                 [&](const float *q, uint64_t room, uint64_t *first, uint64_t *ids, float *d, uint64_t *total) {
                                   check(phnsw_search_exact_radius_labeled(ix_, labels.handle(), q, nullptr, nq, nullptr, want.data(),
                                                                           radius.data(), room, first, ids, d, total));
                                 });
}
inline std::vector<SearchResult> Hnsw::search_many_exact_radius_ranged(const std::vector<const float *> &queries,
                                                                       const std::vector<float> &radius, const Attribute &attr,
                                                                       const std::vector<uint32_t> &lo,
                                                                       const std::vector<uint32_t> &hi) const {
  const uint64_t nq = queries.size();
  if (lo.size() != nq || hi.size() != nq) throw Error(PHNSW_E_INVALID, "search_many_exact_radius_ranged: one lo and one hi per query");
  return detail::radius_segments(queries, c_->dim(), radius, "search_many_exact_radius_ranged",
                                 [&](const float *q, uint64_t room, uint64_t *first, uint64_t *ids, float *d, uint64_t *total) {
                                   check(phnsw_search_exact_radius_ranged(ix_, attr.handle(), q, nullptr, nq, nullptr, lo.data(),
                                                                          hi.data(), radius.data(), room, first, ids, d, total));
                                 });
}
inline void Hnsw::search_exact_radius_labeled_device(const Labels &labels, const float *queries_dev, uint32_t ldq,
                                                     const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                     const uint32_t *want_dev, const float *radius_dev, uint64_t cap,
                                                     uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                                     uint32_t *status_dev, uint64_t *out_total_dev, void *stream) const {
  check(phnsw_search_exact_radius_labeled_device(ix_, labels.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, want_dev,
                                                 radius_dev, cap, out_first_dev, out_ids_dev, out_d_dev, status_dev, out_total_dev,
                                                 stream));
}
inline void Hnsw::search_exact_radius_ranged_device(const Attribute &attr, const float *queries_dev, uint32_t ldq,
                                                    const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                    const uint32_t *lo_dev, const uint32_t *hi_dev, const float *radius_dev,
                                                    uint64_t cap, uint64_t *out_first_dev, uint32_t *out_ids_dev, float *out_d_dev,
                                                    uint32_t *status_dev, uint64_t *out_total_dev, void *stream) const {
  check(phnsw_search_exact_radius_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, lo_dev, hi_dev,
                                                radius_dev, cap, out_first_dev, out_ids_dev, out_d_dev, status_dev, out_total_dev,
                                                stream));
}
inline std::vector<SearchResult> Hnsw::search_many_ranged(const std::vector<const float *> &queries, const SearchParameters &sp,
                                                          uint64_t k, const Attribute &attr, const std::vector<uint32_t> &lo,
                                                          const std::vector<uint32_t> &hi, bool strict) const {
  if (k == 0) k = sp.number_of_candidates;  // the C call's "whole row"; the buffers are sized by it
  if (k > sp.number_of_candidates) throw Error(PHNSW_E_INVALID, "search_many_ranged: k exceeds number_of_candidates");
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_ranged",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_batch_ranged(ix_, attr.handle(), q, nullptr, nq, &sp, 0, nullptr, lo.data(),
                                                               hi.data(), strict ? PHNSW_FILTER_STRICT : 0u, k, ids, d, len,
                                                               nullptr));
                             });
}
inline void Hnsw::search_batch_ranged_device(const Attribute &attr, const float *queries_dev, uint32_t ldq,
                                             const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                             uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *lo_dev,
                                             const uint32_t *hi_dev, bool strict, uint32_t *out_ids_dev, float *out_d_dev,
                                             uint32_t *out_len_dev, uint32_t *out_stats_dev, uint32_t *status_dev,
                                             void *stream) const {
  check(phnsw_search_batch_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, &sp, upto_layers, exclude_dev, lo_dev,
                                         hi_dev, strict ? PHNSW_FILTER_STRICT : 0u, out_ids_dev, out_d_dev, out_len_dev,
                                         out_stats_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_ranged_auto(const std::vector<const float *> &queries,
                                                               const SearchParameters &sp, uint64_t k, const Attribute &attr,
                                                               const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi,
                                                               uint64_t scan_below, std::vector<uint32_t> *routes) const {
  if (k == 0 || k > sp.number_of_candidates)
    throw Error(PHNSW_E_INVALID, "search_many_ranged_auto: k must be 1..number_of_candidates");
  if (routes) routes->assign(queries.size(), 0u);
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_ranged_auto",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_ranged_auto(ix_, attr.handle(), q, nullptr, nq, &sp, nullptr, lo.data(), hi.data(),
                                                              k, scan_below, ids, d, len, routes ? routes->data() : nullptr));
                             });
}
inline void Hnsw::search_ranged_auto_device(const Attribute &attr, const float *queries_dev, uint32_t ldq,
                                            const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                            const uint32_t *exclude_dev, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k,
                                            uint64_t scan_below, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                            uint32_t *out_route_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_ranged_auto_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, &sp, exclude_dev, lo_dev, hi_dev, k,
                                        scan_below, out_ids_dev, out_d_dev, out_len_dev, out_route_dev, status_dev, stream));
}

// phnsw_label_attr: one u32 label and one u32 key per vector of the index's store, sorted once on the device by
// (label << 32) | key, then by id (20 bytes per vector).  A vector is listed iff it carries both and the index's bottom
// layer holds it.  A snapshot like Attribute.  The Hnsw must outlive its use
class LabeledAttribute {
 public:
  static constexpr uint32_t NONE = 0xFFFFFFFFu;  // PHNSW_LABEL_NONE and PHNSW_ATTR_NONE: no label, no value
  LabeledAttribute(const Hnsw &hnsw, const std::vector<uint32_t> &labels, const std::vector<uint32_t> &keys) {
    if (labels.size() != keys.size()) throw Error(PHNSW_E_INVALID, "LabeledAttribute: one label and one key per vector");
    check(phnsw_label_attr_create(hnsw.handle(), labels.data(), keys.data(), keys.size(), &h_));
  }
  // labels_dev, keys_dev: u32 [store n] each in device memory, read on `stream`, which is synchronised
  LabeledAttribute(const Hnsw &hnsw, const uint32_t *labels_dev, const uint32_t *keys_dev, uint64_t n, void *stream) {
    check(phnsw_label_attr_create_device(hnsw.handle(), labels_dev, keys_dev, n, stream, &h_));
  }
  LabeledAttribute(const LabeledAttribute &) = delete;
  LabeledAttribute &operator=(const LabeledAttribute &) = delete;
  LabeledAttribute(LabeledAttribute &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~LabeledAttribute() { phnsw_label_attr_destroy(h_); }
  uint64_t listed() const {
    uint64_t v = 0;
    check(phnsw_label_attr_info(h_, nullptr, &v, nullptr, nullptr));
    return v;
  }
  // the distinct labels that list a row, and the most rows listed under one of them
  std::pair<uint64_t, uint64_t> label_stats() const {
    uint64_t a = 0, b = 0;
    check(phnsw_label_attr_info(h_, nullptr, nullptr, &a, &b));
    return {a, b};
  }
  void count_device(const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t nq, uint32_t *out_count_dev,
                    void *stream) const {
    check(phnsw_label_attr_count_device(h_, want_dev, lo_dev, hi_dev, nq, out_count_dev, stream));
  }
  // per query the summed span lengths of the distinct labels of its set inside its range (CSR, as
  // search_exact_labelset_ranged_device); 0 for a query that call would refuse
  void count_set_device(const uint32_t *want_first_dev, const uint32_t *want_values_dev, const uint32_t *lo_dev,
                        const uint32_t *hi_dev, uint64_t nq, uint64_t nwant, uint32_t *out_count_dev, void *stream) const {
    check(phnsw_label_attr_count_set_device(h_, want_first_dev, want_values_dev, lo_dev, hi_dev, nq, nwant, out_count_dev, stream));
  }
  phnsw_label_attr *handle() const { return h_; }

 private:
  phnsw_label_attr *h_ = nullptr;
};

inline std::vector<SearchResult> Hnsw::search_many_exact_label_ranged(const std::vector<const float *> &queries, uint64_t k,
                                                                      const LabeledAttribute &attr,
                                                                      const std::vector<uint32_t> &want,
                                                                      const std::vector<uint32_t> &lo,
                                                                      const std::vector<uint32_t> &hi) const {
  if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_label_ranged: k must be 1..1024");
  if (want.size() != queries.size()) throw Error(PHNSW_E_INVALID, "search_many_exact_label_ranged: one wanted label per query");
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_exact_label_ranged",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_exact_label_ranged(ix_, attr.handle(), q, nullptr, nq, nullptr, want.data(),
                                                                     lo.data(), hi.data(), k, ids, d, len));
                             });
}
inline void Hnsw::search_exact_label_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                   const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                   const uint32_t *want_dev, const uint32_t *lo_dev, const uint32_t *hi_dev,
                                                   uint64_t k, uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                   uint32_t *status_dev, void *stream) const {
  check(phnsw_search_exact_label_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, want_dev, lo_dev,
                                               hi_dev, k, out_ids_dev, out_d_dev, out_len_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_label_ranged(const std::vector<const float *> &queries,
                                                                const SearchParameters &sp, uint64_t k,
                                                                const LabeledAttribute &attr, const std::vector<uint32_t> &want,
                                                                const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi,
                                                                bool strict) const {
  if (k == 0) k = sp.number_of_candidates;  // the C call's "whole row"; the buffers are sized by it
  if (k > sp.number_of_candidates) throw Error(PHNSW_E_INVALID, "search_many_label_ranged: k exceeds number_of_candidates");
  if (want.size() != queries.size()) throw Error(PHNSW_E_INVALID, "search_many_label_ranged: one wanted label per query");
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_label_ranged",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_batch_label_ranged(ix_, attr.handle(), q, nullptr, nq, &sp, 0, nullptr,
                                                                     want.data(), lo.data(), hi.data(),
                                                                     strict ? PHNSW_FILTER_STRICT : 0u, k, ids, d, len, nullptr));
                             });
}
inline void Hnsw::search_batch_label_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                   const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                   uint32_t upto_layers, const uint32_t *exclude_dev, const uint32_t *want_dev,
                                                   const uint32_t *lo_dev, const uint32_t *hi_dev, bool strict,
                                                   uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                   uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_batch_label_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, &sp, upto_layers, exclude_dev,
                                               want_dev, lo_dev, hi_dev, strict ? PHNSW_FILTER_STRICT : 0u, out_ids_dev, out_d_dev,
                                               out_len_dev, out_stats_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_label_ranged_auto(const std::vector<const float *> &queries,
                                                                     const SearchParameters &sp, uint64_t k,
                                                                     const LabeledAttribute &attr,
                                                                     const std::vector<uint32_t> &want,
                                                                     const std::vector<uint32_t> &lo,
                                                                     const std::vector<uint32_t> &hi, uint64_t scan_below,
                                                                     std::vector<uint32_t> *routes) const {
  if (k == 0 || k > sp.number_of_candidates)
    throw Error(PHNSW_E_INVALID, "search_many_label_ranged_auto: k must be 1..number_of_candidates");
  if (want.size() != queries.size()) throw Error(PHNSW_E_INVALID, "search_many_label_ranged_auto: one wanted label per query");
  if (routes) routes->assign(queries.size(), 0u);
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_label_ranged_auto",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_label_ranged_auto(ix_, attr.handle(), q, nullptr, nq, &sp, nullptr, want.data(),
                                                                    lo.data(), hi.data(), k, scan_below, ids, d, len,
                                                                    routes ? routes->data() : nullptr));
                             });
}
inline void Hnsw::search_label_ranged_auto_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                  const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                  const uint32_t *exclude_dev, const uint32_t *want_dev, const uint32_t *lo_dev,
                                                  const uint32_t *hi_dev, uint64_t k, uint64_t scan_below, uint32_t *out_ids_dev,
                                                  float *out_d_dev, uint32_t *out_len_dev, uint32_t *out_route_dev,
                                                  uint32_t *status_dev, void *stream) const {
  check(phnsw_search_label_ranged_auto_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, &sp, exclude_dev, want_dev, lo_dev,
                                              hi_dev, k, scan_below, out_ids_dev, out_d_dev, out_len_dev, out_route_dev, status_dev,
                                              stream));
}

inline std::vector<SearchResult> Hnsw::search_many_exact_labelset_ranged(const std::vector<const float *> &queries, uint64_t k,
                                                                         const LabeledAttribute &attr,
                                                                         const std::vector<std::vector<uint32_t>> &want,
                                                                         const std::vector<uint32_t> &lo,
                                                                         const std::vector<uint32_t> &hi) const {
  if (k == 0 || k > 1024) throw Error(PHNSW_E_INVALID, "search_many_exact_labelset_ranged: k must be 1..1024");
  std::vector<uint32_t> first, values;
  pack_label_sets(want, queries.size(), "search_many_exact_labelset_ranged", &first, &values);
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_exact_labelset_ranged",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_exact_labelset_ranged(ix_, attr.handle(), q, nullptr, nq, nullptr, first.data(),
                                                                        values.data(), lo.data(), hi.data(), k, ids, d, len));
                             });
}
inline void Hnsw::search_exact_labelset_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                      const uint32_t *qids_dev, uint64_t nq, const uint32_t *exclude_dev,
                                                      const uint32_t *want_first_dev, const uint32_t *want_values_dev,
                                                      uint64_t nwant, const uint32_t *lo_dev, const uint32_t *hi_dev, uint64_t k,
                                                      uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                      uint32_t *status_dev, void *stream) const {
  check(phnsw_search_exact_labelset_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, exclude_dev, want_first_dev,
                                                  want_values_dev, nwant, lo_dev, hi_dev, k, out_ids_dev, out_d_dev, out_len_dev,
                                                  status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_labelset_ranged(const std::vector<const float *> &queries,
                                                                   const SearchParameters &sp, uint64_t k,
                                                                   const LabeledAttribute &attr,
                                                                   const std::vector<std::vector<uint32_t>> &want,
                                                                   const std::vector<uint32_t> &lo, const std::vector<uint32_t> &hi,
                                                                   bool strict) const {
  if (k == 0) k = sp.number_of_candidates;  // the C call's "whole row"; the buffers are sized by it
  if (k > sp.number_of_candidates) throw Error(PHNSW_E_INVALID, "search_many_labelset_ranged: k exceeds number_of_candidates");
  std::vector<uint32_t> first, values;
  pack_label_sets(want, queries.size(), "search_many_labelset_ranged", &first, &values);
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_labelset_ranged",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_batch_labelset_ranged(ix_, attr.handle(), q, nullptr, nq, &sp, 0, nullptr,
                                                                        first.data(), values.data(), lo.data(), hi.data(),
                                                                        strict ? PHNSW_FILTER_STRICT : 0u, k, ids, d, len, nullptr));
                             });
}
inline void Hnsw::search_batch_labelset_ranged_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                      const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                      uint32_t upto_layers, const uint32_t *exclude_dev,
                                                      const uint32_t *want_first_dev, const uint32_t *want_values_dev,
                                                      uint64_t nwant, const uint32_t *lo_dev, const uint32_t *hi_dev, bool strict,
                                                      uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                      uint32_t *out_stats_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_batch_labelset_ranged_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, &sp, upto_layers, exclude_dev,
                                                  want_first_dev, want_values_dev, nwant, lo_dev, hi_dev,
                                                  strict ? PHNSW_FILTER_STRICT : 0u, out_ids_dev, out_d_dev, out_len_dev,
                                                  out_stats_dev, status_dev, stream));
}
inline std::vector<SearchResult> Hnsw::search_many_labelset_ranged_auto(const std::vector<const float *> &queries,
                                                                        const SearchParameters &sp, uint64_t k,
                                                                        const LabeledAttribute &attr,
                                                                        const std::vector<std::vector<uint32_t>> &want,
                                                                        const std::vector<uint32_t> &lo,
                                                                        const std::vector<uint32_t> &hi, uint64_t scan_below,
                                                                        std::vector<uint32_t> *routes) const {
  if (k == 0 || k > sp.number_of_candidates)
    throw Error(PHNSW_E_INVALID, "search_many_labelset_ranged_auto: k must be 1..number_of_candidates");
  std::vector<uint32_t> first, values;
  pack_label_sets(want, queries.size(), "search_many_labelset_ranged_auto", &first, &values);
  if (routes) routes->assign(queries.size(), 0u);
  return detail::ranged_rows(queries, c_->dim(), k, lo, hi, "search_many_labelset_ranged_auto",
                             [&](const float *q, uint64_t nq, uint64_t *ids, float *d, uint64_t *len) {
                               check(phnsw_search_labelset_ranged_auto(ix_, attr.handle(), q, nullptr, nq, &sp, nullptr,
                                                                       first.data(), values.data(), lo.data(), hi.data(), k,
                                                                       scan_below, ids, d, len, routes ? routes->data() : nullptr));
                             });
}
inline void Hnsw::search_labelset_ranged_auto_device(const LabeledAttribute &attr, const float *queries_dev, uint32_t ldq,
                                                     const uint32_t *qids_dev, uint64_t nq, const SearchParameters &sp,
                                                     const uint32_t *exclude_dev, const uint32_t *want_first_dev,
                                                     const uint32_t *want_values_dev, uint64_t nwant, const uint32_t *lo_dev,
                                                     const uint32_t *hi_dev, uint64_t k, uint64_t scan_below,
                                                     uint32_t *out_ids_dev, float *out_d_dev, uint32_t *out_len_dev,
                                                     uint32_t *out_route_dev, uint32_t *status_dev, void *stream) const {
  check(phnsw_search_labelset_ranged_auto_device(ix_, attr.handle(), queries_dev, ldq, qids_dev, nq, &sp, exclude_dev,
                                                 want_first_dev, want_values_dev, nwant, lo_dev, hi_dev, k, scan_below, out_ids_dev,
                                                 out_d_dev, out_len_dev, out_route_dev, status_dev, stream));
}

// QuantizedHnsw  pq.rs:120-131, 287-364 (per-sub-space codebooks, u8 codes)
class QuantizedHnsw {
 public:
  // QuantizedHnsw::new(number_of_centroids, comparator, bp)
  QuantizedHnsw(uint32_t number_of_centroids, const Comparator &full, uint32_t m, BuildParameters bp = no_promotion(),
                uint64_t seed = 0, bool table_f16 = false)
      : full_(&full) {
    phnsw_store *ps = nullptr;
    check(phnsw_store_create_pq(full.handle(), m, number_of_centroids, seed, &ps));
    codes_.reset(new Comparator(ps));
    if (table_f16) check(phnsw_pq_set_table_f16(ps, 1));
    std::vector<VectorId> vs(full.len());
    for (uint64_t i = 0; i < vs.size(); i++) vs[i] = i;
    hnsw_.reset(new Hnsw(Hnsw::generate(*codes_, vs, bp)));
  }
  // QuantizedHnsw::search(v, sp)  pq.rs:346-364 (quantize_query = the reference's symmetric form)
  SearchResult search(const float *v, const SearchParameters &sp, bool quantize_query = false) const {
    const uint64_t ef = sp.number_of_candidates;
    std::vector<uint64_t> ids(ef), len(1);
    std::vector<float> d(ef);
    check(phnsw_pq_search_batch(hnsw_->handle(), full_->handle(), v, 1, &sp, quantize_query, ids.data(), d.data(), len.data(), nullptr));
    SearchResult r;
    for (uint64_t j = 0; j < len[0]; j++) r.push_back({ids[j], d[j]});
    return r;
  }
  uint64_t vector_count() const { return hnsw_->vector_count(); }
  static BuildParameters no_promotion() {
    BuildParameters bp;
    bp.promote = 0;
    return bp;
  }

 private:
  const Comparator *full_;
  std::unique_ptr<Comparator> codes_;
  std::unique_ptr<Hnsw> hnsw_;
};

}  // namespace phnsw
