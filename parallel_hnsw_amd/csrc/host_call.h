// The unpipelined host form of the filtered and exact calls, written once (phnsw_search_exact_shared, _exact_grouped,
// _exact_labeled, _exact_labelset, _batch_labeled, _batch_labelset, _filtered_auto, _labeled_auto and _labelset_auto): host
// arrays in, one stream of the call's scratch set (call_set.h), host arrays out.  ph_search_host (hostpath.hip) is another
// thing: pinned, chunked, two streams.
//
// A caller checks its arguments (ph_stored_ids_check among them, where its order of checks has it), acquires a set by
// its owner's policy and then
//   PhHostCall h(pool, set);
//   h.stage_in(...)    the set's stream; queries padded to the store's row length; `small`; the result blocks
//   ... its own uploads into h.extra() or h.blocks, h.fill(call), its run on h.st ...
//   h.finish(...)      the take, the downloads, the synchronisation
//
// `small` is one layout for every form, [nq] words each unless said:
//   qid | exclude | len | status | the caller's extras (h.extra(): those the host reads back first)
#pragma once
#include <algorithm>

#include "call_set.h"

// device blocks of one host call: handed back only after the stream they were used on has drained, whichever way the
// call ends
struct HostBlocks {
  hipStream_t stream;
  std::vector<void *> blocks;
  template <class T>
  int alloc(T **p, size_t bytes) {
    void *v = nullptr;
    PH_HIP(ph_pool_alloc(&v, std::max<size_t>(bytes, 4)));
    blocks.push_back(v);
    *p = (T *)v;
    return 0;
  }
  ~HostBlocks() {
    hipStreamSynchronize(stream);
    for (void *b : blocks) ph_pool_free(b);
  }
};

// the Stored query ids of a host form against the store's n; `who` opens the message ("search" or the call's name)
static inline int ph_stored_ids_check(const uint64_t *qids, uint64_t nq, uint64_t n, const char *who, bool name_query = false) {
  for (uint64_t i = 0; qids && i < nq; i++)
    if (qids[i] >= n) {
      if (name_query)
        ph_set_error("%s: query %llu: stored query id %llu out of range", who, (unsigned long long)i, (unsigned long long)qids[i]);
      else
        ph_set_error("%s: stored query id %llu out of range", who, (unsigned long long)qids[i]);
      return PHNSW_E_INVALID;
    }
  return 0;
}

struct PhHostCall {
  // THE LIFETIME RULE OF A HOST CALL LIVES HERE, in the order of these three declarations (members are destroyed in
  // reverse): `blocks` goes first -- it drains the stream, then returns the device blocks; then `guard` records the
  // set's event and hands the set back; the host staging vectors, which asynchronous copies read and write, go last.
  // So it holds on every return path of every form, and no call site declares any of the three.  h_list is for host
  // words of a caller's own that a copy reads (the walk's redo list): upload_list() is the only way they reach the
  // stream, so they too outlive the drain.
  std::vector<uint32_t> h_in, h_out, h_list;
  PhSetGuard guard;
  HostBlocks blocks;

  hipStream_t st = nullptr;  // the set's own
  uint64_t nq = 0;
  uint32_t ld = 0, row = 0, k = 0;
  const float *queries = nullptr;             // [nq][ld] or nullptr: Stored queries
  const uint32_t *qids = nullptr, *exclude = nullptr;  // inside small, or nullptr
  uint32_t *small = nullptr;
  uint32_t *ids = nullptr;  // [nq][row]: what the call writes
  float *d = nullptr;
  uint64_t *ids64 = nullptr;  // [nq][k]: what the take leaves of it
  float *dk = nullptr;
  bool words_enqueued = false, taken = false;

  PhHostCall(PhCallPool &pool, PhCallSet *set) : guard{pool, set, set->stream}, blocks{set->stream, {}} {}

  // extra_words: words of `small` behind the common [4][nq]; the first read_extra * nq of them come back to the host
  // with len and status.  The call stages rows of `row` entries, the host gets the leading k of each.
  int stage_in(const phnsw_store *s, const float *queries_h, const uint64_t *qids_h, const uint64_t *exclude_h, uint64_t nq_,
               size_t extra_words, uint32_t read_extra, uint32_t row_, uint32_t k_) {
    PhCallSet *const set = guard.set;
    if (!set->stream) {
      hipError_t e = hipStreamCreateWithFlags(&set->stream, hipStreamNonBlocking);
      if (e != hipSuccess) return ph_hip_fail(e, "host path: stream", __FILE__, __LINE__);
    }
    st = guard.stream = blocks.stream = set->stream;
    nq = nq_, ld = s->ld, row = row_, k = k_;
    h_out.resize((2u + read_extra) * nq);
    if (queries_h) {  // rows padded to the store's row length
      float *q = nullptr;
      PH_TRY(blocks.alloc(&q, (size_t)nq * ld * 4u));
      if (ld != s->dim) {
        PH_HIP(hipMemsetAsync(q, 0, (size_t)nq * ld * 4u, st));
        PH_HIP(hipMemcpy2DAsync(q, (size_t)ld * 4u, queries_h, (size_t)s->dim * 4u, (size_t)s->dim * 4u, nq, hipMemcpyHostToDevice, st));
      } else {
        PH_HIP(hipMemcpyAsync(q, queries_h, (size_t)nq * ld * 4u, hipMemcpyHostToDevice, st));
      }
      queries = q;
    }
    PH_TRY(blocks.alloc(&small, ((size_t)nq * 4u + extra_words) * 4u));
    if (qids_h || exclude_h) {
      h_in.resize(2u * nq);
      if (qids_h)
        for (uint64_t i = 0; i < nq; i++) h_in[i] = (uint32_t)qids_h[i];
      if (exclude_h)
        for (uint64_t i = 0; i < nq; i++) h_in[nq + i] = exclude_h[i] >= s->n ? PH_EMPTY32 : (uint32_t)exclude_h[i];
      PH_HIP(hipMemcpyAsync(small, h_in.data(), (size_t)nq * 2u * 4u, hipMemcpyHostToDevice, st));
      if (qids_h) qids = small;
      if (exclude_h) exclude = small + nq;
    }
    PH_TRY(blocks.alloc(&ids, (size_t)nq * row * 4u));
    PH_TRY(blocks.alloc(&d, (size_t)nq * row * 4u));
    PH_TRY(blocks.alloc(&ids64, (size_t)nq * k * 8u));
    PH_TRY(blocks.alloc(&dk, (size_t)nq * k * 4u));
    return 0;
  }
  uint32_t *extra() const { return small + 4u * nq; }
  // the fields every request struct of these calls has
  template <class Call>
  void fill(Call &c) const {
    c.queries = queries, c.ldq = queries ? ld : 0u, c.qids = qids, c.exclude = exclude, c.nq = nq;
    c.out_ids = ids, c.out_d = d, c.out_len = small + 2u * nq, c.status = small + 3u * nq;
    c.stream = st;
  }

  // h_list -> dev; the caller changes h_list again only after a sync()
  int upload_list(uint32_t *dev) {
    PH_HIP(hipMemcpyAsync(dev, h_list.data(), h_list.size() * 4u, hipMemcpyHostToDevice, st));
    return 0;
  }
  // len | status | the read_extra words, as they stand on the stream now; valid after sync()
  int download_words() {
    PH_HIP(hipMemcpyAsync(h_out.data(), small + 2u * nq, h_out.size() * 4u, hipMemcpyDeviceToHost, st));
    words_enqueued = true;
    return 0;
  }
  int sync() {
    PH_HIP(hipStreamSynchronize(st));
    return 0;
  }
  uint32_t len(uint64_t i) const { return h_out[i]; }
  uint32_t status(uint64_t i) const { return h_out[nq + i]; }
  uint32_t read_extra(uint32_t word, uint64_t i) const { return h_out[(2u + word) * nq + i]; }

  // u32 -> u64 ids, 0xFFFFFFFF -> PHNSW_EMPTY: the leading k of every staged row.  finish() does it; a caller that reads
  // the words first (grouped: a status keeps the rows from being copied out) enqueues it in front of that read
  int take() {
    PH_TRY(ph_take_launch(ids, d, row, k, nq, ids64, dk, st));
    taken = true;
    return 0;
  }
  // the take, the words unless the caller has read them already, the rows, the synchronisation; out_len (nullable: the
  // caller widens len itself) gets min(len, k)
  int finish(uint64_t *out_ids, float *out_d, uint64_t *out_len) {
    if (!taken) PH_TRY(take());
    if (!words_enqueued) PH_TRY(download_words());
    PH_HIP(hipMemcpyAsync(out_ids, ids64, (size_t)nq * k * 8u, hipMemcpyDeviceToHost, st));
    PH_HIP(hipMemcpyAsync(out_d, dk, (size_t)nq * k * 4u, hipMemcpyDeviceToHost, st));
    PH_TRY(sync());
    if (out_len)
      for (uint64_t i = 0; i < nq; i++) out_len[i] = std::min(len(i), k);
    return 0;
  }
};
