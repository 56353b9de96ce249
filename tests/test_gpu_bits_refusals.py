"""What a bits store refuses: everything but the plain walk, the distance batch and the re-ranked search -- on the host,
before any launch, with PHNSW_E_UNSUPPORTED and a message that names the call and "bits".  The kernels behind these
calls read rows through an f32 / f16 / i8 row policy; a 96-byte bit row is none of those, so this list is the audit of
every dispatch on a row kind (DESIGN has the table), confirmed call by call.  The handles (Labels, Attribute,
LabeledAttribute) are made over the f32 index: the refusal comes before a handle is looked at.

Wall time of the file on an MI355X: 2.3 s."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd._lib import lib
from parallel_hnsw_amd.hnsw import _p

import bits_reference as br
from test_gpu_i8 import adopt, bits

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -7
N, DIM = 2000, 32


@functools.lru_cache(maxsize=None)
def pair():
    full = ph.VectorStore.synthetic(N, DIM, seed=42)
    g = ph.Hnsw.generate(full, np.arange(N, dtype=np.uint64), ph.BuildParameters(seed=1))
    st = ph.BitStore.from_full(full)
    return full, g, st, adopt(st, g)


def refused(name, fn):
    with pytest.raises(ph.PhnswError) as e:
        fn()
    msg = str(e.value)
    assert e.value.code == E_UNSUPPORTED, (name, msg)
    assert name in msg and "bits" in msg, (name, msg)


def test_every_filtered_exact_table_and_radius_search_refuses_by_name():
    full, g, st, hix = pair()
    q = oracle.synth_rows(2 ** 32, 4, DIM)[:, :DIM].copy()
    sp = ph.SearchParameters(32, 32, 2)
    allow = np.ones(N, dtype=bool)
    lab = (np.arange(N) % 5).astype(np.uint32)
    keys = np.arange(N, dtype=np.uint32)
    labels, attr, lattr = ph.Labels(g, lab), ph.Attribute(g, keys), ph.LabeledAttribute(g, lab, keys)
    want, sets = np.array([0, 1, 2, 3]), [[0, 1], [2], [3, 4], [0]]
    calls = {
        # bitmap filters: walk, collecting walk, exact scan, routed call, the tables
        "phnsw_search_batch_filtered": lambda: hix.search_batch_filtered(queries=q, sp=sp, allow=allow),
        "phnsw_search_collect": lambda: hix.search_collect(queries=q, sp=sp, allow=allow),
        "phnsw_search_exact_filtered": lambda: hix.search_exact_filtered(queries=q, allow=allow),
        "phnsw_search_filtered_auto": lambda: hix.search_filtered(queries=q, sp=sp, allow=allow),
        "phnsw_search_exact_shared": lambda: hix.search_exact_shared(queries=q, allow=allow),
        "phnsw_search_exact_grouped": lambda: hix.search_exact_grouped(queries=q, allows=allow[None, :], allow_of=np.zeros(4, dtype=np.int64)),
        # radius: the walk and the exact tables / scans
        "phnsw_search_batch_radius": lambda: hix.search_radius(queries=q, radius=0.4, sp=sp),
        "phnsw_search_exact_radius": lambda: hix.search_exact_radius(queries=q, radius=0.4),
        "phnsw_search_exact_radius_labeled": lambda: hix.search_exact_radius_labeled(queries=q, labels=labels, want=want, radius=0.4),
        "phnsw_search_exact_radius_ranged": lambda: hix.search_exact_radius_ranged(queries=q, attr=attr, lo=0, hi=100, radius=0.4),
        # labels
        "phnsw_search_batch_labeled": lambda: hix.search_batch_labeled(queries=q, sp=sp, labels=labels, want=want),
        "phnsw_search_collect_labeled": lambda: hix.search_collect_labeled(queries=q, sp=sp, labels=labels, want=want),
        "phnsw_search_exact_labeled": lambda: hix.search_exact_labeled(queries=q, labels=labels, want=want),
        "phnsw_search_labeled_auto": lambda: hix.search_labeled(queries=q, sp=sp, labels=labels, want=want),
        "phnsw_search_batch_labelset": lambda: hix.search_batch_labelset(queries=q, sp=sp, labels=labels, want=sets),
        "phnsw_search_exact_labelset": lambda: hix.search_exact_labelset(queries=q, labels=labels, want=sets),
        "phnsw_search_labelset_auto": lambda: hix.search_labelset(queries=q, sp=sp, labels=labels, want=sets),
        # ranges
        "phnsw_search_batch_ranged": lambda: hix.search_batch_ranged(queries=q, sp=sp, attr=attr, lo=0, hi=100),
        "phnsw_search_exact_ranged": lambda: hix.search_exact_ranged(queries=q, attr=attr, lo=0, hi=100),
        "phnsw_search_ranged_auto": lambda: hix.search_ranged(queries=q, sp=sp, attr=attr, lo=0, hi=100),
        # label and range, label set and range
        "phnsw_search_batch_label_ranged": lambda: hix.search_batch_label_ranged(queries=q, sp=sp, attr=lattr, want=want, lo=0, hi=100),
        "phnsw_search_exact_label_ranged": lambda: hix.search_exact_label_ranged(queries=q, attr=lattr, want=want, lo=0, hi=100),
        "phnsw_search_label_ranged_auto": lambda: hix.search_label_ranged(queries=q, sp=sp, attr=lattr, want=want, lo=0, hi=100),
        "phnsw_search_batch_labelset_ranged": lambda: hix.search_batch_labelset_ranged(queries=q, sp=sp, attr=lattr, want=sets, lo=0, hi=100),
        "phnsw_search_exact_labelset_ranged": lambda: hix.search_exact_labelset_ranged(queries=q, attr=lattr, want=sets, lo=0, hi=100),
        "phnsw_search_labelset_ranged_auto": lambda: hix.search_labelset_ranged(queries=q, sp=sp, attr=lattr, want=sets, lo=0, hi=100),
    }
    for name, call in calls.items():
        refused(name, call)
    # the index still searches afterwards, and returns the restatement's distances
    got = hix.search_batch(queries=q, sp=sp)
    w = st.words()
    for i in range(4):
        ids = got[0][i, :int(got[2][i])].astype(np.int64)
        np.testing.assert_array_equal(bits(got[1][i, :len(ids)]), bits(br.distances(w[ids], br.pack(q[i])[0], DIM, oracle.METRIC_COSINE_HALF)))


def test_build_append_serialise_pq_bruteforce_and_bulk_queries_refuse_by_name():
    """the list the other search-only stores refuse, with the same codes: what an i8 store returns, a bits store returns"""
    full, g, st, hix = pair()
    L = lib()
    bp, sp, op = ph.BuildParameters(), ph.SearchParameters(), ph.BuildParameters().optimization
    vids = np.arange(N, dtype=np.uint64)
    q = oracle.synth_rows(2 ** 32, 4, DIM)[:, :DIM].copy()
    out_h, out_u64, out_f, out_i = C.c_void_p(), C.c_uint64(), C.c_float(), C.c_int()
    big_u64 = np.zeros(N * 64, dtype=np.uint64)
    big_f = np.zeros(N * 64, dtype=np.float32)
    path = b"/tmp/phnsw_bits_unsupported"
    calls = {
        "phnsw_build": lambda: L.phnsw_build(st._h, _p(vids), N, C.byref(bp), None, None, C.byref(out_h)),
        "phnsw_build_sharded": lambda: L.phnsw_build_sharded(st._h, _p(vids), N, C.byref(bp), None, ph._lib.PROGRESS_CB(),
                                                             None, C.byref(out_h), None),
        "phnsw_index_create": lambda: L.phnsw_index_create(st._h, C.byref(bp), C.byref(out_h)),
        "phnsw_generate_layer": lambda: L.phnsw_generate_layer(hix._h, _p(vids), 10, 24, C.byref(bp)),
        "phnsw_link_layer": lambda: L.phnsw_link_layer(hix._h, 0, C.byref(sp), 24, C.byref(out_u64)),
        "phnsw_improve_index": lambda: L.phnsw_improve_index(hix._h, C.byref(bp), float("nan"), None, None, C.byref(out_f)),
        "phnsw_improve_neighbors_upto": lambda: L.phnsw_improve_neighbors_upto(hix._h, 1, C.byref(bp), float("nan"), C.byref(out_f)),
        "phnsw_improve_index_sharded": lambda: L.phnsw_improve_index_sharded(hix._h, C.byref(bp), float("nan"), None,
                                                                             C.byref(out_f), None),
        "phnsw_extend_layer": lambda: L.phnsw_extend_layer(hix._h, 0, _p(vids), 1),
        "phnsw_promote_at_layer": lambda: L.phnsw_promote_at_layer(hix._h, 0, C.byref(bp), C.byref(out_i)),
        "phnsw_discover_unreachable": lambda: L.phnsw_discover_unreachable(hix._h, 0, C.byref(sp), _p(big_u64), C.byref(out_u64)),
        "phnsw_stochastic_recall_at": lambda: L.phnsw_stochastic_recall_at(hix._h, 0, C.byref(op), C.byref(out_f)),
        "phnsw_knn": lambda: L.phnsw_knn(hix._h, 3, 2, _p(big_u64), _p(big_f), _p(big_u64)),
        "phnsw_threshold_nn": lambda: L.phnsw_threshold_nn(hix._h, 0.1, 2, 8, 64, _p(big_u64), _p(big_f), _p(big_u64)),
        "phnsw_search_instrumented": lambda: L.phnsw_search_instrumented(hix._h, _p(q), None, 4, C.byref(sp), _p(big_u64),
                                                                         _p(big_f), _p(big_u64), _p(big_u64)),
        "phnsw_store_append": lambda: L.phnsw_store_append(st._h, _p(q), 4, C.byref(out_u64)),
        "phnsw_store_create_pq": lambda: L.phnsw_store_create_pq(st._h, 8, 16, 0, C.byref(out_h)),
        "phnsw_store_create_pq_kmeans": lambda: L.phnsw_store_create_pq_kmeans(st._h, 8, 16, 0, 2, 0, C.byref(out_h)),
        "phnsw_store_create_pq_shared": lambda: L.phnsw_store_create_pq_shared(st._h, 4, 64, 0, C.byref(bp), C.byref(sp), 2,
                                                                               C.byref(out_h)),
        "phnsw_bruteforce_topk": lambda: L.phnsw_bruteforce_topk(st._h, _p(q), 4, 5, _p(big_u64), _p(big_f)),
        "phnsw_index_serialize": lambda: L.phnsw_index_serialize(hix._h, path),
        "phnsw_index_deserialize": lambda: L.phnsw_index_deserialize(st._h, path, C.byref(out_h)),
    }
    i8ix = adopt(ph.I8Store.from_full(full), g)
    for name, call in calls.items():
        rc = call()
        msg = (L.phnsw_last_error() or b"").decode()
        assert rc == E_UNSUPPORTED, (name, rc, msg)
        assert "bits store" in msg and name.replace("_kmeans", "") in msg, (name, msg)
        assert not out_h.value
    # the restrictions of the converted stores return what they return for i8
    for make in (lambda ix: L.phnsw_knn(ix._h, 3, 2, _p(big_u64), _p(big_f), _p(big_u64)),
                 lambda ix: L.phnsw_search_instrumented(ix._h, _p(q), None, 4, C.byref(sp), _p(big_u64), _p(big_f), _p(big_u64),
                                                        _p(big_u64))):
        assert make(hix) == make(i8ix) == E_UNSUPPORTED
    # the locality cells of the store
    cells = C.c_uint32()
    assert L.phnsw_debug_store_cells(st._h, None, None, C.byref(cells)) == E_UNSUPPORTED
    assert b"phnsw_debug_store_cells" in L.phnsw_last_error() and b"bits" in L.phnsw_last_error()
    pos = np.zeros(N, dtype=np.uint32)
    assert L.phnsw_debug_layer_cells(hix._h, hix.layer_count() - 1, _p(pos)) == E_UNSUPPORTED
    assert b"phnsw_debug_layer_cells" in L.phnsw_last_error() and b"bits" in L.phnsw_last_error()
