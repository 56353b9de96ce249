"""CPU-only checks of the i8q store (int8 rows, int8 query, integer dot products).  The yardstick first: on `lattice`
rows (codes times a power of two) the numpy restatement of the i8q distance equals, bit for bit, the unchanged f32
oracle over the dequantised rows in both of its summation orders -- every partial sum of the oracle is an integer
multiple of one power of two and stays below 2^24, so no addition rounds -- which is what lets the GPU tests check an
i8q search against that oracle.  Then the new prototypes: declared alike in the header, the ctypes table, phnsw.hpp and
both Rust crates, and failing with the library's error where there is no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

import i8q_reference
from i8_reference import dequantize, quantize
from test_i8_cpu import args_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"phnsw_store_create_i8q": 2, "phnsw_i8q_search_batch": 9, "phnsw_i8q_search_batch_device": 13}
DIMS = [6, 100, 768, 1040, 1536]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("dim", DIMS)
def test_lattice_rows_quantise_to_their_own_codes_and_scales(dim):
    rows, c, k = i8q_reference.lattice(200, dim, np.random.default_rng(dim))
    codes, scales = quantize(rows)
    np.testing.assert_array_equal(codes, c)
    np.testing.assert_array_equal(bits(scales), bits(np.exp2(k.astype(np.float64)).astype(np.float32)))
    np.testing.assert_array_equal(bits(dequantize(codes, scales)), bits(rows))
    assert (np.abs(c).max(axis=1) == 127).all()


@pytest.mark.parametrize("metric", [oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT])
@pytest.mark.parametrize("dim", DIMS)
def test_the_unchanged_oracle_gives_the_i8q_distance_on_lattice_rows(dim, metric):
    rng = np.random.default_rng(1000 + dim)
    rows, c, k = i8q_reference.lattice(120, dim, rng)
    queries, cq, kq = i8q_reference.lattice(4, dim, rng)
    # the bound the argument needs, on these inputs: no partial sum of |cq * cr| reaches 2^24
    assert int(np.abs(c.astype(np.int64)).sum(axis=1).max()) * 127 < 2 ** 24
    codes, scales = quantize(rows)
    ix = oracle.Index(rows, metric=metric)
    for q in queries:
        want = i8q_reference.distance(q, codes, scales, metric)
        for mode in (oracle.SUM_BLOCKED64, oracle.SUM_SEQ):
            got = np.array([ix.distance(q, r, mode) for r in rows], dtype=np.float32)
            np.testing.assert_array_equal(bits(got), bits(want))
    # a stored query: the row's own codes and scale
    want = i8q_reference.distance_codes(codes[3], scales[3], codes, scales, metric)
    got = np.array([ix.distance(rows[3], r, oracle.SUM_BLOCKED64) for r in rows], dtype=np.float32)
    np.testing.assert_array_equal(bits(got), bits(want))


def test_reference_distance_on_hand_made_values():
    codes = np.array([[127, -3, 0, 2], [0, 0, 0, 0], [-127, 127, 127, -127]], dtype=np.int8)
    scales = np.array([0.5, 0.0, 0.25], dtype=np.float32)
    q = np.array([127.0, 1.0, -2.0, 0.0], dtype=np.float32)  # quantises to itself with scale 1
    d = i8q_reference.distance(q, codes, scales, oracle.METRIC_ONE_MINUS_DOT)
    np.testing.assert_array_equal(d, np.array([1 - 0.5 * (127 * 127 - 3), 1.0, 1 - 0.25 * (-127 * 127 + 127 - 254)], dtype=np.float32))
    z = i8q_reference.distance(np.zeros(4, dtype=np.float32), codes, scales, oracle.METRIC_COSINE_HALF)
    np.testing.assert_array_equal(z, np.full(3, 0.5, dtype=np.float32))  # a query of zeros: scale 0, dot 0


# ---------------------------------------------------------------- the inputs of tests/test_gpu_i8q_exhaustive.py
# can tell a wrong kernel from a right one
@pytest.mark.parametrize("dim", [1536, 1532])
def test_saturated_rows_have_dot_products_past_2_to_the_24_that_tell_the_roundings_apart(dim):
    rng = np.random.default_rng(dim)
    rows, c, k = i8q_reference.saturated(200, dim, rng)
    queries, cq, kq = i8q_reference.saturated(65, dim, rng)
    for x, cx, kx in ((rows, c, k), (queries, cq, kq)):
        codes, scales = quantize(x)
        np.testing.assert_array_equal(codes, cx)
        np.testing.assert_array_equal(bits(scales), bits(np.exp2(kx.astype(np.float64)).astype(np.float32)))
    idot = i8q_reference.idots(cq, c)
    i8q_reference.assert_saturated(idot)
    rne = idot.astype(np.float32).astype(np.int64)  # numpy converts int64 -> f32 with round to nearest even
    big = np.abs(idot) > 2 ** 24
    odd = big & (idot % 2 != 0)
    assert (rne[odd] % 4 == 0).all() and (np.abs(rne - idot)[odd] == 1).all()  # ties went to the even mantissa
    trunc = np.sign(idot) * (np.abs(idot) // 2 * 2)          # toward zero: what a truncating conversion gives past 2^24
    away = np.sign(idot) * ((np.abs(idot) + 1) // 2 * 2)     # half away from zero
    assert int((rne != trunc)[big].sum()) >= 50 and int((rne != away)[big].sum()) >= 50
    # an f32 running sum of the 1536 products loses what the integer sum keeps
    run = np.zeros(idot.shape, dtype=np.float32)
    for j in range(dim):
        run += (cq[:, j].astype(np.float32)[:, None] * c[:, j].astype(np.float32)[None, :])
    assert int((run != idot.astype(np.float32)).sum()) >= 50
    # and the distance keeps every bit of the converted sum: two dot products a float apart never share a distance
    for metric in (oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT):
        d = i8q_reference.distance_codes(cq[0], np.exp2(np.float32(kq[0])), c, np.exp2(k.astype(np.float32)), metric)
        half = np.float32(2.0) if metric == oracle.METRIC_COSINE_HALF else np.float32(1.0)
        back = -(d * half) / (np.exp2(np.float32(kq[0])) * np.exp2(k.astype(np.float32)))
        np.testing.assert_array_equal(back[big[0]].astype(np.int64), rne[0][big[0]])


@pytest.mark.parametrize("dim", [4, 6, 100, 132, 260, 1536])
def test_quantiser_edge_queries_quantise_to_their_hand_written_codes_and_scales(dim):
    edges = i8q_reference.quantiser_edges(dim)
    assert [e[0] for e in edges] == ["ties", "max_negative", "max_first", "max_last", "all_equal", "one_component",
                                     "subnormal", "huge", "zeros"]
    for name, q, want_codes, want_scale, row_scale in edges:
        codes, scales = quantize(q[None, :])
        np.testing.assert_array_equal(codes[0], want_codes, err_msg=name)
        np.testing.assert_array_equal(bits(scales), bits(want_scale), err_msg=name)
    by = {e[0]: e for e in edges}
    tiny = np.finfo(np.float32).tiny
    assert 0 < np.abs(by["subnormal"][1]).max() < tiny and 0 < by["subnormal"][3] < tiny
    assert np.abs(by["huge"][1]).max() > 1.0e18
    assert by["max_negative"][1].min() == -np.abs(by["max_negative"][1]).max() and by["max_negative"][2].min() == -127
    assert by["max_first"][2][0] == 127 and by["max_last"][2][dim - 1] == 127
    assert set(by["ties"][2].tolist()) >= {0, 2, -2}  # k + 1/2 for even k, odd k and a negative one, at the least
    # over general rows times the case's power of two: every distance finite, no product of scales lost to underflow, and
    # the query's codes in the distance bits -- rows with different dot products get different distances
    rows = oracle.synth_rows(0, 200, dim)[:, :dim]
    for name, q, want_codes, want_scale, row_scale in edges:
        codes, scales = quantize(rows * np.float32(row_scale))
        prod = (want_scale * scales).astype(np.float32)
        for metric in (oracle.METRIC_COSINE_HALF, oracle.METRIC_ONE_MINUS_DOT):
            d = i8q_reference.distance(q, codes, scales, metric)
            assert np.isfinite(d).all(), name
            if name == "zeros":
                assert (prod == 0).all() and (d == (0.5 if metric == oracle.METRIC_COSINE_HALF else 1.0)).all()
                continue
            assert (prod >= tiny).all(), name + ": sq * sr is a normal number"
            idot = i8q_reference.idots(want_codes[None, :], codes)[0]
            assert len(np.unique(bits(d))) >= 0.9 * len(np.unique(idot)), name


RING_SHAPES = [(3, 6, 1), (33, 100, 1), (65, 128, 1), (129, 132, 1), (200, 1536, 1), (300, 768, 1), (200, 100, 12), (200, 6, 32)]


@pytest.mark.parametrize("n,dim,reach", RING_SHAPES)
def test_a_ring_searched_with_ef_n_evaluates_and_returns_every_node(n, dim, reach):
    """the premise of the exhaustive GPU test, against the unchanged oracle on lattice rows (where its f32 arithmetic is
    the i8q distance): length n, n evaluations, and ids and distance bits those of i8q_reference.all_pairs"""
    rng = np.random.default_rng(n + dim)
    rows, c, k = i8q_reference.lattice(n, dim, rng)
    q, cq, kq = i8q_reference.lattice(7, dim, rng)
    assert int(np.abs(c.astype(np.int64)).sum(axis=1).max()) * 127 < 2 ** 24
    codes, scales = quantize(rows)
    ix = oracle.Index(rows, sum_mode=oracle.SUM_BLOCKED64)
    for nodes, nb in i8q_reference.circulant(n, reach):
        ix.push_layer(nodes, nb, nb.shape[1])
    qids = np.arange(0, n, max(1, n // 5), dtype=np.uint64)  # the first is the entry vector, which exclude does not drop
    pd = 2 if reach == 1 else n + 1
    for kw in (dict(queries=q), dict(qids=qids), dict(qids=qids, exclude=qids)):
        ci, cd, cl, cs = ix.search(sp=(n, n, pd), stats=True, **kw)
        wi, wd = i8q_reference.ranked(i8q_reference.matrix(q, codes, scales, oracle.METRIC_COSINE_HALF, kw.get("qids")),
                                      kw.get("exclude"))
        assert (cs[:, 0] == n).all()
        if reach == 1:
            assert (cs[:, 1] == n).all()  # n - 2 hops that find a node, then two that find none
        for i in range(len(cl)):
            w = len(wi[i])
            assert w == (n - 1 if "exclude" in kw and i > 0 else n) and cl[i] == w
            np.testing.assert_array_equal(ci[i, :w].astype(np.int64), wi[i])
            np.testing.assert_array_equal(bits(cd[i, :w]), bits(wd[i]))


def test_new_prototypes_are_declared_everywhere_with_matching_argument_counts():
    strip = lambda s: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))
    header = strip(open(os.path.join(ROOT, "include", "phnsw.h")).read())
    hpp = strip(open(os.path.join(ROOT, "include", "phnsw.hpp")).read())
    sys_rs = strip(open(os.path.join(ROOT, "rust", "phnsw-sys", "src", "lib.rs")).read())
    gpu_rs = strip(open(os.path.join(ROOT, "rust", "parallel-hnsw-gpu", "src", "lib.rs")).read())
    L = C.CDLL(_lib.LIB_PATH)
    for name, argc in NEW.items():
        assert args_of(header, r"\bint\s+%s\s*\(" % name) == argc, name + ": include/phnsw.h"
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == argc, name + ": _lib.SYMBOLS"
        assert hasattr(L, name), "libphnsw.so does not export " + name
        assert hasattr(ph.lib(), name)
        assert args_of(hpp, r"\b%s\s*\(" % name) == argc, name + ": include/phnsw.hpp"
        assert args_of(sys_rs, r"\bpub\s+fn\s+%s\s*\(" % name) == argc, name + ": phnsw-sys"
        assert args_of(gpu_rs, r"\bsys::%s\s*\(" % name) == argc, name + ": parallel-hnsw-gpu"
    assert issubclass(ph.I8QStore, ph.VectorStore) and not issubclass(ph.I8QStore, ph.I8Store)
    assert ph.I8QStore.from_full and ph.I8QStore.codes and ph.I8QStore.scales


def test_null_arguments_are_invalid():
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_i8q(None, C.byref(out)) == -1  # PHNSW_E_INVALID
    assert b"phnsw_store_create_i8q" in ph.lib().phnsw_last_error()
    assert not out.value
    sp = ph.SearchParameters(16, 16, 2)
    assert ph.lib().phnsw_i8q_search_batch(None, None, None, 0, C.byref(sp), 1, None, None, None) == -1
    assert b"phnsw_i8q_search_batch" in ph.lib().phnsw_last_error()
    assert ph.lib().phnsw_i8q_search_batch_device(None, None, None, 0, 0, C.byref(sp), 1, None, None, None, None, None,
                                                  None) == -1


@pytest.mark.skipif(ph.lib().phnsw_device_count() != 0, reason="a GPU is visible")
def test_no_cpu_fallback():
    fake = C.create_string_buffer(4096)
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_i8q(C.cast(fake, C.c_void_p), C.byref(out)) == -2  # PHNSW_E_NO_DEVICE
    assert not out.value
