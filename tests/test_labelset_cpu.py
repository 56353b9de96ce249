"""What the calls by label SET (phnsw_labels_count_set_device, phnsw_search_exact_labelset[_device]) answer without a
GPU: how pack_label_sets packs and what it refuses, the reference masks against a brute-force loop, the three prototypes
declared alike in the header, the ctypes table, phnsw.hpp and both Rust crates, and -- over the oracle's distances --
that the union reference of one-label sets is the labeled reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib
from parallel_hnsw_amd.hnsw import pack_label_sets

import exact_filter_reference as xr
import labeled_reference as lr
import labelset_reference as sr
from test_exact_labeled_cpu import fake_index, fake_labels, last_error
from test_i8_cpu import args_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"phnsw_labels_count_set_device": 7, "phnsw_search_exact_labelset": 12, "phnsw_search_exact_labelset_device": 16}
NONE = lr.LABEL_NONE


def test_sets_pack_into_csr():
    first, values = pack_label_sets([[5, 7], [], [-1, 5, 5], [NONE], np.array([0xFFFFFFFE], dtype=np.uint64), ()], 6)
    assert first.dtype == values.dtype == np.uint32
    assert first.tolist() == [0, 2, 2, 5, 6, 7, 7]
    assert values.tolist() == [5, 7, NONE, 5, 5, NONE, 0xFFFFFFFE]
    first, values = pack_label_sets([[], []], 2)  # nothing wanted at all
    assert first.tolist() == [0, 0, 0] and values.shape == (0,) and values.dtype == np.uint32
    first, values = pack_label_sets([], 0)
    assert first.tolist() == [0] and values.shape == (0,)
    # a ready pair passes through, checked
    f2, v2 = pack_label_sets((np.array([0, 1, 1, 3]), np.array([4, -1, 6])), 3)
    assert f2.tolist() == [0, 1, 1, 3] and v2.tolist() == [4, NONE, 6] and f2.dtype == v2.dtype == np.uint32


def test_what_packing_refuses():
    with pytest.raises(ValueError, match="32-bit"):  # u64 values past u32
        pack_label_sets([[1], np.array([1 << 32], dtype=np.uint64)], 2)
    with pytest.raises(ValueError, match="32-bit"):
        pack_label_sets([[1, 1 << 32]], 1)
    with pytest.raises(ValueError, match="32-bit"):
        pack_label_sets([[-2]], 1)
    with pytest.raises(TypeError, match="integer"):
        pack_label_sets([[1.5]], 1)
    with pytest.raises(ValueError, match="one per query"):  # a wrong nq
        pack_label_sets([[1], [2]], 3)
    with pytest.raises(ValueError, match="nq \\+ 1"):
        pack_label_sets((np.array([0, 1, 2]), np.array([4, 5])), 3)
    with pytest.raises(ValueError, match="backwards \\(query 1\\)"):  # offsets that run backwards
        pack_label_sets((np.array([0, 2, 1, 3]), np.array([4, 5, 6])), 3)
    with pytest.raises(ValueError, match="start at 0"):
        pack_label_sets((np.array([1, 2, 3]), np.array([4, 5, 6])), 2)
    with pytest.raises(ValueError, match="want values"):  # fewer values than the offsets promise
        pack_label_sets((np.array([0, 2, 4]), np.array([4, 5, 6])), 2)
    with pytest.raises(ValueError, match="required"):
        pack_label_sets(None, 2)
    with pytest.raises(ValueError, match="not a sequence"):
        pack_label_sets([3, 4], 2)


def test_the_reference_s_masks_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    labels = rng.integers(0, 9, 200).astype(np.int64)
    labels[rng.permutation(200)[:20]] = -1
    labels[rng.permutation(200)[:5]] = NONE
    sets = [[], [3], [3, 3], [0, 8, 4], [-1], [NONE, 2], [77], [77, 1, -1, 1], list(range(9)), [5, 77]]
    first, values = sr.csr(sets)
    m = sr.masks_of_sets(labels, first, values)
    assert m.shape == (len(sets), 200)
    for q, s in enumerate(sets):
        for v in range(200):
            lab = int(labels[v])
            listed = lab not in (-1, NONE)
            assert m[q, v] == (listed and lab in [w for w in s if w not in (-1, NONE)]), (q, v)
    assert not m[0].any() and not m[4].any() and not m[6].any()
    np.testing.assert_array_equal(m[1], m[2])
    np.testing.assert_array_equal(m[8], ~np.isin(labels, (-1, NONE)))


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
    assert "search_many_exact_labelset" in hpp and "search_many_exact_labelset" in gpu_rs


def test_without_an_index_every_form_fails_by_name():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    for k in (10, 0, 1025):  # the index is looked at before k, the handle and nq == 0
        assert L.phnsw_search_exact_labelset(None, None, buf, None, 1, None, buf, buf, k, buf, buf, buf) == -1
        assert last_error() == "phnsw_search_exact_labelset: null index or index without layers"
        assert L.phnsw_search_exact_labelset_device(None, None, None, 0, buf, 0, None, buf, buf, 1, k, buf, buf, buf, buf,
                                                    None) == -1
        assert last_error() == "phnsw_search_exact_labelset_device: null index or index without layers"
    assert L.phnsw_labels_count_set_device(None, buf, buf, 1, 1, buf, None) == -1
    assert last_error() == "phnsw_labels_count_set_device: null labels"
    # the Python layer: its own checks first, then the library's refusal by name
    ix = fake_index()
    lb = fake_labels(ix)
    q = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="exactly one"):
        ix.search_exact_labelset(labels=lb, want=[[1], [], [2]])
    with pytest.raises(TypeError, match="labels"):
        ix.search_exact_labelset(queries=q, want=[[1], [], [2]])
    with pytest.raises(ValueError, match="one per query"):
        ix.search_exact_labelset(queries=q, labels=lb, want=[[1], []])
    with pytest.raises(TypeError, match="labels"):
        ix.search_exact_labelset_device(None, 3, 2, 5, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_exact_labelset(queries=q, labels=lb, want=[[1], [], [2, 2]], k=5)
    assert e.value.code == -1 and "phnsw_search_exact_labelset:" in str(e.value)
    with pytest.raises(ph.PhnswError) as e:
        ix.search_exact_labelset_device(lb, 3, 2, 5, 8, 8, 8, 8, qids=8, want_first=8, want_values=8)
    assert e.value.code == -1 and "phnsw_search_exact_labelset_device:" in str(e.value)


def test_one_label_sets_have_the_labeled_reference_s_rows_over_the_oracle_s_distances():
    n, dim = 300, 24
    rows = oracle.synth_rows(0, n, dim)[:, :dim].copy()
    rows[[40, 170, 298]] = rows[3]  # ties, under different labels below
    ix = oracle.Index(rows, metric=oracle.METRIC_COSINE_HALF)
    queries = [rows[3], rows[100], oracle.synth_rows(2 ** 33, 1, dim)[0, :dim].copy()]
    D = np.array([[ix.distance(q, r, oracle.SUM_BLOCKED64) for r in rows] for q in queries], dtype=np.float32)
    labels = (np.arange(n) % 7).astype(np.int64)
    labels[::13] = -1
    want = np.array([3, 5, 99])
    first, values = sr.csr([[w] for w in want])
    for k in (1, 10, 64):
        a = xr.exact_topk(D, sr.masks_of_sets(labels, first, values), None, None, k)
        b = xr.exact_topk(D, lr.masks_of(labels, want), None, None, k)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x,
                                          np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
    # and the union orders its ties by id across labels: rows 3, 40, 170 and 298 carry labels 3, 5, 2 and 4
    first, values = sr.csr([[5, 4, 3, 2], [5], [2]])
    ids, d, ln = xr.exact_topk(D, sr.masks_of_sets(labels, first, values), None, None, 4)
    assert ids[0].tolist() == [3, 40, 170, 298] and len(set(d[0].view(np.uint32).tolist())) == 1
