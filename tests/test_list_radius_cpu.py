"""The exact radius search by row label and by numeric range without a GPU: the integer rules of
parallel_hnsw_amd/csrc/list_radius_plan.h in a stand-alone host program under AddressSanitizer and UBSan
(tests/cpp/test_list_radius_plan.cpp, compiled with g++ and run as a process of its own; nothing loaded into Python), the
numpy restatement the GPU tests compare against (tests/list_radius_reference.py) pinned to the restatement of the exact
top-k cut at the radius, the bindings' argument counts against the header, and what the entry points answer to a null
index."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

import exact_filter_reference as xr
import list_radius_reference as lr
import radius_reference as rr
from test_radius_cpu import matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("phnsw_search_exact_radius_labeled", "phnsw_search_exact_radius_labeled_device", "phnsw_search_exact_radius_ranged",
         "phnsw_search_exact_radius_ranged_device")


def test_list_radius_plan_rules_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "test_list_radius_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "test_list_radius_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout


def world():
    D = matrix()
    nq, n = D.shape
    rng = np.random.default_rng(3)
    labels = rng.integers(0, 4, n).astype(np.uint32)
    labels[rng.random(n) < 0.1] = lr.NONE
    labels[[7, 11, 13]] = 2  # the +inf, the NaN and the -0.0 column are listed under one label
    keys = rng.integers(0, 30, n).astype(np.uint32)  # ties
    keys[rng.random(n) < 0.1] = lr.NONE
    keys[[7, 11, 13]] = 12
    members = np.arange(n) % 5 != 0
    exclude = np.arange(nq, dtype=np.uint64) * 3
    radius = np.array([0.5, 1.0, 2.5, 5.0, 5.125, np.inf, 0.0, -1.0, np.nan], dtype=np.float32)
    return D, labels, keys, members, exclude, radius


def pinned(D, radius, masks, exclude, members, got):
    """got is, segment by segment, exact_topk over the query's mask cut at d < radius"""
    nq, n = D.shape
    first, ids, d = got
    assert first[0] == 0 and first[nq] == len(ids) == len(d) and (np.diff(first.astype(np.int64)) >= 0).all()
    ti, td, tl = xr.exact_topk(D, masks, exclude, members, n)
    for q in range(nq):
        si, sd = rr.segment(got, q)
        row_d = td[q, :int(tl[q])]
        with np.errstate(invalid="ignore"):
            keep = (row_d < radius[q]) if radius[q] > 0 else np.zeros(len(row_d), dtype=bool)
        assert not keep.any() or keep[:keep.sum()].all()
        np.testing.assert_array_equal(si, ti[q, :keep.sum()])
        np.testing.assert_array_equal((sd + np.float32(0)).view(np.uint32), (row_d[:keep.sum()] + np.float32(0)).view(np.uint32))
        assert not np.isin(si, [7, 11]).any()  # +inf and NaN: never inside a radius, not even +inf
        assert not (sd.view(np.uint32) == 0x80000000).any()  # -0.0 is reported as +0.0


def test_the_labeled_restatement_is_the_exact_top_k_of_the_query_s_label_cut_at_the_radius():
    D, labels, _, members, exclude, radius = world()
    nq, n = D.shape
    want = np.array([0, 1, 2, 3, 2, 2, 2, 1, 0])
    for e, m in ((None, None), (exclude, members)):
        got = lr.exact_radius_labeled(D, radius, labels, want, e, m)
        pinned(D, radius, lr.label_masks(labels, want), e, m, got)
    got = lr.exact_radius_labeled(D, radius, labels, want)
    assert 13 in rr.segment(got, 2)[0] and len(rr.segment(got, 5)[0]) == (labels == 2).sum() - 2  # +inf radius: all but inf, NaN
    assert got[0][6] == got[0][7] == got[0][8] == got[0][9]  # 0, -1 and NaN match nothing
    # NONE, -1 and a label nobody carries: empty segments, the others as they were
    odd = want.copy()
    odd[[0, 2, 4]] = [lr.NONE, -1, 77]
    got2 = lr.exact_radius_labeled(D, np.float32(np.inf), labels, odd)
    n2 = np.diff(got2[0].astype(np.int64))
    assert not n2[[0, 2, 4]].any() and n2[1] == (labels == 1).sum()
    # one label for the whole batch is the shared-bitmap call's restatement
    same = lr.exact_radius_labeled(D, radius, labels, np.full(nq, 2))
    ref = rr.exact_radius(D, radius, labels == 2)
    for a, b in zip(same, ref):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)


def test_the_ranged_restatement_is_the_exact_top_k_of_the_query_s_window_cut_at_the_radius():
    D, _, keys, members, exclude, radius = world()
    nq, n = D.shape
    lo = np.array([0, 5, 12, 12, 0, 0, 3, 20, 29], dtype=np.uint32)
    hi = np.array([29, 10, 12, 11, 0xFFFFFFFF, 12, 9, 0xFFFFFFFF, 29], dtype=np.uint32)
    for e, m in ((None, None), (exclude, members)):
        got = lr.exact_radius_ranged(D, radius, keys, lo, hi, e, m)
        pinned(D, radius, lr.range_masks(keys, lo, hi), e, m, got)
    inf = lr.exact_radius_ranged(D, np.float32(np.inf), keys, lo, hi)
    n_in = np.diff(inf[0].astype(np.int64))
    listed = keys != lr.NONE
    assert n_in[3] == 0  # lo > hi
    assert n_in[4] == listed.sum() - 2 and n_in[0] == listed.sum() - 2  # hi = 0xFFFFFFFF: no row without a value passes
    assert n_in[2] == (keys == 12).sum() - 2 and n_in[7] == (listed & (keys >= 20)).sum()
    only_none = lr.exact_radius_ranged(D[:1], np.float32(np.inf), keys, [0xFFFFFFFF], [0xFFFFFFFF])  # rows without a value only
    assert len(only_none[1]) == 0


def header_arity(name):
    src = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "phnsw.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, src, flags=re.S)
    assert m, name
    return len(m.group(1).split(","))


def test_the_entry_points_are_bound_with_the_header_s_arity():
    for name, arity in zip(CALLS, (13, 16, 14, 17)):
        assert header_arity(name) == arity == len(_lib.SYMBOLS[name][1]), name
    # the handle and want (or lo, hi) in the bitmap's place: one and two arguments more than the call they extend
    assert header_arity("phnsw_search_exact_radius") + 1 == 13 and header_arity("phnsw_search_exact_radius_device") + 2 == 17
    sys_rs = open(os.path.join(ROOT, "rust", "phnsw-sys", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "phnsw.hpp")).read()
    for name in CALLS:
        assert "pub fn %s(" % name in sys_rs and name + "(" in hpp, name


def test_a_null_index_is_refused_first_by_every_entry_point():
    L = ph.lib()
    buf = (C.c_uint64 * 8)()
    for cap in (10, 0, 1 << 31):  # the index is looked at before cap, the handle and nq
        for nq in (1, 0):
            assert L.phnsw_search_exact_radius_labeled(None, None, buf, None, nq, None, buf, buf, cap, buf, buf, buf, buf) == -1
            assert L.phnsw_search_exact_radius_labeled_device(None, None, None, 0, buf, nq, None, buf, buf, cap, buf, buf, buf, buf,
                                                              buf, None) == -1
            assert L.phnsw_search_exact_radius_ranged(None, None, buf, None, nq, None, buf, buf, buf, cap, buf, buf, buf, buf) == -1
            assert L.phnsw_search_exact_radius_ranged_device(None, None, None, 0, buf, nq, None, buf, buf, buf, cap, buf, buf, buf,
                                                             buf, buf, None) == -1
            assert L.phnsw_last_error().decode() == "phnsw_search_exact_radius_ranged_device: null index or index without layers"


def test_python_argument_handling_runs_before_the_call():
    from test_exact_shared_cpu import fake_index
    ix = fake_index()
    q = np.zeros((3, 4), dtype=np.float32)
    for method in (ix.search_exact_radius_labeled, ix.count_exact_radius_labeled):
        with pytest.raises(TypeError, match="Labels"):
            method(queries=q, labels=object(), want=[1, 2, 3], radius=1.0)
    for method in (ix.search_exact_radius_ranged, ix.count_exact_radius_ranged):
        with pytest.raises(TypeError, match="Attribute"):
            method(queries=q, attr=object(), lo=0, hi=5, radius=1.0)
    with pytest.raises(TypeError):
        ix.search_exact_radius_labeled_device(None, 3, 8, 0, 8, 0, 0, 8, 8, qids=8, want=8)
    with pytest.raises(TypeError):
        ix.search_exact_radius_ranged_device(None, 3, 8, 0, 8, 0, 0, 8, 8, qids=8, lo=8, hi=8)
