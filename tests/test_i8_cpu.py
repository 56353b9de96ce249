"""CPU-only checks of the i8 store: the numpy restatement of its quantiser has the properties the format promises, the
four new prototypes are declared with the same argument counts in the header, the ctypes table, phnsw.hpp and both
Rust crates, and without a GPU the calls fail with the library's error instead of crashing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import parallel_hnsw_amd as ph
from parallel_hnsw_amd import _lib

from i8_reference import dequantize, quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"phnsw_store_create_i8": 2, "phnsw_i8_read": 3, "phnsw_i8_search_batch": 9, "phnsw_i8_search_batch_device": 13}


def sample_rows():
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((64, 100)).astype(np.float32)
    rows[1] *= np.float32(1.0e-3)
    rows[2] *= np.float32(1.0e6)
    rows[3, 5] = -40.0  # the max-abs component is negative
    rows[4] = np.abs(rows[4])
    return rows


def test_codes_are_in_range_and_the_max_abs_component_is_127():
    rows = sample_rows()
    codes, scales = quantize(rows)
    assert codes.dtype == np.int8 and scales.dtype == np.float32
    assert codes.min() >= -127 and codes.max() <= 127
    j = np.abs(rows).argmax(axis=1)
    r = np.arange(len(rows))
    np.testing.assert_array_equal(codes[r, j], (127 * np.sign(rows[r, j])).astype(np.int8))
    assert codes[3, 5] == -127


def test_dequantised_value_is_within_half_a_step():
    rows = sample_rows()
    codes, scales = quantize(rows)
    err = np.abs(dequantize(codes, scales).astype(np.float64) - rows.astype(np.float64))
    # half a step, plus one ulp of the value for the roundings of x / scale and scale * code
    bound = scales[:, None].astype(np.float64) / 2 + np.spacing(np.abs(rows)).astype(np.float64)
    assert (err <= bound).all(), float((err - bound).max())


def test_zero_row_has_scale_zero_and_codes_zero():
    rows = sample_rows()
    rows[9] = 0.0
    codes, scales = quantize(rows)
    assert scales[9] == 0.0 and not codes[9].any()
    assert not dequantize(codes, scales)[9].any()
    assert scales[8] > 0


def args_of(text, pattern):
    """argument count of the first parenthesised list that follows `pattern` in `text`"""
    m = re.search(pattern, text)
    assert m, pattern
    depth, i, start = 0, m.end() - 1, m.end()
    assert text[i] == "("
    commas = 0
    for i in range(m.end() - 1, len(text)):
        ch = text[i]
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
            if depth == 0:
                break
        elif ch == "," and depth == 1:
            commas += 1
    assert text[start:i].strip()
    return commas + 1


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
    assert ph.I8Store.from_full and ph.I8Store.codes and ph.I8Store.scales and ph.Hnsw.search_batch_reranked


def test_null_arguments_are_invalid():
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_i8(None, C.byref(out)) == -1  # PHNSW_E_INVALID
    assert b"phnsw_store_create_i8" in ph.lib().phnsw_last_error()
    assert not out.value
    assert ph.lib().phnsw_i8_read(None, None, None) == -1
    sp = ph.SearchParameters(16, 16, 2)
    assert ph.lib().phnsw_i8_search_batch(None, None, None, 0, C.byref(sp), 1, None, None, None) == -1
    assert b"phnsw_i8_search_batch" in ph.lib().phnsw_last_error()
    assert ph.lib().phnsw_i8_search_batch_device(None, None, None, 0, 0, C.byref(sp), 1, None, None, None, None, None,
                                                 None) == -1


@pytest.mark.skipif(ph.lib().phnsw_device_count() != 0, reason="a GPU is visible")
def test_no_cpu_fallback():
    """on a box without a GPU phnsw_store_create_i8 answers PHNSW_E_NO_DEVICE before it looks at its source (a zeroed
    block stands in for the store no GPU-less box can make), and so does the Python path, whose f32 store fails first"""
    fake = C.create_string_buffer(4096)
    out = C.c_void_p()
    assert ph.lib().phnsw_store_create_i8(C.cast(fake, C.c_void_p), C.byref(out)) == -2  # PHNSW_E_NO_DEVICE
    assert not out.value
    with pytest.raises(ph.PhnswError) as e:
        ph.I8Store.from_full(ph.VectorStore(np.zeros((4, 8), dtype=np.float32)))
    assert e.value.code == -2
