"""The numpy quantiser and decoder of tests/fp4_reference.py on a hand-written table; the oracle over decoded rows."""
import numpy as np
import pytest

import oracle

from fp4_reference import decode, quantize

# every grid value, the seven ties, two values that saturate; the block maximum 7.9 fixes the scale at 2^X
TABLE = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, .25, .75, 1.25, 1.75, 2.5, 3.5, 5, 6.5, 7.9])
MAGS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 2, 2, 4, 4, 6, 6, 7, 7])


@pytest.mark.parametrize("X", [0, -125, 125], ids=["X=0", "lower clamp", "upper clamp"])
def test_grid_ties_saturation_and_zero_block(X):
    block = np.ldexp(np.concatenate([TABLE, -TABLE[:15]]), X).astype(np.float32)  # 32 components, exact at every X
    rows = np.concatenate([block, np.zeros(32, dtype=np.float32)])[None, :]
    codes, scales = quantize(rows)
    assert scales.tolist() == [[X + 127, 2]]  # a block of zeros takes the lower clamp
    q = np.stack([codes[0] & 15, codes[0] >> 4], axis=1).reshape(-1)
    np.testing.assert_array_equal(q[:17], MAGS)
    np.testing.assert_array_equal(q[17:32], np.where(MAGS[:15] > 0, MAGS[:15] | 8, 0))  # the sign bit; never a -0
    assert not q[32:].any()
    want = np.array([0, .5, 1, 1.5, 2, 3, 4, 6])[MAGS]
    np.testing.assert_array_equal(decode(codes, scales, 64)[0, :17], np.ldexp(want, X).astype(np.float32))


@pytest.mark.parametrize("dim", [4, 36, 100, 768])
def test_quantising_a_decoded_row_changes_nothing(dim):
    rows = (np.random.default_rng(dim).standard_normal((50, dim)) * 10.0 ** np.arange(-25, 25)[:, None]).astype(np.float32)
    codes, scales = quantize(rows)
    again = quantize(decode(codes, scales, dim))  # (a block's maximum decodes to 4 or 6 times its scale: the scale stays)
    np.testing.assert_array_equal(again[0], codes)
    np.testing.assert_array_equal(again[1], scales)


def test_the_oracle_needs_no_change_for_decoded_rows():
    # half-integer components, small integer queries: every partial sum is exact in any order, so the chain is 1 - <q, row>
    rng = np.random.default_rng(4)
    codes = rng.integers(0, 256, size=(20, 50), dtype=np.uint8)
    held = decode(codes, np.full((20, 4), 127, dtype=np.uint8), 100)
    q = rng.integers(-3, 4, size=100).astype(np.float32)
    ix = oracle.Index(held, metric=oracle.METRIC_ONE_MINUS_DOT, sum_mode=oracle.SUM_BLOCKED64)
    got = np.array([ix.distance(q, held[i], oracle.SUM_BLOCKED64) for i in range(20)], dtype=np.float32)
    np.testing.assert_array_equal(got.view(np.uint32), (1.0 - held.astype(np.float64) @ q).astype(np.float32).view(np.uint32))
