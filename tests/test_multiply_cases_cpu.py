"""The `m` bound of tests/multiply_cases.py tells double from float accumulation, on the inputs of tests/test_gpu_multiply_cases.py and
for every shape of the reference's `bench multi`: the correctly rounded float64 product lies within it everywhere, the oracle's float
sums lie outside it on at least half of the elements of the non-empty Y blocks (the empty ones are exact zeros in any precision)."""
import numpy as np
import pytest

import multiply_cases as MC


@pytest.mark.parametrize("shape", MC.ALL_SHAPES)
def test_m_bound_separates_double_from_float_sums(oracle, shape):
    LM, LN = shape
    starts, pairs, A, X = MC.case(LM, LN, np.float32)
    Y64, env, n = MC.reference(oracle, LM, LN, starts, pairs, A, X)
    bm = MC.bound_m(Y64, env, n)
    rounded = Y64.astype(np.float32).astype(np.float64)
    assert np.all(np.abs(rounded - Y64) <= bm), shape
    fsum = MC.oracle_y(oracle, "c", LM, LN, starts, pairs, A, X).astype(np.float64)
    live = np.diff(starts.astype(np.int64)) > 0
    outside = float((np.abs(fsum - Y64) > bm)[live].mean())
    print("%d x %d: float sums outside the m bound on %.1f %% of the elements" % (LM, LN, 100 * outside))
    assert outside >= 0.5, (shape, outside)
