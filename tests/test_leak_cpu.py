"""tfqmrgpuExt_truncationLeak (include/tfqmrgpu_ext.h section 11) without a GPU: the numpy restatement (tests/leak_ref.py) on cases that
can be derived by hand and against the sum rule, the library's pattern-only counts -- createPlan, bufferSize and the leak listing are host
code -- against it, and the argument checks that come before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import leak_ref as LR
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import offset1
from helpers import random_x
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED = 3, 7, 14
SENTINEL = -12345.0

CASES = {
    "full columns": dict(nx=4, ny=4, LM=4, LN=4, ncols=3, radius=None),
    "ragged": dict(nx=4, ny=4, LM=4, LN=5, ncols=3, radius=[None, 1.1, 2.3]),
    "chain": dict(nx=13, ny=1, LM=4, LN=4, ncols=3, radius=1.0),
    "9 points": dict(nx=7, ny=6, LM=4, LN=8, ncols=4, radius=1.5, points=9),
    "13 points": dict(nx=6, ny=7, LM=8, LN=8, ncols=2, radius=[2.0, 0.5], points=13),
}


def _problem(name):
    kw = dict(CASES[name])
    return PR.stencil_2d(kw.pop("nx"), kw.pop("ny"), kw.pop("LM"), kw.pop("LN"), seed=31, **kw)


# ---- the reference on cases that can be derived by hand ------------------------------------------------------------------------------
def test_full_columns_leak_nothing():
    pr = _problem("full columns")
    assert LR.counts(pr) == (0, 0)
    ref = LR.leak(pr, pr.A, random_x(pr, 1))
    assert (ref["n_leak_blocks"], ref["n_leak_pairs"]) == (0, 0)
    assert np.all(ref["leak2"] == 0.0) and np.all(ref["bound"] == 0.0)


def test_chain_leaks_two_positions_per_column():
    """1-D chain, 3-point stencil, radius 1 around interior sources: column c holds the rows s - 1, s, s + 1; A reaches s - 2 from
    s - 1 and s + 2 from s + 1 and nothing else outside: two positions, one product each"""
    pr = _problem("chain")
    assert np.array_equal(np.bincount(pr.colIndX), [3, 3, 3])
    assert LR.counts(pr) == (6, 6)
    X = random_x(pr, 2)
    ref = LR.leak(pr, pr.A, X)
    assert list(ref["blocks_per_column"]) == [2, 2, 2] and list(ref["pairs_per_column"]) == [2, 2, 2]
    # ... and the value, by hand, for the first column: source row 2, rows 1 2 3 held, rows 0 and 4 reached
    rowsA = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    blockA = {(int(i), int(k)): q for q, (i, k) in enumerate(zip(rowsA, pr.colIndA))}
    rowsX = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))
    blockX = {(int(k), int(c)): x for x, (k, c) in enumerate(zip(rowsX, pr.colIndX))}
    by_hand = sum((np.abs(pr.A[blockA[(i, k)]] @ X[blockX[(k, 0)]]) ** 2).sum(axis=0) for i, k in ((0, 1), (4, 3)))
    assert np.allclose(ref["leak2"][0], by_hand, rtol=1e-14, atol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_counts_agree_between_sets_and_scatter(name):
    pr = _problem(name)
    ref = LR.leak(pr, pr.A, random_x(pr, 3))
    assert LR.counts(pr) == (ref["n_leak_blocks"], ref["n_leak_pairs"])
    assert np.all((ref["leak2"] > 0) == (ref["blocks_per_column"] > 0)[:, None])
    assert np.all(ref["bound"] <= 1e-11 * ref["leak2"])             # the bound is a rounding bound, not a tolerance


@pytest.mark.parametrize("name", list(CASES))
def test_sum_rule_in_numpy(oracle, name):
    """the residual of the padded problem (full columns, X zero-padded) = residual2 + leak2 of the truncated one"""
    pr = _problem(name)
    X = random_x(pr, 4)
    twin, Xp = LR.padded(pr, X)
    whole = RR.residual(oracle, twin, twin.A, Xp)["residual2"]
    parts = RR.residual(oracle, pr, pr.A, X)["residual2"] + LR.leak(pr, pr.A, X)["leak2"]
    assert whole.shape == parts.shape
    assert np.all(np.abs(whole - parts) <= 1e-12 * whole)


# ---- the library's listing, host code: counts without a device -------------------------------------------------------------------------
@pytest.mark.parametrize("one_based", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_library_counts_without_a_device(name, one_based):
    pr = _problem(name)
    want = LR.counts(pr)
    if one_based:
        pr = offset1(pr)
        assert LR.counts(pr) == want
    with T.Solver() as s:
        s.create_plan(pr)
        s.buffer_size(pr.LM, pr.LN, "z")
        assert s.leak_counts() == want                              # no buffer, no A: the patterns alone
        cols = np.full(len(np.unique(pr.colIndX)), -77, np.int32)
        st = T.lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, None, cols.ctypes.data_as(C.c_void_p), None, None)
        assert st == 0 and np.array_equal(cols, np.unique(pr.colIndX))
        units = np.zeros(len(cols), np.uint32)
        total = T.lib.tfqmrgpuExt_leakUnits(s.plan, units.ctypes.data_as(C.c_void_p))
        blocks = LR.leak(pr, pr.A, np.zeros((pr.nnzbX, pr.LM, pr.LN)))["blocks_per_column"]
        assert total == units.sum() and np.array_equal(units > 0, blocks > 0)
        s.buffer_size(pr.LM, pr.LN, "c")                            # bufferSize drops the listing; it is rebuilt on demand
        assert T.lib.tfqmrgpuExt_leakUnits(s.plan, None) == 0
        assert s.leak_counts() == want


def test_long_shell_is_cut_into_units_of_whole_positions():
    pr = PR.stencil_2d(40, 40, 4, 4, ncols=2, seed=40, radius=24.5, points=13)
    ref = LR.leak(pr, pr.A, np.zeros((pr.nnzbX, 4, 4)))
    with T.Solver() as s:
        s.create_plan(pr)
        s.buffer_size(4, 4, "z")
        assert s.leak_counts() == (ref["n_leak_blocks"], ref["n_leak_pairs"])
        units = np.zeros(2, np.uint32)
        T.lib.tfqmrgpuExt_leakUnits(s.plan, units.ctypes.data_as(C.c_void_p))
    assert ref["blocks_per_column"].min() >= 60 and units.min() > 1
    # at most 64 products per unit at 4 x 4, and a position is never cut: no fewer units than that allows
    assert np.all(units >= -(-ref["pairs_per_column"] // 64))


# ---- the argument checks, in the header's order -----------------------------------------------------------------------------------------
def test_symbols_header_and_binding():
    assert "tfqmrgpuExt_truncationLeak" in T.EXT_SYMBOLS and "tfqmrgpuExt_leakUnits" in T.EXT_SYMBOLS
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read())
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_truncationLeak(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, "
            "double *leak2, int32_t *columns, uint64_t *nLeakBlocks, uint64_t *nLeakPairs);") in flat
    assert "(11) truncation leak" in flat
    assert callable(T.Solver.truncation_leak) and callable(T.Solver.leak_counts)


def test_argument_checks_in_order_without_a_device():
    pr = _problem("ragged")
    leak2, cols = np.full((3, pr.LN), SENTINEL), np.full(3, -77, np.int32)
    nb, npairs = C.c_uint64(777), C.c_uint64(777)

    def raw(handle, plan, with_leak2=True, others=True):
        return T.lib.tfqmrgpuExt_truncationLeak(handle, plan, leak2.ctypes.data_as(C.c_void_p) if with_leak2 else None,
                                                cols.ctypes.data_as(C.c_void_p) if others else None,
                                                C.byref(nb) if others else None, C.byref(npairs) if others else None)

    def untouched():
        return bool((leak2 == SENTINEL).all() and (cols == -77).all() and nb.value == 777 and npairs.value == 777)

    assert T.decode(raw(None, None))[::2] == (POINTER_INVALID, 0)
    with T.Solver() as s:
        s.create_plan(pr)
        assert T.decode(raw(None, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.handle, None))[::2] == (POINTER_INVALID, 0)
        # no bufferSize yet: before the look at the outputs, for the counts as well
        assert T.decode(raw(s.handle, s.plan))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, with_leak2=False))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, False, False))[::2] == (UNDOCUMENTED, 0)
        s.buffer_size(pr.LM, pr.LN, "z")
        assert raw(s.handle, s.plan, False, False) == NO_INFO_PASSED
        # no buffer: leak2 needs one, and nothing is written -- not the counts either, which the call could have given
        assert T.decode(raw(s.handle, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.handle, s.plan, True, False))[::2] == (POINTER_INVALID, 0)
        assert untouched()
        with pytest.raises(T.TfqmrError) as e:
            s.truncation_leak()
        assert T.decode(e.value.status)[0] == POINTER_INVALID
        assert untouched()
        assert raw(s.handle, s.plan, with_leak2=False) == 0
        assert (nb.value, npairs.value) == LR.counts(pr) and list(cols) == [0, 1, 2] and (leak2 == SENTINEL).all()
