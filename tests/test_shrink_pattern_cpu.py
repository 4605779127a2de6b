"""tfqmrgpuExt_shrinkPattern and the host part of tfqmrgpuExt_dropCost (include/tfqmrgpu_ext.h section 13) without a GPU: createPlan and
the shrunk pattern are host code.  The shrunk pattern against Python lists (tests/drop_cost_ref.py) as a set and in order, the round trip
with growPattern, that no column of a plan can empty, the product count, and every status that comes before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import drop_cost_ref as DR
import leak_map_ref as MR
import tfqmrgpu_amd as T
from helpers import ptr, stencil, unordered_pattern
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED = 3, 7, 14
SENTINEL = -12345.0


def _planned(pr):
    """createPlan only: shrinkPattern needs no bufferSize"""
    s = T.Solver()
    s.create_plan(pr)
    return s


def _droppable(pr):
    carries_b = set(DR.b_blocks(pr))
    return [n for n in range(pr.nnzbX) if n not in carries_b]


# ---- the shrunk pattern ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["stencil", "stencil 1-based", "unordered"])
def test_shrunk_pattern(which):
    pr = unordered_pattern() if which == "unordered" else stencil(one_based=which.endswith("1-based"))
    free = _droppable(pr)
    assert 0 < len(free) < pr.nnzbX
    old = MR.pattern_set(pr, pr.rowPtrX - pr.index_offset)
    with _planned(pr) as s:
        drops = {"none": [], "one": [free[len(free) // 2]], "every third, backwards": free[::-3], "all but B": free}
        for name, drop in drops.items():
            rowPtrX, colIndX, oldBlock = s.shrink_pattern(drop)
            want = DR.shrunk(pr, drop)
            for got, ref in zip((rowPtrX, colIndX, oldBlock), want):    # in order: every block row keeps its other blocks in their order
                assert got.dtype == np.int32 and np.array_equal(got, ref), name
            new = MR.pattern_set(pr, rowPtrX - pr.index_offset, colIndX)
            assert set(new) == set(old) - {old[n] for n in drop} and len(new) == pr.nnzbX - len(drop)     # as a set
            assert np.all(oldBlock >= 0) and [old[n] for n in oldBlock] == new
            if name == "none":                                       # reproduces the input
                assert np.array_equal(rowPtrX, pr.rowPtrX) and np.array_equal(colIndX, pr.colIndX)
                assert np.array_equal(oldBlock, np.arange(pr.nnzbX))
            # createPlan accepts the result
            small = s.shrink_problem(pr, drop)
            assert small.index_offset == pr.index_offset and small.nnzbX == pr.nnzbX - len(drop) and small.A is pr.A and small.B is pr.B
            with _planned(small) as t:
                view = t.plan_view()
                assert view["nnzbX"] == small.nnzbX and view["nnzbB"] == pr.nnzbB


def test_no_blocks_to_drop_with_a_null_list():
    pr = stencil()
    with _planned(pr) as s:
        g = T.GrownPattern()
        assert T.lib.tfqmrgpuExt_shrinkPattern(s.plan, 0, None, C.byref(g)) == 0
        assert (g.mb, g.nnzbX) == (pr.mb, pr.nnzbX)
        assert np.array_equal(np.ctypeslib.as_array(g.colIndX, (g.nnzbX,)), pr.colIndX)
        assert np.array_equal(np.ctypeslib.as_array(g.oldBlock, (g.nnzbX,)), np.arange(pr.nnzbX))
        T.lib.tfqmrgpuExt_freeGrownPattern(C.byref(g))


@pytest.mark.parametrize("one_based", [False, True])
def test_grow_then_shrink_is_the_identity(one_based):
    pr = stencil(one_based=one_based)
    with _planned(pr) as s:
        s.buffer_size(pr.LM, pr.LN, "z")                             # growPattern needs it
        take = list(range(0, s.leak_counts()[0], 2))
        grown = s.grow_problem(pr, take)
        _, _, old = s.grow_pattern(take)
    added = np.flatnonzero(old < 0)
    assert len(added) == len(take) > 0
    with _planned(grown) as g:
        rowPtrX, colIndX, back = g.shrink_pattern(added)
    assert np.array_equal(rowPtrX, pr.rowPtrX) and np.array_equal(colIndX, pr.colIndX)
    assert np.array_equal(old[back], np.arange(pr.nnzbX))           # the two maps compose to the identity


def test_values_stay_with_their_blocks():
    pr = stencil()
    pr.X = PR.hashed_uniform(5, (pr.nnzbX, pr.LM, pr.LN)) + 0j
    drop = _droppable(pr)[1::2]
    with _planned(pr) as s:
        small = s.shrink_problem(pr, drop)
        _, _, old = s.shrink_pattern(drop)
    assert np.array_equal(small.X, pr.X[old]) and len(old) == pr.nnzbX - len(drop)


def test_no_column_of_a_plan_can_empty():
    """createPlan accepts a pattern only if every block column of X holds a block of B (TFQMRGPU_B_HAS_A_ZERO_COLUMN), and a block that
    carries B cannot be dropped: the smallest pattern is B's own, with every column still there.  (A column WITHOUT B would vanish with
    its last block -- scripts/shrink_pattern_check.cpp shows that on the plain function, where no createPlan stands in front.)"""
    mb, LM, LN = 4, 4, 4
    rpA, ciA = [0], []
    for r in range(mb):
        ciA += [c for c in (r - 1, r, r + 1) if 0 <= c < mb]
        rpA.append(len(ciA))
    rpX, ciX = np.arange(mb + 1) * 3, np.tile([0, 1, 2], mb)
    zeros = np.zeros((len(ciA), LM, LM))
    with pytest.raises(T.TfqmrError) as e:                           # column 1 without B: no such plan
        _planned(T.Problem(rpA, ciA, zeros, rpX, ciX, [0, 2, 2, 2, 2], [0, 2], np.zeros((2, LM, LN))))
    assert T.decode(e.value.status)[0] == 11
    pr = T.Problem(rpA, ciA, zeros, rpX, ciX, [0, 2, 2, 3, 3], [0, 2, 1], np.zeros((3, LM, LN)))
    middle = np.flatnonzero(ciX == 1)
    with _planned(pr) as s:
        with pytest.raises(T.TfqmrError) as e:
            s.shrink_pattern(middle)                                 # the whole column 1: its B block is among them
        assert T.decode(e.value.status)[::2] == (UNDOCUMENTED, ord("B"))
        small = s.shrink_problem(pr, _droppable(pr))
    assert np.array_equal(small.rowPtrX, pr.rowPtrB) and np.array_equal(small.colIndX, pr.colIndB)
    with _planned(small) as t:
        view = t.plan_view()
        assert view["nCols"] == 3 and view["original_bsrColIndX"].tolist() == [0, 1, 2]


# ---- the product count --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["stencil", "stencil 1-based", "unordered"])
def test_product_count_without_a_buffer(which):
    pr = unordered_pattern() if which == "unordered" else stencil(one_based=which.endswith("1-based"))
    LM, LN = (4, 4) if which == "unordered" else (pr.LM, pr.LN)
    with _planned(pr) as s:
        s.buffer_size(LM, LN, "z")
        got = s.drop_cost(cost=False, weight=False)
        assert got["cost2"] is None and got["weight2"] is None
        assert got["n_products"] == s.plan_view()["nPairs"] == sum(len(q) for q in DR.products(pr)) > 0


# ---- statuses ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_binding():
    for name in ("tfqmrgpuExt_dropCost", "tfqmrgpuExt_shrinkPattern"):
        assert name in T.EXT_SYMBOLS and hasattr(T.lib, name)
    flat = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_dropCost(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double *cost2, double *weight2, "
            "uint64_t *nProducts);") in flat
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_shrinkPattern(tfqmrgpuBsrsvPlan_t plan, uint64_t nDrop, int32_t const *drop , "
            "tfqmrgpuGrownPattern_t *shrunk);") in flat
    assert callable(T.Solver.drop_cost) and callable(T.Solver.shrink_pattern) and callable(T.Solver.shrink_problem)


def test_drop_cost_argument_checks_in_order_without_a_device():
    pr = stencil()
    cost2, weight2 = np.full((pr.nnzbX, pr.LN), SENTINEL), np.full((pr.nnzbX, pr.LN), SENTINEL)
    count = C.c_uint64(777)

    def raw(handle, plan, cost=True, weight=True, with_count=True):
        return T.lib.tfqmrgpuExt_dropCost(handle, plan, ptr(cost2) if cost else None, ptr(weight2) if weight else None,
                                          C.byref(count) if with_count else None)

    def untouched():
        return bool((cost2 == SENTINEL).all() and (weight2 == SENTINEL).all() and count.value == 777)

    assert T.decode(raw(None, None))[::2] == (POINTER_INVALID, 0)
    with T.Solver() as s:
        s.create_plan(pr)
        assert T.decode(raw(None, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.handle, None))[::2] == (POINTER_INVALID, 0)
        # no bufferSize yet: before the look at the outputs, for the count alone as well
        assert T.decode(raw(s.handle, s.plan))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, cost=False, weight=False))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, cost=False, weight=False, with_count=False))[::2] == (UNDOCUMENTED, 0)
        s.buffer_size(pr.LM, pr.LN, "z")
        assert raw(s.handle, s.plan, cost=False, weight=False, with_count=False) == NO_INFO_PASSED
        # no buffer: an array needs one, and nothing is written, the count included
        for cost, weight in ((True, True), (True, False), (False, True)):
            assert T.decode(raw(s.handle, s.plan, cost=cost, weight=weight))[::2] == (POINTER_INVALID, 0)
            assert T.decode(raw(s.handle, s.plan, cost=cost, weight=weight, with_count=False))[::2] == (POINTER_INVALID, 0)
        assert untouched()
        with pytest.raises(T.TfqmrError) as e:
            s.drop_cost()
        assert T.decode(e.value.status)[0] == POINTER_INVALID
        assert raw(s.handle, s.plan, cost=False, weight=False) == 0 and count.value == s.plan_view()["nPairs"]   # the plan alone
        assert (cost2 == SENTINEL).all() and (weight2 == SENTINEL).all()


def test_shrink_pattern_statuses():
    pr = stencil(one_based=True)
    free, carries_b = _droppable(pr), DR.b_blocks(pr)
    n = pr.nnzbX
    assert len(carries_b) == pr.nnzbB == 3

    def raw(plan, drop, g, null_list=False):
        idx = np.asarray(drop, dtype=np.int32)
        return T.lib.tfqmrgpuExt_shrinkPattern(plan, len(idx), None if null_list else ptr(idx), C.byref(g) if g is not None else None)

    def zeroed(g):
        return (g.mb, g.nnzbX) == (0, 0) and not g.rowPtrX and not g.colIndX and not g.oldBlock

    with T.Solver() as s:
        s.create_plan(pr)                                            # no bufferSize: not needed
        g = T.GrownPattern(mb=5, nnzbX=5)
        assert T.decode(raw(None, [free[0]], g))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.plan, [free[0]], None))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.plan, [free[0]], g, null_list=True))[::2] == (POINTER_INVALID, 0) and zeroed(g)
        for bad in ([n], [-1], [free[0], n + 5], [free[1], free[1]], [free[0], free[3], free[2], free[3]], [2 ** 31 - 1],
                    list(range(n)) + [free[0]], [carries_b[0], carries_b[0]]):
            g = T.GrownPattern(mb=5, nnzbX=5)
            assert T.decode(raw(s.plan, bad, g))[::2] == (UNDOCUMENTED, ord("X")), bad
            assert zeroed(g)
        for bad in ([carries_b[0]], [free[0], carries_b[2], free[1]], list(range(n))):
            g = T.GrownPattern(mb=5, nnzbX=5)
            assert T.decode(raw(s.plan, bad, g))[::2] == (UNDOCUMENTED, ord("B")), bad
            assert zeroed(g)
        with pytest.raises(T.TfqmrError) as e:
            s.shrink_pattern([carries_b[1]])
        assert T.decode(e.value.status)[::2] == (UNDOCUMENTED, ord("B"))
        g = T.GrownPattern()
        assert raw(s.plan, [free[-1], free[0]], g) == 0 and (g.mb, g.nnzbX) == (pr.mb, n - 2) and g.rowPtrX and g.oldBlock
        assert g.rowPtrX[0] == 1                                     # the plan's index offset
        T.lib.tfqmrgpuExt_freeGrownPattern(C.byref(g))
        assert zeroed(g)
