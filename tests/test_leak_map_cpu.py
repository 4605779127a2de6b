"""tfqmrgpuExt_leakMap and tfqmrgpuExt_growPattern (include/tfqmrgpu_ext.h section 12) without a GPU: createPlan, bufferSize, the leak
listing and the grown pattern are host code.  The positions against the numpy restatement (tests/leak_map_ref.py, Python sets), the grown
pattern against set arithmetic, the closure of repeated growing, and every status that comes before the first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import leak_map_ref as MR
import leak_ref as LR
import tfqmrgpu_amd as T
from helpers import ptr, stencil, unordered_pattern
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED = 3, 7, 14
SENTINEL = -12345.0


def _open(pr, LM=None, LN=None, prec="z"):
    s = T.Solver()
    s.create_plan(pr)
    s.buffer_size(LM or pr.LM, LN or pr.LN, prec)
    return s


# ---- the positions: rows, cols, count ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_based", [False, True])
@pytest.mark.parametrize("LM,LN", [(4, 5), (16, 16)])
def test_positions_of_the_stencil(LM, LN, one_based):
    pr = stencil(LM, LN, one_based)
    want = MR.positions(pr)
    assert len(want) == LR.counts(pr)[0] > 0
    with _open(pr) as s:
        got = s.leak_map(values=False)                               # no buffer, no A: the patterns alone
        assert got["pos2"] is None and got["n_leak_blocks"] == len(want) == s.leak_counts()[0]
        assert list(zip(got["cols"].tolist(), got["rows"].tolist())) == want      # (column, row) ascending: the public order
        assert got["rows"].dtype == np.int32 and got["cols"].dtype == np.int32
    assert 0 not in got["cols"]                                      # the full column contributes no position
    assert got["rows"].min() >= 0 and got["rows"].max() < pr.mb      # 0-based whatever the index offset


def test_positions_of_the_unordered_pattern():
    pr = unordered_pattern()
    want = MR.positions(pr)
    assert len(want) > 0
    with _open(pr, 4, 4) as s:
        got = s.leak_map(values=False)
    assert list(zip(got["cols"].tolist(), got["rows"].tolist())) == want


# ---- the grown pattern -----------------------------------------------------------------------------------------------------------------
def _check_grown(pr, old, take, rowPtrX, colIndX, oldBlock, positions, columns):
    """as a set the old pattern and the taken positions; every block row: its old blocks in their old order, then the added ones
    ascending by the caller's column index; oldBlock maps onto the old blocks"""
    off = pr.index_offset
    assert rowPtrX[0] == off and len(rowPtrX) == pr.mb + 1 and rowPtrX[-1] - off == len(colIndX) == len(oldBlock) == len(old) + len(take)
    new = MR.pattern_set(pr, rowPtrX - off, colIndX)
    taken = [(positions[p][1], int(columns[positions[p][0]])) for p in take]
    assert sorted(new) == sorted(old + taken) and len(set(taken)) == len(taken)
    kept = np.flatnonzero(oldBlock >= 0)
    assert np.array_equal(oldBlock[kept], np.arange(len(old)))      # every old block once, in the old order
    assert [new[n] for n in kept] == old
    for r in range(pr.mb):
        lo, hi = rowPtrX[r] - off, rowPtrX[r + 1] - off
        n_old = int((oldBlock[lo:hi] >= 0).sum())
        assert np.all(oldBlock[lo:lo + n_old] >= 0) and np.all(oldBlock[lo + n_old:hi] == -1)
        added = colIndX[lo + n_old:hi]
        assert np.all(np.diff(added) > 0)


@pytest.mark.parametrize("which", ["stencil", "stencil 1-based", "unordered"])
def test_grown_pattern(which):
    pr = unordered_pattern() if which == "unordered" else stencil(one_based=which.endswith("1-based"))
    LM, LN = (4, 4) if which == "unordered" else (pr.LM, pr.LN)
    positions = MR.positions(pr)
    columns = np.unique(pr.colIndX)
    old = MR.pattern_set(pr, pr.rowPtrX - pr.index_offset)
    n = len(positions)
    with _open(pr, LM, LN) as s:
        takes = {"none": [], "all": None, "every third, backwards": list(range(n - 1, -1, -3)), "one": [n // 2]}
        for name, take in takes.items():
            rowPtrX, colIndX, oldBlock = s.grow_pattern(take)
            _check_grown(pr, old, list(range(n)) if take is None else take, rowPtrX, colIndX, oldBlock, positions, columns)
            if name == "none":                                       # reproduces the input
                assert np.array_equal(rowPtrX, pr.rowPtrX) and np.array_equal(colIndX, pr.colIndX)
                assert np.array_equal(oldBlock, np.arange(pr.nnzbX))
            # createPlan accepts the result, and what it took no longer leaks
            grown = s.grow_problem(pr, take)
            assert grown.index_offset == pr.index_offset and grown.nnzbX == len(colIndX) and grown.A is pr.A and grown.B is pr.B
            with _open(grown, LM, LN) as g:
                after = set(MR.positions(grown))
                assert g.leak_counts()[0] == len(after)
                assert after.isdisjoint(positions[p] for p in (range(n) if take is None else take))


def test_closure_of_repeated_growing():
    """grow with all positions until nothing leaks: every round adds blocks, and within mb rounds every block column is full"""
    pr = PR.stencil_2d(4, 4, 4, 4, ncols=3, seed=404, radius=[None, 1.1, 2.3])
    counts = [pr.nnzbX]
    for _ in range(pr.mb):
        with _open(pr) as s:
            if s.leak_counts()[0] == 0:
                break
            pr = s.grow_problem(pr)
        assert pr.nnzbX > counts[-1]
        counts.append(pr.nnzbX)
    with _open(pr) as s:
        assert s.leak_counts() == (0, 0)
    assert len(counts) > 2 and pr.nnzbX == 3 * pr.mb
    assert sorted(MR.pattern_set(pr)) == [(r, c) for r in range(pr.mb) for c in range(3)]


def test_values_move_with_their_blocks():
    pr = stencil()
    pr.X = PR.hashed_uniform(5, (pr.nnzbX, pr.LM, pr.LN)) + 0j
    with _open(pr) as s:
        grown = s.grow_problem(pr)
        _, _, old = s.grow_pattern()
    assert np.array_equal(grown.X[old >= 0], pr.X) and np.all(grown.X[old < 0] == 0)


# ---- statuses ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_header_and_binding():
    for name in ("tfqmrgpuExt_leakMap", "tfqmrgpuExt_growPattern", "tfqmrgpuExt_freeGrownPattern"):
        assert name in T.EXT_SYMBOLS and hasattr(T.lib, name)
    flat = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_leakMap(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, uint64_t capacity, int32_t *rows, "
            "int32_t *cols, double *pos2, uint64_t *nLeakBlocks);") in flat
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_growPattern(tfqmrgpuBsrsvPlan_t plan, uint64_t nTake, uint64_t const *take , "
            "tfqmrgpuGrownPattern_t *grown);") in flat
    assert "void tfqmrgpuExt_freeGrownPattern(tfqmrgpuGrownPattern_t *grown);" in flat
    assert callable(T.Solver.leak_map) and callable(T.Solver.grow_pattern) and callable(T.Solver.grow_problem)


def test_leak_map_argument_checks_in_order_without_a_device():
    pr = stencil()
    n = len(MR.positions(pr))
    rows, cols = np.full(n, -77, np.int32), np.full(n, -77, np.int32)
    pos2 = np.full((n, pr.LN), SENTINEL)
    nb = C.c_uint64(777)

    def raw(handle, plan, capacity=n, with_pos2=True, lists=True, count=True):
        return T.lib.tfqmrgpuExt_leakMap(handle, plan, capacity, ptr(rows) if lists else None, ptr(cols) if lists else None,
                                         ptr(pos2) if with_pos2 else None, C.byref(nb) if count else None)

    def untouched(count=True):
        return bool((rows == -77).all() and (cols == -77).all() and (pos2 == SENTINEL).all() and (not count or nb.value == 777))

    assert T.decode(raw(None, None))[::2] == (POINTER_INVALID, 0)
    with T.Solver() as s:
        s.create_plan(pr)
        assert T.decode(raw(None, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.handle, None))[::2] == (POINTER_INVALID, 0)
        # no bufferSize yet: before the look at the outputs, for the patterns-only form as well
        assert T.decode(raw(s.handle, s.plan))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, with_pos2=False))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, with_pos2=False, lists=False, count=False))[::2] == (UNDOCUMENTED, 0)
        s.buffer_size(pr.LM, pr.LN, "z")
        assert raw(s.handle, s.plan, with_pos2=False, lists=False, count=False) == NO_INFO_PASSED
        # no buffer: pos2 needs one, and nothing is written -- the small capacity comes behind it
        assert T.decode(raw(s.handle, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.handle, s.plan, capacity=0))[::2] == (POINTER_INVALID, 0)
        assert untouched()
        with pytest.raises(T.TfqmrError) as e:
            s.leak_map()
        assert T.decode(e.value.status)[0] == POINTER_INVALID
        # a capacity below the number of positions with an array given: key 'X', the count filled in and nothing else
        for capacity in (0, n - 1):
            nb.value = 777
            assert T.decode(raw(s.handle, s.plan, capacity=capacity, with_pos2=False))[::2] == (UNDOCUMENTED, ord("X"))
            assert nb.value == n and untouched(count=False)
        assert T.decode(raw(s.handle, s.plan, capacity=n - 1, with_pos2=False, count=False))[::2] == (UNDOCUMENTED, ord("X"))
        assert untouched(count=False)
        nb.value = 777
        assert raw(s.handle, s.plan, capacity=0, with_pos2=False, lists=False) == 0 and nb.value == n       # the count alone needs no room
        assert untouched(count=False)
        assert raw(s.handle, s.plan, with_pos2=False) == 0           # ... and the patterns-only form
        assert list(zip(cols.tolist(), rows.tolist())) == MR.positions(pr) and (pos2 == SENTINEL).all()
        s.buffer_size(pr.LM, pr.LN, "c")                             # bufferSize drops the listing; it is rebuilt on demand
        assert T.lib.tfqmrgpuExt_leakUnits(s.plan, None) == 0
        assert s.leak_map(values=False)["n_leak_blocks"] == n


def test_grow_pattern_statuses():
    pr = stencil()
    n = len(MR.positions(pr))

    def raw(plan, take, g):
        idx = np.asarray(take, dtype=np.uint64)
        return T.lib.tfqmrgpuExt_growPattern(plan, len(idx), ptr(idx), C.byref(g) if g is not None else None)

    def zeroed(g):
        return (g.mb, g.nnzbX) == (0, 0) and not g.rowPtrX and not g.colIndX and not g.oldBlock

    with T.Solver() as s:
        s.create_plan(pr)
        g = T.GrownPattern(mb=5, nnzbX=5)
        assert T.decode(raw(None, [0], g))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.plan, [0], None))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.plan, [0], g))[::2] == (UNDOCUMENTED, 0) and zeroed(g)     # no bufferSize yet
        s.buffer_size(pr.LM, pr.LN, "z")
        for bad in ([n], [0, n + 5], [1, 1], [0, 3, 2, 3], [2 ** 40], list(range(n)) + [0]):
            g = T.GrownPattern(mb=5, nnzbX=5)
            assert T.decode(raw(s.plan, bad, g))[::2] == (UNDOCUMENTED, ord("X")), bad
            assert zeroed(g)
        with pytest.raises(T.TfqmrError) as e:
            s.grow_pattern([n])
        assert T.decode(e.value.status)[::2] == (UNDOCUMENTED, ord("X"))
        g = T.GrownPattern()
        assert raw(s.plan, [n - 1, 0], g) == 0 and (g.mb, g.nnzbX) == (pr.mb, pr.nnzbX + 2) and g.rowPtrX and g.oldBlock
        T.lib.tfqmrgpuExt_freeGrownPattern(C.byref(g))
        assert zeroed(g)
        T.lib.tfqmrgpuExt_freeGrownPattern(C.byref(g))                # twice, and NULL: harmless
        T.lib.tfqmrgpuExt_freeGrownPattern(None)
