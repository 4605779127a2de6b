"""tfqmrgpuExt_dropCost and the loop it closes (include/tfqmrgpu_ext.h section 13) on the GPU, through the C-ABI: per block of X and
right-hand side the sum of |A_ik X_kc (:, j)|^2 over the plan's products with that block, and |X_kc (:, j)|^2, against the numpy restatement
(tests/drop_cost_ref.py) with the a-priori bound derived there -- the kernel and numpy sum the same exact-or-double products in double
and differ in the order of the sums only.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import drop_cost_ref as DR
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import load_problem, offset1
from helpers import random_x, unordered_pattern
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
          (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]                       # kAllowedBlockSizes
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 3, 7, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
SENTINEL = -12345.0


def _compare(got, ref, what=""):
    """the count exact; every cost2 and weight2 entry within its a-priori bound; cost2 > 0 where the reference is, and exactly 0.0 for
    a block without products"""
    assert got["n_products"] == ref["n_products"]
    for key, bound in (("cost2", "bound"), ("weight2", "bound_w")):
        assert got[key].shape == ref[key].shape and got[key].dtype == np.float64
        dev = np.abs(got[key] - ref[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            print(what, "%s: largest deviation / bound: %.3g" % (key, np.nanmax(np.where(ref[bound] > 0, dev / ref[bound], 0.0)) if dev.size else 0.0),
                  "blocks", got[key].shape[0], "products", got["n_products"])
        assert np.all(dev <= ref[bound]), (what, key, float(dev.max()), float(ref[bound].min()))
    assert np.all(got["cost2"][ref["cost2"] > 0] > 0)
    assert np.all(got["cost2"][ref["products_per_block"] == 0] == 0.0)


def _graded(pr, prec, X, what=""):
    """set A, B and a caller's X on a fresh plan, do not solve, compare with numpy on the data as the plan stores it"""
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", X)
        got = s.drop_cost()
    ref = DR.drop_cost(pr, DR.stored(pr.A, prec), DR.stored(X, prec))
    _compare(got, ref, "%dx%d %s%s" % (pr.LM, pr.LN, prec, what))
    return got, ref


# ---- 1. every shape, every precision -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("LM,LN", SHAPES)
def test_every_shape_and_precision(LM, LN, prec):
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN, radius=[None, 1.1, 2.3])
    got, ref = _graded(pr, prec, random_x(pr, 7 * LM + LN))
    assert np.all(ref["products_per_block"] > 0) and np.all(got["cost2"] > 0) and np.all(got["weight2"] > 0)


def test_a_block_without_products_costs_exactly_zero():
    """block column 0 holds the block rows 0 and 1; block column 1 of A has its only block in block row 2, outside that pattern: the X
    block (1, 0) meets no product"""
    LM, LN = 4, 5
    A = PR.hashed_uniform(1, (5, LM, LM)) + 1j * PR.hashed_uniform(2, (5, LM, LM))
    B = PR.hashed_uniform(3, (1, LM, LN)) + 0j
    pr = T.Problem([0, 1, 3, 5], [0, 0, 2, 1, 2], A, [0, 1, 2, 2], [0, 0], [0, 1, 1, 1], [0], B)
    got, ref = _graded(pr, "z", random_x(pr, 4))
    assert ref["products_per_block"].tolist() == [2, 0] and np.all(got["cost2"][1] == 0.0) and np.all(got["weight2"][1] > 0)


# ---- 2. against residual() on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LM,LN,prec", [(4, 5, "z"), (8, 8, "c"), (16, 16, "z"), (32, 32, "m")])
def test_one_block_per_column_is_the_residual(oracle, LM, LN, prec):
    """B = 0 and X zero except for one block per block column: A X consists of the products of that block alone, each on a block of its
    own, so that residual2 of the column IS cost2 of the block -- within the sum of the two a-priori bounds, the kernels add in different
    orders -- and every other block has cost2 = weight2 = 0.0 exactly"""
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=LM + 3 * LN, radius=[None, 1.1, 2.3])
    cols = np.unique(pr.colIndX, return_inverse=True)[1]
    chosen = [int(np.flatnonzero(cols == c)[len(np.flatnonzero(cols == c)) // 2]) for c in range(3)]
    X = np.zeros((pr.nnzbX, LM, LN), dtype=np.complex128)
    X[chosen] = random_x(pr, 17)[chosen]
    B0 = np.zeros_like(pr.B)
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", B0)
        s.set_matrix("X", X)
        got, res = s.drop_cost(), s.residual()
    A_, X_ = DR.stored(pr.A, prec), DR.stored(X, prec)
    ref, ref_res = DR.drop_cost(pr, A_, X_), RR.residual(oracle, pr, A_, X_, B0)
    _compare(got, ref, "one block per column %dx%d %s" % (LM, LN, prec))
    for c, n in enumerate(chosen):
        dev, tol = np.abs(res["residual2"][c] - got["cost2"][n]), ref_res["bound_r2"][c] + ref["bound"][n]
        print("column", c, "block", n, "largest deviation / bound %.3g" % np.max(dev / tol))
        assert np.all(got["cost2"][n] > 0) and np.all(dev <= tol)
    others = np.setdiff1d(np.arange(pr.nnzbX), chosen)
    assert np.all(got["cost2"][others] == 0.0) and np.all(got["weight2"][others] == 0.0)


# ---- 3. 1-based indices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LM,LN,prec", [(4, 5, "z"), (8, 8, "c"), (16, 16, "z"), (16, 32, "m")])
def test_index_offset(LM, LN, prec):
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=LM + LN, radius=[None, 1.1, 2.3])
    zero, _ = _graded(pr, prec, random_x(pr, 3))
    one, _ = _graded(offset1(pr), prec, random_x(pr, 3), " 1-based")
    for key in ("cost2", "weight2"):                                 # the same listing, the same sums, the same bits
        assert np.array_equal(zero[key], one[key]), key


# ---- 4. the caller's block order -----------------------------------------------------------------------------------------------------------
def test_callers_block_order_unordered_pattern():
    """the unordered pattern (4490 block rows): five block columns whose blocks start at column row % 5 in every block row and wrap
    around -- the caller's order is neither sorted inside a row nor the plan's internal (column, row) order"""
    LM, LN = 4, 4
    pat = unordered_pattern()
    A = (PR.hashed_uniform(11, (pat.nnzbA, LM, LM)) + 1j * PR.hashed_uniform(12, (pat.nnzbA, LM, LM))) / LM
    B = PR.hashed_uniform(13, (pat.nnzbB, LM, LN)) + 1j * PR.hashed_uniform(14, (pat.nnzbB, LM, LN))
    pr = T.Problem(pat.rowPtrA, pat.colIndA, A, pat.rowPtrX, pat.colIndX, pat.rowPtrB, pat.colIndB, B)
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))
    assert np.any((np.diff(pr.colIndX) < 0) & (np.diff(rows) == 0))
    got, ref = _graded(pr, "z", random_x(pr, 15), " unordered")
    assert len(set(ref["products_per_block"].tolist())) > 2          # blocks of different product counts: a permuted answer would show


@pytest.mark.parametrize("LM,LN,prec", [(16, 16, "c"), (8, 10, "z")])
def test_callers_block_order_reversed_rows(LM, LN, prec):
    """the stencil problem with the blocks of every block row of X in descending column order"""
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=5 * LM + LN, radius=[None, 1.1, 2.3])
    ciX = np.concatenate([pr.colIndX[pr.rowPtrX[r]:pr.rowPtrX[r + 1]][::-1] for r in range(pr.mb)])
    assert not np.array_equal(ciX, pr.colIndX)
    rev = T.Problem(pr.rowPtrA, pr.colIndA, pr.A, pr.rowPtrX, ciX, pr.rowPtrB, pr.colIndB, pr.B)
    _graded(rev, prec, random_x(rev, 16), " reversed rows")


# ---- 5. many products per block, many blocks per work group ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_many_products_per_block(prec):
    pr = load_problem("dense_random")                                # A dense: mb products per X block
    got, ref = _graded(pr, prec, random_x(pr, 23), " dense")
    assert np.all(ref["products_per_block"] == pr.mb) and pr.mb == 5


def test_many_blocks_per_work_group():
    """16 x 16 `z`: a wave takes a whole X block, and every fourth block of its work group's run of 32 -- more than four blocks per
    work group, eight per wave in the first, and a second work group that is partly filled"""
    pr = PR.stencil_2d(9, 9, 16, 16, ncols=3, seed=88, radius=2.3)
    assert 32 + 4 < pr.nnzbX < 64 and pr.nnzbX % 4 != 0
    _graded(pr, "z", random_x(pr, 89), " many blocks per work group")


# ---- 6. preconditioned plans ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM", [("z", 8), ("m", 16)])
def test_preconditioned_plan(prec, LM):
    pr = PR.stencil_2d(4, 4, LM, LM, 2, seed=LM, radius=[1.5, 2.1])
    # without the kept copy the caller's A is gone after the first solve: status 19 for cost2, nothing written; the weights need no A
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 200) == 0
        cost2, weight2 = np.full((pr.nnzbX, LM), SENTINEL), np.full((pr.nnzbX, LM), SENTINEL)
        count = C.c_uint64(777)
        for with_weight in (True, False):
            st = T.lib.tfqmrgpuExt_dropCost(s.handle, s.plan, C.c_void_p(cost2.ctypes.data),
                                            C.c_void_p(weight2.ctypes.data) if with_weight else None, C.byref(count))
            assert T.decode(st)[::2] == (NO_IMPLEMENTATION, 0)
            assert (cost2 == SENTINEL).all() and (weight2 == SENTINEL).all() and count.value == 777
        X = s.get_matrix()
        got = s.drop_cost(cost=False)
        assert got["cost2"] is None and got["n_products"] == s.plan_view()["nPairs"]
        ref = DR.drop_cost(pr, pr.A, X)
        assert np.all(np.abs(got["weight2"] - ref["weight2"]) <= ref["bound_w"])
    # with it: the caller's A and the back-transformed X, not the Y of the scaled system
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 200) == 0
        X = s.get_matrix()
        got = s.drop_cost()
        _compare(got, DR.drop_cost(pr, pr.A, X), "kept A %s" % prec)
        # a patch that no set-up has seen yet counts already
        d = np.arange(0, pr.nnzbA, 2, dtype=np.int32)
        A1 = pr.A.copy()
        A1[d] *= (1.5 + 0.5j)
        s.set_blocks("A", d, A1[d])
        patched = s.drop_cost()
        _compare(patched, DR.drop_cost(pr, A1, X), "kept A %s, patched" % prec)
        assert not np.array_equal(patched["cost2"], got["cost2"]) and np.array_equal(patched["weight2"], got["weight2"])


# ---- 7. non-destructive and deterministic, between two solves ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM,LN", [("z", 16, 16), ("c", 4, 5), ("z", 8, 32)])
def test_non_destructive_and_deterministic(prec, LM, LN):
    pr = PR.stencil_2d(5, 4, LM, LN, ncols=3, seed=LM + 2 * LN, radius=2.2)
    tol = 1e-9 if prec == "z" else 1e-4

    def run(with_call):
        with T.Solver.open(pr, prec) as s:
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            assert s.solve(tol, 200) == 0
            res, leak, lmap = s.residual(), s.truncation_leak(), s.leak_map()
            if with_call:
                vectors = [s.get_work_vector(k) for k in (1, 4, 5, 6, 7, 8, 9)]
                history, info = s.bound_history(), s.get_info()
                first = s.drop_cost()
                second = s.drop_cost()
                apart = (s.drop_cost(weight=False), s.drop_cost(cost=False))
                for key in ("cost2", "weight2"):
                    assert np.array_equal(first[key], second[key]), key
                assert np.array_equal(apart[0]["cost2"], first["cost2"]) and np.array_equal(apart[1]["weight2"], first["weight2"])
                assert np.all(first["cost2"] > 0)
                for k, v in zip((1, 4, 5, 6, 7, 8, 9), vectors):
                    assert np.array_equal(s.get_work_vector(k), v, equal_nan=True), k
                assert np.array_equal(s.bound_history(), history) and s.get_info() == info
                again, leak_again, lmap_again = s.residual(), s.truncation_leak(), s.leak_map()
                for key in ("residual2", "bnorm2", "columns"):
                    assert np.array_equal(res[key], again[key]), key
                for key in ("leak2", "columns", "units"):
                    assert np.array_equal(leak[key], leak_again[key]), key
                for key in ("rows", "cols", "pos2"):
                    assert np.array_equal(lmap[key], lmap_again[key]), key
            st = s.solve(tol, 200)
            return st, s.get_info()["iterations"], s.get_matrix(), s.bound_history(), res, leak, lmap

    st0, it0, X0, h0, res0, leak0, lmap0 = run(False)
    st1, it1, X1, h1, res1, leak1, lmap1 = run(True)
    assert (st0, it0) == (st1, it1) and np.array_equal(X0, X1) and np.array_equal(h0, h1)
    assert np.array_equal(res0["residual2"], res1["residual2"]) and np.array_equal(leak0["leak2"], leak1["leak2"])
    assert np.array_equal(lmap0["pos2"], lmap1["pos2"])


# ---- 8. end to end: solve, drop cost, shrunk pattern, new plan ------------------------------------------------------------------------------
def _dense(pr, rows):
    """the block rows and columns `rows` of A as a dense matrix"""
    LM, at = pr.LM, {r: n for n, r in enumerate(rows)}
    M = np.zeros((len(rows) * LM, len(rows) * LM), dtype=np.complex128)
    for q, (r, c) in enumerate(zip(np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA)).tolist(), pr.colIndA.tolist())):
        if r in at and c in at:
            M[at[r] * LM:(at[r] + 1) * LM, at[c] * LM:(at[c] + 1) * LM] = pr.A[q]
    return M


def test_chain_end_to_end():
    """1-D chain of 16 block rows of 4 x 4, tridiagonal A = 2 + random / 12 (cond 1.37, |A^-1| = 0.59), one full block column with B in
    block row 0, solved to 1e-9: the solution falls by a factor of about 15 per block row, the solve reaches 12 block rows and leaves
    the others zero.  Dropped: every block with sqrt(cost2) <= 1e-3 * threshold * sqrt(bnorm2) for all j, never the block of B.

    With P the old pattern, K the kept rows, D the dropped ones, R and R' the residuals of the old and the new solve:
        A_KK (X' - X_K) = A_KD X_D + R_K - R',    |A_KD X_D (:, j)| <= sum over the dropped blocks of sqrt(cost2[n, j]),
        A_PP (X'~ - X)  = [R_K - R' ; leak' + R_D]  (X'~: X' with zero blocks on D; leak': what A X' puts on D, section 11),
    so per right-hand side |X' - X_K| <= |A_KK^-1| (sum sqrt(cost2) + |R| + |R'|) and <= |A_PP^-1| (sqrt(leak2') + |R| + |R'|); the norms
    of the inverses come from numpy on the same A, everything else from the device.  The same run on the CPU (the oracle's solver, numpy
    sums): rows 11 ... 15 dropped, sum sqrt(cost2) = 0.9e-13 ... 1.3e-13, |R|, |R'| = 4e-12 ... 2e-10, tolerance 5e-12 ... 2.4e-10 against
    a deviation of 4.5e-15 ... 6.4e-13: passed by 340 x to 1100 x.  (On an MI355X: the same rows dropped, tolerance 2.7e-12 ... 5.7e-11
    against a deviation of 3.3e-15 ... 8.8e-14.)"""
    mb, LM, LN, threshold = 16, 4, 4, 1e-9
    rpA, ciA = [0], []
    for r in range(mb):
        ciA += [c for c in (r - 1, r, r + 1) if 0 <= c < mb]
        rpA.append(len(ciA))
    A = (PR.hashed_uniform(1, (len(ciA), LM, LM)) + 1j * PR.hashed_uniform(2, (len(ciA), LM, LM))) / (3 * LM)
    for q, (r, c) in enumerate(zip(np.repeat(np.arange(mb), np.diff(rpA)), ciA)):
        if r == c:
            A[q] += 2.0 * np.eye(LM)
    B = PR.hashed_uniform(3, (1, LM, LN)) + 1j * PR.hashed_uniform(4, (1, LM, LN))
    pr = T.Problem(rpA, ciA, A, np.arange(mb + 1), np.zeros(mb, np.int32), [0] + [1] * mb, [0], B)
    with T.Solver.open(pr, "z") as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(threshold, 200) == 0
        X, res, got = s.get_matrix(), s.residual(), s.drop_cost()
        _compare(got, DR.drop_cost(pr, pr.A, X), "chain")
        carries_b = set(s.plan_view()["subset"].tolist())
        assert carries_b == {0}
        small_enough = np.all(np.sqrt(got["cost2"]) <= 1e-3 * threshold * np.sqrt(res["bnorm2"][0]), axis=1)
        drop = [int(n) for n in np.flatnonzero(small_enough) if int(n) not in carries_b]
        keep = [n for n in range(mb) if n not in drop]
        print("dropped", drop, "sqrt(cost2) per block", np.sqrt(got["cost2"]).max(axis=1))
        assert len(drop) >= 1 and len(keep) >= 2                      # something goes, something besides B stays
        pr.X = X
        small = s.shrink_problem(pr, drop)
        assert small.nnzbX == len(keep) and np.array_equal(small.X, X[keep])
    with T.Solver.open(small, "z") as s:
        s.set_matrix("A", small.A)
        s.set_matrix("B", small.B)
        assert s.solve(threshold, 200) == 0                          # the shrunk plan converges
        X1, res1, leak1 = s.get_matrix(), s.residual(), s.truncation_leak()
        assert res1["worst"] < 10 * threshold
    r_both = np.sqrt(res["residual2"][0]) + np.sqrt(res1["residual2"][0])
    by_cost = np.linalg.norm(np.linalg.inv(_dense(pr, keep)), 2) * (np.sqrt(got["cost2"][drop]).sum(axis=0) + r_both)
    by_leak = np.linalg.norm(np.linalg.inv(_dense(pr, list(range(mb)))), 2) * (np.sqrt(leak1["leak2"][0]) + r_both)
    dev = np.sqrt((np.abs(X1 - X[keep]) ** 2).sum(axis=(0, 1)))
    print("deviation", dev, "tolerance from the dropped cost", by_cost, "from the new leak", by_leak)
    assert np.all(dev <= by_cost) and np.all(dev <= by_leak)
    assert np.all(by_cost < 1e-6 * np.sqrt((np.abs(X[keep]) ** 2).sum(axis=(0, 1))))     # ... and that says something about X


# ---- 9. statuses ---------------------------------------------------------------------------------------------------------------------------
def test_statuses_change_nothing():
    pr = PR.stencil_2d(4, 4, 4, 5, 2, seed=9, radius=1.5)
    n = pr.nnzbX

    def call(s, cost=True, weight=True, with_count=True, expect_written=False):
        cost2, weight2 = np.full((n, 5), SENTINEL), np.full((n, 5), SENTINEL)
        count = C.c_uint64(777)
        st = T.lib.tfqmrgpuExt_dropCost(s.handle, s.plan, C.c_void_p(cost2.ctypes.data) if cost else None,
                                        C.c_void_p(weight2.ctypes.data) if weight else None, C.byref(count) if with_count else None)
        if not expect_written:
            assert (cost2 == SENTINEL).all() and (weight2 == SENTINEL).all()
            assert count.value == (s.plan_view()["nPairs"] if st == 0 else 777)
        return st

    with T.Solver.open(pr, "z", buffer=False) as s:                         # no buffer
        assert call(s, cost=False, weight=False, with_count=False) == NO_INFO_PASSED       # ... comes behind the look at the outputs
        assert call(s, cost=False, weight=False) == 0               # the count needs neither a buffer nor A
        assert T.decode(call(s))[::2] == (POINTER_INVALID, 0)
        assert T.decode(call(s, cost=False))[::2] == (POINTER_INVALID, 0)
    with T.Solver.open(pr, "z") as s:                                       # no A
        s.set_matrix("B", pr.B)
        x_before = s.get_work_vector(1)
        s.set_operator(lambda *a: 0.0)                              # a user-defined operator comes before the missing A
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        assert T.decode(call(s, cost=False))[::2] == (NO_IMPLEMENTATION, 0)     # ... for the weights as well
        s.set_operator(None)
        assert T.decode(call(s))[::2] == (UNDOCUMENTED, ord("A"))
        assert T.decode(call(s, weight=False))[::2] == (UNDOCUMENTED, ord("A"))
        assert call(s, cost=False, weight=False) == 0
        only_weight = s.drop_cost(cost=False)                       # the weights do not read A
        assert only_weight["cost2"] is None and only_weight["weight2"].shape == (n, 5)
        s.set_matrix("A", pr.A)
        assert call(s, cost=False, weight=False, with_count=False) == NO_INFO_PASSED       # all three outputs NULL
        s.set_operator(lambda *a: 0.0)
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert np.array_equal(s.get_work_vector(1), x_before, equal_nan=True)
        X = random_x(pr, 5)
        s.set_matrix("X", X)
        got = s.drop_cost()                                         # ... and the call works again
        _compare(got, DR.drop_cost(pr, pr.A, X), "after the refusals")
