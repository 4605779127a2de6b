"""tfqmrgpuExt_truncationLeak (include/tfqmrgpu_ext.h section 11) on the GPU, through the C-ABI: what A X puts outside the pattern of X,
|.|^2 per (block column, right-hand side), against the numpy restatement (tests/leak_ref.py) with the a-priori bound derived there -- the
kernel and numpy sum the same exact-or-double products in double and differ in the order of the sums only.  Needs an MI355X
(`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import leak_ref as LR
import precond_ref as PC
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import load_problem, offset1
from helpers import random_x
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
          (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]                       # kAllowedBlockSizes
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 3, 7, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
SENTINEL = -12345.0


def _compare(got, ref, what=""):
    """leak2 within the a-priori bound, entry by entry; counts and columns exact"""
    dev = np.abs(got["leak2"] - ref["leak2"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(what, "leak2: largest deviation / bound: %.3g" % np.nanmax(np.where(ref["bound"] > 0, dev / ref["bound"], 0.0)),
              "positions", got["n_leak_blocks"], "products", got["n_leak_pairs"], "units", list(got["units"]))
    assert got["leak2"].shape == ref["leak2"].shape and got["leak2"].dtype == np.float64
    assert np.all(dev <= ref["bound"]), (what, float(dev.max()), float(ref["bound"].min()))
    assert (got["n_leak_blocks"], got["n_leak_pairs"]) == (ref["n_leak_blocks"], ref["n_leak_pairs"])
    assert np.array_equal(got["columns"], ref["columns"])
    assert np.array_equal(got["units"] > 0, ref["blocks_per_column"] > 0)
    assert np.all(got["leak2"][ref["blocks_per_column"] == 0] == 0.0)          # no position, no unit: exactly 0


def _graded(pr, prec, X, what=""):
    """set A, B and a caller's X on a fresh plan, do not solve, compare with numpy on the data as the plan stores it"""
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", X)
        got = s.truncation_leak()
        assert s.leak_counts() == (got["n_leak_blocks"], got["n_leak_pairs"])
        view = s.plan_view()
    ref = LR.leak(pr, LR.stored(pr.A, prec), LR.stored(X, prec))
    _compare(got, ref, "%dx%d %s%s" % (pr.LM, pr.LN, prec, what))
    assert np.array_equal(got["columns"], view["original_bsrColIndX"])
    assert got["leak2"].shape == (view["nCols"], pr.LN)
    return got, ref


# ---- 1. every shape, every precision ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("LM,LN", SHAPES)
def test_every_shape_and_precision(LM, LN, prec):
    """one full column -- no position, no unit, exactly 0.0 -- and two truncated ones"""
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN, radius=[None, 1.1, 2.3])
    got, ref = _graded(pr, prec, random_x(pr, 7 * LM + LN))
    assert list(ref["blocks_per_column"] > 0) == [False, True, True]
    assert np.all(got["leak2"][0] == 0.0) and np.all(got["leak2"][1:] > 0)


# ---- 2. 1-based indices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LM,LN,prec", [(4, 5, "z"), (8, 8, "c"), (16, 16, "z"), (16, 32, "m")])
def test_index_offset(LM, LN, prec):
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=LM + LN, radius=[None, 1.1, 2.3])
    got, _ = _graded(offset1(pr), prec, random_x(pr, 3), " 1-based")
    assert list(got["columns"]) == [1, 2, 3]
    assert np.all(got["leak2"][0] == 0.0) and np.all(got["leak2"][1:] > 0)
    zero, _ = _graded(pr, prec, random_x(pr, 3))
    assert np.array_equal(zero["leak2"], got["leak2"])               # the same listing, the same sums, the same bits


# ---- 3. long shells of several work units ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_long_shells_of_several_units(prec):
    """40 x 40 block rows of 4 x 4, the 13-point stencil, two block columns cut at 24.5 grid steps around sources on the grid's edge: half
    rings of 92 leak positions with 272 products each (184 and 544 in all; the generator's sources sit on the edge, 190 positions is the
    most two columns give).  A unit takes at most 64 products at 4 x 4: several units per column, added in order by k_leak_col"""
    pr = PR.stencil_2d(40, 40, 4, 4, ncols=2, seed=40, radius=24.5, points=13)
    got, ref = _graded(pr, prec, random_x(pr, 41))
    assert ref["n_leak_blocks"] >= 180 and ref["n_leak_pairs"] >= 500
    assert np.all(got["units"] > 1), got["units"]
    assert np.all(got["units"] >= -(-ref["pairs_per_column"] // 64))


# ---- 4. the sum rule on the device: residual of the padded twin = residual + leak of the truncated plan ------------------------------
@pytest.mark.parametrize("prec,LM,LN", [("z", 16, 16), ("c", 4, 8)])
def test_sum_rule_on_the_device(oracle, prec, LM, LN):
    pr = PR.stencil_2d(5, 4, LM, LN, ncols=3, seed=LM + 3 * LN, radius=[1.5, 2.2, 1.1])
    X = random_x(pr, 9)
    twin, Xp = LR.padded(pr, X)
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", X)
        res, leak = s.residual(), s.truncation_leak()
    with T.Solver.open(twin, prec) as s:
        s.set_matrix("A", twin.A)
        s.set_matrix("B", twin.B)
        s.set_matrix("X", Xp)
        whole = s.residual()
        assert s.leak_counts() == (0, 0)
        assert np.all(s.truncation_leak()["leak2"] == 0.0)
    A, Xs, B = LR.stored(pr.A, prec), LR.stored(X, prec), LR.stored(pr.B, prec)
    tol = (RR.residual(oracle, pr, A, Xs, B)["bound_r2"] + LR.leak(pr, A, Xs)["bound"]
           + RR.residual(oracle, twin, A, LR.stored(Xp, prec), B)["bound_r2"])
    dev = np.abs(whole["residual2"] - (res["residual2"] + leak["leak2"]))
    print("sum rule %s %dx%d: largest deviation / bound %.3g, leak2 / residual2 up to %.3g" % (
        prec, LM, LN, (dev / tol).max(), (leak["leak2"] / res["residual2"]).max()))
    assert np.array_equal(whole["columns"], leak["columns"]) and np.all(leak["leak2"] > 0)
    assert np.all(dev <= tol)


# ---- 5. after a solve --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fd_16x16_small", "dense_random_rect"])
def test_fixtures_after_a_solve(name):
    """fd_16x16_small: X is truncated around its sources, 64 leak positions with 96 products.  dense_random_rect: every block row in
    every block column of X -- full columns, so its leak follows from the pattern: no position, exactly 0.0"""
    pr = load_problem(name)
    with T.Solver.open(pr, "z", shadow_mode=T.SHADOW_GLIBC_RAND) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 2000) == 0
        X = s.get_matrix()
        got = s.truncation_leak()
        res = s.residual()
    ref = LR.leak(pr, pr.A, X)
    _compare(got, ref, name)
    if name == "dense_random_rect":
        assert (got["n_leak_blocks"], got["n_leak_pairs"]) == (0, 0) and np.all(got["leak2"] == 0.0) and np.all(got["units"] == 0)
    else:
        assert (got["n_leak_blocks"], got["n_leak_pairs"]) == (64, 96) and np.all(got["leak2"] > 0)
        with np.errstate(divide="ignore"):
            print(name, "untruncated relative residual up to %.3e (truncated: %.3e)" % (
                np.sqrt((res["residual2"] + got["leak2"]) / res["bnorm2"]).max(), res["worst"]))


# ---- 6. preconditioned plans ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM", [("z", 8), ("m", 16)])
def test_preconditioned_plan(prec, LM):
    pr = PR.stencil_2d(4, 4, LM, LM, 2, seed=LM, radius=[1.5, 2.1])
    n_cols = 2
    # without the kept copy the caller's A is gone after the first solve: status 19, nothing written; the counts need no A
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        before = s.truncation_leak()                                 # not scaled yet: the buffer's A
        assert s.solve(1e-9, 200) == 0
        leak2, cols = np.full((n_cols, LM), SENTINEL), np.full(n_cols, -77, np.int32)
        nb, npairs = C.c_uint64(777), C.c_uint64(777)
        st = T.lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, leak2.ctypes.data_as(C.c_void_p), cols.ctypes.data_as(C.c_void_p),
                                              C.byref(nb), C.byref(npairs))
        assert T.decode(st)[::2] == (NO_IMPLEMENTATION, 0)
        assert (leak2 == SENTINEL).all() and (cols == -77).all() and nb.value == 777 and npairs.value == 777
        assert s.leak_counts() == (before["n_leak_blocks"], before["n_leak_pairs"])
    # with it: the caller's A and the back-transformed X
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 200) == 0
        X = s.get_matrix()
        got = s.truncation_leak()
        _compare(got, LR.leak(pr, pr.A, X), "kept A %s" % prec)
        assert np.all(got["leak2"] > 0)
        # a patch that no set-up has seen yet counts already: off-diagonal blocks carry the leak, so patch every second block of A
        d = np.arange(0, pr.nnzbA, 2, dtype=np.int32)
        A1 = pr.A.copy()
        A1[d] *= (1.5 + 0.5j)
        s.set_blocks("A", d, A1[d])
        patched = s.truncation_leak()
        _compare(patched, LR.leak(pr, A1, X), "kept A %s, patched" % prec)
        assert not np.array_equal(patched["leak2"], got["leak2"])


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
            res = s.residual()
            if with_call:
                vectors = [s.get_work_vector(k) for k in (1, 4, 5, 6, 7, 8, 9)]
                history, info = s.bound_history(), s.get_info()
                first = s.truncation_leak()
                second = s.truncation_leak()
                for key in ("leak2", "columns", "units"):
                    assert np.array_equal(first[key], second[key]), key
                assert np.all(first["leak2"] > 0)
                for k, v in zip((1, 4, 5, 6, 7, 8, 9), vectors):
                    assert np.array_equal(s.get_work_vector(k), v, equal_nan=True), k
                assert np.array_equal(s.bound_history(), history) and s.get_info() == info
                again = s.residual()
                for key in ("residual2", "bnorm2", "columns"):
                    assert np.array_equal(res[key], again[key]), key
            st = s.solve(tol, 200)
            return st, s.get_info()["iterations"], s.get_matrix(), s.bound_history(), res

    st0, it0, X0, h0, res0 = run(False)
    st1, it1, X1, h1, res1 = run(True)
    assert (st0, it0) == (st1, it1) and np.array_equal(X0, X1) and np.array_equal(h0, h1)
    assert np.array_equal(res0["residual2"], res1["residual2"])


# ---- 8. statuses ---------------------------------------------------------------------------------------------------------------------------
def test_statuses_change_nothing():
    pr = PR.stencil_2d(4, 4, 4, 5, 2, seed=9, radius=1.5)
    want = LR.counts(pr)
    assert want[0] > 0

    def call(s, null=False, counts_only=False):
        leak2, cols = np.full((2, 5), SENTINEL), np.full(2, -77, np.int32)
        nb, npairs = C.c_uint64(777), C.c_uint64(777)
        if null:
            return T.lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, None, None, None, None)
        st = T.lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, None if counts_only else leak2.ctypes.data_as(C.c_void_p),
                                              cols.ctypes.data_as(C.c_void_p), C.byref(nb), C.byref(npairs))
        if counts_only:
            assert st == 0 and (nb.value, npairs.value) == want and list(cols) == [0, 1] and (leak2 == SENTINEL).all()
        else:
            assert (leak2 == SENTINEL).all() and (cols == -77).all() and nb.value == 777 and npairs.value == 777
        return st

    with T.Solver.open(pr, "z", buffer=False) as s:                         # no buffer
        assert call(s, null=True) == NO_INFO_PASSED                 # ... comes behind the look at the outputs
        assert T.decode(call(s))[::2] == (POINTER_INVALID, 0)
        call(s, counts_only=True)                                   # the counts need neither a buffer nor A
        assert s.leak_counts() == want
    with T.Solver.open(pr, "z") as s:                                       # no A
        s.set_matrix("B", pr.B)
        x_before = s.get_work_vector(1)
        s.set_operator(lambda *a: 0.0)                              # a user-defined operator comes before the missing A
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert T.decode(call(s))[::2] == (UNDOCUMENTED, ord("A"))
        call(s, counts_only=True)
        s.set_matrix("A", pr.A)
        assert call(s, null=True) == NO_INFO_PASSED                 # all four outputs NULL
        s.set_operator(lambda *a: 0.0)
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert np.array_equal(s.get_work_vector(1), x_before, equal_nan=True)
        got = s.truncation_leak()                                   # ... and the call works again
        assert got["leak2"].shape == (2, 5) and (got["n_leak_blocks"], got["n_leak_pairs"]) == want
