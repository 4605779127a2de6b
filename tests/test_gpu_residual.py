"""tfqmrgpuExt_residual (include/tfqmrgpu_ext.h section 10) on the GPU, through the C-ABI: |B - A X|^2 and |B|^2 per (block column,
right-hand side) against the numpy restatement (tests/residual_ref.py), with the a-priori bound derived there -- the kernel and numpy sum
the same exact-or-double products in double and differ in the order of the sums only.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import precond_ref as PC
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import random_x
from tfqmrgpu_amd import problems as PR
from tolerances import Z_TOL

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
          (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]                       # kAllowedBlockSizes
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 3, 7, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
SENTINEL = -12345.0


def _compare(got, ref, what=""):
    """residual2 and bnorm2 within the a-priori bound, entry by entry; columns exact"""
    for key, bound in (("residual2", "bound_r2"), ("bnorm2", "bound_b2")):
        dev = np.abs(got[key] - ref[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            print(what, key, "largest deviation / bound: %.3g" % np.nanmax(np.where(ref[bound] > 0, dev / ref[bound], 0.0)))
        assert got[key].shape == ref[key].shape
        assert np.all(dev <= ref[bound]), (what, key, float(dev.max()), float(ref[bound].min()))
    assert np.array_equal(got["columns"], ref["columns"])


def _compare_worst(got_worst, ref, what=""):
    w, dq = RR.worst(ref)
    print(what, "worst %.6e reference %.6e, |difference of squares| %.3g, bound %.3g" % (got_worst, w, abs(got_worst ** 2 - w ** 2), dq))
    assert abs(got_worst ** 2 - w ** 2) <= dq
    return w


def _graded(oracle, pr, prec, X, seed_note=""):
    """set A, B and a caller's X on a fresh plan, do not solve, compare with numpy on the data as the plan stores it"""
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", X)
        got = s.residual()
        view = s.plan_view()
    ref = RR.residual(oracle, pr, RR.stored(pr.A, prec), RR.stored(X, prec), RR.stored(pr.B, prec))
    _compare(got, ref, "%dx%d %s%s" % (pr.LM, pr.LN, prec, seed_note))
    assert np.array_equal(got["columns"], view["original_bsrColIndX"])
    assert got["residual2"].shape == (view["nCols"], pr.LN)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(got["relative"], np.sqrt(got["residual2"] / got["bnorm2"]))
    assert got["worst"] == np.nanmax(got["relative"])
    assert got["residual2"].min() > 0.01 * got["bnorm2"].min()       # the residual is O(1): every element matters
    return got


# ---- 1. every shape, every precision -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("LM,LN", SHAPES)
def test_every_shape_and_precision(oracle, LM, LN, prec):
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN)
    _graded(oracle, pr, prec, random_x(pr, 7 * LM + LN))


@pytest.mark.parametrize("LM,LN,prec", [(4, 5, "z"), (8, 8, "c"), (16, 16, "z"), (16, 32, "m")])
def test_ragged_columns_and_index_offset(oracle, LM, LN, prec):
    """block columns of different lengths (truncated around their sources), most X blocks without a B block, 1-based indices"""
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=LM + LN, radius=[None, 1.1, 2.3])
    assert len(set(np.bincount(pr.colIndX))) == 3
    one = T.Problem(pr.rowPtrA + 1, pr.colIndA + 1, pr.A, pr.rowPtrX + 1, pr.colIndX + 1, pr.rowPtrB + 1, pr.colIndB + 1, pr.B, None,
                    pr.tolerance, 1)
    got = _graded(oracle, one, prec, random_x(pr, 3))
    assert list(got["columns"]) == [1, 2, 3]


# ---- 2. several chunks per block column ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_long_columns_of_several_chunks(oracle, prec):
    """40 x 40 block rows of 4 x 4: a block column holds 1600 blocks of 256 | 128 bytes, a chunk at most 16 KiB of them (tfq_plan.cpp:
    cutChunks), so every column is cut into 25 chunks or more: the chunk records and the order of k_residual_col"""
    pr = PR.stencil_2d(40, 40, 4, 4, ncols=2, seed=40)
    assert np.bincount(pr.colIndX).min() == 1600 and 1600 * 2 * 4 * 4 * 4 > 16 * 1024
    _graded(oracle, pr, prec, random_x(pr, 41))


# ---- 3. the golden fixtures, after a solve -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fd_4x4_2d", "dense_random_rect", "julia_kat", "fd_16x16_small"])
def test_fixtures_after_a_solve(oracle, name):
    pr = load_problem(name)
    with T.Solver.open(pr, "z", shadow_mode=T.SHADOW_GLIBC_RAND) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        st = s.solve(1e-9, 2000)
        info, X = s.get_info(), s.get_matrix()
        got = s.residual()
    ref = RR.residual(oracle, pr, pr.A, X)
    _compare(got, ref, name)
    w = _compare_worst(got["worst"], ref, name)
    helper = PC.worst_relative_residual(oracle, pr, X)
    assert abs(helper ** 2 - w ** 2) <= RR.worst(ref)[1]             # the two numpy restatements are the same sums
    assert abs(got["worst"] ** 2 - helper ** 2) <= RR.worst(ref)[1]
    print(name, "status", st, "iterations", info["iterations"], "residuum_reached %.6e worst %.6e" % (info["residual"], got["worst"]))
    if st == 0:
        assert got["worst"] <= 1e-9
    # getInfo's figure is the solver's own probe of the same X (double on a 'z' plan, another order of the sums): the relative
    # difference that the fixture's entry allows for residuals
    assert abs(info["residual"] - got["worst"]) <= Z_TOL[name]["res"] * max(info["residual"], got["worst"])


# ---- 4. what float cannot see ----------------------------------------------------------------------------------------------------------
def test_float_plan_graded_in_double(oracle):
    """fd_16x16_small in 'c', iterated to the float floor: the call's double sums over the float data against numpy's.
    How far getInfo's float probe is from it is recorded, not asserted."""
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "c") as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        st = s.solve(1e-9, 300)                                      # out of reach in float: the solve runs into its floor
        info, X = s.get_info(), s.get_matrix()
        got = s.residual()
    assert np.array_equal(X, X.astype(np.complex64))                 # float data, as the plan holds it
    ref = RR.residual(oracle, pr, RR.stored(pr.A, "c"), X.astype(np.complex128), RR.stored(pr.B, "c"))
    _compare(got, ref, "fd_16x16_small c")
    _compare_worst(got["worst"], ref, "fd_16x16_small c")
    print("fd_16x16_small c: status %d after %d iterations, residuum_reached (float probe) %.6e, worst (double) %.6e, ratio %.4f"
          % (st, info["iterations"], info["residual"], got["worst"], info["residual"] / got["worst"]))


# ---- 5. preconditioned plans -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM", [("z", 8), ("m", 16)])
def test_preconditioned_plan(oracle, prec, LM):
    pr = PR.stencil_2d(4, 4, LM, LM, 2, seed=LM)
    n_cols = 2
    # without the kept copy the caller's A is gone after the solve: status 19, nothing written
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 200) == 0
        r2, b2 = np.full((n_cols, LM), SENTINEL), np.full((n_cols, LM), SENTINEL)
        cols, worst = np.full(n_cols, -77, np.int32), C.c_double(SENTINEL)
        st = T.lib.tfqmrgpuExt_residual(s.handle, s.plan, r2.ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p),
                                        cols.ctypes.data_as(C.c_void_p), C.byref(worst))
        assert T.decode(st)[::2] == (NO_IMPLEMENTATION, 0)
        assert (r2 == SENTINEL).all() and (b2 == SENTINEL).all() and (cols == -77).all() and worst.value == SENTINEL
    # with it: the caller's A and the back-transformed X
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", np.zeros((pr.nnzbX, LM, LM), np.complex128))
        before = s.residual()                                        # not scaled yet: the buffer's A; X = 0, so r = -b exactly
        assert np.array_equal(before["residual2"], before["bnorm2"]) and before["worst"] == 1.0
        assert s.solve(1e-9, 200) == 0
        X = s.get_matrix()
        got = s.residual()
        ref = RR.residual(oracle, pr, pr.A, X)
        _compare(got, ref, "kept A %s" % prec)
        _compare_worst(got["worst"], ref, "kept A %s" % prec)
        assert got["worst"] <= 1e-9
        # a patch of the diagonal blocks that no set-up has seen yet counts already
        d = PC.diagonal_blocks(pr)
        d = d[d >= 0].astype(np.int32)[::2]
        A1 = pr.A.copy()
        A1[d] += 0.3 * np.eye(LM) * (1 + 0.5j)
        s.set_blocks("A", d, A1[d])
        patched = s.residual()
        ref1 = RR.residual(oracle, pr, A1, X)
        _compare(patched, ref1, "kept A %s, patched" % prec)
        assert patched["worst"] > 1e-3                               # the old solution does not solve the patched system
    assert np.array_equal(before["bnorm2"], got["bnorm2"])


# ---- 6. non-destructive and deterministic --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM,LN", [("z", 16, 16), ("c", 4, 5), ("z", 8, 32)])
def test_non_destructive_and_deterministic(prec, LM, LN):
    pr = PR.stencil_2d(5, 4, LM, LN, ncols=3, seed=LM + 2 * LN, radius=2.2)
    tol = 1e-9 if prec == "z" else 1e-4

    def run(with_call):
        with T.Solver.open(pr, prec) as s:
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            assert s.solve(tol, 200) == 0
            first = None
            if with_call:
                vectors = [s.get_work_vector(k) for k in (1, 4, 5, 6, 7, 8, 9)]
                history, info = s.bound_history(), s.get_info()
                first = s.residual()
                second = s.residual()
                for key in ("residual2", "bnorm2", "columns", "relative"):
                    assert np.array_equal(first[key], second[key], equal_nan=(key == "relative")), key
                assert first["worst"] == second["worst"]
                for k, v in zip((1, 4, 5, 6, 7, 8, 9), vectors):
                    assert np.array_equal(s.get_work_vector(k), v, equal_nan=True), k
                assert np.array_equal(s.bound_history(), history) and s.get_info() == info
            st = s.solve(tol, 200)
            return st, s.get_info()["iterations"], s.get_matrix(), s.bound_history(), first

    st0, it0, X0, h0, _ = run(False)
    st1, it1, X1, h1, first = run(True)
    assert (st0, it0) == (st1, it1) and np.array_equal(X0, X1) and np.array_equal(h0, h1)
    if prec == "z":                                                  # (a float probe certifies its own sums, not the double ones)
        assert first["worst"] <= tol


# ---- 7. a right-hand side that is zero ---------------------------------------------------------------------------------------------------
def test_zero_right_hand_side(oracle):
    # (the problem of tests/test_gpu_parity.py: test_edge_zero_right_hand_side_column)
    pr = PR.stencil_2d(4, 4, 4, 8, 2, seed=17, radius=2.0)
    pr.B[:, :, 5] = 0
    with T.Solver.open(pr, "z", shadow_mode=T.SHADOW_GLIBC_RAND) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.solve(1e-9, 100)
        got = s.residual()
        keep = [j for j in range(8) if j != 5]
        assert np.all(got["bnorm2"][:, 5] == 0) and np.all(got["bnorm2"][:, keep] > 0)
        assert np.all(np.isnan(got["relative"][:, 5]))               # 0 / 0, or a NaN solution: NaN either way
        assert np.all(np.isfinite(got["relative"][:, keep]))
        assert got["worst"] == got["relative"][:, keep].max()        # NaN entries are left out
        # X = 0 there: r = b = 0 exactly
        X = random_x(pr, 5)
        X[:, :, 5] = 0
        s.set_matrix("X", X)
        got = s.residual()
        assert np.all(got["residual2"][:, 5] == 0) and np.all(np.isnan(got["relative"][:, 5]))
        assert np.isfinite(got["worst"]) and got["worst"] == got["relative"][:, keep].max()
        # a non-zero X there: r > 0 = b
        s.set_matrix("X", random_x(pr, 6))
        got = s.residual()
        assert np.all(np.isposinf(got["relative"][:, 5])) and np.isposinf(got["worst"])
        _compare(got, RR.residual(oracle, pr, pr.A, random_x(pr, 6)), "zero right-hand side")
    # every right-hand side zero: worst is NaN only then
    pr.B[:] = 0
    with T.Solver.open(pr, "z") as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", np.zeros((pr.nnzbX, 4, 8), np.complex128))
        got = s.residual()
        assert np.all(np.isnan(got["relative"])) and np.isnan(got["worst"])


# ---- 8. statuses ---------------------------------------------------------------------------------------------------------------------------
def test_statuses_change_nothing():
    pr = PR.stencil_2d(4, 4, 4, 5, 2, seed=9)

    def call(s, null=False):
        r2, b2 = np.full((2, 5), SENTINEL), np.full((2, 5), SENTINEL)
        cols, worst = np.full(2, -77, np.int32), C.c_double(SENTINEL)
        if null:
            return T.lib.tfqmrgpuExt_residual(s.handle, s.plan, None, None, None, None)
        st = T.lib.tfqmrgpuExt_residual(s.handle, s.plan, r2.ctypes.data_as(C.c_void_p), b2.ctypes.data_as(C.c_void_p),
                                        cols.ctypes.data_as(C.c_void_p), C.byref(worst))
        assert (r2 == SENTINEL).all() and (b2 == SENTINEL).all() and (cols == -77).all() and worst.value == SENTINEL
        return st

    with T.Solver.open(pr, "z", buffer=False) as s:                         # no buffer
        assert T.decode(call(s))[::2] == (POINTER_INVALID, 0)
    with T.Solver.open(pr, "z") as s:                                       # no A
        s.set_matrix("B", pr.B)
        assert T.decode(call(s))[::2] == (UNDOCUMENTED, ord("A"))
        s.set_matrix("A", pr.A)
        assert call(s, null=True) == NO_INFO_PASSED                 # all four outputs NULL
        x_before = s.get_work_vector(1)
        s.set_operator(lambda *a: 0.0)                              # a user-defined operator is the caller's to apply
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert np.array_equal(s.get_work_vector(1), x_before, equal_nan=True)
        assert s.residual()["residual2"].shape == (2, 5)            # ... and the call works again
