"""tfqmrgpuExt_leakMap and the loop it closes (include/tfqmrgpu_ext.h section 12) on the GPU, through the C-ABI: |(A X)(i, c)(:, j)|^2 for
every leak position, against the numpy restatement (tests/leak_map_ref.py) with the a-priori bound derived there -- the kernel and numpy
sum the same exact-or-double products in double and differ in the order of the sums only.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import leak_map_ref as MR
import leak_ref as LR
import tfqmrgpu_amd as T
from conftest import offset1
from helpers import random_x
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

SHAPES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
          (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]                       # kAllowedBlockSizes
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 3, 7, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
SENTINEL = -12345.0


def _compare(got, ref, what=""):
    """rows, cols and the count exact; every pos2 entry within its a-priori bound"""
    assert got["n_leak_blocks"] == ref["n_leak_blocks"]
    assert np.array_equal(got["rows"], ref["rows"]) and np.array_equal(got["cols"], ref["cols"])
    assert got["pos2"].shape == ref["pos2"].shape and got["pos2"].dtype == np.float64
    dev = np.abs(got["pos2"] - ref["pos2"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(what, "pos2: largest deviation / bound: %.3g" % (np.nanmax(np.where(ref["bound"] > 0, dev / ref["bound"], 0.0)) if dev.size else 0.0),
              "positions", got["n_leak_blocks"])
    assert np.all(dev <= ref["bound"]), (what, float(dev.max()), float(ref["bound"].min()))


def _graded(pr, prec, X, what=""):
    """set A, B and a caller's X on a fresh plan, do not solve, compare with numpy on the data as the plan stores it"""
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        s.set_matrix("X", X)
        got = s.leak_map()
        leak = s.truncation_leak()
    ref = MR.leak_map(pr, MR.stored(pr.A, prec), MR.stored(X, prec))
    _compare(got, ref, "%dx%d %s%s" % (pr.LM, pr.LN, prec, what))
    return got, ref, leak


def _column_sums(pos2, cols, n_cols):
    """per block column the pos2 of its positions, added in position order"""
    out = np.zeros((n_cols, pos2.shape[1]))
    for p in range(len(cols)):
        out[cols[p]] += pos2[p]
    return out


def _sum_rule(pr, prec, X, got, ref, leak, what=""):
    """per (block column, right-hand side): the positions of the map add up to leak2 of truncation_leak(), within the sum of the two
    a-priori bounds (not bit for bit: the two kernels add in different orders)"""
    n_cols = leak["leak2"].shape[0]
    tol = LR.leak(pr, LR.stored(pr.A, prec), LR.stored(X, prec))["bound"] + _column_sums(ref["bound"], ref["cols"], n_cols)
    dev = np.abs(_column_sums(got["pos2"], got["cols"], n_cols) - leak["leak2"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(what, "sum rule: largest deviation / bound %.3g" % np.nanmax(np.where(tol > 0, dev / tol, 0.0)))
    assert got["n_leak_blocks"] == leak["n_leak_blocks"]
    assert np.all(dev <= tol)


# ---- 1. every shape, every precision; the sum rule ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("LM,LN", SHAPES)
def test_every_shape_and_precision(LM, LN, prec):
    """one full column -- it contributes no position -- and two truncated ones"""
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN, radius=[None, 1.1, 2.3])
    X = random_x(pr, 7 * LM + LN)
    got, ref, leak = _graded(pr, prec, X)
    assert got["n_leak_blocks"] > 0 and 0 not in got["cols"] and {1, 2} == set(got["cols"].tolist())
    assert np.all(got["pos2"] > 0)
    _sum_rule(pr, prec, X, got, ref, leak, "%dx%d %s" % (LM, LN, prec))


# ---- 2. 1-based indices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LM,LN,prec", [(4, 5, "z"), (8, 8, "c"), (16, 16, "z"), (16, 32, "m")])
def test_index_offset(LM, LN, prec):
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=LM + LN, radius=[None, 1.1, 2.3])
    zero, _, _ = _graded(pr, prec, random_x(pr, 3))
    one, _, _ = _graded(offset1(pr), prec, random_x(pr, 3), " 1-based")
    for key in ("rows", "cols", "pos2"):                             # the same listing, the same sums, the same bits
        assert np.array_equal(zero[key], one[key]), key


# ---- 3. long shells -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_long_shells(prec):
    """40 x 40 block rows of 4 x 4, the 13-point stencil, two block columns cut at 24.5 grid steps: 184 positions with one to four
    products each -- several work units of section 11 per column, several work groups and rounds of the map"""
    pr = PR.stencil_2d(40, 40, 4, 4, ncols=2, seed=40, radius=24.5, points=13)
    X = random_x(pr, 41)
    got, ref, leak = _graded(pr, prec, X)
    assert got["n_leak_blocks"] >= 180 and np.all(leak["units"] > 1)
    with T.Solver.open(pr, prec, buffer=False) as s:
        view = s.plan_view()
    assert leak["n_leak_pairs"] > got["n_leak_blocks"] and view["nCols"] == 2      # positions of different product counts
    _sum_rule(pr, prec, X, got, ref, leak, "long shells %s" % prec)


def test_many_positions_per_wave():
    """16 x 16 `z`: a wave takes a whole position, and every fourth position of its work group's run of 32 -- 38 positions: eight per
    wave in the first work group, a second work group whose last two waves have one position and the others two"""
    pr = PR.stencil_2d(9, 9, 16, 16, ncols=3, seed=88, radius=2.3)
    X = random_x(pr, 89)
    got, ref, leak = _graded(pr, "z", X)
    assert 32 + 4 < got["n_leak_blocks"] < 64
    _sum_rule(pr, "z", X, got, ref, leak, "many positions per wave")


# ---- 4. preconditioned plans ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM", [("z", 8), ("m", 16)])
def test_preconditioned_plan(prec, LM):
    pr = PR.stencil_2d(4, 4, LM, LM, 2, seed=LM, radius=[1.5, 2.1])
    # without the kept copy the caller's A is gone after the first solve: status 19, nothing written; the positions need no A
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        before = s.leak_map()                                        # not scaled yet: the buffer's A
        assert s.solve(1e-9, 200) == 0
        n = before["n_leak_blocks"]
        rows, cols, pos2 = np.full(n, -77, np.int32), np.full(n, -77, np.int32), np.full((n, LM), SENTINEL)
        nb = C.c_uint64(777)
        st = T.lib.tfqmrgpuExt_leakMap(s.handle, s.plan, n, C.c_void_p(rows.ctypes.data), C.c_void_p(cols.ctypes.data),
                                       C.c_void_p(pos2.ctypes.data), C.byref(nb))
        assert T.decode(st)[::2] == (NO_IMPLEMENTATION, 0)
        assert (pos2 == SENTINEL).all() and (rows == -77).all() and (cols == -77).all() and nb.value == 777
        again = s.leak_map(values=False)
        assert np.array_equal(again["rows"], before["rows"]) and np.array_equal(again["cols"], before["cols"])
    # with it: the caller's A and the back-transformed X
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 200) == 0
        X = s.get_matrix()
        got = s.leak_map()
        _compare(got, MR.leak_map(pr, pr.A, X), "kept A %s" % prec)
        # a patch that no set-up has seen yet counts already: off-diagonal blocks carry the leak, so patch every second block of A
        d = np.arange(0, pr.nnzbA, 2, dtype=np.int32)
        A1 = pr.A.copy()
        A1[d] *= (1.5 + 0.5j)
        s.set_blocks("A", d, A1[d])
        patched = s.leak_map()
        _compare(patched, MR.leak_map(pr, A1, X), "kept A %s, patched" % prec)
        assert not np.array_equal(patched["pos2"], got["pos2"])


# ---- 5. non-destructive and deterministic, between two solves ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM,LN", [("z", 16, 16), ("c", 4, 5), ("z", 8, 32)])
def test_non_destructive_and_deterministic(prec, LM, LN):
    pr = PR.stencil_2d(5, 4, LM, LN, ncols=3, seed=LM + 2 * LN, radius=2.2)
    tol = 1e-9 if prec == "z" else 1e-4

    def run(with_call):
        with T.Solver.open(pr, prec) as s:
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            assert s.solve(tol, 200) == 0
            res, leak = s.residual(), s.truncation_leak()
            if with_call:
                vectors = [s.get_work_vector(k) for k in (1, 4, 5, 6, 7, 8, 9)]
                history, info = s.bound_history(), s.get_info()
                first = s.leak_map()
                second = s.leak_map()
                for key in ("rows", "cols", "pos2"):
                    assert np.array_equal(first[key], second[key]), key
                assert np.all(first["pos2"] > 0)
                for k, v in zip((1, 4, 5, 6, 7, 8, 9), vectors):
                    assert np.array_equal(s.get_work_vector(k), v, equal_nan=True), k
                assert np.array_equal(s.bound_history(), history) and s.get_info() == info
                again, leak_again = s.residual(), s.truncation_leak()
                for key in ("residual2", "bnorm2", "columns"):
                    assert np.array_equal(res[key], again[key]), key
                for key in ("leak2", "columns", "units"):
                    assert np.array_equal(leak[key], leak_again[key]), key
            st = s.solve(tol, 200)
            return st, s.get_info()["iterations"], s.get_matrix(), s.bound_history(), res, leak

    st0, it0, X0, h0, res0, leak0 = run(False)
    st1, it1, X1, h1, res1, leak1 = run(True)
    assert (st0, it0) == (st1, it1) and np.array_equal(X0, X1) and np.array_equal(h0, h1)
    assert np.array_equal(res0["residual2"], res1["residual2"]) and np.array_equal(leak0["leak2"], leak1["leak2"])


# ---- 6. end to end: solve, leak map, grown pattern, new plan -------------------------------------------------------------------------------
def test_chain_end_to_end():
    """1-D chain of 4 block rows, tridiagonal A, one block column cut to the rows 0, 1, 2: the map names exactly row 3, and the plan of
    the grown pattern leaks nothing"""
    mb, LM, LN = 4, 4, 4
    rpA, ciA = [0], []
    for r in range(mb):
        ciA += [c for c in (r - 1, r, r + 1) if 0 <= c < mb]
        rpA.append(len(ciA))
    A = (PR.hashed_uniform(1, (len(ciA), LM, LM)) + 1j * PR.hashed_uniform(2, (len(ciA), LM, LM))) / (3 * LM)
    for q, (r, c) in enumerate(zip(np.repeat(np.arange(mb), np.diff(rpA)), ciA)):
        if r == c:
            A[q] += 2.0 * np.eye(LM)
    B = PR.hashed_uniform(3, (1, LM, LN)) + 1j * PR.hashed_uniform(4, (1, LM, LN))
    pr = T.Problem(rpA, ciA, A, [0, 1, 2, 3, 3], [0, 0, 0], [0, 0, 1, 1, 1], [0], B)
    with T.Solver.open(pr, "z") as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 200) == 0
        got = s.leak_map()
        assert got["rows"].tolist() == [3] and got["cols"].tolist() == [0] and np.all(got["pos2"] > 0)
        _compare(got, MR.leak_map(pr, pr.A, s.get_matrix()), "chain")
        grown = s.grow_problem(pr, [0])
        assert np.array_equal(grown.rowPtrX, [0, 1, 2, 3, 4]) and np.array_equal(grown.colIndX, [0, 0, 0, 0])
    with T.Solver.open(grown, "z") as s:
        assert s.leak_counts() == (0, 0)
        s.set_matrix("A", grown.A)
        s.set_matrix("B", grown.B)
        assert s.solve(1e-9, 200) == 0
        assert np.all(s.truncation_leak()["leak2"] == 0.0)
        empty = s.leak_map()
        assert empty["n_leak_blocks"] == 0 and empty["pos2"].shape == (0, LN)
        assert s.residual()["worst"] < 1e-8


# ---- 7. statuses ---------------------------------------------------------------------------------------------------------------------------
def test_statuses_change_nothing():
    pr = PR.stencil_2d(4, 4, 4, 5, 2, seed=9, radius=1.5)
    want = MR.positions(pr)
    n = len(want)
    assert n > 0

    def call(s, null=False, patterns_only=False, capacity=n):
        rows, cols, pos2 = np.full(n, -77, np.int32), np.full(n, -77, np.int32), np.full((n, 5), SENTINEL)
        nb = C.c_uint64(777)
        if null:
            return T.lib.tfqmrgpuExt_leakMap(s.handle, s.plan, n, None, None, None, None)
        st = T.lib.tfqmrgpuExt_leakMap(s.handle, s.plan, capacity, C.c_void_p(rows.ctypes.data), C.c_void_p(cols.ctypes.data),
                                       None if patterns_only else C.c_void_p(pos2.ctypes.data), C.byref(nb))
        if patterns_only:
            assert st == 0 and nb.value == n and list(zip(cols.tolist(), rows.tolist())) == want and (pos2 == SENTINEL).all()
        else:
            assert (pos2 == SENTINEL).all() and (rows == -77).all() and (cols == -77).all()
            assert nb.value == (n if T.decode(st)[2] == ord("X") else 777)
        return st

    with T.Solver.open(pr, "z", buffer=False) as s:                         # no buffer
        assert call(s, null=True) == NO_INFO_PASSED                 # ... comes behind the look at the outputs
        assert T.decode(call(s))[::2] == (POINTER_INVALID, 0)
        call(s, patterns_only=True)                                 # the positions need neither a buffer nor A
    with T.Solver.open(pr, "z") as s:                                       # no A
        s.set_matrix("B", pr.B)
        x_before = s.get_work_vector(1)
        s.set_operator(lambda *a: 0.0)                              # a user-defined operator comes before the missing A
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert T.decode(call(s))[::2] == (UNDOCUMENTED, ord("A"))
        assert T.decode(call(s, capacity=0))[::2] == (UNDOCUMENTED, ord("A"))     # ... and before the small capacity
        call(s, patterns_only=True)
        s.set_matrix("A", pr.A)
        assert call(s, null=True) == NO_INFO_PASSED                 # all four outputs NULL
        assert T.decode(call(s, capacity=n - 1))[::2] == (UNDOCUMENTED, ord("X"))  # the count is filled in, nothing else
        s.set_operator(lambda *a: 0.0)
        assert T.decode(call(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert np.array_equal(s.get_work_vector(1), x_before, equal_nan=True)
        got = s.leak_map()                                          # ... and the call works again
        assert got["pos2"].shape == (n, 5) and list(zip(got["cols"].tolist(), got["rows"].tolist())) == want
