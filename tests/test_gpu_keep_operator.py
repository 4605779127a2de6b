"""tfqmrgpuExt_keepOperator (include/tfqmrgpu_ext.h section 9) on the GPU, through the C-ABI: a preconditioned plan that keeps the caller's A
takes setBlocks('A') and a change of the preconditioner kind.  The yardstick is always the path that is pinned to the oracle already
(tests/test_gpu_precond.py): a FRESH plan, whole setMatrix('A') of the patched matrix, preconditioned solve.  The partial set-up shares
its element loops with the whole one, so "the same" is exact (np.array_equal): status, iteration count, bound history, getInfo's
residual, X, M^-1 and the number of unit matrices, for 'm' also the refinement history.  Needs an MI355X (`pytest -m gpu`)."""
import numpy as np
import pytest

import precond_ref as PC
import tfqmrgpu_amd as T
from helpers import user_array, with_a
from solve_helpers import (BJ, MAXIT, TOL, changed, fresh_solve, patch_blocks, present_diagonal, same_record, solve_and_check_residual,
                           solve_record, system_with_two_unit_rows)
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

def _system(LM, seed=None):
    """the smallest system with more than one block per block column and per work group: 4 x 4 grid, 16 block rows, 64 blocks of A"""
    return PR.stencil_2d(4, 4, LM, LM, 2, seed=LM if seed is None else seed)


# ---- 1. all diagonal blocks: the energy loop -----------------------------------------------------------------------------------------
# LM 4 ... 16: one wave inverts a block, 32 and 64: four waves; 'z' 8 and 16, 'c' 16: interleaved element orders; 'm': two copies of A
CASES = [("z", 4), ("z", 8), ("z", 16), ("z", 32), ("z", 64), ("c", 16), ("m", 16)]


@pytest.fixture(scope="module")
def energy_loop():
    """per case, computed once: (problem, A1, what the patched plan's two solves left behind)"""
    cache = {}

    def run(prec, LM):
        if (prec, LM) not in cache:
            pr = _system(LM)
            diag = present_diagonal(pr)
            assert len(diag) == pr.mb
            A1 = changed(pr, pr.A, diag, seed=70 + LM)
            with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
                s.set_matrix("A", pr.A)
                s.set_matrix("B", pr.B)
                first = solve_record(s, prec)
                patch_blocks(s, diag, A1)                                 # status 19 without the kept copy
                second = solve_record(s, prec)
            cache[(prec, LM)] = (pr, A1, first, second)
        return cache[(prec, LM)]
    return run


@pytest.mark.parametrize("prec,LM", CASES)
def test_all_diagonal_blocks_patched(energy_loop, prec, LM):
    pr, A1, first, second = energy_loop(prec, LM)
    same_record(first, fresh_solve(pr, pr.A, prec))                                 # the copy does not change the first solve
    same_record(second, fresh_solve(pr, A1, prec))
    assert second["status"] == 0 and second["n_identity"] == 0
    assert not np.array_equal(second["Minv"], first["Minv"]) and not np.array_equal(second["X"], first["X"])


# ---- 8. the same solve by a residual that the library has no part in ----------------------------------------------------------------
def test_patched_solve_by_the_float64_residual(oracle, energy_loop):
    """max over the right-hand sides of |B - A1 X| / |B| in float64 with numpy, truncated to the pattern of X (tests/precond_ref.py), held
    as tests/test_gpu_precond.py: _solve_and_check_residual holds its own fixtures: not above the threshold, and within 1e-4 of the
    residual that the library reports ('z')"""
    prec, tol = "z", TOL["z"]
    pr, A1, _, second = energy_loop(prec, 16)
    worst = PC.worst_relative_residual(oracle, with_a(pr, A1), second["X"])
    print("keep_operator residual: %d iterations, threshold %.0e, reported %.6e, recomputed %.6e (%.2e of it apart)" % (
        second["iterations"], tol, second["residual"], worst, abs(worst - second["residual"]) / second["residual"]))
    assert second["status"] == 0
    assert worst <= tol, worst
    assert abs(worst - second["residual"]) <= 1e-4 * second["residual"], (worst, second["residual"])
    # and the helper itself on the patched system: the fresh solve it runs ends at the same residual
    _, info = solve_and_check_residual(oracle, with_a(pr, A1), prec, tol, maxit=MAXIT)
    assert info["residual"] == second["residual"] and info["iterations"] == second["iterations"]


# ---- 2. a sparse patch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LM,trans,layout", [(16, "n", T.LAYOUT_RIRIRIRI), (8, "t", T.LAYOUT_RRRRIIII)])
def test_sparse_patch(LM, trans, layout):
    """two diagonal blocks and one off-diagonal block of a third block column: two rows are inverted again, three columns scaled again"""
    prec = "z"
    pr = _system(LM)
    diag = PC.diagonal_blocks(pr)
    rows, cols = PC.block_rows(pr.rowPtrA), pr.colIndA
    off = int(np.flatnonzero((cols == 9) & (rows != 9))[0])
    blocks = np.array([diag[13], off, diag[2]], dtype=np.int32)          # not in ascending order
    assert len({int(cols[b]) for b in blocks}) == 3
    A1 = changed(pr, pr.A, blocks, seed=31)
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", user_array(pr.A, layout, trans), trans, layout)
        s.set_matrix("B", pr.B)
        first = solve_record(s, prec)
        patch_blocks(s, blocks, A1, trans, layout)
        second = solve_record(s, prec)
    want = fresh_solve(pr, A1, prec, trans=trans, layout=layout)
    same_record(second, want)
    untouched = np.setdiff1d(np.arange(pr.mb), [13, 2])
    assert np.array_equal(second["Minv"][untouched], first["Minv"][untouched])
    assert not np.array_equal(second["Minv"][13], first["Minv"][13]) and not np.array_equal(second["Minv"][2], first["Minv"][2])


# ---- 3. patches add up ---------------------------------------------------------------------------------------------------------------
def test_patches_accumulate():
    prec, LM = "z", 16
    pr = _system(LM)
    diag = PC.diagonal_blocks(pr).astype(np.int32)
    rows, cols = PC.block_rows(pr.rowPtrA), pr.colIndA
    off = int(np.flatnonzero((cols == 6) & (rows != 6))[0])
    list1, list2, list3 = diag[[1, 4]], np.array([diag[11], off, diag[4]], dtype=np.int32), diag[[4, 15]]   # block diag[4] in all three
    A1 = changed(pr, pr.A, list1, seed=41)
    A2 = changed(pr, A1, list2, seed=43)
    A3 = changed(pr, A2, list3, seed=45)
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        solve_record(s, prec)
        patch_blocks(s, list1, A1)
        patch_blocks(s, list2, A2)
        second = solve_record(s, prec)
        patch_blocks(s, list3, A3)
        third = solve_record(s, prec)
    same_record(second, fresh_solve(pr, A2, prec))
    same_record(third, fresh_solve(pr, A3, prec))
    assert not np.array_equal(third["X"], second["X"])


# ---- 4. rows that become regular, rows that become singular -------------------------------------------------------------------------------
def test_singular_rows_follow_the_patches():
    """tests/test_gpu_precond.py: _system_with_two_unit_rows: block row 3 has no diagonal block, that of block row 7 a zero row"""
    prec = "z"
    pr = system_with_two_unit_rows()
    diag = PC.diagonal_blocks(pr)
    A1 = pr.A.copy()
    A1[diag[7], 1, :] = 0.01
    A1[diag[7], 1, 1] = 2.0                                              # regular again
    A2 = A1.copy()
    A2[diag[12]] = 0                                                     # no pivot at all
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        first = solve_record(s, prec)
        patch_blocks(s, np.array([diag[7]], dtype=np.int32), A1)
        second = solve_record(s, prec)
        patch_blocks(s, np.array([diag[12]], dtype=np.int32), A2)
        third = solve_record(s, prec)
    assert (first["n_identity"], second["n_identity"], third["n_identity"]) == (2, 1, 2)
    assert np.array_equal(second["Minv"][3], np.eye(8)) and not np.array_equal(second["Minv"][7], np.eye(8))
    assert np.array_equal(third["Minv"][12], np.eye(8))
    for got, A in ((first, pr.A), (second, A1), (third, A2)):
        same_record(got, fresh_solve(pr, A, prec))


# ---- 5. the kind changes without a new matrix -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "m"])
def test_kind_switch_without_a_new_matrix(prec):
    pr = _system(16)
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        scaled = solve_record(s, prec)
        s.set_preconditioner(T.PRECOND_NONE)                             # status 14, key 'A', without the kept copy
        plain = solve_record(s, prec, precond=False)
        s.set_preconditioner(BJ)
        again = solve_record(s, prec)
    same_record(plain, fresh_solve(pr, pr.A, prec, kind=None))
    same_record(again, scaled)
    same_record(scaled, fresh_solve(pr, pr.A, prec))


# ---- 6. off is off -------------------------------------------------------------------------------------------------------------------
def test_off_is_off():
    prec = "z"
    pr = _system(16)
    diag = present_diagonal(pr)
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.keep_operator(True)
        s.keep_operator(False)
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        same_record(solve_record(s, prec), fresh_solve(pr, pr.A, prec))
        st = T.lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, b"A", 1, T._ptr(diag[:1]), T._ptr(np.ascontiguousarray(pr.A[diag[:1]])), b"z", b"n",
                                         T.LAYOUT_RIRIRIRI)
        assert T.decode(st)[0] == 19                                     # TFQMRGPU_NO_IMPLEMENTATION, as ever
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:        # switched off AFTER the copy was made: the copy goes, 19 again
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        solve_record(s, prec)
        s.keep_operator(False)
        st = T.lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, b"A", 1, T._ptr(diag[:1]), T._ptr(np.ascontiguousarray(pr.A[diag[:1]])), b"z", b"n",
                                         T.LAYOUT_RIRIRIRI)
        assert T.decode(st)[0] == 19
        s.set_preconditioner(T.PRECOND_NONE)
        assert T.decode(T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, TOL[prec], MAXIT))[::2] == (14, ord("A"))


@pytest.mark.parametrize("prec", ["z", "c", "m"])
def test_on_without_a_patch_changes_nothing(prec):
    pr = _system(16)
    B2 = pr.B * (1.5 - 0.5j)
    got = []
    for keep in (False, True):
        with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=keep) as s:
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            a = solve_record(s, prec)
            s.set_matrix("B", B2)                                        # same A: nothing is set up again
            got.append((a, solve_record(s, prec)))
    same_record(got[1][0], got[0][0])
    same_record(got[1][1], got[0][1])


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def test_switching_on_a_scaled_plan_is_refused():
    pr = _system(16)
    with T.Solver.open(pr, "z", preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, MAXIT) == 0                                  # the A in the buffer is A M^-1 now, and nobody kept A
        assert T.decode(T.lib.tfqmrgpuExt_keepOperator(s.plan, 1))[::2] == (14, ord("A"))
        s.set_matrix("A", pr.A)                                          # the caller's A again: now it can be kept
        s.keep_operator(True)
        assert s.solve(1e-9, MAXIT) == 0
        s.keep_operator(True)                                            # on and kept: nothing to refuse
        patch_blocks(s, present_diagonal(pr)[:2], pr.A)


def test_a_refused_list_changes_nothing():
    prec = "z"
    pr = _system(16)
    diag = present_diagonal(pr)
    A1 = changed(pr, pr.A, diag, seed=5)
    twice = np.array([diag[3], diag[8], diag[3]], dtype=np.int32)
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        first = solve_record(s, prec)
        for bad in (twice, np.array([diag[3], pr.nnzbA], dtype=np.int32)):
            with pytest.raises(T.TfqmrError) as e:
                s.set_blocks("A", bad, A1[np.minimum(bad, pr.nnzbA - 1)])
            assert T.decode(e.value.status)[::2] == (14, ord("A"))
        same_record(solve_record(s, prec), first)
