"""tfqmrgpuExt_refineFrom (include/tfqmrgpu_ext.h section 16) on the GPU: the mixed-precision refinement started from the X in the plan.
The oracle has no 'm' mode; as in tests/test_gpu_mixed.py the call is graded against the system itself -- residual() of section 10 (an
independent double kernel), true_residual (dense numpy, tests/plan_paths.py) and the oracle's 'z' solution -- and against
the cold solve, solve_from and its own second run where bits are promised.
get_info()["flops_all"] is the sum over every solve of the plan: where two runs of different length are compared, the fields that
describe the LAST solve (residual, iterations, flops) are compared bit for bit and flops_all is checked to have grown by flops."""
import numpy as np
import pytest

import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import bits, diagonal_blocks, same_bits
from plan_paths import true_residual
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

POINTER_INVALID, BREAKDOWN, MAX_ITERATIONS, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 6, 9, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
SIZES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
         (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]


def _last(info):
    """what get_info() says about the last solve alone"""
    return {k: v for k, v in info.items() if k != "flops_all"}


def _results(s):
    """everything the last solve left for the getters"""
    h, it = s.refinement_history(with_iterations=True)
    return s.get_matrix(), h, it, s.bound_history(), s.get_info()


def _same_results(a, b):
    return all(same_bits(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


# ---- 1. it continues, all 15 block shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("LM,LN", SIZES)
def test_continues_on_all_block_sizes(oracle, LM, LN):
    """solve(1e-5), then refine_from(1e-9): converges in double from where the first solve stopped, with at most the float iterations of
    a cold solve(1e-9) of the same plan (both printed: profiles/refine_from.txt records them)"""
    pr = PR.stencil_2d(5, 4, LM, LN, 2, seed=100 + LM + LN)
    st0, Xz, _ = oracle.solve(pr, "z", threshold=1e-9, max_iterations=300)
    assert st0 == 0
    with T.Solver.open(pr, "m").load() as s:
        assert s.solve(1e-5, 300) == 0
        first = s.get_info()["iterations"]
        w0 = s.residual()["worst"]
        assert s.refine_from(1e-9, 300) == 0
        info, h, worst, X = s.get_info(), s.refinement_history(), s.residual()["worst"], s.get_matrix()
        assert s.solve(1e-9, 300) == 0
        cold = s.get_info()["iterations"]
        print("refine_from %2d x %2d: solve(1e-5) %3d | refine_from(1e-9) %3d | cold solve(1e-9) %3d float iterations; first residual %.3e, final %.3e" % (
            LM, LN, first, info["iterations"], cold, h[0], info["residual"]))
        assert worst <= 1.01e-9 and info["residual"] <= 1e-9
        assert h[0] == pytest.approx(w0, rel=1e-9) and h[0] < 1 and h[-1] == info["residual"]
        assert np.abs(X - Xz).max() <= 1e-7 * np.abs(Xz).max()
        assert abs(true_residual(pr, X, "z")[0] - info["residual"]) <= 1e-3 * info["residual"]
        assert info["iterations"] <= cold
        assert info["flops"] > 0


# ---- 2. already converged, no iterations, deterministic --------------------------------------------------------------------------------------
def test_already_converged_and_no_iterations():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "m").load() as s:
        assert s.solve(1e-9, 300) == 0
        X0 = s.get_matrix()
        assert s.refine_from(1e-8, 300) == 0
        info, h = s.get_info(), s.refinement_history()
        assert info["iterations"] == 0 and same_bits(s.get_matrix(), X0)
        assert len(h) == 1 and h[0] == info["residual"] <= 1e-9 * 1.01 and len(s.bound_history()) == 0
        for it in (0, -2):
            assert T.lib.tfqmrgpuExt_refineFrom(s.handle, s.plan, 1e-12, it) == MAX_ITERATIONS
            assert same_bits(s.get_matrix(), X0)
            assert s.get_info()["iterations"] == it and len(s.bound_history()) == 0 and len(s.refinement_history()) == 0


def test_two_calls_give_the_same_bits():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "m").load() as s:
        assert s.solve(1e-4, 300) == 0
        X0 = s.get_matrix()
        out = []
        for _ in range(2):
            s.set_matrix("X", X0)
            assert same_bits(s.get_matrix(), X0)
            st = s.refine_from(1e-9, 300)
            out.append((st,) + _results(s))
        a, b = out
        assert a[0] == b[0] == 0 and a[5]["iterations"] > 0
        assert all(same_bits(x, y) for x, y in zip(a[1:5], b[1:5])) and _last(a[5]) == _last(b[5])
        assert b[5]["flops_all"] == pytest.approx(a[5]["flops_all"] + a[5]["flops"], rel=1e-12)
        assert not same_bits(a[1], X0)


# ---- 3. exact and zero right-hand sides ----------------------------------------------------------------------------------------------------
def test_exact_right_hand_side_keeps_its_bits():
    """A = the unit matrix, so that R is exactly zero where X0 = B: right-hand sides 2 and 5 (b != 0, r = 0) keep X0 bit for bit through
    every cycle and are no breakdown; the others (X0 = B / 2) are refined to 1e-12 -- a float solve of the unit matrix returns r rounded to
    float, so every cycle gains 7 digits"""
    mb, LM, LN = 3, 4, 8
    A = np.tile(np.eye(LM, dtype=complex), (mb, 1, 1))
    B = PR.hashed_uniform(5, (mb, LM, LN)) + 1j * PR.hashed_uniform(6, (mb, LM, LN)) + 0.25
    ptr, ind = np.arange(mb + 1), np.zeros(mb, int)
    pr = T.Problem(np.arange(mb + 1), np.arange(mb), A, ptr, ind, ptr, ind, B)
    thr = 1e-12
    with T.Solver.open(pr, "m").load() as s:
        X0 = 0.5 * B
        X0[:, :, 5] = B[:, :, 5]
        X0[:, :, 2] = B[:, :, 2]
        s.set_matrix("X", X0)
        X0 = s.get_matrix()
        assert s.refine_from(thr, 50) == 0
        X, h = s.get_matrix(), s.refinement_history()
        for j in (2, 5):
            assert same_bits(X[:, :, j], X0[:, :, j]), j
        assert len(h) >= 2 and np.all(np.isfinite(h)) and np.all(np.isfinite(s.bound_history()))
        assert h[0] == pytest.approx(0.5, rel=1e-12) and h[-1] <= thr
        assert np.abs(X - B).max() <= 10 * thr * np.abs(B).max()
        # every right-hand side exact: converged at once, not a breakdown
        s.set_matrix("X", B)
        assert s.refine_from(thr, 50) == 0 and s.get_info()["iterations"] == 0 and s.get_info()["residual"] <= thr
        assert same_bits(s.get_matrix(), B.astype(X.dtype))


def test_zero_right_hand_side_inside_a_block():
    """b = 0 and X0 = 0 in one column of every block (so r = 0 there): that column stays exactly 0.0, the others converge"""
    pr = PR.stencil_2d(4, 4, 4, 8, 2, seed=17, radius=2.0)
    pr.B[:, :, 5] = 0
    thr = 1e-9
    with T.Solver.open(pr, "m").load() as s:
        assert s.solve(1e-30, 2) == MAX_ITERATIONS
        X0 = s.get_matrix()
        assert np.all(X0[:, :, 5] == 0)
        assert s.refine_from(thr, 100) == 0
        X, h = s.get_matrix(), s.refinement_history()
        assert np.all(X[:, :, 5] == 0)
        assert np.all(np.isfinite(X.real)) and np.all(np.isfinite(X.imag)) and np.all(np.isfinite(h)) and np.all(np.isfinite(s.bound_history()))
        keep = [j for j in range(8) if j != 5]
        rel = s.residual()["relative"]
        assert np.nanmax(rel[:, keep]) <= 1.01 * thr and np.all(np.isnan(rel[:, 5]))
        assert 0 < h[0] < 1 and h[-1] <= thr


# ---- 4. energy step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [False, True])
def test_energy_step(precond):
    """solve A, shift the diagonal blocks by 1e-3 with set_blocks('A'), refine_from: converges to the PATCHED system -- residual() reads the
    caller's A, the kept copy on the preconditioned plan, where the patch is still pending when R is formed"""
    pr = load_problem("fd_16x16_small")
    thr = 1e-9
    diag = diagonal_blocks(pr)
    assert len(diag) == pr.mb
    shifted = pr.A.copy()
    shifted[diag] += 1e-3 * np.eye(pr.LM)
    with T.Solver.open(pr, "m", preconditioner=BJ if precond else None, keep_operator=precond).load() as s:
        assert s.solve(thr, 500) == 0
        cold_its = s.get_info()["iterations"]
        s.set_blocks("A", diag, shifted[diag])
        stale = s.residual()["worst"]
        assert stale > thr                                  # the old X does not solve the new system
        assert s.refine_from(thr, 500) == 0
        info, got, h = s.get_info(), s.residual(), s.refinement_history()
        print("energy step m precond=%d: cold %d float iterations | stale residual %.2e | warm %d float iterations, residual %.3e" % (
            precond, cold_its, stale, info["iterations"], got["worst"]))
        assert got["worst"] <= 1.01 * thr and info["residual"] <= thr
        assert h[0] == pytest.approx(stale, rel=1e-9)
        patched = T.Problem(pr.rowPtrA, pr.colIndA, shifted, pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B, None, thr, pr.index_offset)
        assert true_residual(patched, s.get_matrix(), "z")[0] <= 1.01 * thr


def test_preconditioned_without_a_kept_copy_is_refused():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "m", preconditioner=BJ).load() as s:
        assert s.solve(1e-9, 300) == 0
        before = _results(s)
        assert T.decode(T.lib.tfqmrgpuExt_refineFrom(s.handle, s.plan, 1e-10, 100))[::2] == (NO_IMPLEMENTATION, 0)
        assert _same_results(_results(s), before)
    # not scaled yet: R is formed from the buffer's A, then the set-up scales it
    with T.Solver.open(pr, "m", preconditioner=BJ).load() as s:
        s.set_matrix("X", 0.5 * before[0])
        assert s.refine_from(1e-9, 300) == 0
        assert s.refinement_history()[0] == pytest.approx(0.5, rel=1e-6)
        X = s.get_matrix()
    assert true_residual(pr, X, "z")[0] <= 1.01e-9


# ---- 5. seeding across precisions and patterns --------------------------------------------------------------------------------------------------
def test_c_solve_on_the_old_pattern_seeds_the_m_plan_on_the_grown_one():
    """the 1-D chain of tests/test_gpu_solve_from.py::test_grown_pattern_end_to_end: a 'c' solve on the old pattern, the pattern grown by
    its one leak position, a new 'm' plan that adopts A, B and X on the device (X through oldBlock), refine_from"""
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
    with T.Solver.open(pr, "c").load() as src:
        assert src.solve(1e-4, 200) == 0
        coarse_its = src.get_info()["iterations"]
        grown = src.grow_problem(pr, [0])
        old = src.grow_pattern([0])[2]
        assert grown.nnzbX == 4 and list(old) == [0, 1, 2, -1]
        with T.Solver.open(grown, "m") as s:
            s.adopt(src, old)
            assert np.all(s.get_matrix()[3] == 0)
            assert s.refine_from(1e-9, 200) == 0
            h, info = s.refinement_history(), s.get_info()
            print("seeded: 'c' %d iterations on the old pattern | 'm' refine_from %d float iterations on the grown one, first residual %.2e" % (
                coarse_its, info["iterations"], h[0]))
            assert s.residual()["worst"] <= 1.01e-9
            assert np.abs(s.get_matrix()[3]).max() > 0
            assert h[0] < 0.1


# ---- 6. the cold path is untouched ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fd_16x16_small", "stencil_8x32", "fd_4x4_2d"])
def test_cold_solve_does_not_depend_on_a_refine_in_between(name):
    """solve, solve against solve, refine_from, solve on a fresh plan: the last solves agree bit for bit -- refine_from leaves the float
    floor (Plan::mixedFloor) and the buffer as a cold solve expects them.  fd_4x4_2d is the fixture whose float solves run into their
    floor (tests/test_gpu_mixed.py: test_mixed_where_float_iterations_stagnate); here the first solve has learnt it before the
    refine_from runs, so this test alone does not see a refine_from that writes the floor: the next test does"""
    pr = load_problem(name)
    runs = []
    for calls in (("solve", "solve"), ("solve", "refine_from", "solve")):
        with T.Solver.open(pr, "m").load() as s:
            sts, flops = [], []
            for what in calls:
                sts.append(getattr(s, what)(1e-9, 300))
                flops.append(s.get_info()["flops"])
            runs.append((sts, flops) + _results(s))
    a, b = runs
    assert a[0][-1] == b[0][-1] and a[0][0] == b[0][0]
    assert all(same_bits(x, y) for x, y in zip(a[2:6], b[2:6]))
    assert _last(a[6]) == _last(b[6])
    assert a[6]["flops_all"] == pytest.approx(sum(a[1]), rel=1e-12) and b[6]["flops_all"] == pytest.approx(sum(b[1]), rel=1e-12)


def test_refine_from_teaches_the_plan_no_float_floor():
    """fd_4x4_2d, whose float solves end at their floor: the SECOND cold solve of a plan differs from the first, because the first one has
    learnt the floor (Plan::mixedFloor).  A refine_from from X = 0 is a cold solve in everything but that: the solve behind it must still
    be the plan's FIRST cold solve, bit for bit"""
    pr = load_problem("fd_4x4_2d")
    zero = np.zeros((pr.nnzbX, pr.LM, pr.LN), complex)
    runs = {}
    for calls in (("solve",), ("solve", "solve"), ("refine_from", "solve")):
        with T.Solver.open(pr, "m").load() as s:
            s.set_matrix("X", zero)
            sts = [getattr(s, what)(1e-9, 300) for what in calls]
            runs[calls] = (sts[-1],) + _results(s)
    first, second, behind = runs[("solve",)], runs[("solve", "solve")], runs[("refine_from", "solve")]
    assert not (same_bits(first[2], second[2]) and same_bits(first[3], second[3])), "this fixture no longer learns a floor: the test shows nothing"
    assert first[0] == behind[0] and all(same_bits(x, y) for x, y in zip(first[1:5], behind[1:5])) and _last(first[5]) == _last(behind[5])


# ---- 7. 'z' / 'c' forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("fd_8x8_3d", "c")])
def test_z_and_c_plans_forward_to_solve_from(name, prec):
    pr = load_problem(name)
    out = []
    for what in ("solve_from", "refine_from"):
        with T.Solver.open(pr, prec).load() as s:
            assert s.solve(pr.tolerance, 3) == MAX_ITERATIONS
            X0 = s.get_matrix()
            st = getattr(s, what)(pr.tolerance, 6)
            out.append((st, s.get_matrix(), s.bound_history(), s.get_info(), X0))
    a, b = out
    assert same_bits(a[4], b[4])
    assert a[0] == b[0] and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and a[3] == b[3]
    assert len(a[2]) > 0 and not same_bits(a[1], a[4])


# ---- 8. statuses that need a device ----------------------------------------------------------------------------------------------------------
def test_statuses_change_nothing():
    pr = load_problem("fd_16x16_small")
    raw = lambda s, it=100: T.lib.tfqmrgpuExt_refineFrom(s.handle, s.plan, 1e-10, it)      # noqa: E731
    with T.Solver.open(pr, "m").load() as s:
        assert s.solve(1e-9, 300) == 0
        before = _results(s)
        # a user-defined operator: refused before A is looked at
        s.set_operator(lambda *a: 0.0)
        assert T.decode(raw(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert _same_results(_results(s), before)
        # several ranks (a reduce callback): refused through the mixed solve's own first collective, exactly one
        calls = []
        s.set_reduce_callback(lambda values, n: calls.append([values[i] for i in range(n)]))
        assert T.decode(raw(s))[::2] == (NO_IMPLEMENTATION, 0)
        assert len(calls) == 1 and len(calls[0]) == 3 and calls[0][2] == 1.0
        s.set_reduce_callback(None)
        assert _same_results(_results(s), before)
        # ... and the plan still solves as it did
        assert s.refine_from(1e-8, 300) == 0 and s.get_info()["iterations"] == 0 and same_bits(s.get_matrix(), before[0])
    # A has never been set on this buffer
    with T.Solver.open(pr, "m") as s:
        s.set_matrix("B", pr.B)
        s.set_matrix("X", before[0])
        info0 = s.get_info()
        assert T.decode(raw(s))[::2] == (UNDOCUMENTED, ord("A"))
        assert same_bits(s.get_matrix(), before[0]) and s.get_info() == info0 and len(s.refinement_history()) == 0
    with T.Solver.open(pr, "m", buffer=False) as s:
        assert T.decode(raw(s))[::2] == (POINTER_INVALID, 0)
