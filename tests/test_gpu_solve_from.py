"""tfqmrgpuExt_solveFrom (include/tfqmrgpu_ext.h section 14) on the GPU: the warm start against the CPU oracle's solve of the correction
problem (tests/warm_ref.py), what it promises about threshold, special right-hand sides, the preconditioner and the cold solve, and the
statuses that need a device."""
import ctypes as C

import numpy as np
import pytest

import residual_ref as RR
import tfqmrgpu_amd as T
import warm_cases as WC
import warm_ref as WR
from conftest import load_problem
from helpers import diagonal_blocks, same_bits
from tfqmrgpu_amd import problems as PR
from tolerances import C_TOL

pytestmark = pytest.mark.gpu

POINTER_INVALID, MAX_ITERATIONS, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 9, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
# the smallest shapes at which each path can go wrong: LDS-patch shapes, interleaved MFMA shapes, the quad order (two), LM != LN
FIXTURES = ["fd_4x4_2d", "fd_16x16_small", "fd_8x8_3d", "stencil_8x32", "dense_random_rect"]
X_TOL_Z = 1e-7          # cold parity of 'z' (tests/test_gpu_parity.py); 'c': tests/tolerances.py C_TOL[name]["x"] where the table has the fixture


# ---- 1. parity with the oracle at a fixed iteration count -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_with_the_oracle(oracle, name, prec):
    """X0 = a cold solve stopped after 3 iterations; solve_from(1e-30, k) for k = 1 (X0 as the solve left it) and k = 4 (X0 brought by
    set_matrix('X')) against X0 + the oracle's k iterations on A D = R, both with the glibc shadow vector.
    Tolerance: the cold parity's -- 1e-7 max|X| for 'z', C_TOL[name]["x"] for 'c'.  The 'c' table has no entry for fd_4x4_2d, stencil_8x32
    and dense_random_rect: there k = 1 takes warm_cases.allowance_of for this X0 -- the cold solve's state bound plus what the oracle's own
    iterate moves by when R changes by its a-priori rounding bound, relative to max|D| -- and k = 4, where a float trajectory depends on
    cancellation in the shadow-vector dots, asks only that both solves run out of iterations with a finite history; its deviation is
    printed.  MI355X, deviation of solve_from at k = 1 and k = 4: fd_4x4_2d 1.4e-7, 2.1e-3; stencil_8x32 2.8e-7, 2.8e-7; dense_random_rect
    8.3e-7, 1.5e-6.  'z': at most 1.0e-11 everywhere."""
    pr = load_problem(name)
    A, B = RR.stored(pr.A, prec), RR.stored(pr.B, prec)
    with T.Solver.open(pr, prec, shadow_mode=T.SHADOW_GLIBC_RAND).load() as s:
        assert s.solve(1e-30, 3) == MAX_ITERATIONS
        X0 = s.get_matrix()
        for k in (1, 4):
            if k > 1:
                s.set_matrix("X", X0)
                assert same_bits(s.get_matrix(), X0)
            assert s.solve_from(1e-30, k) == MAX_ITERATIONS
            X = s.get_matrix()
            assert len(s.bound_history()) == k and np.all(np.isfinite(s.bound_history()))
            cp = WR.correction_problem(oracle, pr, X0, A, B)
            st0, D, info0 = oracle.solve(cp, prec, threshold=1e-30, max_iterations=k, dump_iteration=k)
            assert st0 == MAX_ITERATIONS and np.all(np.isfinite(info0["bound_history"]))
            want = X0 + info0["vectors"][1]
            scale = np.abs(want).max()
            dev = np.abs(X - want).max() / scale
            tol = X_TOL_Z if prec == "z" else C_TOL.get(name, {}).get("x")
            how = ""
            if tol is None and k == 1:
                cs = WC.build(oracle, pr, prec, X0, 7, v3=oracle.shadow_glibc(X0.size * 2))
                base = WC.state(oracle, cs, cs.R, 1)
                assert np.array_equal(base[1], info0["vectors"][1])
                tol = WC.allowance_of(cs, 1, WC.spread_of(oracle, cs, 1, base), base)[1] * np.abs(base[1]).max() / scale
                how = " (warm_cases.allowance_of)"
            print("solve_from parity %-18s %s k=%d: deviation %.2e, allowed %s%s" % (name, prec, k, dev, "-" if tol is None else "%.2e" % tol, how))
            assert tol is None or dev <= tol, (name, prec, k, dev, tol)
            # the bound history is relative to |B|: it starts at 3 |r|^2 / |b|^2-ish, far below the cold solve's first entry
            h = s.bound_history()
            assert h[0] > 0


# ---- 2. it continues --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,thr,margin", [("z", 1e-9, 2.0), ("c", 1e-4, 2.0)])
def test_continues_a_solve_that_ran_out_of_iterations(prec, thr, margin):
    """fd_16x16_small: a cold solve converges in k2 iterations (oracle: 14 'z', 8 'c'); stopped at k2 // 2 it returns MAX_ITERATIONS,
    solve_from then converges in at most k2 iterations (oracle, with the threshold scaled to |B| by the strictest right-hand side:
    9 'z', 6 'c') to a residual -- residual(), in double -- of at most `margin` x the cold solve's.  MI355X: 'z' 8 iterations, 5.05e-10
    against 2.80e-10 cold (1.8 x; the margin of 2 is the issue's); 'c' 5 iterations, 6.61e-5 against 4.28e-5 cold: 1.55 x measured, so
    the same margin of 2 is kept for 'c'."""
    pr = load_problem("fd_16x16_small")
    N = 500
    with T.Solver.open(pr, prec).load() as s:
        assert s.solve(thr, N) == 0
        k2 = s.get_info()["iterations"]
        cold = s.residual()["worst"]
        assert k2 >= 4 and cold <= 1.01 * thr
        assert s.solve(thr, k2 // 2) == MAX_ITERATIONS
        half = s.residual()["worst"]
        assert half > thr
        assert s.solve_from(thr, N) == 0
        info, warm = s.get_info(), s.residual()["worst"]
        print("continues %s: cold %d iterations, residual %.3e | half %.3e | warm %d iterations, residual %.3e, getInfo %.3e" % (
            prec, k2, cold, half, info["iterations"], warm, info["residual"]))
        assert 1 <= info["iterations"] <= k2 and len(s.bound_history()) == info["iterations"]
        assert info["residual"] <= thr                      # relative to |B|, as after solve
        assert warm <= margin * cold
        assert info["flops"] > 0


# ---- 3. already converged -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,thr", [("z", 1e-9), ("c", 1e-4)])
def test_already_converged(prec, thr):
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, prec).load() as s:
        assert s.solve(thr, 500) == 0
        X0 = s.get_matrix()
        assert s.solve_from(10 * thr, 500) == 0
        assert s.get_info()["iterations"] <= 1 and s.get_info()["residual"] <= 10 * thr
        moved = np.abs(s.get_matrix() - X0).max() / np.abs(X0).max()
        print("already converged %s: X moved by %.2e" % (prec, moved))
        assert moved <= (X_TOL_Z if prec == "z" else C_TOL["fd_16x16_small"]["x"])


# ---- 4. R = 0 and b = 0 right-hand sides ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_zero_right_hand_side_inside_a_block(prec):
    """b = 0 and X0 = 0 in one column of every block (so r = 0 there): that column stays exactly 0.0, the others converge"""
    pr = PR.stencil_2d(4, 4, 4, 8, 2, seed=17, radius=2.0)
    pr.B[:, :, 5] = 0
    thr = 1e-9 if prec == "z" else 1e-4
    with T.Solver.open(pr, prec).load() as s:
        assert s.solve(1e-30, 2) == MAX_ITERATIONS
        X0 = s.get_matrix()
        assert np.all(X0[:, :, 5] == 0)
        assert s.solve_from(thr, 100) == 0
        X, h = s.get_matrix(), s.bound_history()
        assert np.all(X[:, :, 5] == 0)
        assert np.all(np.isfinite(X.real)) and np.all(np.isfinite(X.imag)) and np.all(np.isfinite(h))
        keep = [j for j in range(8) if j != 5]
        rel = s.residual()["relative"]
        assert np.nanmax(rel[:, keep]) <= 1.01 * thr and np.all(np.isnan(rel[:, 5]))


@pytest.mark.parametrize("prec", ["z", "c"])
def test_exact_right_hand_side_keeps_its_bits(prec):
    """A = the unit matrix, so that R is exactly zero where X0 = B: right-hand side 5 (b != 0, r = 0) keeps X0 bit for bit and is no
    breakdown, and so does right-hand side 2; the others (X0 = B / 2) are solved"""
    mb, LM, LN = 3, 4, 8
    A = np.tile(np.eye(LM, dtype=complex), (mb, 1, 1))
    B = PR.hashed_uniform(5, (mb, LM, LN)) + 1j * PR.hashed_uniform(6, (mb, LM, LN)) + 0.25
    ptr, ind = np.arange(mb + 1), np.zeros(mb, int)
    pr = T.Problem(np.arange(mb + 1), np.arange(mb), A, ptr, ind, ptr, ind, B)
    thr = 1e-12 if prec == "z" else 1e-5
    with T.Solver.open(pr, prec).load() as s:
        Bs = RR.stored(B, prec)
        X0 = 0.5 * Bs
        X0[:, :, 5] = Bs[:, :, 5]
        X0[:, :, 2] = Bs[:, :, 2]
        s.set_matrix("X", X0)
        X0 = s.get_matrix()
        assert s.solve_from(thr, 50) == 0
        X = s.get_matrix()
        for j in (2, 5):
            assert same_bits(X[:, :, j], X0[:, :, j]), j
        assert np.all(np.isfinite(s.bound_history()))
        assert np.abs(X - Bs).max() <= 10 * thr * np.abs(Bs).max()
        # every right-hand side exact: converged at once, not a breakdown
        s.set_matrix("X", Bs)
        assert s.solve_from(thr, 50) == 0 and s.get_info()["iterations"] == 1
        assert same_bits(s.get_matrix(), RR.stored(Bs, prec).astype(X.dtype))


# ---- 5. energy step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,thr", [("z", 1e-9), ("c", 1e-4)])
@pytest.mark.parametrize("precond", [False, True])
def test_energy_step(oracle, prec, thr, precond):
    """solve A, shift the diagonal blocks by 1e-3 with set_blocks('A'), solve_from: converges to the PATCHED system -- residual() reads
    the caller's A, the kept copy on the preconditioned plan, where the patch is still pending when R is formed"""
    pr = load_problem("fd_16x16_small")
    diag = diagonal_blocks(pr)
    assert len(diag) == pr.mb
    shifted = pr.A.copy()
    shifted[diag] += 1e-3 * np.eye(pr.LM)
    with T.Solver.open(pr, prec, preconditioner=BJ if precond else None, keep_operator=precond).load() as s:
        assert s.solve(thr, 500) == 0
        cold_its = s.get_info()["iterations"]
        s.set_blocks("A", diag, shifted[diag])
        stale = s.residual()["worst"]
        assert stale > thr                                  # the old X does not solve the new system
        assert s.solve_from(thr, 500) == 0
        info, got = s.get_info(), s.residual()
        print("energy step %s precond=%d: cold %d iterations | stale residual %.2e | warm %d iterations, residual %.3e" % (
            prec, precond, cold_its, stale, info["iterations"], got["worst"]))
        assert got["worst"] <= 1.01 * thr and info["residual"] <= thr
        ref = RR.residual(oracle, pr, RR.stored(shifted, prec), s.get_matrix(), RR.stored(pr.B, prec))
        assert np.allclose(got["residual2"], ref["residual2"], rtol=0, atol=float(ref["bound_r2"].max()) + 1e-300)


def test_preconditioned_without_a_kept_copy_is_refused():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "z", preconditioner=BJ).load() as s:
        assert s.solve(1e-9, 3) == MAX_ITERATIONS
        X0, h0, info0 = s.get_matrix(), s.bound_history(), s.get_info()
        assert T.decode(T.lib.tfqmrgpuExt_solveFrom(s.handle, s.plan, 1e-9, 100))[::2] == (NO_IMPLEMENTATION, 0)
        assert same_bits(s.get_matrix(), X0) and np.array_equal(s.bound_history(), h0) and s.get_info() == info0
    # not scaled yet: R is formed from the buffer's A, then the set-up scales it
    with T.Solver.open(pr, "z", preconditioner=BJ).load() as s:
        s.set_matrix("X", X0)
        assert s.solve_from(1e-9, 100) == 0
        assert T.decode(T.lib.tfqmrgpuExt_residual(s.handle, s.plan, None, None, None, C.byref(C.c_double(0))))[0] == NO_IMPLEMENTATION
        X = s.get_matrix()
    with T.Solver.open(pr, "z").load() as s:
        s.set_matrix("X", X)
        assert s.residual()["worst"] <= 1.01e-9


# ---- 6. grown pattern end to end ------------------------------------------------------------------------------------------------------------
def test_grown_pattern_end_to_end():
    """the 1-D chain of tests/test_gpu_leak_map.py: solve, grow the pattern by its one leak position, a new plan, the old values mapped
    through oldBlock with zeros elsewhere, solve_from"""
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
    with T.Solver.open(pr, "z").load() as s:
        assert s.solve(1e-9, 200) == 0
        cold_its = s.get_info()["iterations"]
        pr.X = s.get_matrix()
        grown = s.grow_problem(pr, [0])
    assert grown.nnzbX == 4 and np.all(grown.X[3] == 0) and np.array_equal(grown.X[:3], pr.X)
    with T.Solver.open(grown, "z").load() as s:
        s.set_matrix("X", grown.X)
        assert s.solve_from(1e-9, 200) == 0
        assert np.all(s.truncation_leak()["leak2"] == 0.0)
        assert s.residual()["worst"] <= 1.01e-9
        print("grown pattern: cold %d iterations on the old pattern, warm %d on the grown one" % (cold_its, s.get_info()["iterations"]))
        assert np.abs(s.get_matrix()[3]).max() > 0


# ---- 7. the cold path is untouched ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("fd_4x4_2d", "c"), ("stencil_8x32", "z")])
def test_cold_solve_is_bit_for_bit_the_solve_it_was(name, prec):
    pr = load_problem(name)
    with T.Solver.open(pr, prec).load() as s:
        runs = []
        for what in ("solve", "solve_from", "solve"):
            st = getattr(s, what)(pr.tolerance, 9)
            info = s.get_info()
            runs.append((st, s.get_matrix(), s.bound_history(), info["residual"], info["iterations"], info["flops"],
                         {w: s.get_work_vector(w) for w in (4, 5, 6, 7, 8, 9)}))
        a, b = runs[0], runs[2]
        assert a[0] == b[0] and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and a[3:6] == b[3:6]
        for w in a[6]:
            assert same_bits(a[6][w], b[6][w]), w


# ---- 8. statuses that need a device -----------------------------------------------------------------------------------------------------------
def test_statuses_change_nothing():
    pr = load_problem("fd_16x16_small")
    raw = lambda s, it=100: T.lib.tfqmrgpuExt_solveFrom(s.handle, s.plan, 1e-9, it)      # noqa: E731
    # 'm': refused, X and the results of the last solve as they were
    with T.Solver.open(pr, "m").load() as s:
        assert s.solve(1e-9, 500) == 0
        X0, info0 = s.get_matrix(), s.get_info()
        assert T.decode(raw(s))[::2] == (NO_IMPLEMENTATION, 0)
        assert same_bits(s.get_matrix(), X0) and s.get_info() == info0
    with T.Solver.open(pr, "z").load() as s:
        assert s.solve(1e-9, 3) == MAX_ITERATIONS
        X0, h0 = s.get_matrix(), s.bound_history()
        # a user-defined operator: refused before A is looked at
        s.set_operator(lambda *a: 0.0)
        assert T.decode(raw(s))[::2] == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        # several ranks (a reduce callback): refused through the vote in front of a solve, one collective
        calls = []
        s.set_reduce_callback(lambda values, n: calls.append([values[i] for i in range(n)]))
        assert T.decode(raw(s))[::2] == (NO_IMPLEMENTATION, 0)
        assert len(calls) == 1 and calls[0][1] == 1.0
        s.set_reduce_callback(None)
        assert same_bits(s.get_matrix(), X0) and np.array_equal(s.bound_history(), h0)
        # no iteration at all: X0 is the answer, bit for bit; the status of a cold solve without an iteration
        for it in (0, -2):
            assert s.solve(1e-9, it) == MAX_ITERATIONS      # (the cold solve: X = 0)
            s.set_matrix("X", X0)
            assert raw(s, it) == MAX_ITERATIONS
            assert same_bits(s.get_matrix(), X0) and len(s.bound_history()) == 0 and s.get_info()["iterations"] == it
    # A has never been set on this buffer
    with T.Solver.open(pr, "z") as s:
        s.set_matrix("B", pr.B)
        s.set_matrix("X", X0)
        assert T.decode(raw(s))[::2] == (UNDOCUMENTED, ord("A"))
        assert same_bits(s.get_matrix(), X0)
    with T.Solver.open(pr, "z", buffer=False) as s:
        assert T.decode(raw(s))[::2] == (POINTER_INVALID, 0)


# ---- 9. deterministic -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("fd_8x8_3d", "c"), ("dense_random_rect", "z")])
def test_two_calls_give_the_same_bits(name, prec):
    pr = load_problem(name)
    with T.Solver.open(pr, prec).load() as s:
        assert s.solve(pr.tolerance, 3) == MAX_ITERATIONS
        X0 = s.get_matrix()
        out = []
        for _ in range(2):
            s.set_matrix("X", X0)
            st = s.solve_from(pr.tolerance, 6)
            out.append((st, s.get_matrix(), s.bound_history(), s.get_info()["residual"]))
        assert out[0][0] == out[1][0] and same_bits(out[0][1], out[1][1]) and same_bits(out[0][2], out[1][2]) and out[0][3] == out[1][3]
        assert not same_bits(out[0][1], X0)
