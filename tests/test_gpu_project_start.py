"""Start projection (include/tfqmrgpu_ext.h section 17) on the GPU against its numpy restatement (tests/project_ref.py): the coefficients
and the projected X, the optimality of the projected residual, the edge cases of the pivot rule, the preconditioned plan, determinism and
side effects, two ranks, and the energy loop it is for.  The shifts of every fixture are those that tests/test_project_start_cpu.py has
checked on the CPU: every pivot ratio a factor 100 away from the threshold."""
import ctypes as C

import numpy as np
import pytest

import project_ref as P
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import deviations, run_ranks, same_bits
from precond_ref import _product, diagonal_blocks

pytestmark = pytest.mark.gpu

POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
THR = {"z": 1e-9, "c": 1e-4, "m": 1e-9}      # what "converged" means for the starts


def _converged(s, prec, what):
    assert s.solve(THR[prec], 200) == 0, (what, prec)


def _energy_loop(name, prec, fifth=False):
    """a Solver that has solved at all but the last shift, with push_start after each, and holds A(last shift); the starts as read
    back, newest first; A and B as the plan stores them"""
    pr = load_problem(name)
    sig = P.shifts(pr, name, fifth)
    s = T.Solver.open(pr, prec, keep_starts=len(sig) - 1)
    s.set_matrix("B", pr.B)
    starts = []
    for k, sigma in enumerate(sig[:-1]):
        s.set_matrix("A", P.shifted(pr, sigma))
        _converged(s, prec, (name, sigma))
        s.push_start()
        assert s.start_count() == k + 1
        starts.insert(0, s.get_matrix())
    s.set_matrix("A", P.shifted(pr, sig[-1]))
    return pr, s, starts, RR.stored(P.shifted(pr, sig[-1]), prec), RR.stored(pr.B, prec)


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("name", P.FIXTURES)
def test_parity_with_the_reference(oracle, name, prec):
    """gamma and X against project_ref fed with the starts as read back.  Allowed: 100 eps_storage / rho relative on gamma (rho: the smallest
    pivot ratio of a kept start of that right-hand side), that plus one storage rounding on X.
    MI355X, worst deviation as a fraction of the allowed one, gamma | X: 'z' 0.29 | 0.14, 'c' 0.019 | 0.016, 'm' 0.24 | 0.11 (all on
    fd_4x4_2d); depth 4 on stencil_8x32 0.13 | 0.09 ('z'), 0.06 | 0.05 ('c'); every fixture: profiles/project_start.txt."""
    pr, s, starts, A, B = _energy_loop(name, prec)
    with s:
        got = s.project_start()
        X = s.get_matrix()
        assert s.start_count() == 3
    ref = P.project(oracle, pr, A, starts, B, prec)
    assert np.array_equal(got["n_used"], ref["n_used"]) and np.all(got["n_used"] == 3)
    dg, bg, dx, bx = deviations(pr, ref, got, X, starts, prec)
    print("project parity %-18s %s: gamma %.2e of allowed (abs %.2e), X %.2e of allowed (abs %.2e)" % (
        name, prec, (dg / bg).max(), dg.max(), (dx / bx).max(), dx.max()))
    assert np.all(dg <= bg), (name, prec, (dg / bg).max())
    assert np.all(dx <= bx), (name, prec, (dx / bx).max())


# ---- 2. optimality -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("name", P.FIXTURES)
def test_projected_residual_is_optimal(oracle, name, prec):
    """residual() after project_start <= residual() of X = S_0 per right-hand side ('c': plus the float floor, the residual of the
    reference's combination rounded to float minus that of the unrounded one), and equal to the reference's projected residual within
    the bound of test 1 carried to the residual: (100 eps / rho) max|gamma| sum |W_i|, plus the floor for 'c', plus the rounding of
    residual() itself carried from r^2 to r (residual_ref: bound_r2 / (2 r)).  MI355X: the deviation is at most 1.3e-3 of that in 'z' and
    'm' and 1.3e-4 in 'c' -- at its minimum the residual moves with the SQUARE of an error of gamma, the bound is of first order."""
    pr, s, starts, A, B = _energy_loop(name, prec)
    with s:
        s.set_matrix("X", starts[0])
        r0 = np.sqrt(s.residual()["residual2"])
        s.project_start()
        rp = np.sqrt(s.residual()["residual2"])
    ref = P.project(oracle, pr, A, starts, B, prec)
    exact = RR.residual(oracle, pr, A, ref["X"], B)
    rounded = RR.residual(oracle, pr, A, RR.stored(ref["X"], prec), B)
    floor = np.abs(np.sqrt(rounded["residual2"]) - np.sqrt(exact["residual2"]))
    an = ref["an"]
    col = an["colindx"].astype(np.int64)
    wnorm = np.zeros_like(r0)
    for S in starts:
        np.add.at(wnorm, col, np.sqrt((np.abs(_product(an, pr, A, S)) ** 2).sum(axis=1)))
    want = np.sqrt(exact["residual2"])
    if prec != "c":
        floor = np.zeros_like(floor)                      # the issue adds the floor for float storage only
    # (bound_r2 bounds the rounding of residual() on r^2: on r that is bound_r2 / (rp + want))
    carried = P.gamma_tolerance(ref, prec) * np.abs(ref["gamma"]).max(axis=-1) * wnorm + floor + exact["bound_r2"] / (rp + want)
    print("project optimality %-18s %s: |B - A X| / |B| worst %.3e from S_0, %.3e projected (reference %.3e); deviation %.2e of allowed" % (
        name, prec, (r0 / np.sqrt(exact["bnorm2"])).max(), (rp / np.sqrt(exact["bnorm2"])).max(), (want / np.sqrt(exact["bnorm2"])).max(),
        (np.abs(rp - want) / carried).max()))
    assert np.all(rp <= r0 + floor)
    nz = exact["bnorm2"] > 0
    assert np.all(rp[nz] < r0[nz])                        # (the CPU check has shown a strict gain on every right-hand side with b != 0)
    assert np.all(np.abs(rp - want) <= carried)


# ---- 3. edge cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_edge_cases_of_the_pivot_rule(oracle, prec):
    name = "dense_random_rect"
    pr = load_problem(name)
    pr.B[:, :, 5] = 0                                      # a zero column of B
    sig = P.shifts(pr, name)
    A, B = RR.stored(P.shifted(pr, sig[3]), prec), RR.stored(pr.B, prec)
    an = oracle.analyse(pr)
    col = an["colindx"].astype(np.int64)
    live = [j for j in range(pr.LN) if j != 5]
    with T.Solver.open(pr, prec, keep_starts=1) as s:
        s.set_matrix("B", pr.B)
        s.set_matrix("A", P.shifted(pr, sig[0]))
        _converged(s, prec, "start")
        s.push_start()
        S0 = s.get_matrix()
        s.set_matrix("A", P.shifted(pr, sig[3]))
        # k = 1: gamma = <w, b> / <w, w>
        got = s.project_start()
        W = RR.stored(_product(an, pr, A, S0), prec)
        Bx = np.zeros_like(W)
        Bx[an["subset"].astype(np.int64)] = B
        wb, ww = np.zeros((an["nCols"], pr.LN), complex), np.zeros((an["nCols"], pr.LN))
        np.add.at(wb, col, (np.conj(W) * Bx).sum(axis=1))
        np.add.at(ww, col, (np.abs(W) ** 2).sum(axis=1))
        g = got["coefficients"][:, :, 0]
        assert np.all(got["n_used"][:, live] == 1)
        assert np.allclose(g[:, live], wb[:, live] / ww[:, live], rtol=100 * P.EPS[prec], atol=0)
        # b = 0: gamma = 0, nothing used, x exactly 0
        assert np.all(g[:, 5] == 0) and np.all(got["n_used"][:, 5] == 0) and np.all(s.get_matrix()[:, :, 5] == 0)
        # the same X pushed twice: the older copy is dropped
        assert s.keep_starts(3) == 0 and s.start_count() == 1
        s.set_matrix("X", S0)
        s.push_start()
        assert s.start_count() == 2
        twice = s.project_start()
        assert np.all(twice["n_used"][:, live] == 1) and np.all(twice["coefficients"][:, :, 1:] == 0)
        assert np.all(np.isfinite(twice["coefficients"])) and np.all(np.isfinite(s.get_matrix()))
        assert same_bits(twice["coefficients"][:, :, 0], g)
        # a zero start, the newest: dropped, the start behind it is used
        s.set_matrix("X", np.zeros_like(S0))
        s.push_start()
        assert s.start_count() == 3
        zero = s.project_start()
        assert np.all(zero["n_used"][:, live] == 1) and np.all(zero["coefficients"][:, :, 0] == 0) and np.all(zero["coefficients"][:, :, 2] == 0)
        assert same_bits(zero["coefficients"][:, :, 1], g)
        # shrinking the depth drops the oldest starts: the zero start alone is left, and nothing can be used
        assert s.keep_starts(1) == 0 and s.start_count() == 1
        none = s.project_start()
        assert np.all(none["n_used"] == 0) and np.all(none["coefficients"] == 0) and np.all(s.get_matrix() == 0)


@pytest.mark.parametrize("prec", ["z", "c"])
def test_depth_four(oracle, prec):
    """four starts on stencil_8x32: the largest record (25 planes), which leaves the Gram kernel's LDS in rounds"""
    pr, s, starts, A, B = _energy_loop("stencil_8x32", prec, fifth=True)
    with s:
        got = s.project_start()
        X = s.get_matrix()
    ref = P.project(oracle, pr, A, starts, B, prec)
    assert np.all(got["n_used"] == 4) and np.array_equal(got["n_used"], ref["n_used"])
    dg, bg, dx, bx = deviations(pr, ref, got, X, starts, prec)
    print("project depth 4 stencil_8x32 %s: gamma %.2e of allowed, X %.2e of allowed" % (prec, (dg / bg).max(), (dx / bx).max()))
    assert np.all(dg <= bg) and np.all(dx <= bx)


# ---- 4. preconditioner ---------------------------------------------------------------------------------------------------------------------
def test_preconditioned_plan_reads_the_kept_copy_with_its_patch(oracle):
    name, prec = "fd_16x16_small", "z"
    pr = load_problem(name)
    sig = P.shifts(pr, name)
    diag = diagonal_blocks(pr)
    with T.Solver.open(pr, prec, keep_starts=2, preconditioner=BJ, keep_operator=True) as s:
        s.set_matrix("B", pr.B)
        starts = []
        s.set_matrix("A", P.shifted(pr, sig[0]))
        for k in (0, 1):
            if k:
                s.set_blocks("A", diag, P.shifted(pr, sig[k])[diag])      # the buffer is scaled: the patch goes into the kept copy
            _converged(s, prec, "start")
            s.push_start()
            starts.insert(0, s.get_matrix())
        s.set_blocks("A", diag, P.shifted(pr, sig[3])[diag])              # pending: no set-up has seen it
        got = s.project_start()
        X = s.get_matrix()
    A, B = RR.stored(P.shifted(pr, sig[3]), prec), RR.stored(pr.B, prec)
    ref = P.project(oracle, pr, A, starts, B, prec)
    assert np.array_equal(got["n_used"], ref["n_used"])
    dg, bg, dx, bx = deviations(pr, ref, got, X, starts, prec)
    print("project preconditioned: gamma %.2e of allowed, X %.2e of allowed" % ((dg / bg).max(), (dx / bx).max()))
    assert np.all(dg <= bg) and np.all(dx <= bx)
    # scaled and no copy kept: refused, X untouched
    with T.Solver.open(pr, prec, keep_starts=2, preconditioner=BJ) as s:
        s.set_matrix("B", pr.B)
        s.set_matrix("A", P.shifted(pr, sig[0]))
        _converged(s, prec, "start")
        s.push_start()
        X0 = s.get_matrix()
        g = np.full((int(s.plan_view()["nCols"]), pr.LN, 2, 2), 7.0)
        assert T.decode(T.lib.tfqmrgpuExt_projectStart(s.handle, s.plan, g.ctypes.data_as(C.c_void_p), None))[::2] == (NO_IMPLEMENTATION, 0)
        assert same_bits(s.get_matrix(), X0) and np.all(g == 7.0)


# ---- 5. determinism and side effects -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("fd_8x8_3d", "c"), ("stencil_8x32", "m")])
def test_deterministic_and_without_side_effects(name, prec):
    pr, s, starts, A, B = _energy_loop(name, prec)
    with s:
        # (host arrays of set_matrix / get_matrix are staged through v4 ... v9: nothing of that kind between the two readings; 'm' plans
        #  give no work vectors)
        vectors = lambda: {} if prec == "m" else {w: s.get_work_vector(w) for w in range(4, 10)}      # noqa: E731
        before = (vectors(), s.bound_history(), s.get_info(), s.refinement_history())
        first = s.project_start()
        s.push_start()
        assert s.keep_starts(3) == 0 and s.start_count() == 3
        after = (vectors(), s.bound_history(), s.get_info(), s.refinement_history())
        assert all(same_bits(before[0][w], after[0][w]) for w in before[0])
        assert same_bits(before[1], after[1]) and before[2] == after[2] and same_bits(before[3], after[3])
        # two calls give the same bits (the ring: the projected X on top of the two newest starts)
        out = []
        for _ in range(2):
            got = s.project_start()
            out.append((got["coefficients"], got["n_used"], s.get_matrix()))
        assert all(same_bits(a, b) for a, b in zip(out[0], out[1]))
        assert not same_bits(out[0][2], starts[0]) and np.all(np.isfinite(first["coefficients"]))
        # a cold solve on this plan is the cold solve of a plan that keeps nothing
        st = s.solve(THR[prec], 7)
        cold = (st, s.get_matrix(), s.bound_history(), s.get_info()["residual"], s.get_info()["iterations"])
        with T.Solver.open(pr, prec) as t:
            t.set_matrix("B", pr.B)
            t.set_matrix("A", P.shifted(pr, P.shifts(pr, name)[-1]))
            st = t.solve(THR[prec], 7)
            plain = (st, t.get_matrix(), t.bound_history(), t.get_info()["residual"], t.get_info()["iterations"])
        assert cold[0] == plain[0] and same_bits(cold[1], plain[1]) and same_bits(cold[2], plain[2]) and cold[3:] == plain[3:]
        # keep_starts(0) releases everything
        assert s.keep_starts(0) == 0 and s.start_count() == 0
        assert T.decode(T.lib.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None))[::2] == (UNDOCUMENTED, ord("X"))
        assert T.decode(T.lib.tfqmrgpuExt_pushStart(s.handle, s.plan))[::2] == (UNDOCUMENTED, ord("X"))


def test_statuses_that_need_a_device():
    pr = load_problem("dense_random_rect")
    raw = lambda s: T.decode(T.lib.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None))[::2]      # noqa: E731
    with T.Solver.open(pr, "z", keep_starts=2) as s:
        s.set_matrix("B", pr.B)
        X0 = s.get_matrix()
        s.push_start()
        assert raw(s) == (UNDOCUMENTED, ord("A"))           # A never set whole
        s.set_matrix("A", pr.A)
        s.set_operator(lambda *a: 0.0)
        assert raw(s) == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert same_bits(s.get_matrix(), X0)
        # the starts belong to the buffer: setBuffer releases them, the depth stays
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, "z"))
        assert s.start_count() == 0
        s.set_matrix("A", pr.A)
        assert raw(s) == (UNDOCUMENTED, ord("X"))
        s.push_start()
        assert s.start_count() == 1 and raw(s) == (0, 0)    # both outputs NULL: it still projects


# ---- 6. ranks ------------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_give_the_bits_of_one(tmp_path):
    name, prec = "fd_16x16_small", "z"
    pr, s, starts, A, B = _energy_loop(name, prec)
    with s:
        got = s.project_start()
        X = s.get_matrix()
    src, out = str(tmp_path / "starts.npz"), str(tmp_path / "sharded.npz")
    np.savez(src, A=P.shifted(pr, P.shifts(pr, name)[-1]), starts=np.array(starts))
    g = run_ranks(2, "project", out, name, prec, src, timeout=300)
    assert len(g["n_cols"]) == 2 and all(n > 0 for n in g["n_cols"]) and list(g["calls"]) == [0, 0]      # local: no collective
    assert same_bits(g["gamma"], got["coefficients"]) and np.array_equal(g["used"], got["n_used"]) and same_bits(g["X"], X)


# ---- 7. the loop ---------------------------------------------------------------------------------------------------------------------------
def test_the_energy_loop():
    """fd_16x16_small 'z': solve_from after project_start (3 starts) against solve_from from S_0 alone; both reach the threshold.  The
    iteration counts are a measurement, not a promise (profiles/project_start.txt): one synthetic shift family, not an energy mesh.
    MI355X: residual 1.455 from S_0 and 0.365 projected, 19 iterations either way (the shifts of this fixture sit at its resonance, far apart)"""
    name, prec = "fd_16x16_small", "z"
    pr, s, starts, A, B = _energy_loop(name, prec)
    with s:
        s.set_matrix("X", starts[0])
        from_s0 = s.residual()["worst"]
        assert s.solve_from(THR[prec], 500) == 0
        its_s0, res_s0 = s.get_info()["iterations"], s.residual()["worst"]
        s.project_start()
        projected = s.residual()["worst"]
        assert s.solve_from(THR[prec], 500) == 0
        its_p, res_p = s.get_info()["iterations"], s.residual()["worst"]
        s.push_start()
        assert s.start_count() == 3
    print("energy loop %s %s: from S_0 residual %.3e, %d iterations -> %.3e | projected residual %.3e, %d iterations -> %.3e" % (
        name, prec, from_s0, its_s0, res_s0, projected, its_p, res_p))
    assert res_s0 <= 1.01 * THR[prec] and res_p <= 1.01 * THR[prec] and projected <= from_s0
