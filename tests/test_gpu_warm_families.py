"""The warm start (include/tfqmrgpu_ext.h sections 14 and 16) in every fused multiply family, on every block shape and chunk edge,
against the CPU oracle's solve of the correction problem A D = R (tests/warm_ref.py) on planted starts (tests/warm_cases.py;
tests/test_warm_cases_cpu.py has checked them on the CPU).  While a warm solve runs DevPlan::R is set, so every fused multiply reads its
right-hand side X-shaped from d.R: the first-iteration variants of EPI_XPAY_DOT and EPI_AXPY_NRM_DOT, EPI_RESIDUAL, and ld_rhs of the unfolded
vector kernels -- in double only here.  In front of it k_warm_residual, k_warm_init_col and k_warm_update (tfq_warm.hip) run per shape.

Every case: set_matrix('X', X0) keeps the bits; after exactly k iterations the work vectors v4 ... v9 are the oracle's for A D = R and
X is X0 + D, within warm_cases.allowance(k) -- the cold solve's state bound plus what the oracle itself moves by when R changes by its
a-priori rounding bound; a solve to the threshold reports the residual of the caller's system.  No tolerance is derived from an output of
the library.  A failure with the CPU conditions met: v5 | v9 alone point to the first-iteration epilogue, x alone to k_warm_update,
everything to k_warm_residual or ld_b_under_x.  Figures per case: profiles/warm_families.txt."""
import numpy as np
import pytest

import plan_paths as PP
import residual_ref as RR
import tfqmrgpu_amd as T
import warm_cases as WC
from conftest import offset1
from helpers import same_bits

pytestmark = pytest.mark.gpu

MAX_ITERATIONS = 9
BJ = T.PRECOND_BLOCK_JACOBI


def _open(cs, **options):
    pr = offset1(cs.pr) if cs.key == WC.OFFSET1 else cs.pr
    return T.Solver.open(pr, cs.prec, three_products=cs.three, **options).load()


def _start(s, cs):
    """a. the planted start arrives bit for bit"""
    s.set_matrix("X", cs.X0)
    assert same_bits(s.get_matrix().astype(np.complex128), cs.X0), cs.key


def _state_after(oracle, cs, k):
    """b. exactly k iterations from X0 on a fresh plan; returns the largest deviation as a fraction of its allowance"""
    want, allowed = WC.reference(oracle, cs.key, k), WC.allowance(oracle, cs.key, k)
    with _open(cs) as s:
        if cs.family is not None:
            assert s.multiply_kernel() == cs.family, (cs.key, s.multiply_kernel())
        _start(s, cs)
        assert s.solve_from(1e-30, k) == MAX_ITERATIONS, cs.key
        got = {w: s.get_work_vector(w) for w in WC.VECTORS}
        assert same_bits(got[1], s.get_matrix().astype(np.complex128)), cs.key
    frac = {}
    for w in WC.VECTORS:
        scale = np.abs(want[w]).max()
        ref = cs.X0 + want[1] if w == 1 else want[w]
        assert np.all(np.isfinite(got[w])), (cs.key, k, w)
        frac[w] = float(np.abs(got[w] - ref).max() / scale / allowed[w])
    print("warm families %s k=%d: %s worst %.3e of the allowance %.3e" % (
        WC.case_id(cs.key), k, " ".join("v%d %.2e" % (w, f) for w, f in frac.items()), max(frac.values()), allowed[4]))
    assert max(frac.values()) <= 1, (cs.key, k, frac)
    return max(frac.values())


def _solves_the_callers_system(oracle, cs, thr, **options):
    """c. to the threshold from X0: the reported residual (the EPI_RESIDUAL epilogue, which read d.R) is that of B - A X in float64 within its
    a-priori rounding bound, and residual() agrees with its numpy restatement"""
    with _open(cs, **options) as s:
        _start(s, cs)
        assert s.solve_from(thr, 300) == 0, cs.key
        info, X, got = s.get_info(), s.get_matrix().astype(np.complex128), s.residual()
        n_identity = s.get_preconditioner(values=False)[1] if options else None
    res, bound = PP.true_residual(cs.pr, X, cs.prec)
    print("warm families %s%s: %d iterations, residual %.3e reported, %.3e in float64, bound of the difference %.2e" % (
        WC.case_id(cs.key), " preconditioned" if options else "", info["iterations"], info["residual"], res, bound))
    assert info["residual"] <= thr, (cs.key, info["residual"])
    assert abs(info["residual"] - res) <= bound, (cs.key, info["residual"], res, bound)
    ref = RR.residual(oracle, cs.pr, cs.A, X, cs.B)
    assert np.allclose(got["residual2"], ref["residual2"], rtol=0, atol=float(ref["bound_r2"].max()) + 1e-300), cs.key
    return n_identity


@pytest.mark.parametrize("key", WC.EVERY_CASE, ids=WC.case_id)
def test_warm_start_against_the_oracle(oracle, key):
    """F: every row of family_cases.ROWS (its family asserted first).  S: the 15 shapes x 'z', 'c' on columns of 16, 4 and 8 blocks, and B
    under every second X block on the ragged shapes, 16 x 16 'c' and 64 x 64 'z' (one case on 1-based indices).  E: columns of 25 | 50
    chunks with and without a short last chunk, 18 chunks of eight trips a lane, the second batch of column_sum<64, 1>, a column of one block.
    MI355X, worst deviation as a fraction of the allowance: 'z' 0.995 (F-ilv16_16x16_z_segmented, k = 1, v5: the first iteration's scalar
    is a dot over 67 200 dense terms a right-hand side, the cold bound was measured on dots of 16), 'c' 0.425 (F-ilvf_64x64_c); every case
    and k: profiles/warm_families.txt"""
    cs = WC.case(oracle, key)
    for k in sorted(WC.BOUND[cs.store]):
        _state_after(oracle, cs, k)
    _solves_the_callers_system(oracle, cs, WC.THRESHOLD[cs.store])


def test_every_row_shape_and_edge_is_among_the_cases():
    ids = {WC.case_id(k) for k in WC.EVERY_CASE}
    assert all("F-" + r[0] in ids for r in WC.FC.ROWS)
    assert all("S-%dx%d-%s-full" % (LM, LN, p) in ids for LM, LN in WC.SHAPES for p in "zc")
    assert all(any(i.startswith("E-" + name + "-") for i in ids) for name in WC.PC.PATTERNS)


@pytest.mark.parametrize("key", WC.TWICE, ids=WC.case_id)
def test_two_calls_give_the_same_bits(oracle, key):
    """d. an unfolded 'z' plan, a ragged 'c' plan and a segmented column: X, the bound history and get_info of the last solve"""
    cs = WC.case(oracle, key)
    out = []
    with _open(cs) as s:
        for _ in range(2):
            _start(s, cs)
            st = s.solve_from(WC.THRESHOLD[cs.store], 6)
            info = s.get_info()
            out.append((st, s.get_matrix(), s.bound_history(), {k: v for k, v in info.items() if k != "flops_all"}))
    a, b = out
    assert a[0] == b[0] and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and a[3] == b[3], key
    assert len(a[2]) > 0 and not same_bits(a[1].astype(np.complex128), cs.X0)


@pytest.mark.parametrize("key", WC.PRECONDITIONED, ids=WC.case_id)
def test_preconditioned_with_a_kept_operator(oracle, key):
    """e. block Jacobi with keep_operator: R formed from the kept A, precond_back on D, the update; every block row has its M_ii"""
    cs = WC.case(oracle, key)
    assert _solves_the_callers_system(oracle, cs, WC.THRESHOLD[cs.store], preconditioner=BJ, keep_operator=True) == 0


# ---- 'm': refine_from ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", WC.CASES_M, ids=WC.case_id)
def test_refine_from_on_the_float_plans_chunk_tables(oracle, key):
    """k_warm_residual<double> and k_warm_bn2_col on the float plan's chunk tables (two trips a lane on the long columns): the first entry of
    the refinement history is the residual of X0, within the bound of its numpy restatement on the square; the refinement converges to the
    oracle's 'z' solution; a second call from the same X0 gives the same bits"""
    cs = WC.case(oracle, key)
    want, bound2 = RR.worst(RR.residual(oracle, cs.pr, cs.A, cs.X0, cs.B))
    st0, Xz, _ = oracle.solve(cs.pr, "z", threshold=1e-9, max_iterations=300)
    assert st0 == 0
    out = []
    with _open(cs) as s:
        for _ in range(2):
            _start(s, cs)
            assert s.refine_from(1e-9, 300) == 0, key
            h, it = s.refinement_history(with_iterations=True)
            out.append((s.get_matrix(), h, it, s.bound_history(), s.get_info()["residual"], s.residual()["worst"]))
    X, h, worst = out[0][0], out[0][1], out[0][5]
    print("warm families %s: first residual %.6e, numpy %.6e, |difference of the squares| %.2e, bound %.2e; final %.3e; X off the oracle's by %.2e" % (
        WC.case_id(key), h[0], want, abs(h[0] ** 2 - want ** 2), bound2, worst, np.abs(X - Xz).max() / np.abs(Xz).max()))
    assert abs(h[0] ** 2 - want ** 2) <= bound2, (key, h[0], want, bound2)
    assert worst <= 1.01e-9, (key, worst)
    assert np.abs(X - Xz).max() <= 1e-7 * np.abs(Xz).max(), key
    assert all(same_bits(a, b) for a, b in zip(out[0][:4], out[1][:4])) and out[0][4:] == out[1][4:], key
