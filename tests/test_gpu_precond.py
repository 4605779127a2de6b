"""Block-Jacobi right preconditioner (include/tfqmrgpu_ext.h section 7) on the GPU, through the C-ABI: M^-1 itself against the
float64 inverse, the preconditioned solve judged by the residual of the ORIGINAL system in float64 and against the CPU oracle fed with
the library's own M^-1, fewer iterations on the finite-difference fixtures, nothing changed when it is off, reuse over solves, the
edge cases and the mixed-precision mode.  Needs an MI355X (`pytest -m gpu`)."""
import numpy as np
import pytest

import precond_ref as PC
import tfqmrgpu_amd as T
from conftest import ALL_NAMES, FD_NAMES, load_problem
from solve_helpers import solve_and_check_residual, system_with_two_unit_rows
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

BJ = T.PRECOND_BLOCK_JACOBI
SIZES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
         (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]


# ---- M^-1 itself ----------------------------------------------------------------------------------------------------------------
def _diagonal_system(LM, seed):
    """block-diagonal A of 12 non-symmetric blocks that need row exchanges: random entries, no dominant diagonal; block 0 has a zero
    in (0, 0), block 1 a zero first column but for its last row, block 2 is a permutation matrix times a random diagonal"""
    rng = np.random.default_rng(seed)
    mb = 12
    A = rng.standard_normal((mb, LM, LM)) + 1j * rng.standard_normal((mb, LM, LM))
    A[0, 0, 0] = 0
    A[1, :-1, 0] = 0
    A[2] = np.eye(LM)[rng.permutation(LM)] * (rng.uniform(0.5, 2, LM) * np.exp(2j * np.pi * rng.random(LM)))
    A[3] *= 1e-3
    A[4] *= 1e+3
    B = rng.standard_normal((mb, LM, LM)) + 0j
    return T.Problem(np.arange(mb + 1), np.arange(mb), A, np.arange(mb + 1), np.zeros(mb, int), np.arange(mb + 1), np.zeros(mb, int), B, None, 1e-9)


@pytest.mark.parametrize("prec", ["z", "c"])
@pytest.mark.parametrize("LM", [4, 8, 16, 32, 64])
def test_inverse_of_the_diagonal_blocks(prec, LM):
    """|M^-1 M - 1|_inf <= K LM eps kappa_inf(M), eps of the precision M^-1 is stored in (tests/precond_ref.py: MINV_K)"""
    pr = _diagonal_system(LM, seed=100 + LM)
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        Minv, n_identity = s.get_preconditioner()
    assert n_identity == 0
    # what the library was given: the blocks as they were stored (complex<float> plans round them)
    M = pr.A.astype(np.complex64).astype(np.complex128) if prec == "c" else pr.A
    eps = np.finfo(np.float32 if prec == "c" else np.float64).eps
    inf_norm = lambda a: np.abs(a).sum(axis=-1).max(axis=-1)        # noqa: E731
    kappa = inf_norm(M) * inf_norm(np.linalg.inv(M))
    defect = inf_norm(Minv @ M - np.eye(LM))
    ratio = defect / (LM * eps * kappa)
    print("precond M^-1 %s LM=%d: largest |M^-1 M - 1| / (LM eps kappa) = %.3e (block %d), kappa up to %.1e" % (
        prec, LM, ratio.max(), int(ratio.argmax()), kappa.max()))
    assert np.all(np.isfinite(Minv))
    assert np.all(ratio <= PC.MINV_K), (ratio.max(), int(ratio.argmax()))


# ---- the solve, judged without an oracle ---------------------------------------------------------------------------------------
# every system with stored results under tests/golden but julia_kat: its solve ends at 5e-15, in the rounding noise of double
# (tests/tolerances.py: "converges to 5e-15"), where no two summation orders agree to 1e-4 of the residual -- with or without M^-1
# (its diagonal blocks are unit matrices: the preconditioner does nothing there)
@pytest.mark.parametrize("name", [n for n in ALL_NAMES if n != "julia_kat"])
def test_solve_of_the_fixtures_by_the_float64_residual(oracle, name):
    solve_and_check_residual(oracle, load_problem(name), "z", 1e-9)


# complex<float> cases.  A float residual can only be held against the float64 residual of the returned X to 2e-2 where it is far above
# what the storage in float alone moves it by: X, A M^-1 and M^-1 are each rounded to 2^-24 = 6e-8 relative, which moves |B - A X| / |B|
# by a few 1e-7 (| |A||X| | / |B| is 2 ... 5 on these systems).  2e-2 of the residual is safely more than that from 3e-5 on.  The strongly
# diagonally dominant stencils of the 'z' cases gain three digits per iteration in float and end anywhere between 2e-7 and 8e-5, so the
# 'c' cases are chosen with the CPU oracle, not with the library: a 6 x 6 stencil whose diagonal blocks are weakened from 2 + .. to
# 0.35 + .. (about a digit per iteration), and the first threshold of C_THRESHOLDS at which the ORACLE's preconditioned complex<float>
# solve ends at 3e-5 or above.  Both sides use the glibc shadow vector, so that the library stops where the oracle does.
C_THRESHOLDS = (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2)
C_MIN_RESIDUAL = 3e-5


def _float_case(oracle, LM, LN):
    pr = PR.stencil_2d(6, 6, LM, LN, 2, seed=LM + LN)
    pr.A[PC.diagonal_blocks(pr)] -= 1.65 * np.eye(LM)
    Minv, n_identity = PC.inverse_blocks(pr)
    assert n_identity == 0
    for tol in C_THRESHOLDS:
        st, _, info = PC.solve_with_oracle(oracle, pr, Minv, "c", threshold=tol, max_iterations=100)
        if st == 0 and info["residual"] >= C_MIN_RESIDUAL:
            return pr, tol, info
    raise AssertionError("no threshold of C_THRESHOLDS leaves the oracle's float solve of the %d x %d case at %.0e or above" % (LM, LN, C_MIN_RESIDUAL))


def _check_flop_count(oracle, pr, info):
    # getInfo counts the back transform, 8 LM LM LN nnzbX, on top of the reference's flop model (iterations and residual probes)
    LM, LN = pr.LM, pr.LN
    blk, nX, nPairs = LM * LN, pr.nnzbX, oracle.analyse(pr)["nPairs"]
    fMult, fDot, fNrm, fAxp = nPairs * 8.0 * LM * blk, nX * 8.0 * blk, nX * 4.0 * blk, nX * 8.0 * blk
    rest = info["flops"] - 8.0 * LM * LM * LN * nX - fNrm - info["iterations"] * (2 * fMult + 2 * fDot + 2 * fNrm + 10 * fAxp)
    probes = rest / (fMult + fNrm)
    assert probes >= 1 and probes == int(probes), probes


@pytest.mark.parametrize("size", SIZES)
def test_solve_of_every_block_shape_by_the_float64_residual(oracle, size):
    LM, LN = size
    pr = PR.stencil_2d(4, 4, LM, LN, 2, seed=LM + LN, radius=2.3)
    _, info = solve_and_check_residual(oracle, pr, "z", 1e-9, maxit=100)
    assert info["n_identity"] == 0
    _check_flop_count(oracle, pr, info)


@pytest.mark.parametrize("size", SIZES)
def test_float_solve_of_every_block_shape_by_the_float64_residual(oracle, size):
    LM, LN = size
    pr, tol, info0 = _float_case(oracle, LM, LN)
    _, info = solve_and_check_residual(oracle, pr, "c", tol, maxit=100, shadow=T.SHADOW_GLIBC_RAND)
    print("precond float case %dx%d: oracle %d iterations, residual %.3e" % (LM, LN, info0["iterations"], info0["residual"]))
    assert info["n_identity"] == 0
    _check_flop_count(oracle, pr, info)


# ---- the solve against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FD_NAMES + ["dense_random", "stencil_8x8"])
def test_solve_matches_the_oracle_fed_with_the_librarys_inverse(oracle, name):
    """glibc shadow vector on both sides; the oracle solves (A M^-1) Y = B with the library's own M^-1 (A M^-1 formed in float64 by
    numpy) and X = M^-1 Y: equal iteration counts, X within 1e-7 max|X| (the tolerance of tests/test_gpu_parity.py for 'z')"""
    pr = load_problem(name)
    tol = 1e-9
    with T.Solver.open(pr, "z", preconditioner=BJ, shadow_mode=T.SHADOW_GLIBC_RAND) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        Minv, n_identity = s.get_preconditioner()
        st = s.solve(tol, 2000)
        info, X, hist = s.get_info(), s.get_matrix(), s.bound_history()
    st0, X0, info0 = PC.solve_with_oracle(oracle, pr, Minv, "z", threshold=tol, max_iterations=2000)
    print("precond oracle %s: %d | %d iterations, residual %.3e | %.3e, max|X - X0| / max|X0| = %.2e" % (
        name, info["iterations"], info0["iterations"], info["residual"], info0["residual"], np.abs(X - X0).max() / np.abs(X0).max()))
    assert st == st0 == 0 and n_identity == 0
    assert info["iterations"] == info0["iterations"]
    assert np.abs(X - X0).max() <= 1e-7 * np.abs(X0).max()
    assert len(hist) == len(info0["bound_history"])


# ---- fewer iterations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,expected", [("fd_16x16_2d", 7), ("fd_16x16_small", 7), ("fd_8x8_3d", 27), ("fd_4x4_2d", 21)])
def test_block_jacobi_needs_fewer_iterations(name, expected):
    pr = load_problem(name)
    st0, X0, plain = T.solve_problem(pr, "z", threshold=1e-9, shadow_mode=T.SHADOW_GLIBC_RAND)
    st1, X1, jacobi = T.solve_problem(pr, "z", threshold=1e-9, shadow_mode=T.SHADOW_GLIBC_RAND, preconditioner=BJ)
    print("precond iterations %s: plain %d, block Jacobi %d" % (name, plain["iterations"], jacobi["iterations"]))
    assert st0 == st1 == 0
    assert jacobi["iterations"] < plain["iterations"]
    assert jacobi["iterations"] == expected
    assert np.abs(X1 - X0).max() <= 1e-7 * np.abs(X0).max()        # both stop at 1e-9


# ---- nothing changes when it is off ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,name", [("z", "fd_16x16_small"), ("c", "fd_16x16_2d"), ("m", "fd_16x16_small"), ("z", "stencil_8x32")])
def test_off_is_bit_identical_to_never_asked(prec, name):
    pr = load_problem(name)
    tol = 1e-4 if prec == "c" else 1e-9
    got = []
    for kind in (None, T.PRECOND_NONE):
        with T.Solver.open(pr, prec, preconditioner=kind) as s:
            nbytes = s.buffer_bytes
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(tol, 500)
            got.append((st, nbytes, s.get_info(), s.bound_history(), s.get_matrix(), s.refinement_history()))
    a, b = got
    assert a[0] == b[0] == 0 and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:                 # and a plan with block Jacobi has the same buffer
        assert s.buffer_bytes == a[1]


# ---- reuse ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "m"])
def test_reuse_over_solves_and_a_new_matrix(oracle, prec):
    pr = load_problem("fd_16x16_small")
    rng = np.random.default_rng(8)
    B2 = pr.B * (1.5 - 0.5j) + 0.1 * rng.standard_normal(pr.B.shape)
    A2 = pr.A * (1 + 0.05 * rng.standard_normal(pr.A.shape))

    def fresh(A, B):
        with T.Solver.open(pr, prec, preconditioner=BJ) as s:
            s.set_matrix("A", A)
            s.set_matrix("B", B)
            assert s.solve(1e-9, 500) == 0
            return s.get_info(), s.get_matrix(), s.bound_history()
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 500) == 0
        first = (s.get_info(), s.get_matrix(), s.bound_history())
        Minv1 = s.get_preconditioner()[0]
        s.set_matrix("B", B2)                                        # same A, new B: M^-1 and the scaled A are reused
        assert s.solve(1e-9, 500) == 0
        second = (s.get_info(), s.get_matrix(), s.bound_history())
        assert np.array_equal(s.get_preconditioner()[0], Minv1)
        s.set_matrix("A", A2)                                        # a new A is picked up
        assert s.solve(1e-9, 500) == 0
        third = (s.get_info(), s.get_matrix(), s.bound_history())
        assert not np.array_equal(s.get_preconditioner()[0], Minv1)
    for got, (A, B) in ((first, (pr.A, pr.B)), (second, (pr.A, B2)), (third, (A2, B2))):
        want = fresh(A, B)
        assert got[0]["iterations"] == want[0]["iterations"] and got[0]["residual"] == want[0]["residual"]
        assert got[0]["flops"] == want[0]["flops"]
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert second[0]["flops_all"] == first[0]["flops"] + second[0]["flops"]
    pr2 = T.Problem(pr.rowPtrA, pr.colIndA, A2, pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, B2, None, 1e-9)
    assert PC.worst_relative_residual(oracle, pr2, third[1]) <= 1e-9


# ---- edge cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_rows_without_an_invertible_diagonal_block(oracle, prec):
    pr = system_with_two_unit_rows()
    tol = 1e-9 if prec == "z" else 1e-4
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(tol, 500) == 0
        info, X = s.get_info(), s.get_matrix()
        Minv, n_identity = s.get_preconditioner()
    assert n_identity == 2
    assert np.array_equal(Minv[3], np.eye(8)) and np.array_equal(Minv[7], np.eye(8))
    assert PC.inverse_blocks(pr)[1] == 2
    worst = PC.worst_relative_residual(oracle, pr, X)
    print("precond edge %s: %d iterations, reported %.6e, recomputed %.6e" % (prec, info["iterations"], info["residual"], worst))
    assert worst <= tol
    assert abs(worst - info["residual"]) <= (1e-4 if prec == "z" else 2e-2) * info["residual"]


def test_non_finite_diagonal_block_gets_the_unit_matrix():
    pr = _diagonal_system(16, seed=5)
    pr.A[6, 2, 3] = np.nan
    pr.A[9, 0, 0] = np.inf
    with T.Solver.open(pr, "z", preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        Minv, n_identity = s.get_preconditioner()
    assert n_identity == 2 and np.array_equal(Minv[6], np.eye(16)) and np.array_equal(Minv[9], np.eye(16))
    assert np.all(np.isfinite(Minv))


@pytest.mark.parametrize("prec,tiny", [("z", 1e-310), ("c", 1e-40)])
def test_inverse_that_overflows_its_storage_gets_the_unit_matrix(prec, tiny):
    """a regular block of denormal numbers: every pivot is finite and not zero, the inverse is not representable in the precision M^-1 is
    stored in -- nothing but finite numbers is stored, the row is counted"""
    pr = _diagonal_system(8, seed=6)
    pr.A[5] *= tiny
    with T.Solver.open(pr, prec, preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        Minv, n_identity = s.get_preconditioner()
    assert np.all(np.isfinite(Minv))
    assert n_identity == 1 and np.array_equal(Minv[5], np.eye(8))


def test_user_operator_plans_refuse():
    pr = load_problem("fd_16x16_small")
    for prec in "zc":
        with T.Solver.open(pr, prec, preconditioner=BJ) as s:
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            s.set_operator(lambda *a: 0.0)
            st = T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, 1e-9, 100)
            assert T.decode(st)[0] == 19                              # TFQMRGPU_NO_IMPLEMENTATION
            s.set_operator(None)
            assert s.solve(1e-9 if prec == "z" else 1e-4, 500) == 0   # the built-in operator again: solves


def test_switching_the_kind_needs_a_new_matrix():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "z", preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(1e-9, 500) == 0
        with_bj = (s.get_info()["iterations"], s.get_matrix())
        s.set_preconditioner(T.PRECOND_NONE)                         # the A in the buffer is A M^-1
        st = T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, 1e-9, 500)
        assert T.decode(st)[::2] == (14, ord("A"))                    # the documented status: code 14, key 'A'
        s.set_matrix("A", pr.A)
        assert s.solve(1e-9, 500) == 0
        plain = (s.get_info()["iterations"], s.get_matrix())
        s.set_preconditioner(BJ)                                     # NONE -> BLOCK_JACOBI on an unscaled A needs nothing
        assert s.solve(1e-9, 500) == 0
        again = (s.get_info()["iterations"], s.get_matrix())
        assert T.decode(T.lib.tfqmrgpuExt_setPreconditioner(s.plan, 2))[0] == 14
    st0, X0, info0 = T.solve_problem(pr, "z", threshold=1e-9, max_iterations=500)
    assert plain[0] == info0["iterations"] and np.array_equal(plain[1], X0)
    assert again[0] == with_bj[0] and np.array_equal(again[1], with_bj[1])
    with T.Solver.open(pr, "z") as s:                                            # never set: the getter refuses
        assert T.decode(T.lib.tfqmrgpuExt_getPreconditioner(s.handle, s.plan, None, None))[0] == 14
        s.set_preconditioner(BJ)                                     # no A yet
        assert T.decode(T.lib.tfqmrgpuExt_getPreconditioner(s.handle, s.plan, None, None))[::2] == (14, ord("A"))


def test_work_vector_and_stopped_solves_return_x(oracle):
    """getWorkVector(1) is X like getMatrix('X'); a solve that ends at maxIterations is back-transformed too: its X is M^-1 times the Y
    that the oracle has after the same iterations"""
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "z", preconditioner=BJ, shadow_mode=T.SHADOW_GLIBC_RAND) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        Minv = s.get_preconditioner()[0]
        assert s.solve(1e-9, 3) == 9
        X3 = s.get_matrix()
        assert np.array_equal(s.get_work_vector(1), X3)
    st0, X0, info0 = PC.solve_with_oracle(oracle, pr, Minv, "z", threshold=1e-9, max_iterations=3)
    assert st0 == 9 and np.abs(X3 - X0).max() <= 1e-9 * np.abs(X0).max()


def test_apply_operator_multiplies_with_the_scaled_matrix(oracle):
    pr = load_problem("fd_16x16_small")
    rng = np.random.default_rng(2)
    X = rng.standard_normal((pr.nnzbX, 16, 16)) + 1j * rng.standard_normal((pr.nnzbX, 16, 16))
    an = oracle.analyse(pr)
    with T.Solver.open(pr, "z", preconditioner=BJ) as s:
        s.set_matrix("A", pr.A)
        Minv = s.get_preconditioner()[0]                             # scales A
        s.set_matrix("X", X)
        s.apply_operator()
        got = s.get_matrix()
    want = oracle.from_native(oracle.spmm("z", 16, 16, an["starts"], an["pairs"], oracle.a_native(PC.scaled_A(pr, Minv), np.float64),
                                          oracle.to_native(X, np.float64)))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---- mixed precision --------------------------------------------------------------------------------------------------------------
def test_mixed_precision(oracle):
    pr = load_problem("fd_16x16_2d")
    st, X, info = T.solve_problem(pr, "m", threshold=1e-9, max_iterations=500, preconditioner=BJ)
    worst = PC.worst_relative_residual(oracle, pr, X)
    print("precond mixed: %d float iterations, refinement %s, reported %.6e, recomputed %.6e" % (
        info["iterations"], info["refinement_history"], info["residual"], worst))
    assert st == 0 and info["residual"] <= 1e-9 and worst <= 1e-9
    assert abs(worst - info["residual"]) <= 1e-4 * info["residual"]
    h = info["refinement_history"]
    assert len(h) >= 2 and h[0] == pytest.approx(1.0) and h[-1] == info["residual"]
    stz, Xz, infoz = T.solve_problem(pr, "z", threshold=1e-9, max_iterations=500, preconditioner=BJ)
    assert np.abs(X - Xz).max() <= 1e-7 * np.abs(Xz).max()
