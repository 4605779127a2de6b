"""What the GPU tests that compare whole solves share (helpers.py holds the small pieces): the record a solve leaves behind and its exact
comparison, the patched-operator yardstick of the keep-operator tests, the block-Jacobi residual check, the built-in multiply wrapped as
a user operator, and the cases of the hash-mode tests that tests/parity_report.py prints.  Not a conftest: pytest does not rewrite the
asserts here, so each one that can fail on a result carries its message."""
import numpy as np

import precond_ref as PC
import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import user_array
from tfqmrgpu_amd import problems as PR

BJ = T.PRECOND_BLOCK_JACOBI
TOL = {"z": 1e-9, "c": 1e-4, "m": 1e-9}
MAXIT = 200


# ---- a patched operator against a fresh plan (tests/test_gpu_keep_operator.py, tests/test_gpu_plan_lifecycle.py) ----------------------------
def present_diagonal(pr):
    """positions of the diagonal blocks of A that the pattern has"""
    d = PC.diagonal_blocks(pr)
    return d[d >= 0].astype(np.int32)


def changed(pr, A, blocks, seed):
    """a copy of A with the listed blocks changed by a few per cent of a unit matrix plus noise: the system stays block diagonally dominant"""
    A1 = A.copy()
    shape = (len(blocks), pr.LM, pr.LM)
    A1[blocks] += 0.3 * np.eye(pr.LM) * (1 + 0.5j) + 0.05 * (PR.hashed_uniform(seed, shape) + 1j * PR.hashed_uniform(seed + 1, shape))
    return A1


def solve_record(s, prec, precond=True):
    """everything a solve leaves behind, for exact comparison"""
    st = s.solve(TOL[prec], MAXIT)
    info = s.get_info()
    out = dict(status=st, iterations=info["iterations"], residual=info["residual"], bounds=s.bound_history(), X=s.get_matrix())
    if precond:
        out["Minv"], out["n_identity"] = s.get_preconditioner()
    if prec == "m":
        out["refinement"], out["cycle_iterations"] = s.refinement_history(with_iterations=True)
    return out


def fresh_solve(pr, A, prec, kind=BJ, trans="n", layout=T.LAYOUT_RIRIRIRI):
    """the yardstick: a plan that knows nothing of keepOperator, the whole matrix, one solve"""
    with T.Solver.open(pr, prec, preconditioner=kind) as s:
        s.set_matrix("A", user_array(A, layout, trans), trans, layout)
        s.set_matrix("B", pr.B)
        return solve_record(s, prec, precond=(kind == BJ))


def same_record(got, want):
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert len(want["bounds"]) >= 1 and want["iterations"] >= 1, (len(want["bounds"]), want["iterations"])


def patch_blocks(s, blocks, A, trans="n", layout=T.LAYOUT_RIRIRIRI):
    st = s.set_blocks("A", blocks, user_array(A[blocks], layout, trans), trans, layout)
    assert st == 0, st


# ---- block Jacobi (tests/test_gpu_precond.py, tests/test_gpu_keep_operator.py) ----------------------------------------------------------
def solve_and_check_residual(oracle, pr, prec, tol, maxit=2000, shadow=T.SHADOW_HASH):
    st, X, info = T.solve_problem(pr, prec, threshold=tol, max_iterations=maxit, preconditioner=BJ, shadow_mode=shadow)
    worst = PC.worst_relative_residual(oracle, pr, X)
    print("precond solve %s %dx%d: %d iterations, threshold %.0e, reported %.6e, recomputed %.6e (%.2e of it apart)" % (
        prec, pr.LM, pr.LN, info["iterations"], tol, info["residual"], worst, abs(worst - info["residual"]) / info["residual"]))
    assert st == 0, st
    assert worst <= tol, worst
    # right preconditioning leaves the residual unchanged: the bounds of tests/test_gpu_configs.py: _check_solution_on_device
    assert abs(worst - info["residual"]) <= (2e-2 if prec == "c" else 1e-4) * info["residual"], (worst, info["residual"])
    return X, info


def system_with_two_unit_rows():
    """block row 3 has no diagonal block in the pattern of A, the diagonal block of block row 7 has a zero row (a zero pivot whatever
    the exchanges)"""
    pr = PR.stencil_2d(5, 4, 8, 8, 2, seed=9)
    rows = PC.block_rows(pr.rowPtrA)
    keep = ~((rows == pr.colIndA) & (rows == 3))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=pr.mb))])
    cut = T.Problem(rp, pr.colIndA[keep], pr.A[keep].copy(), pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B, None, 1e-9)
    cut.A[PC.diagonal_blocks(cut)[7], 1, :] = 0
    return cut


# ---- the built-in multiply as a user operator (tests/test_gpu_operator.py, tests/test_gpu_plan_lifecycle.py) --------------------------------
class DevArray:
    """wraps a raw device pointer so that torch can see it (no copy)"""
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


def native_A(torch, pr, prec):
    real = torch.float64 if prec == "z" else torch.float32
    At = pr.A.transpose(0, 2, 1)      # the multiply expects A blocks transposed, [k][i]
    return torch.from_numpy(np.ascontiguousarray(np.stack([At.real, At.imag], axis=1))).to(real).cuda()


def builtin_as_operator(torch, s, pr, prec, view, seen):
    """a callback that computes the same block-sparse product with tfqmrgpuExt_multiply on the caller's block order;
    seen: gets one record of what the first call was handed"""
    An = native_A(torch, pr, prec)
    dS = torch.from_numpy(view["starts"].view(np.int32)).cuda()
    dP = torch.from_numpy(view["pairs"].view(np.int32)).cuda()
    colindx = view["colindx"].copy()

    def multiply(y, x, cols, nnzbX, nCols, lm, ln, precision, stream):
        if not seen:                       # what the reference hands to action_t::multiply
            got = torch.as_tensor(DevArray(cols, (nnzbX,), "<u2"), device="cuda").cpu().numpy()
            seen.append((np.array_equal(got, colindx), nnzbX, nCols, lm, ln, precision))
        T._check(T.lib.tfqmrgpuExt_multiply(s.handle, precision.encode(), lm, ln, nnzbX, dS.data_ptr(), dP.data_ptr(),
                                            An.data_ptr(), x, y), "tfqmrgpuExt_multiply")
        return view["nPairs"] * 8.0 * lm * lm * ln
    return multiply


# ---- the hash-mode cases (tests/test_gpu_hash_mode.py, tests/parity_report.py) ------------------------------------------------------------
HASH_CASES = {
    "fd_16x16_2d": lambda: load_problem("fd_16x16_2d"),
    "fd_16x16_small": lambda: load_problem("fd_16x16_small"),
    "fd_8x8_3d": lambda: load_problem("fd_8x8_3d"),
    "fd_4x4_2d": lambda: load_problem("fd_4x4_2d"),
    "dense_random": lambda: load_problem("dense_random"),
    "stencil_8x8": lambda: load_problem("stencil_8x8"),
    "stencil_8x32": lambda: load_problem("stencil_8x32"),
    "st16x16": lambda: PR.stencil_2d(12, 12, 16, 16, 4, seed=7),          # the bench kernels' shape, 4 block columns
    "st16x16_ragged": lambda: PR.stencil_2d(9, 7, 16, 16, 3, seed=9, radius=3.3),
    "st16x16_onecol": lambda: PR.stencil_2d(12, 12, 16, 16, 1, seed=7),   # one block column: A is used once and streamed past the caches (k_spmm_ilv16 / ilv16f <..., ANT>)
    "st32x32": lambda: PR.stencil_2d(6, 6, 32, 32, 2, seed=3),
}
# work vectors after k iterations: bounds per k = 4 x the worst deviation observed on MI355X (the table of tests/test_gpu_hash_mode.py)
Z_STATE = {1: 7e-14, 2: 2e-10, 5: 1e-9}       # observed 1.6e-14 (st16x16_ragged) / 3.6e-11 (stencil_8x32) / 2.4e-10 (st32x32, stencil_8x32)
STATE_CASES = [("fd_16x16_2d", "z", Z_STATE), ("st16x16_ragged", "z", Z_STATE), ("stencil_8x8", "z", Z_STATE), ("stencil_8x32", "z", Z_STATE),
               ("st32x32", "z", Z_STATE), ("fd_4x4_2d", "z", Z_STATE),
               # float: a dot product with the shadow vector that cancels amplifies the 1e-7 differences of v4 / v5 into alfa, beta
               # and from there into x (seen at k = 2 with the second hash definition: x 1.1e-3, gone again at k = 5)
               ("fd_16x16_2d", "c", {1: 1.2e-6, 2: 5e-3, 5: 7e-2}),     # observed 2.7e-7 / 1.1e-3 / 1.7e-2
               ("st32x32", "c", {1: 6e-5, 2: 1.2e-2})]                 # observed 1.3e-5 / 2.9e-3
STATE_ITERATIONS = [1, 2, 5]
