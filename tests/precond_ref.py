"""numpy restatement of the block-Jacobi right preconditioner (include/tfqmrgpu_ext.h section 7), for the tests: with
M = blockdiag(A) the solver iterates on (A M^-1) Y = B and returns X = M^-1 Y.  Everything here is float64 / complex128 and works
on the caller's block order (T.Problem); the oracle (oracle/pyoracle.py) solves the transformed problem.

Also the bound of the GPU test of M^-1 itself (tests/test_gpu_precond.py), kept here with the observations it rests on."""
import numpy as np

import tfqmrgpu_amd as T

# ---- bound of |M^-1 M - 1| -------------------------------------------------------------------------------------------------------
# test_gpu_precond.py judges the library's M^-1 by  |M^-1 M - 1|_inf <= K * LM * eps * kappa_inf(M),  eps of the precision M^-1 is
# STORED in (the arithmetic of the inversion is double in every precision).
# Where K comes from: Gauss-Jordan with partial pivoting is backward stable row by row of the inverse, |X M - 1|_inf <= c n eps g
# kappa_inf(M) with the growth factor g and a small constant c (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
# section 14.4, X = computed inverse); rounding the entries of X to the storage precision adds at most eps |X| |M| <= eps kappa.
# With g of order 1 for random blocks the ratio  |M^-1 M - 1|_inf / (LM eps kappa_inf)  must come out well below 1.
# Observed on MI355X, the largest ratio over the 12 blocks of tests/test_gpu_precond.py: _diagonal_system per case:
#   z:  LM 4: 1.22e-01   8: 5.26e-02   16: 3.43e-02   32: 1.91e-02   64: 1.04e-02
#   c:  LM 4: 4.19e-02   8: 1.24e-02   16: 6.44e-03   32: 4.21e-03   64: 1.72e-03
# K = 0.5: four times the largest ratio seen, and half of what the bound allows for c g = 1.
MINV_K = 0.5


def block_rows(row_ptr):
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def diagonal_blocks(pr):
    """[mb] index into pr.A of the diagonal block of each block row, -1 where the pattern has none (the first one if a row lists it twice)"""
    rows, cols = block_rows(pr.rowPtrA), pr.colIndA.astype(np.int64) - pr.index_offset
    idx = np.full(pr.mb, -1, dtype=np.int64)
    for q in np.flatnonzero(rows == cols)[::-1]:
        idx[rows[q]] = q
    return idx


def inverse_blocks(pr):
    """M^-1 [mb, LM, LM] from numpy's inverse; the unit matrix for block rows without a diagonal block or with an exactly singular one.
    Returns (Minv, number of unit matrices)."""
    Minv = np.tile(np.eye(pr.LM, dtype=np.complex128), (pr.mb, 1, 1))
    n_identity = 0
    for r, q in enumerate(diagonal_blocks(pr)):
        try:
            if q < 0:
                raise np.linalg.LinAlgError
            Minv[r] = np.linalg.inv(pr.A[q])
        except np.linalg.LinAlgError:
            n_identity += 1
    return Minv, n_identity


def scaled_A(pr, Minv):
    """A_ij M_jj^-1 for every block of A"""
    cols = pr.colIndA.astype(np.int64) - pr.index_offset
    return np.einsum("qik,qkj->qij", pr.A, Minv[cols])


def back_transform(pr, Y, Minv):
    """X_ic = M_ii^-1 Y_ic for every block of an X-shaped operator"""
    return np.einsum("uik,ukj->uij", Minv[block_rows(pr.rowPtrX)], Y)


def preconditioned_problem(pr, Minv):
    return T.Problem(pr.rowPtrA, pr.colIndA, scaled_A(pr, Minv), pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B,
                     None, pr.tolerance, pr.index_offset)


def solve_with_oracle(oracle, pr, Minv, precision="z", threshold=1e-9, max_iterations=2000, v3=None):
    """the oracle's tfQMR on (A M^-1) Y = B, then X = M^-1 Y; returns (status, X, info) like oracle.solve"""
    st, Y, info = oracle.solve(preconditioned_problem(pr, Minv), precision, threshold=threshold, max_iterations=max_iterations, v3=v3)
    return st, back_transform(pr, Y, Minv), info


def _product(an, pr, A, X):
    """A X in float64 / complex128, truncated to the pattern of X like every product of the solver"""
    pairs = an["pairs"].reshape(-1, 2).astype(np.int64)
    y_of_pair = np.repeat(np.arange(pr.nnzbX), np.diff(an["starts"].astype(np.int64)))
    A, X = np.asarray(A), np.asarray(X)
    A, X = A.astype(np.complex128 if np.iscomplexobj(A) else np.float64), X.astype(np.complex128 if np.iscomplexobj(X) else np.float64)
    R = np.zeros((pr.nnzbX, pr.LM, pr.LN), dtype=np.result_type(A, X))
    step = 1 << 14
    for lo in range(0, len(pairs), step):
        sl = slice(lo, lo + step)
        np.add.at(R, y_of_pair[sl], np.einsum("pik,pkj->pij", A[pairs[sl, 0]], X[pairs[sl, 1]]))
    return R


def _worst_column_ratio(an, pr, R):
    """sqrt of max over the right-hand sides of sum |R|^2 / sum |B|^2"""
    sub, col = an["subset"].astype(np.int64), an["colindx"].astype(np.int64)
    res2 = np.zeros((an["nCols"], pr.LN))
    np.add.at(res2, col, (np.abs(R) ** 2).sum(axis=1))
    b2 = np.zeros_like(res2)
    np.add.at(b2, col[sub], (np.abs(pr.B) ** 2).sum(axis=1))
    return float(np.sqrt((res2 / b2).max()))


def worst_relative_residual(oracle, pr, X):
    """max over the right-hand sides of |B - A X| / |B| in float64 with the ORIGINAL A"""
    an = oracle.analyse(pr)
    assert an["status"] == 0
    R = _product(an, pr, pr.A, X)
    R[an["subset"].astype(np.int64)] -= pr.B
    return _worst_column_ratio(an, pr, R)
