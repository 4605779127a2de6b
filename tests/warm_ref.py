"""numpy restatement of the warm start (include/tfqmrgpu_ext.h section 14), for the tests, in complex128: R = B - trunc(A X0) over the
analysis of the oracle -- the product truncated to the pattern of X, as tests/precond_ref.py forms it --, and the correction problem
A D = R as a Problem whose B has the pattern of X, which the oracle solves like any other.  X0 + D is what solveFrom returns."""
import numpy as np

import tfqmrgpu_amd as T
from precond_ref import _product


def residual(oracle, pr, X0, A=None, B=None):
    """R [nnzbX, LM, LN] in the caller's block order of X: B scattered onto the pattern of X, minus the truncated A X0"""
    an = oracle.analyse(pr)
    assert an["status"] == 0
    A = pr.A if A is None else A
    B = pr.B if B is None else B
    R = -_product(an, pr, np.asarray(A, np.complex128), np.asarray(X0, np.complex128))
    R[an["subset"].astype(np.int64)] += B
    return R


def correction_problem(oracle, pr, X0, A=None, B=None):
    """the Problem A D = R: the A and the pattern of X of `pr`, right-hand sides R on the pattern of X"""
    A = pr.A if A is None else A
    return T.Problem(pr.rowPtrA, pr.colIndA, A, pr.rowPtrX, pr.colIndX, pr.rowPtrX, pr.colIndX, residual(oracle, pr, X0, A, B),
                     None, pr.tolerance, pr.index_offset)
