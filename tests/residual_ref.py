"""numpy restatement of tfqmrgpuExt_residual (include/tfqmrgpu_ext.h section 10), for the tests: B - A X in complex128 over the analysis
of the oracle, truncated to the pattern of X, and per (block column, right-hand side) the sums of |B - A X|^2 and of |B|^2 -- the sums of
tests/precond_ref.py (_product, _worst_column_ratio) as [nCols][LN] arrays instead of one maximum.

Also the a-priori bound of the comparison.  The kernel and numpy both sum products that are exact in double (float data) or rounded
once (double data) in double arithmetic and differ only in the order of the sums.  With u = 2^-53, for one element r = sum a x - b of
the residual, a sum of n complex terms: the two values differ by at most
    e = 4 n u (sum |a| |x| + |b|)               (n u sum |terms|, times 4 for the four real products and adds of the complex pattern)
for |r|^2 that is 2 |r| e + e^2, and the sum of the N squares of an entry (N = LM x blocks of the column) adds 4 N u sum |r|^2:
    bound_r2 = sum (2 |r| e + e^2) + 4 N u sum |r|^2,      bound_b2 = 4 N_b u sum |b|^2.
Everything in the bound comes from the operands, nothing from the kernel's output."""
import numpy as np

from precond_ref import _product

U = 2.0 ** -53


def stored(a, precision):
    """complex blocks as a plan of that precision stores them: 'c' rounds to float32, 'z' and 'm' (double copies) keep double"""
    a = np.asarray(a, dtype=np.complex128)
    return a.astype(np.complex64).astype(np.complex128) if precision == "c" else a


def _column_sums(an, pr, per_block, blocks_col):
    out = np.zeros((an["nCols"], pr.LN))
    np.add.at(out, blocks_col, per_block)
    return out


def residual(oracle, pr, A, X, B=None):
    """dict of [nCols][LN] arrays residual2, bnorm2, their bounds bound_r2, bound_b2, and columns (the caller's block column indices)"""
    an = oracle.analyse(pr)
    assert an["status"] == 0
    B = pr.B if B is None else B
    sub, col = an["subset"].astype(np.int64), an["colindx"].astype(np.int64)
    R = _product(an, pr, A, X)
    R[sub] -= B
    mag = _product(an, pr, np.abs(A), np.abs(X))                     # sum |a| |x| per element
    mag[sub] += np.abs(B)
    n_terms = pr.LM * np.diff(an["starts"].astype(np.int64)).astype(np.float64)
    n_terms[sub] += 1
    e = 4 * n_terms[:, None, None] * U * mag
    r2_block, absR = (np.abs(R) ** 2).sum(axis=1), np.abs(R)
    res2 = _column_sums(an, pr, r2_block, col)
    b2 = _column_sums(an, pr, (np.abs(B) ** 2).sum(axis=1), col[sub])
    n_r = pr.LM * np.bincount(col, minlength=an["nCols"]).astype(np.float64)
    n_b = pr.LM * np.bincount(col[sub], minlength=an["nCols"]).astype(np.float64)
    bound_r2 = _column_sums(an, pr, (2 * absR * e + e * e).sum(axis=1), col) + 4 * n_r[:, None] * U * res2
    bound_b2 = 4 * n_b[:, None] * U * b2
    return dict(residual2=res2, bnorm2=b2, bound_r2=bound_r2, bound_b2=bound_b2, columns=an["original_bsrColIndX"].astype(np.int32))


def worst(ref):
    """(sqrt of the largest residual2 / bnorm2 that is not NaN, the bound of its SQUARE): NaN if every quotient is"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ref["residual2"] / ref["bnorm2"]
        # a quotient moves by at most bound_r2 / b2 + q bound_b2 / b2 (first order; the second-order term is 1e-16 of it)
        dq = ref["bound_r2"] / ref["bnorm2"] + q * ref["bound_b2"] / ref["bnorm2"]
    if np.all(np.isnan(q)):
        return float("nan"), 0.0
    return float(np.sqrt(np.nanmax(q))), float(np.nanmax(np.where(np.isfinite(dq), dq, 0.0)))
