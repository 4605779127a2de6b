"""numpy restatement of tfqmrgpuExt_dropCost and tfqmrgpuExt_shrinkPattern (include/tfqmrgpu_ext.h section 13), for the tests.  It uses
neither the library's listing nor planView().pairs: the products of an X block (k, c) are found from the BSR patterns with Python sets --
every A block (i, k) whose block row i lies in the pattern of block column c --, each product A_ik X_kc is formed in complex128 and
squared on its own.  Blocks are numbered in the caller's order of X.

The a-priori bound is built like tests/leak_map_ref.py's.  The kernel and numpy sum products that are exact in double (float data) or
rounded once (double data) in double arithmetic and differ only in the order of the sums.  With u = 2^-53:
  * one element r = sum over k of a x of ONE product is a sum of LM complex terms; the two values differ by at most
        e = 4 LM u sum |a| |x|            (LM u sum |terms|, times 4 for the four real products and adds of the complex pattern);
  * for |r|^2 that is 2 |r| e + e^2, and adding the LM squares of a column of the product block adds 4 LM u sum |r|^2:
        per product:  sum over the LM rows (2 |r| e + e^2) + 4 LM u sum |r|^2;
  * adding the N products of the X block, all non-negative, adds 4 N u cost2:
        bound = sum over the products (sum (2 |r| e + e^2) + 4 LM u sum |r|^2) + 4 N u cost2.
  * weight2 is a sum of the 2 LM real squares of a column of the X block, each rounded once on either side:
        bound_w = 4 LM u weight2.
Everything in the bound comes from the operands, nothing from the kernel's output.  A block without products has cost2 = bound = 0."""
import numpy as np

from leak_ref import _patterns
from residual_ref import U, stored  # noqa: F401


def products(pr):
    """per X block of the caller's order the list of A blocks q = (i, k) that it meets: k its block row, (i, c) in the pattern of X.  Of
    two X blocks on one (block row, block column) only the first has products"""
    rowsA, colsA, rowsX, colsX, _ = _patterns(pr)
    pattern, first = set(), []
    for k, c in zip(rowsX.tolist(), colsX.tolist()):
        first.append((k, c) not in pattern)
        pattern.add((k, c))
    a_of_col = {}
    for q, (i, k) in enumerate(zip(rowsA.tolist(), colsA.tolist())):
        a_of_col.setdefault(k, []).append((q, i))
    return [[q for q, i in a_of_col.get(k, ()) if (i, c) in pattern] if is_first else []
            for k, c, is_first in zip(rowsX.tolist(), colsX.tolist(), first)]


def drop_cost(pr, A, X):
    """dict of cost2, weight2 and their bounds bound, bound_w [nnzbX][LN], n_products, and products_per_block [nnzbX]"""
    A, X = np.asarray(A, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    LM, LN = pr.LM, pr.LN
    lists = products(pr)
    cost2, bound = np.zeros((pr.nnzbX, LN)), np.zeros((pr.nnzbX, LN))
    for n, qs in enumerate(lists):
        if not qs:
            continue
        Y = np.einsum("pik,kj->pij", A[qs], X[n])
        e = 4 * LM * U * np.einsum("pik,kj->pij", np.abs(A[qs]), np.abs(X[n]))
        absY = np.abs(Y)
        per = (absY ** 2).sum(axis=1)                                # [products][LN]
        cost2[n] = per.sum(axis=0)
        bound[n] = ((2 * absY * e + e * e).sum(axis=1) + 4 * LM * U * per).sum(axis=0) + 4 * len(qs) * U * cost2[n]
    weight2 = (X.real ** 2 + X.imag ** 2).sum(axis=1)
    count = np.array([len(qs) for qs in lists], dtype=np.int64)
    return dict(cost2=cost2, weight2=weight2, bound=bound, bound_w=4 * LM * U * weight2, n_products=int(count.sum()),
                products_per_block=count)


def shrunk(pr, drop):
    """(rowPtrX, colIndX, oldBlock) of the pattern of X without the blocks `drop`, with Python lists"""
    off = pr.index_offset
    gone = set(int(d) for d in drop)
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX)).tolist()
    keep = [n for n in range(pr.nnzbX) if n not in gone]
    per_row = np.bincount([rows[n] for n in keep], minlength=pr.mb) if keep else np.zeros(pr.mb, np.int64)
    rowPtrX = np.concatenate([[0], np.cumsum(per_row)]) + off
    return rowPtrX.astype(np.int32), np.asarray(pr.colIndX)[keep].astype(np.int32), np.array(keep, dtype=np.int32)


def b_blocks(pr):
    """the positions in X (the caller's order) of the blocks that carry a block of B"""
    rowsX = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX)).tolist()
    rowsB = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrB)).tolist()
    where = {}
    for n, (r, c) in enumerate(zip(rowsX, np.asarray(pr.colIndX).tolist())):
        where.setdefault((r, c), n)
    return [where[(r, c)] for r, c in zip(rowsB, np.asarray(pr.colIndB).tolist())]
