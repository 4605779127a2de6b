"""numpy restatement of tfqmrgpuExt_leakMap and tfqmrgpuExt_growPattern (include/tfqmrgpu_ext.h section 12), for the tests.  Like
tests/leak_ref.py it uses neither the library's listing nor the oracle's analysis: per block column the FULL-HEIGHT product A X is assembled
from the BSR patterns in complex128, and every block row outside the column's pattern that receives a product is one leak position.
Positions are ordered by (compressed block column, block row).

The a-priori bound is leak_ref's for ONE position.  The kernel and numpy sum products that are exact in double (float data) or rounded
once (double data) in double arithmetic and differ only in the order of the sums.  With u = 2^-53, for one element r = sum a x of the
position, a sum of n complex terms (n = LM x its products), the two values differ by at most
    e = 4 n u sum |a| |x|,
for |r|^2 that is 2 |r| e + e^2, and the sum of the N = LM squares of a column of the block adds 4 N u sum |r|^2:
    bound = sum over the LM rows (2 |r| e + e^2) + 4 LM u sum |r|^2.
Everything in the bound comes from the operands, nothing from the kernel's output."""
import numpy as np

from leak_ref import _patterns
from residual_ref import U, stored  # noqa: F401


def positions(pr):
    """the leak positions from Python sets: sorted list of (compressed block column, block row)"""
    rowsA, colsA, rowsX, colsX, _ = _patterns(pr)
    pattern = set(zip(rowsX.tolist(), colsX.tolist()))
    cols_of_row = {}
    for k, c in pattern:
        cols_of_row.setdefault(k, []).append(c)
    found = set()
    for i, k in zip(rowsA.tolist(), colsA.tolist()):
        for c in cols_of_row.get(k, ()):
            if (i, c) not in pattern:
                found.add((c, i))
    return sorted(found)


def leak_map(pr, A, X):
    """dict of rows, cols [nPos] (block row; compressed block column), pos2 and bound [nPos][LN], columns (the caller's block column
    indices of the compressed columns) and n_leak_blocks"""
    rowsA, colsA, rowsX, colsX, columns = _patterns(pr)
    A, X = np.asarray(A, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    LM, LN = pr.LM, pr.LN
    rows, cols, pos2, bound = [], [], [], []
    for c in range(len(columns)):
        x_of_row = np.full(pr.mb, -1, dtype=np.int64)
        mine = np.flatnonzero(colsX == c)
        x_of_row[rowsX[mine][::-1]] = mine[::-1]                     # of two blocks on one (row, column) the first counts
        hit = np.flatnonzero(x_of_row[colsA] >= 0)                   # A blocks (i, k) with an X block (k, c)
        Y = np.zeros((pr.mb, LM, LN), dtype=np.complex128)
        mag = np.zeros((pr.mb, LM, LN))
        products = np.zeros(pr.mb)
        xs = x_of_row[colsA[hit]]
        np.add.at(Y, rowsA[hit], np.einsum("pik,pkj->pij", A[hit], X[xs]))
        np.add.at(mag, rowsA[hit], np.einsum("pik,pkj->pij", np.abs(A[hit]), np.abs(X[xs])))
        np.add.at(products, rowsA[hit], 1.0)
        products[x_of_row >= 0] = 0                                  # the rows of the column's own pattern: section 10 has them
        for i in np.flatnonzero(products > 0):
            e = 4 * LM * products[i] * U * mag[i]
            absY = np.abs(Y[i])
            p2 = (absY ** 2).sum(axis=0)
            rows.append(i)
            cols.append(c)
            pos2.append(p2)
            bound.append((2 * absY * e + e * e).sum(axis=0) + 4 * LM * U * p2)
    n = len(rows)
    return dict(rows=np.array(rows, np.int32), cols=np.array(cols, np.int32), pos2=np.array(pos2).reshape(n, LN),
                bound=np.array(bound).reshape(n, LN), columns=columns, n_leak_blocks=n)


def pattern_set(pr, rowPtrX=None, colIndX=None):
    """the pattern of X as a list of (block row, the caller's block column index) in block order"""
    rowPtrX = pr.rowPtrX if rowPtrX is None else rowPtrX
    colIndX = pr.colIndX if colIndX is None else colIndX
    rows = np.repeat(np.arange(pr.mb), np.diff(rowPtrX))
    return list(zip(rows.tolist(), np.asarray(colIndX).tolist()))
