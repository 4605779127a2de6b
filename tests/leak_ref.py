"""numpy restatement of tfqmrgpuExt_truncationLeak (include/tfqmrgpu_ext.h section 11), for the tests.  It uses neither the library's
listing nor the oracle's analysis: per block column the FULL-HEIGHT product A X is assembled from the BSR patterns -- A's blocks
scattered by (i, k), X's by (k, c), complex128 --, the block rows inside the column's pattern are masked, and |.|^2 is summed per
(block column, right-hand side).  The counts come from Python sets.

The a-priori bound is built like tests/residual_ref.py's.  The kernel and numpy sum products that are exact in double (float data) or
rounded once (double data) in double arithmetic and differ only in the order of the sums.  With u = 2^-53, for one element r = sum a x of
a leak position, a sum of n complex terms (n = LM x its products), the two values differ by at most
    e = 4 n u sum |a| |x|,
for |r|^2 that is 2 |r| e + e^2, and the sum of the N squares of an entry (N = LM x leak positions of the column) adds 4 N u sum |r|^2:
    bound = sum (2 |r| e + e^2) + 4 N u sum |r|^2.
Everything in the bound comes from the operands, nothing from the kernel's output.  A column without leak positions has leak2 = bound = 0."""
import numpy as np

from residual_ref import U, stored  # noqa: F401  (stored: what a plan of a precision keeps of the caller's values)


def _patterns(pr):
    """zero-based (rowsA, colsA, rowsX, compressed colsX, the caller's index of each compressed column)"""
    off = pr.index_offset
    rowsA = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA)).astype(np.int64)
    colsA = np.asarray(pr.colIndA, dtype=np.int64) - off
    rowsX = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX)).astype(np.int64)
    columns, colsX = np.unique(np.asarray(pr.colIndX, dtype=np.int64), return_inverse=True)
    return rowsA, colsA, rowsX, colsX.astype(np.int64), columns.astype(np.int32)


def counts(pr):
    """(leak positions, block products that land on them), with Python sets: (i, c) outside the pattern of X that some A block (i, k)
    reaches from an X block (k, c)"""
    rowsA, colsA, rowsX, colsX, _ = _patterns(pr)
    pattern = set(zip(rowsX.tolist(), colsX.tolist()))
    cols_of_row = {}
    for k, c in sorted(pattern):
        cols_of_row.setdefault(k, []).append(c)
    positions, n_pairs = set(), 0
    for i, k in zip(rowsA.tolist(), colsA.tolist()):
        for c in cols_of_row.get(k, ()):
            if (i, c) not in pattern:
                positions.add((i, c))
                n_pairs += 1
    return len(positions), n_pairs


def leak(pr, A, X):
    """dict of leak2 and bound [nCols][LN], columns (the caller's block column indices), n_leak_blocks, n_leak_pairs, and
    blocks_per_column / pairs_per_column [nCols]"""
    rowsA, colsA, rowsX, colsX, columns = _patterns(pr)
    A, X = np.asarray(A, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    n_cols, LM, LN = len(columns), pr.LM, pr.LN
    leak2, bound = np.zeros((n_cols, LN)), np.zeros((n_cols, LN))
    blocks, pairs = np.zeros(n_cols, np.int64), np.zeros(n_cols, np.int64)
    for c in range(n_cols):
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
        inside = x_of_row >= 0
        Y[inside], mag[inside], products[inside] = 0, 0, 0           # the rows of the column's own pattern: section 10 has them
        e = 4 * (LM * products)[:, None, None] * U * mag
        absY = np.abs(Y)
        leak2[c] = (absY ** 2).sum(axis=(0, 1))
        blocks[c], pairs[c] = int((products > 0).sum()), int(products.sum())
        bound[c] = (2 * absY * e + e * e).sum(axis=(0, 1)) + 4 * LM * blocks[c] * U * leak2[c]
    return dict(leak2=leak2, bound=bound, columns=columns, n_leak_blocks=int(blocks.sum()), n_leak_pairs=int(pairs.sum()),
                blocks_per_column=blocks, pairs_per_column=pairs)


def padded(pr, X=None):
    """the twin of `pr` with full block columns: the same A and B, X's pattern = every block row in every block column of `pr`; returns
    (problem, X zero-padded onto it or None).  Its truncated residual is the untruncated residual of `pr`."""
    import tfqmrgpu_amd as T
    off = pr.index_offset
    _, _, rowsX, colsX, columns = _patterns(pr)
    n_cols = len(columns)
    rpX = np.arange(pr.mb + 1, dtype=np.int32) * n_cols + off
    ciX = np.tile(columns.astype(np.int32), pr.mb)
    twin = T.Problem(pr.rowPtrA, pr.colIndA, pr.A, rpX, ciX, pr.rowPtrB, pr.colIndB, pr.B, None, pr.tolerance, off)
    if X is None:
        return twin, None
    Xp = np.zeros((pr.mb * n_cols, pr.LM, pr.LN), dtype=np.complex128)
    Xp[(rowsX * n_cols + colsX)[::-1]] = np.asarray(X)[::-1]
    return twin, Xp
