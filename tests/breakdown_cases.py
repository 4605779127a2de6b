"""Fixtures in which single right-hand sides (RHS) break down while their neighbours converge, shared by tests/test_breakdown_cpu.py
(which proves on the CPU oracle that every fixture reaches the branch it stands for), tests/test_gpu_breakdown.py and
tests/_env_worker.py.  Not a conftest: nothing here is a pytest fixture or a hook.

Every fixture is a small ragged stencil (problems.stencil_2d: one block of B per block column, in the column's source row) and is
built with EXACT zeros, so that the branch is hit exactly and not nearly:

  zero_rhs    B[:, :, j*] = 0 in one column: |b| = 0, tau = 0 -> decT, status -3 (after dec35 and dec34 saw z = 0 half a step earlier)
  dec35       the shadow vector v3 is zero for RHS j* of one column in every block: z = v3.v5 = 0 -> dec35, status -1
  dec34       disjoint supports: b_j* and v3_j* live in block row r0 alone and A has no block (r0, r0), so v3.v5 != 0 but
              v3.(A v6) = 0 in the first iteration -> dec34, status -2 (and never -1)
  column      dec35 for every RHS of one column: the column's `alive` record is 0, the other column's 1, the solve goes on
  all         dec35 for every RHS of every column: the solve ends with TFQMRGPU_STATUS_BREAKDOWN in iteration 1
  plus_one    b_j* = one unit vector e whose column of A is e as well, and v3 = 1 at that element: alfa = -1, x = b and r = 0 without a
              rounding in iteration 1, so that the first probe finds res2 == 0 -> status +1

The failing RHS j* is neither the first nor the last and lies in the upper half of the column."""
import ctypes as C

import numpy as np

import tfqmrgpu_amd as T
from tfqmrgpu_amd import problems as PR

# The iteration cap is part of the fixtures.  A RHS that broke down in dec35 or dec34 keeps its v5 = b, so its tau falls as |b|^2 / (2 it + 1)
# and no faster: the residual bound of the stopping test (tfqmrgpu_core.hxx:239-252: (2 it + 1) x the maximum over ALL right-hand sides)
# stays at 1 and no probe is made before the last iteration: the solve runs to the cap, in the reference as in the oracle.  The healthy RHS converge within 6 (z: 16 next to `dec34`) |
# 4 (c: 10) iterations and, iterated on, break down themselves once their tau has underflowed: from iteration 56 (z) | 17 (c) on in the
# oracle.  The caps lie between the two, so that a healthy RHS ends converged AND with status 0 (tests/test_breakdown_cpu.py holds that).
MAX_ITERATIONS = {"z": 20, "c": 12, "m": 300}
THRESHOLD = {"z": 1e-9, "c": 1e-4, "m": 1e-9}
KINDS = ("zero_rhs", "dec35", "dec34", "column", "all", "plus_one")
FIRST = {"zero_rhs": -3, "dec35": -1, "dec34": -2, "column": -1, "all": -1, "plus_one": 1}   # the value the fixture stands for

# the smallest shapes at which each form of the column operations exists: (nx, ny, LM, LN, block columns, seed, radius)
SHAPES = {
    "4x8": (6, 5, 4, 8, 2, 61, 2.5),
    "8x8": (6, 5, 8, 8, 2, 62, 2.5),
    "8x32": (6, 5, 8, 32, 2, 63, 2.5),
    "16x16": (6, 5, 16, 16, 2, 64, 2.5),
    "8x64seg": (20, 15, 8, 64, 1, 5, None),      # stencil:20:15:8:64:1:5:5 of tests/test_gpu_hash_mode.py: one column of 300 chunks, 5 segments
    "8x64seg3": (20, 15, 8, 64, 3, 50, None),    # tests/test_gpu_families.py: three segmented columns (hosts `column`, which needs a second one)
}
FOLD_SHAPES = {"z": ("4x8", "8x8", "16x16"), "c": ("4x8", "8x32", "16x16")}


class Case:
    """pr, v3 (float32 [nnzbX, 2, LM, LN], the shadow vector of GPU and oracle alike), failed (bool [nCols, LN]: the planned failures),
    first (the status value they are first given, in iteration 1 -- `plus_one`: at the first probe), status (what the solve returns)"""

    def __init__(self, name, pr, v3, failed, first, status):
        self.name, self.pr, self.v3, self.failed, self.first, self.status = name, pr, v3, failed, first, status
        self.col_of_block = np.unique(np.asarray(pr.colIndX), return_inverse=True)[1]

    def failed_blocks(self):
        """bool [nnzbX, LN]: the planned failures per block of X"""
        return self.failed[self.col_of_block]


def row_ids(rows):
    """pytest ids of (kind, shape, precision) rows"""
    return ["%s-%s-%s" % r for r in rows]


def j_star(LN):
    return (5 * LN) // 8


def _x_rows(pr):
    return np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))


def _without_diagonal_block(pr, r0):
    """the problem without A's block (r0, r0); the row keeps its other blocks.  The stencil's rows are dominated by their diagonal
    block (2 x unit + small): without it row r0 holds small blocks alone, the system is ill conditioned and the healthy RHS of the other
    columns over-iterate into breakdowns of their own before this column has converged.  So the dominant part moves to the pair of blocks
    (r0, r1), (r1, r0) with the next block row r1 = r0 + 1: the 2 x 2 coupling [[0, 2], [2, 2]] has the eigenvalues 1 +- sqrt(5)."""
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    r1 = r0 + 1
    for a, b in ((r0, r1), (r1, r0)):
        q = np.nonzero((rows == a) & (pr.colIndA == b))[0]
        assert len(q) == 1
        pr.A[q[0]] += 2.0 * np.eye(pr.LM)
    keep = ~((rows == r0) & (pr.colIndA == r0))
    assert keep.sum() == pr.nnzbA - 1 and (rows[keep] == r0).any()
    rowPtr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=pr.mb))])
    return T.Problem(rowPtr, pr.colIndA[keep], pr.A[keep], pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B, None, pr.tolerance)


def case(kind, shape, column=None):
    """the fixture `kind` on SHAPES[shape]; the failures lie in block column `column` (default: the last)"""
    nx, ny, LM, LN, ncols, seed, radius = SHAPES[shape]
    pr = PR.stencil_2d(nx, ny, LM, LN, ncols, seed=seed, radius=radius)
    assert pr.index_offset == 0 and pr.nnzbB == ncols and list(pr.colIndB) == sorted(pr.colIndB)
    col = ncols - 1 if column is None else column
    js = j_star(LN)
    assert 0 < js < LN - 1 and 2 * js >= LN
    v3 = T.hash_shadow_vector(pr).copy()
    failed = np.zeros((ncols, LN), bool)
    in_col = np.asarray(pr.colIndX) == col                                     # blocks of X in the column
    b = int(np.nonzero(np.asarray(pr.colIndB) == col)[0][0])                   # the column's block of B ...
    r0 = int(np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrB))[b])              # ... and its block row
    at_r0 = in_col & (_x_rows(pr) == r0)
    assert at_r0.sum() == 1
    status = 0
    if kind == "zero_rhs":
        pr.B[b, :, js] = 0
        failed[col, js] = True
    elif kind == "dec35":
        v3[in_col, :, :, js] = 0
        failed[col, js] = True
    elif kind == "dec34":
        pr = _without_diagonal_block(pr, r0)
        v3[in_col & ~at_r0, :, :, js] = 0
        failed[col, js] = True
    elif kind == "column":
        assert ncols > 1
        v3[in_col] = 0
        failed[col] = True
    elif kind == "all":
        v3[:] = 0
        failed[:] = True
        status = 6
    elif kind == "plus_one":
        k = 1                                                                   # b_j* = unit vector k of block row r0
        rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
        into = np.asarray(pr.colIndA) == r0                                     # A's blocks that multiply block row r0 of x
        pr.A[into, :, k] = 0
        pr.A[into & (rows == r0), k, k] = 1
        pr.B[b, :, js] = 0
        pr.B[b, k, js] = 1
        v3[at_r0, 0, k, js], v3[at_r0, 1, k, js] = 1, 0                         # z = v3.b = 1: alfa = -rho / z = -1 exactly
        failed[col, js] = True
    else:
        raise ValueError(kind)
    return Case("%s:%s" % (kind, shape), pr, np.ascontiguousarray(v3, np.float32), failed, FIRST[kind], status)


def by_name(name):
    """`kind:shape[:column]`, the form in which tests/_env_worker.py is told a fixture"""
    f = name.split(":")
    return case(f[0], f[1], int(f[2]) if len(f) > 2 else None)


def gpu_solve(c, prec, reduce_callback=None, residual=False, max_iterations=None):
    """one solve of the fixture with its shadow vector: (status, X, info) as T.solve_problem, info["per_rhs"] = Solver.residual() on request"""
    pr = c.pr
    with T.Solver() as s:
        s.create_plan(pr)
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, prec))
        assert T.lib.tfqmrgpuExt_setShadowVector(s.handle, s.plan, c.v3.ctypes.data_as(C.c_void_p)) == 0
        s.set_matrix("A", pr.A, "n")
        s.set_matrix("B", pr.B, "n")
        if reduce_callback is not None:
            s.set_reduce_callback(reduce_callback)
        status = s.solve(THRESHOLD[prec], MAX_ITERATIONS[prec] if max_iterations is None else max_iterations)
        info = s.get_info()
        info["bound_history"] = s.bound_history()
        X = s.get_matrix()
        if residual:
            info["per_rhs"] = s.residual()
    return status, X, info


def oracle_solve(oracle, c, prec, **kw):
    return oracle.solve(c.pr, prec, threshold=THRESHOLD[prec], max_iterations=MAX_ITERATIONS[prec], v3=c.v3.reshape(-1), **kw)
