"""Shared by the GPU tests that pin one code path of the solver to the CPU oracle or to another path (tests/test_gpu_families.py,
tests/test_gpu_hash_mode.py, tests/test_gpu_ranks.py):

- a restatement of the plan's chunk rule (tfq_plan.cpp: chunks of CH blocks inside one block column) and of the segment rule of the
  column sums (tfq_plan.hpp: col_seg_len, col_segments), so that a fixture can assert that it reaches the path it stands for --
  a folded or an unfolded plan, a column summed by one work group or by several -- and fails loudly if the rules move it elsewhere;
- the work-vector comparison after k iterations against the oracle fed with the same shadow vector, and the a-priori rounding bound
  of the reported residual.
Not a conftest: nothing here is a fixture or a hook."""
import numpy as np

import tfqmrgpu_amd as T

FOLD_MAX = 384          # tfq_switch.hpp: kFoldMax, plans of at most this many chunks fold their column operations (if no column is segmented)
EPS = {"z": 2.0 ** -53, "c": 2.0 ** -24}


def col_seg_len(LN):
    return (256 // LN) * 16


def col_segments(n, LN):
    """work groups that sum a column of n chunk records (1: one work group, the column kernels' and the folded tails' sum alike)"""
    return 1 if n <= 4 * col_seg_len(LN) else -(-n // col_seg_len(LN))


def blocks_per_column(pr):
    cols = np.asarray(pr.colIndX, dtype=np.int64) - pr.index_offset
    return np.bincount(np.unique(cols, return_inverse=True)[1])


def chunks_per_column(pr, prec):
    """chunk records of each compressed block column of X (tfq_plan.cpp, the chunk table of createPlan)"""
    real = 8 if prec == "z" else 4
    block = 2 * pr.LM * pr.LN * real
    S = int(pr.nnzbX) * block
    CH = max(1, min(max(S // 4096, 8 * 1024), 16 * 1024) // block)
    if pr.LM % 16 == 0 and pr.LN % 16 == 0:       # a unit of work per wave of the MFMA multiply
        mt = pr.LM // 16
        ms = 2 if (mt % 2 == 0 and 2 * (pr.LN // 16) * real <= 32) else 1
        CH = max(CH, -(-4 // (mt // ms)))
    return [-(-int(n) // CH) for n in blocks_per_column(pr)]


def plan_paths(pr, prec, fold_max=FOLD_MAX):
    """(chunks per column, segments per column, whether a single-rank solve folds the column operations into the multiplies)"""
    ch = chunks_per_column(pr, prec)
    seg = [col_segments(n, pr.LN) for n in ch]
    return ch, seg, sum(ch) <= fold_max and max(seg) == 1


def gpu_state(pr, prec, k, three=False, v3=None, status=9):
    """(multiply kernel family, work vectors 1 and 4-9 after exactly k iterations, X)
    v3: a user shadow vector (float32 [nnzbX, 2, LM, LN]) in place of the default; status: what a solve of k iterations returns"""
    with T.Solver() as s:
        s.create_plan(pr)
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, prec))
        if v3 is not None:
            v3 = np.ascontiguousarray(v3, dtype=np.float32)
            assert T.lib.tfqmrgpuExt_setShadowVector(s.handle, s.plan, T._ptr(v3)) == 0
        if three:
            s.set_three_product_multiply(True)
        family = s.multiply_kernel()
        s.set_matrix("A", pr.A, "n")
        s.set_matrix("B", pr.B, "n")
        st = s.solve(1e-30, k)
        got = {w: s.get_work_vector(w) for w in (1, 4, 5, 6, 7, 8, 9)}
        X = s.get_matrix()
    assert st == status                                       # 9: out of iterations (tfqmrgpu_core.hxx:258)
    assert np.array_equal(got[1], X, equal_nan=v3 is not None)
    return family, got


def state_deviation(oracle, pr, prec, k, got, v3=None, status=9, failed=None):
    """max over the work vectors of max|gpu - oracle| / max|oracle| after k iterations
    failed (bool [nnzbX, LN]): right-hand sides that break down on purpose (tests/breakdown_cases.py).  The deviation is then taken
    over the others alone; on the failed ones the two must agree in what rounding cannot move: the NaN mask, and a zero of the oracle is a
    zero (asserted here, vector by vector)."""
    v3 = T.hash_shadow_vector(pr) if v3 is None else v3
    st0, X0, info0 = oracle.solve(pr, prec, threshold=1e-30, max_iterations=k, v3=np.asarray(v3).reshape(-1), dump_iteration=k)
    assert st0 == status
    worst = {}
    for w, want in info0["vectors"].items():
        if failed is not None:
            dead = np.broadcast_to(failed[:, None, :], want.shape)
            assert np.array_equal(np.isnan(got[w][dead]), np.isnan(want[dead])), (w, k)
            assert np.all(got[w][dead][want[dead] == 0] == 0), (w, k)
            if dead.all():
                continue
            got_w, want = got[w][~dead], want[~dead]
        else:
            got_w = got[w]
        scale = np.abs(want).max()
        assert scale > 0, w
        worst[w] = float(np.abs(got_w - want).max() / scale)
    return worst


def rounding_factor(n, prec):
    """sqrt(2) (n + 3) eps: what one element of A x - b, a complex sum of n rounded products and b, moves by in the plan's precision,
    relative to |A| |x| + |b| (true_residual below has the derivation); n may be an array"""
    return np.sqrt(2.0) * (n + 3) * EPS[prec]


def true_residual(pr, X, prec):
    """(max over right-hand sides of |A x - b| / |b| in float64 from the returned X, the a-priori rounding bound of the GPU's value of it)
    The GPU forms r = A x - b in the plan's precision: per element a complex sum of n = (block products of the row) x LM terms and b, each
    term rounded (complex products: sqrt(2) gamma_(n+2), Higham 3.6), plus the rounding of A and B to that precision.  So
    |r_gpu - r| <= sqrt(2) (n + 3) eps (|A| |x| + |b|) element by element, and by the triangle inequality the norm of each right-hand
    side's residual, relative to |b|, moves by at most the norm of that bound over |b|."""
    off = pr.index_offset
    rowsA = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    colsA = np.asarray(pr.colIndA, dtype=np.int64) - off
    rowsX = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))
    colsX = np.asarray(pr.colIndX, dtype=np.int64) - off
    rowsB = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrB))
    colsB = np.asarray(pr.colIndB, dtype=np.int64) - off
    ucols = np.unique(colsX)
    nc, LM, LN = len(ucols), pr.LM, pr.LN
    xd = np.zeros((pr.mb, nc, LM, LN), complex)
    xd[rowsX, np.searchsorted(ucols, colsX)] = np.asarray(X, complex)
    bd = np.zeros((pr.mb, nc, LM, LN), complex)
    bd[rowsB, np.searchsorted(ucols, colsB)] = pr.B
    has = np.zeros((pr.mb, nc), bool)
    has[rowsX, np.searchsorted(ucols, colsX)] = True
    Ax = np.zeros_like(xd)
    absAx = np.zeros(xd.shape)
    np.add.at(Ax, rowsA, np.einsum("kij,kcjl->kcil", pr.A, xd[colsA]))
    np.add.at(absAx, rowsA, np.einsum("kij,kcjl->kcil", np.abs(pr.A), np.abs(xd[colsA])))
    r = (Ax - bd) * has[:, :, None, None]                     # the residual lives on the pattern of X (tfqmrgpu_core.hxx:265-269)
    envelope = (absAx + np.abs(bd)) * has[:, :, None, None]
    bn = np.sqrt((np.abs(bd) ** 2).sum(axis=(0, 2)))          # [nc, LN]
    rn = np.sqrt((np.abs(r) ** 2).sum(axis=(0, 2))) / bn
    n = int(np.diff(pr.rowPtrA).max()) * LM
    bound = rounding_factor(n, prec) * np.sqrt((envelope ** 2).sum(axis=(0, 2))) / bn
    return float(rn.max()), float(bound.max())
