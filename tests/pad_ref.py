"""numpy restatement of the padded plans (include/tfqmrgpu_ext.h section 18), for the tests: the shape rule of bufferSize, and the padded
problem that a plan of the PLAN's shape is fed through the calls that existed before -- the yardstick of tests/test_gpu_padding.py.  It uses
neither the library's code nor its lists."""
import numpy as np

import tfqmrgpu_amd as T

# the fifteen shapes of tfqmrgpu_bsrsv_allowedBlockSizes, written out
LISTED = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
          (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]


def plan_shape(lm, ln):
    """the listed (LM, LN) with LM >= lm and LN >= ln that has the smallest LM for which such an LN exists, then the smallest such LN;
    None: there is none"""
    fits = sorted((LM, LN) for LM, LN in LISTED if LM >= lm and LN >= ln)      # by LM first, then LN
    return fits[0] if fits else None


def diagonal_flags(pr):
    """True for the blocks of A whose block row equals their block column"""
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    return rows == (pr.colIndA.astype(np.int64) - pr.index_offset)


def pad_blocks(blocks, R, Cn, unit=None):
    """complex [n, r, c] -> [n, R, Cn]: zeros around, and 1 on the padded part of the diagonal of the blocks that `unit` flags"""
    n, r, c = blocks.shape
    out = np.zeros((n, R, Cn), dtype=blocks.dtype)
    out[:, :r, :c] = blocks
    if unit is not None:
        for k in range(min(r, c), min(R, Cn)):
            out[unit, k, k] = 1.0
    return out


def pad_problem(pr, LM, LN):
    """the problem of shape LM x LN whose solve IS the padded solve: every block zero-padded, ones on the padded diagonal of A's diagonal
    blocks.  X is padded too where `pr` carries one"""
    X = None if pr.X is None else pad_blocks(pr.X, LM, LN)
    return T.Problem(pr.rowPtrA, pr.colIndA, pad_blocks(pr.A, LM, LM, diagonal_flags(pr)), pr.rowPtrX, pr.colIndX,
                     pr.rowPtrB, pr.colIndB, pad_blocks(pr.B, LM, LN), X, pr.tolerance, pr.index_offset)


def inside(blocks, lm, ln):
    """the caller's part of padded blocks [n, LM, LN]"""
    return blocks[:, :lm, :ln]
