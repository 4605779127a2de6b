"""numpy restatement of tfqmrgpuExt_selectDrop and tfqmrgpuExt_selectLeak (include/tfqmrgpu_ext.h section 20), for the tests.  The rules
work on records: cost2 [nnzbX][LN] (section 13), pos2 [nPos][LN] with the compressed block column of every position (section 12) and
bnorm2 [nCols][LN] (section 10) -- from the references drop_cost_ref.py, leak_map_ref.py and residual_ref.py in the CPU tests, from the
plan's own drop_cost(), leak_map() and residual() in the GPU tests, where the index lists must then agree entry for entry.

The arithmetic is the header's: eta * eta rounded once in double, its product with bnorm2 rounded once, no fused multiply-add (numpy has
none), and a comparison with a NaN is false.

spent and left are sums of non-negative doubles; the library adds them in another order.  Two orders of a sum of N non-negative terms
differ by at most (N - 1) u sum each side, u = 2^-53, so by less than N 2^-52 sum: `spent_bound`, `left_bound`, with N the blocks
(positions) of the column and the sum of the magnitudes the numpy sum itself.  The square roots are correctly rounded on either side."""
import numpy as np

from leak_ref import _patterns
from drop_cost_ref import b_blocks

EPS = 2.0 ** -52


def block_columns(pr):
    """the compressed block column of every block of X, the caller's order"""
    return _patterns(pr)[3]


def _limit(eta, bnorm2, cols):
    eta2 = np.float64(eta) * np.float64(eta)                         # rounded once
    return eta2 * np.asarray(bnorm2, dtype=np.float64)[cols]         # rounded once, per (item, right-hand side)


def _column_sums(n_cols, LN, cols, values):
    out = np.zeros((n_cols, LN))
    np.add.at(out, cols, values)
    return out


def select_drop(cost2, bnorm2, cols, carries_b, eta):
    """cols [nnzbX]: the compressed block column of every block; carries_b: the blocks that carry a block of B.  dict of blocks (int32,
    ascending), spent and spent_bound [nCols][LN], eligible (blocks without B)"""
    cost2, cols = np.asarray(cost2, dtype=np.float64), np.asarray(cols, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.all(cost2 <= _limit(eta, bnorm2, cols), axis=1)      # a NaN on either side: False
    ok[np.asarray(carries_b, dtype=np.int64)] = False
    blocks = np.flatnonzero(ok)
    n_cols, LN = np.asarray(bnorm2).shape
    spent = _column_sums(n_cols, LN, cols[blocks], np.sqrt(cost2[blocks]))
    per_col = np.bincount(cols, minlength=n_cols).astype(np.float64)
    return dict(blocks=blocks.astype(np.int32), spent=spent, spent_bound=per_col[:, None] * EPS * spent,
                eligible=len(cols) - len(set(np.asarray(carries_b).tolist())))


def select_leak(pos2, bnorm2, cols, eta):
    """cols [nPos]: the compressed block column of every leak position.  dict of take (uint64, ascending), left and left_bound
    [nCols][LN]"""
    pos2, cols = np.asarray(pos2, dtype=np.float64), np.asarray(cols, dtype=np.int64)
    n_cols, LN = np.asarray(bnorm2).shape
    pos2 = pos2.reshape(len(cols), LN)
    b = np.asarray(bnorm2, dtype=np.float64)[cols]
    with np.errstate(invalid="ignore"):
        hit = np.any((b > 0) & (pos2 > _limit(eta, bnorm2, cols)), axis=1)
    stay = np.flatnonzero(~hit)
    left = _column_sums(n_cols, LN, cols[stay], pos2[stay])
    per_col = np.bincount(cols, minlength=n_cols).astype(np.float64)
    with np.errstate(invalid="ignore"):
        bound = per_col[:, None] * EPS * _column_sums(n_cols, LN, cols[stay], np.abs(pos2[stay]))
    return dict(take=np.flatnonzero(hit).astype(np.uint64), left=left, left_bound=bound)


def mixed_eta(cost2, bnorm2, cols, carries_b, lo=0.1, hi=0.9):
    """an eta at which select_drop takes between lo and hi of the eligible blocks: the median over the eligible blocks of the smallest
    eta that lets the block go, max over j of sqrt(cost2 / bnorm2), nudged up so that the median block itself passes.  None if there is
    no such eta (every block needs the same one, say)"""
    cost2, cols = np.asarray(cost2, dtype=np.float64), np.asarray(cols, dtype=np.int64)
    b = np.asarray(bnorm2, dtype=np.float64)[cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        need = np.sqrt(np.nanmax(np.where(b > 0, cost2 / b, np.where(cost2 > 0, np.inf, 0.0)), axis=1))
    free = np.setdiff1d(np.arange(len(cols)), np.asarray(carries_b, dtype=np.int64))
    for q in (0.5, 0.3, 0.7, 0.2, 0.8):
        eta = float(np.quantile(need[free], q)) * (1 + 1e-9)
        if not np.isfinite(eta):
            continue
        share = len(select_drop(cost2, bnorm2, cols, carries_b, eta)["blocks"]) / max(1, len(free))
        if lo <= share <= hi:
            return eta
    return None


def mixed_eta_leak(pos2, bnorm2, cols, lo=0.1, hi=0.9):
    """the same for select_leak: an eta at which between lo and hi of the positions are taken"""
    pos2, cols = np.asarray(pos2, dtype=np.float64), np.asarray(cols, dtype=np.int64)
    b = np.asarray(bnorm2, dtype=np.float64)[cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        reach = np.sqrt(np.nanmax(np.where(b > 0, pos2.reshape(b.shape) / b, 0.0), axis=1))   # taken for every eta below this
    for q in (0.5, 0.3, 0.7, 0.2, 0.8):
        eta = float(np.quantile(reach, q))
        share = len(select_leak(pos2, bnorm2, cols, eta)["take"]) / max(1, len(cols))
        if lo <= share <= hi:
            return eta
    return None


__all__ = ["b_blocks", "block_columns", "select_drop", "select_leak", "mixed_eta", "mixed_eta_leak", "EPS"]
