"""numpy restatement of tfqmrgpuExt_projectStart (include/tfqmrgpu_ext.h section 17), for the tests: the images W_i = A S_i of the kept
starts by the truncated product of tests/residual_ref.py, the Gram sums G_il = <W_i, W_l>, g_i = <W_i, B> and |B|^2 per (compressed block
column, right-hand side) in double, the Cholesky factorisation in the order of the starts with the header's pivot rule and constants, and
the combination X = sum gamma_i S_i.  The pivot ratios d_i / G_ii come back with the result: the tolerance of a comparison follows from
them (first-order perturbation of the normal equations), and tests/test_project_start_cpu.py checks on them that no input of the GPU
tests sits near the threshold, where the device and this file could disagree about WHICH starts are kept."""
import numpy as np

import residual_ref as RR
from precond_ref import _product, diagonal_blocks

PIVOT_DOUBLE = 2.0 ** -26        # TFQMRGPU_PROJECT_PIVOT_DOUBLE: 'z' and 'm' (double storage)
PIVOT_FLOAT = 2.0 ** -12         # TFQMRGPU_PROJECT_PIVOT_FLOAT: 'c'
EPS = {"z": 2.0 ** -53, "m": 2.0 ** -53, "c": 2.0 ** -24}


def pivot_min(precision):
    return PIVOT_FLOAT if precision == "c" else PIVOT_DOUBLE


def shifted(pr, sigma):
    """the blocks of A(sigma) = A + sigma * 1 on the diagonal blocks"""
    A = np.array(pr.A, dtype=np.complex128)
    diag = diagonal_blocks(pr)
    A[diag[diag >= 0]] += sigma * np.eye(pr.LM)
    return A


def _column_dot(an, pr, U, V):
    """<U, V> = sum conj(U) V per (compressed block column, right-hand side)"""
    out = np.zeros((an["nCols"], pr.LN), dtype=np.complex128)
    np.add.at(out, an["colindx"].astype(np.int64), (np.conj(U) * V).sum(axis=1))
    return out


def project(oracle, pr, A, starts, B, precision):
    """starts: the k kept starts, newest first, complex [nnzbX, LM, LN] as get_matrix returns them; A, B as the plan stores them
    (residual_ref.stored).  Returns a dict: gamma [nCols, LN, k] complex, n_used [nCols, LN], ratio [nCols, LN, k] = d_i / G_ii (NaN where
    G_ii = 0), kept [nCols, LN, k] bool, X [nnzbX, LM, LN] = the combination in complex128 (not rounded), bnorm2 [nCols, LN]"""
    an = oracle.analyse(pr)
    assert an["status"] == 0
    k = len(starts)
    col, sub = an["colindx"].astype(np.int64), an["subset"].astype(np.int64)
    S = [np.asarray(s, dtype=np.complex128) for s in starts]
    W = [RR.stored(_product(an, pr, A, s), precision) for s in S]          # the device keeps W_i in the storage type
    Bx = np.zeros((pr.nnzbX, pr.LM, pr.LN), dtype=np.complex128)
    Bx[sub] = B
    G = np.empty((k, k), dtype=object)
    for i in range(k):
        for l in range(i, k):
            G[i, l] = _column_dot(an, pr, W[i], W[l])
            G[l, i] = np.conj(G[i, l])
    g = [_column_dot(an, pr, W[i], Bx) for i in range(k)]
    b2 = _column_dot(an, pr, Bx, Bx).real
    shape = b2.shape
    thr = pivot_min(precision)
    L = [[np.zeros(shape, complex) for _ in range(k)] for _ in range(k)]
    inv = [np.zeros(shape) for _ in range(k)]
    kept = np.zeros(shape + (k,), bool)
    ratio = np.full(shape + (k,), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(k):
            gii = G[i, i].real
            d = gii.copy()
            for l in range(i):
                x = G[i, l].copy()
                for m in range(l):
                    x -= L[i][m] * np.conj(L[l][m])
                L[i][l] = x * inv[l]
                d -= np.abs(L[i][l]) ** 2
            kept[..., i] = d > gii * thr
            ratio[..., i] = d / gii
            inv[i] = np.where(kept[..., i], 1.0 / np.sqrt(np.where(kept[..., i], d, 1.0)), 0.0)
    y = [None] * k
    for i in range(k):
        x = g[i].copy()
        for l in range(i):
            x -= L[i][l] * y[l]
        y[i] = x * inv[i]
    gam = [None] * k
    for i in range(k - 1, -1, -1):
        x = y[i].copy()
        for l in range(i + 1, k):
            x -= np.conj(L[l][i]) * gam[l]
        gam[i] = x * inv[i]
    gamma = np.stack(gam, axis=-1)
    zero_b = ~(b2 > 0)
    gamma[zero_b] = 0
    gamma[~kept] = 0
    n_used = np.where(zero_b, 0, kept.sum(axis=-1)).astype(np.int32)
    X = np.zeros((pr.nnzbX, pr.LM, pr.LN), dtype=np.complex128)
    for i in range(k):
        X += gamma[col, :, i][:, None, :] * S[i]
    return dict(gamma=gamma, n_used=n_used, ratio=ratio, kept=kept, X=X, bnorm2=b2, an=an)


def gamma_tolerance(ref, precision):
    """[nCols, LN]: what gamma of a right-hand side may deviate by, relative to its largest |gamma_i|: 100 * eps_storage / rho, rho the
    smallest pivot ratio of a kept start -- the first-order perturbation bound of the normal equations.  1 / rho is used as the condition
    estimate of the Gram matrix scaled to a unit diagonal; its entries carry the rounding of W in the storage type, eps_storage."""
    rho = np.where(ref["kept"], ref["ratio"], np.inf).min(axis=-1)
    return 100.0 * EPS[precision] / rho


# ---- the inputs of the GPU tests (tests/test_gpu_project_start.py), checked on the CPU by tests/test_project_start_cpu.py ----------------
# The family A(sigma) = A + sigma * 1 on the diagonal blocks.  Shifts far from the spectrum give solutions that are all nearly parallel to
# B / (diagonal + sigma): their pivot ratios fall between 1e-6 and 1e-2, inside the factor 100 around the float threshold.  The sets below
# sit where the shifted diagonal is comparable to the off-diagonal blocks, sigma = -centre * (mean diagonal element) + scale * base, so that
# the solutions differ in shape and every pivot ratio stays above 2e-2.
FIXTURES = ["fd_4x4_2d", "fd_16x16_small", "fd_8x8_3d", "stencil_8x32", "dense_random_rect"]
_SQUARE = (1 + 1j, -1 + 1j, -1 - 1j, 1 - 1j)
SHIFT_SETS = {   # name: (centre, scale, base); the first three are solved and pushed, the fourth is projected onto
    # (float solves of this fixture stall near its resonance and at sigma = 0; these four were searched on the CPU among the shifts at which
    #  a float solve reaches 1e-5 within 40 iterations)
    "fd_4x4_2d": (0.0, 1.0, (-8 - 2j, -8 + 3j, 4 - 1j, -6 + 3j)),
    "fd_8x8_3d": (0.0, 1.0, (-10.5 + 4j, -3 - 2j, -12 - 3j, -7.5 + 4j)),      # (searched in the same way)
    "fd_16x16_small": (1.0, 4.0, _SQUARE),
    "dense_random_rect": (1.0, 4.0, _SQUARE),
    "stencil_8x32": (1.0, 0.15, _SQUARE),
}
# depth 4 on stencil_8x32: the four corners are solved and pushed, the centre is projected onto
FIFTH = 0


def mean_diagonal(pr):
    diag = diagonal_blocks(pr)
    return float(np.mean([np.trace(pr.A[q]).real / pr.LM for q in diag[diag >= 0]]))


def shifts(pr, name, fifth=False):
    centre, scale, base = SHIFT_SETS[name]
    base = tuple(base) + ((FIFTH,) if fifth else ())
    return [complex(-centre * mean_diagonal(pr) + scale * b) for b in base]
