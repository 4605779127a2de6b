"""numpy restatements for the energy mesh (include/tfqmrgpu_ext.h section 19), for the tests: the diagonal blocks that a caller would send
through set_blocks('A') instead of shift_diagonal, and the weighted sum in real arithmetic, operation for operation.  They use neither the
library's code nor its lists."""
import numpy as np

import tfqmrgpu_amd as T
from helpers import diagonal_blocks  # noqa: F401  (the tests reach it as mesh_ref.diagonal_blocks)


def shifted_diagonal_blocks(A, diag, prec, sigma):
    """A[diag] + sigma * 1, formed in the storage precision: float32 for 'c' (sigma rounded to float once), double for 'z' and 'm', per
    component.  Only the diagonal elements are touched, the others keep their bits; complex64 for 'c', complex128 otherwise"""
    sigma = complex(sigma)
    real = np.float32 if prec == "c" else np.float64
    blocks = np.asarray(A)[diag].astype(np.complex64 if prec == "c" else np.complex128)
    k = np.arange(blocks.shape[1])
    d = blocks[:, k, k]
    new = np.empty_like(d)
    new.real = d.real + real(sigma.real)
    new.imag = d.imag + real(sigma.imag)
    assert new.real.dtype == real
    blocks[:, k, k] = new
    return blocks


def weighted_sum(terms, shape):
    """S = sum w * X over terms [(w, X complex blocks)], every product and every sum rounded once to double, in the order of section 19b"""
    re, im = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    for w, X in terms:
        w = complex(w)
        wr, wi = np.float64(w.real), np.float64(w.imag)
        xr, xi = np.asarray(X.real, dtype=np.float64), np.asarray(X.imag, dtype=np.float64)
        t1 = wr * xr
        t2 = wi * xi
        re = re + (t1 - t2)
        t3 = wr * xi
        t4 = wi * xr
        im = im + (t3 + t4)
    out = np.empty(shape, np.complex128)
    out.real, out.imag = re, im
    return out


def no_diagonal_problem(LM=4, LN=5):
    """three block rows; A has the blocks (0,0), (0,1), (1,0), (1,2), (2,2): block row 1 has no diagonal block"""
    rng = np.random.default_rng(3)
    rpA, ciA = [0, 2, 4, 5], [0, 1, 0, 2, 2]
    A = rng.standard_normal((5, LM, LM)) + 1j * rng.standard_normal((5, LM, LM)) + 4 * np.eye(LM)
    B = rng.standard_normal((1, LM, LN)) + 1j * rng.standard_normal((1, LM, LN))
    return T.Problem(rpA, ciA, A, [0, 1, 2, 3], [0, 0, 0], [0, 1, 1, 1], [0], B)
