"""Block-Jacobi right preconditioner (include/tfqmrgpu_ext.h section 7) without a GPU: the interface is declared and exported, and
the numpy restatement of the transformation (tests/precond_ref.py), solved by the CPU oracle, needs the iterations that the
issue's table states and returns a solution of the ORIGINAL system."""
import os
import re
import subprocess

import numpy as np
import pytest

import precond_ref as PC
import tfqmrgpu_amd as T
from conftest import ROOT, load_problem
from tfqmrgpu_amd import problems as PR


def test_header_declares_and_library_exports_the_interface():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    assert re.search(r"enum\s*\{\s*TFQMRGPU_PRECOND_NONE\s*=\s*0\s*,\s*TFQMRGPU_PRECOND_BLOCK_JACOBI\s*=\s*1\s*\}", text)
    assert re.search(r"tfqmrgpuStatus_t\s+tfqmrgpuExt_setPreconditioner\s*\(\s*tfqmrgpuBsrsvPlan_t\s+plan\s*,\s*int\s+kind\s*\)\s*;", text)
    assert re.search(r"tfqmrgpuStatus_t\s+tfqmrgpuExt_getPreconditioner\s*\(\s*tfqmrgpuHandle_t\s+\w*\s*,\s*tfqmrgpuBsrsvPlan_t\s+plan\s*,"
                     r"\s*void\s*\*\s*Minv[^;]*int32_t\s*\*\s*nIdentity\s*\)\s*;", text)
    out = subprocess.check_output(["nm", "-D", "--defined-only", T.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in ("tfqmrgpuExt_setPreconditioner", "tfqmrgpuExt_getPreconditioner"):
        assert name in exported and name in T.EXT_SYMBOLS
    assert (T.PRECOND_NONE, T.PRECOND_BLOCK_JACOBI) == (0, 1)
    assert "preconditioner" in T.solve_problem.__code__.co_varnames


# iterations of the oracle at threshold 1e-9, complex<double>, glibc shadow vector: plain, and with block Jacobi (M^-1 from numpy)
TABLE = [
    ("fd_16x16_2d", 13, 7), ("fd_16x16_small", 14, 7), ("fd_8x8_3d", 42, 27), ("fd_4x4_2d", 32, 21),
    ("stencil_10x10_16", 5, 4), ("stencil_12x12_8", 5, 5), ("dense_random", 12, 12),
]


def _problem(name):
    if name == "stencil_10x10_16":
        return PR.stencil_2d(10, 10, 16, 16, 3)
    if name == "stencil_12x12_8":
        return PR.stencil_2d(12, 12, 8, 8, 3)
    return load_problem(name)


@pytest.mark.parametrize("name,plain,jacobi", TABLE)
def test_oracle_iterations_with_and_without_block_jacobi(oracle, name, plain, jacobi):
    pr = _problem(name)
    tol = 1e-9
    st0, X0, info0 = oracle.solve(pr, "z", threshold=tol, max_iterations=2000)
    Minv, n_identity = PC.inverse_blocks(pr)
    st1, X1, info1 = PC.solve_with_oracle(oracle, pr, Minv, "z", threshold=tol, max_iterations=2000)
    assert st0 == st1 == 0 and n_identity == 0
    assert (info0["iterations"], info1["iterations"]) == (plain, jacobi)
    # right preconditioning leaves the residual what it is: the back-transformed X solves the caller's system
    assert PC.worst_relative_residual(oracle, pr, X1) <= tol
    assert PC.worst_relative_residual(oracle, pr, X0) <= tol
    assert np.abs(X1 - X0).max() <= 1e-8 * np.abs(X0).max()          # both stop at 1e-9


def test_rows_without_a_diagonal_block_get_the_unit_matrix(oracle):
    pr = PR.stencil_2d(5, 4, 8, 8, 2, seed=9)
    rows = PC.block_rows(pr.rowPtrA)
    keep = ~((rows == pr.colIndA) & (rows == 3))                    # drop the diagonal block of block row 3 from the pattern
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=pr.mb))])
    cut = T.Problem(rp, pr.colIndA[keep], pr.A[keep], pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B, None, 1e-9)
    assert PC.diagonal_blocks(cut)[3] == -1 and np.all(np.delete(PC.diagonal_blocks(cut), 3) >= 0)
    Minv, n_identity = PC.inverse_blocks(cut)
    assert n_identity == 1 and np.array_equal(Minv[3], np.eye(8))
    As = PC.scaled_A(cut, Minv)
    q = int(np.flatnonzero(cut.colIndA == 3)[0])
    assert np.array_equal(As[q], cut.A[q])                           # block column 3 is multiplied by 1
    Y = np.ones((cut.nnzbX, 8, 8), dtype=np.complex128)
    X = PC.back_transform(cut, Y, Minv)
    u = int(np.flatnonzero(PC.block_rows(cut.rowPtrX) == 3)[0])
    assert np.array_equal(X[u], Y[u])
