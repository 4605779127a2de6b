"""One copy of what the test files share: small helpers around problems, patterns and arrays, the comparison pieces that several files
use, the launcher of the multi-rank worker, and the `torch_cuda` fixture, which a test file imports by name.  A plan is opened with tfqmrgpu_amd.Solver.open.
Not a conftest, like plan_paths.py: pytest does not rewrite the asserts here, so each one that can fail on a result carries its message."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import tfqmrgpu_amd as T
import project_ref as P
from conftest import GOLDEN, ROOT, offset1, torchrun
from tfqmrgpu_amd import problems as PR

Z_BOUND = {1: 7e-14, 2: 2e-10}     # work vectors after k iterations against the oracle (tests/test_gpu_hash_mode.py: Z_STATE)
C_BOUND = {1: 1e-4}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    return torch


# ---- several ranks ------------------------------------------------------------------------------------------------------------------------
def run_ranks(world, scenario, out, *args, timeout):
    """tests/rank_worker.py <scenario> <out> <args> on `world` ranks (gloo; the scenarios of the product share cuda:0) in a fresh child:
    what rank 0 wrote to `out`.  A rank that hangs ends the child, and the test, at `timeout` seconds"""
    env = dict(os.environ, OMP_NUM_THREADS="2" if world < 4 else "1", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = torchrun(world) + [os.path.join(ROOT, "tests", "rank_worker.py"), scenario, out] + [str(a) for a in args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


# ---- arrays ------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_typed_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and same_bits(a, b)


def real_dtype(prec):
    return np.float32 if prec == "c" else np.float64


def exact_random_blocks(rng, n, rows, cols, prec):
    """complex blocks that the precision `prec` holds exactly"""
    v = rng.standard_normal((n, rows, cols)) + 1j * rng.standard_normal((n, rows, cols))
    return v.astype(np.complex64).astype(np.complex128) if prec == "c" else v


def user_array(blocks, layout, trans):
    """what a caller hands over for complex blocks [n, R, C] in that layout and transposition"""
    m = {"n": blocks, "t": blocks.transpose(0, 2, 1), "*": blocks.conj(), "c": blocks.conj().transpose(0, 2, 1)}[trans]
    if layout == T.LAYOUT_RIRIRIRI:
        return np.stack([m.real, m.imag], axis=-1).reshape(len(m), -1)
    if layout == T.LAYOUT_RRRRIIII:
        return np.stack([m.real, m.imag], axis=1).reshape(len(m), -1)
    return np.stack([m.real, m.imag], axis=2).reshape(len(m), -1)  # RRIIRRII


def ptr(a):
    """the address of a host array, also of one without entries"""
    return C.c_void_p(a.ctypes.data)


# ---- problems ----------------------------------------------------------------------------------------------------------------------------
def random_x(pr, seed):
    shape = (pr.nnzbX, pr.LM, pr.LN)
    return PR.hashed_uniform(seed, shape) - 0.5 + 1j * (PR.hashed_uniform(seed + 1, shape) - 0.5)


def diagonal_blocks(pr):
    """positions (the caller's block order of A) of the blocks whose block row equals their block column"""
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    return np.flatnonzero(rows == np.asarray(pr.colIndA, dtype=np.int64) - pr.index_offset)


def with_a(pr, A):
    return T.Problem(pr.rowPtrA, pr.colIndA, A, pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B, None, pr.tolerance, pr.index_offset)


def stencil(LM=4, LN=5, one_based=False):
    """one full block column and two truncated ones: the problem of the pattern tests that run without a GPU"""
    pr = PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN, radius=[None, 1.1, 2.3])
    return offset1(pr) if one_based else pr


def index_problem(rpA, ciA, rpX, ciX, rpB, ciB):
    """index arrays only: the plan never looks at a value"""
    return T.Problem(rpA, ciA, np.zeros((len(ciA), 1, 1)), rpX, ciX, rpB, ciB, np.zeros((len(ciB), 1, 1)))


def first_blocks(mb, rpX, ciX):
    """B: the first block of every block column of X, as (rowPtrB, colIndB)"""
    rows = np.repeat(np.arange(mb), np.diff(rpX))
    first = np.sort(np.unique(ciX, return_index=True)[1])
    return np.concatenate([[0], np.cumsum(np.bincount(rows[first], minlength=mb))]), np.asarray(ciX)[first]


def unordered_pattern():
    """An unsorted pattern from the reference's multiplication plan file ("#nnzb_for_Y_A_X= nY nA nX", then iY iA iX beta; despite its
    name the file lists every iY group in ascending order): A has a block (iY, iX) for every line, the odd block rows in the file's order
    reversed (columns descending); X has five block columns, column c missing in the rows with (row + c) % 3 == 0, and the blocks of a
    row start at column row % 5 and wrap around."""
    with gzip.open(os.path.join(GOLDEN, "plan_unordered.14-287-16.gz"), "rt") as f:
        mb = int(f.readline().split()[1])
        lines = np.loadtxt(f, dtype=np.int64)
    rpA = np.concatenate([[0], np.cumsum(np.bincount(lines[:, 0], minlength=mb))])
    ciA = np.concatenate([lines[rpA[r]:rpA[r + 1], 2][::-1 if r % 2 else 1] for r in range(mb)])
    rpX, ciX = [0], []
    for r in range(mb):
        ciX += [c for c in ((r + k) % 5 for k in range(5)) if (r + c) % 3]
        rpX.append(len(ciX))
    return index_problem(rpA, ciA, rpX, ciX, *first_blocks(mb, np.array(rpX), ciX))


# ---- yardsticks --------------------------------------------------------------------------------------------------------------------------
def deviations(pr, ref, got, X, starts, prec):
    """start projection: (gamma deviation, its bound, X deviation, its bound) per right-hand side | element, against project_ref"""
    tol = P.gamma_tolerance(ref, prec)                                   # [nCols, LN], relative to the largest |gamma_i|
    gmax = np.abs(ref["gamma"]).max(axis=-1)
    dg = np.abs(got["coefficients"] - ref["gamma"]).max(axis=-1)
    col = ref["an"]["colindx"].astype(np.int64)
    reach = sum(np.abs(np.asarray(S)) for S in starts)                   # sum |S_i| per element
    bound_x = (tol * gmax)[col][:, None, :] * reach + P.EPS[prec] * np.abs(ref["X"]) + 1e-300
    return dg, tol * gmax + 1e-300, np.abs(X - ref["X"]), bound_x
