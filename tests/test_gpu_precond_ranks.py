"""The block-Jacobi right preconditioner (include/tfqmrgpu_ext.h section 7) on several ranks: 1, 2 and 3 ranks share cuda:0, block
columns sharded with tfqmrgpuExt_shardColumns, every rank inverts the diagonal blocks of the whole A itself and back-transforms its
own block columns.  The solution blocks must be bit-identical whatever the number of ranks, the iterations equal, and equal to those
of a plain single-process solve with the preconditioner.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import tfqmrgpu_amd as T
from _env_worker import problem
from helpers import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,prec,tol", [("fd_16x16_small", "z", 1e-9), ("fd_16x16_2d", "m", 1e-9)])
def test_block_jacobi_on_ranks_sharing_one_gpu(tmp_path, name, prec, tol):
    pr = problem(name)
    runs = {}
    for world in (1, 2, 3):
        runs[world] = run_ranks(world, "solve", str(tmp_path / ("sharded%d.npz" % world)), name, prec, tol, "jacobi", timeout=600)
    st, X, info = T.solve_problem(pr, prec, threshold=tol, max_iterations=300, preconditioner=T.PRECOND_BLOCK_JACOBI)
    assert st == 0
    for world, g in runs.items():
        assert list(g["status"]) == [0] * world and list(g["n_identity"]) == [0] * world
        assert list(g["iterations"]) == [info["iterations"]] * world
        assert max(g["residual"]) == info["residual"]
        for h in g["history"]:
            assert np.array_equal(h, info["bound_history"])
        for m in g["Minv"]:                                           # every rank holds all of A: the same M^-1 everywhere
            assert np.array_equal(m, g["Minv"][0]) and np.array_equal(m, runs[1]["Minv"][0])
        assert np.array_equal(g["X"], X)                              # bit-identical solution blocks
