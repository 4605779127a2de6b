"""Multi-rank path on the CPU (gloo, world_size 2 and 3): block columns of X/B sharded with the
product's tfqmrgpuExt_shardColumns, stopping test max-reduced over ranks.  The sharded run must take
exactly the iterations of the single-rank run and return bit-identical solution blocks, because the
columns are independent systems and all ranks take the same continue/probe/stop decisions
(SURVEY.md section 8e)."""
import numpy as np
import pytest

from _env_worker import problem
from helpers import run_ranks


# (8 ranks on the pattern of BASELINE config 4 -- 16x16 complex<double> stencil, block columns split over the ranks, here 6 x 6 rows and
#  16 block columns = 2 per rank -- is the rank count of the driver's scaling run)
@pytest.mark.parametrize("world,name,tol", [(2, "fd_16x16_small", 1e-9), (3, "stencil_8x8", 1e-9), (2, "fd_4x4_2d", 1e-9), (8, "cfg4:6:16", 1e-9)])
def test_sharded_solve_equals_single_rank(oracle, tmp_path, world, name, tol):
    g = run_ranks(world, "oracle", str(tmp_path / "sharded.npz"), name, tol, timeout=600)
    pr = problem(name)
    st, X, info = oracle.solve(pr, "z", threshold=tol, max_iterations=300)
    assert st == 0
    assert list(g["status"]) == [0] * world
    assert list(g["iterations"]) == [info["iterations"]] * world      # same decisions on every rank
    assert sum(g["n_cols"]) == len(np.unique(pr.colIndX)) and min(g["n_cols"]) >= 1
    for h in g["history"]:                                            # the reduced bound is the global one
        assert np.array_equal(h, info["bound_history"])
    assert max(g["residual"]) == info["residual"]
    assert np.array_equal(g["X"], X)                                  # bit-identical solution blocks
    assert min(g["calls"]) >= info["iterations"]
