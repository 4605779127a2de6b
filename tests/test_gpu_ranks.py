"""Multi-rank path of the PRODUCT on the GPU box: 2 and 3 ranks share cuda:0, block columns sharded with
tfqmrgpuExt_shardColumns, stopping test max-reduced over ranks through the host callback (gloo).  The sharded run
must take the iterations of the single-rank run and return bit-identical solution blocks:
columns are independent systems, the default shadow vector is a hash of (column, row, element), every reduction is
in a fixed order.  At most 4 processes touch the GPU.  Run with `pytest -m gpu`."""
import numpy as np
import pytest

import tfqmrgpu_amd as T
from _env_worker import problem
from helpers import run_ranks
from plan_paths import FOLD_MAX, plan_paths

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,name,prec,tol", [(2, "fd_16x16_small", "z", 1e-9), (3, "stencil_8x8", "z", 1e-9),
                                                 (2, "fd_16x16_2d", "c", 1e-4),
                                                 (2, "fd_16x16_2d", "m", 1e-9),     # mixed precision: the refinement's residual rides the same max-reduction
                                                 # 8 x 64 z, a dense column of 300 chunks (5 segments) and one of 29: one rank alone has 329 chunks
                                                 # (<= 384, the folding size), each of two ranks runs unfolded -- the long column is summed in the
                                                 # same order either way
                                                 (2, "stencil:20:15:8:64:2:5:5:-,3", "z", 1e-9)])
def test_ranks_sharing_one_gpu(tmp_path, world, name, prec, tol):
    g = run_ranks(world, "solve", str(tmp_path / "sharded.npz"), name, prec, tol, timeout=600)
    pr = problem(name)
    if name.startswith("stencil:"):
        ch, seg, folds = plan_paths(pr, prec)
        assert ch == [300, 29] and seg == [5, 1] and sum(ch) <= FOLD_MAX and not folds
    with T.Solver() as s:                       # single rank, same settings
        s.create_plan(pr)
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, prec))
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        st = s.solve(tol, 300)
        info, X, hist = s.get_info(), s.get_matrix(), s.bound_history()
    assert st == 0 and list(g["status"]) == [0] * world
    assert list(g["iterations"]) == [info["iterations"]] * world      # same decisions on every rank
    assert sum(g["n_cols"]) == len(np.unique(pr.colIndX)) and min(g["n_cols"]) >= 1
    for h in g["history"]:                                            # the reduced bound is the global one
        assert np.array_equal(h, hist)
    assert max(g["residual"]) == info["residual"]
    assert np.array_equal(g["X"], X)                                  # bit-identical solution blocks
    assert min(g["calls"]) >= info["iterations"]


def test_a_failing_rank_stops_every_rank(tmp_path):
    """a rank whose operator fails completes its slot with the failure marked in the reduced record: every rank stops at that
    slot and returns an error, none waits in an all-reduce for ever (the reduction carries {bound, alive, a rank failed})"""
    g = run_ranks(2, "fail_operator", str(tmp_path / "status.npz"), "fd_16x16_small", 1, 5, timeout=300)    # a hang would end here
    assert len(g["status"]) == 2
    (st0, st1), (calls0, calls1) = g["status"].tolist(), g["operator_calls"].tolist()      # by rank
    assert T.decode(st1)[0] == 14                       # the failing rank returns its operator's status
    assert st0 != 0 and T.decode(st0)[0] == 2           # the other one: stopped by a peer (LAUNCH_FAILED class)
    assert calls1 in (5, 6) and calls0 in (5, 6)        # both stopped in the slot of the failure (2 operator calls per iteration), far from the 300 iterations asked for


@pytest.mark.parametrize("how", ["nobuffer", "operator"])
def test_a_refusing_rank_ends_a_mixed_precision_solve_on_every_rank(tmp_path, how):
    """'m' plans: a rank that cannot start -- no work buffer, or a user-defined operator, which mixed-precision plans refuse --
    takes part in the FIRST collective its peers enter, the refinement's max-reduction of 3 doubles, with "a rank failed" set; every rank
    leaves there: same number and sizes of reductions on both ranks, the refusing rank returns its own status (7 | 19), the other one 2."""
    g = run_ranks(2, "refuse_mixed", str(tmp_path / "status.npz"), "fd_16x16_small", 1, how, timeout=300)    # a hang would end here
    assert len(g["status"]) == 2
    (st0, st1), (n0, n1), (sz0, sz1) = g["status"].tolist(), g["calls"].tolist(), g["sizes"].tolist()      # by rank; sizes: "n,n,..."
    assert T.decode(st1)[0] == (7 if how == "nobuffer" else 19)           # the refusing rank: its own status
    assert st0 != 0 and T.decode(st0)[0] == 2                             # its peer: stopped by a rank's failure
    assert n0 == n1 == 1 and sz0 == sz1 == "3"                            # ONE collective, the same on both: the refinement's {res^2, not finite, a rank failed}
