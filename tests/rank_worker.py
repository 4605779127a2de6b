"""One rank of a column-sharded run, launched by helpers.run_ranks through torch.distributed.run (gloo): rank_worker.py <scenario> <out>
<problem> [args...].  Every rank cuts its block columns out of the problem with the product's tfqmrgpuExt_shardColumns and max-reduces
the stopping test over the ranks through the host callback (Solver.set_reduce_callback), the same protocol and the same enqueue pattern
as the RCCL path, which needs one GPU per rank; here the ranks share cuda:0.  A scenario is a function below: it does its own steps on
the shard and returns what this rank reports.  Rank 0 gathers the reports and writes <out> (.npz): X assembled from the ranks' blocks,
the values under "per_column" concatenated in rank order, which is the order of the block columns, every other value once per rank."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tfqmrgpu_amd as T  # noqa: E402
from _env_worker import problem  # noqa: E402      a golden fixture, a `stencil:` or a `cfg4:` spec


def solve(r, prec, tol, option=""):
    """the sharded solve: plain, with the block-Jacobi right preconditioner (`jacobi`: every rank holds all of A and computes M^-1
    itself) or on a padded plan (`pad`)"""
    with T.Solver.open(r.sub, prec, preconditioner=T.PRECOND_BLOCK_JACOBI if option == "jacobi" else None,
                       allow_padding=option == "pad").load() as s:
        s.set_reduce_callback(r.reduce_max)
        st = s.solve(float(tol), 300)
        info = s.get_info()
        mine = dict(status=st, iterations=info["iterations"], residual=info["residual"], history=s.bound_history(), X=s.get_matrix())
        if option == "jacobi":
            mine["Minv"], mine["n_identity"] = s.get_preconditioner()
        if option == "pad":
            mine["shape"] = s.padded_shape()
    return mine


def project(r, prec, src):
    """the start projection: the starts and A come from the file `src`, every rank takes its own block columns of them.  The handle
    carries the reduce callback, as in a sharded solve: the projection is local to a rank and makes no collective"""
    given = np.load(src)
    with T.Solver.open(r.sub, prec, keep_starts=3) as s:
        s.set_reduce_callback(r.reduce_max)
        s.load(A=given["A"])
        for S in given["starts"][::-1]:                   # oldest first: the newest ends up in slot 0
            s.set_matrix("X", S[r.xb])
            s.push_start()
        got = s.project_start()
        return dict(X=s.get_matrix(), per_column=dict(gamma=got["coefficients"], used=got["n_used"]))


def fail_operator(r, bad_rank, bad_call):
    """every rank solves with a user-defined operator that repeats the built-in multiply; that of rank `bad_rank` fails in its call
    number `bad_call`.  Every rank must come back from tfqmrgpu_bsrsv_solve (none may wait in a reduction for ever) with a status"""
    from solve_helpers import builtin_as_operator
    calls = [0]
    with T.Solver.open(r.sub, "z").load() as s:
        builtin = builtin_as_operator(torch, s, r.sub, "z", s.plan_view(), [])

        def multiply(*args):
            calls[0] += 1
            if r.rank == int(bad_rank) and calls[0] == int(bad_call):
                raise RuntimeError("injected operator failure")      # the thunk turns it into status 14
            return builtin(*args)

        s.set_reduce_callback(r.reduce_max)
        s.set_operator(multiply)
        st = T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, 1e-9, 300)      # raw: Solver.solve raises on these statuses
    return dict(status=int(st), operator_calls=calls[0])


def refuse_mixed(r, bad_rank, how):
    """a mixed-precision ('m') plan on every rank; rank `bad_rank` refuses the solve in the way `how` says: `nobuffer` (no work buffer
    registered) or `operator` (a user-defined operator, which 'm' plans do not take).  Every rank must come back with a status and after
    the SAME reductions -- a refusing rank that entered another collective than its peers (the vote of the inner solve, 2 doubles,
    against the refinement's reduction, 3 doubles) would hang or corrupt them"""
    bad = r.rank == int(bad_rank)
    with T.Solver.open(r.sub, "m", buffer=False) as s:
        s.set_reduce_callback(r.reduce_max)               # a call on the handle: before a buffer exists
        if not (bad and how == "nobuffer"):
            s.set_buffer(nbytes=s.buffer_bytes)
            s.load()
        if bad and how == "operator":
            s.set_operator(lambda *a: 0.0)
        st = T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, 1e-9, 300)      # raw: Solver.solve raises on these statuses
    return dict(status=int(st))


def oracle_solve(r, tol):
    """the CPU oracle's tfQMR in place of the product, with this rank's slice of the GLOBAL shadow vector (results must not depend on
    the rank count) and the same reductions as the HIP solver: {max tau/|b|^2, any RHS alive} per iteration, {max res^2, any RHS
    open} per probe"""
    from oracle import pyoracle as O
    E = 2 * r.pr.LM * r.pr.LN
    v3 = O.shadow_glibc(r.pr.nnzbX * E).reshape(r.pr.nnzbX, E)[r.xb].reshape(-1)
    st, X, info = O.solve(r.sub, "z", threshold=float(tol), max_iterations=300, v3=v3, reduce=lambda ctx, values, n: r.reduce_max(values, n))
    return dict(status=st, iterations=info["iterations"], residual=info["residual"], history=info["bound_history"], X=X)


SCENARIOS = dict(solve=solve, project=project, fail_operator=fail_operator, refuse_mixed=refuse_mixed, oracle=oracle_solve)


def main():
    scenario, out, name, args = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    if scenario != "oracle":
        assert torch.cuda.is_available(), "no GPU: the product has no CPU fallback"
        torch.cuda.set_device(0)
    pr = problem(name)
    sub, xb, bb = T.shard_columns(pr, world, rank)
    sizes = []                                            # of every reduction this rank entered

    def reduce_max(values, n):
        sizes.append(int(n))
        t = torch.tensor([values[i] for i in range(n)] + [float(n)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)          # (a mismatch of the sizes between the ranks would fail or hang right here)
        for i in range(n):
            values[i] = float(t[i])

    mine = SCENARIOS[scenario](SimpleNamespace(rank=rank, pr=pr, sub=sub, xb=xb, reduce_max=reduce_max), *args)
    mine.update(xb=xb, n_cols=sub.n_cols, calls=len(sizes), sizes=",".join(str(n) for n in sizes))
    gathered = [None] * world
    dist.all_gather_object(gathered, mine)
    if rank == 0:
        res = {k: np.array([g[k] for g in gathered]) for k in mine if k not in ("X", "xb", "per_column")}
        if "X" in mine:
            res["X"] = np.zeros((pr.nnzbX, pr.LM, pr.LN), dtype=mine["X"].dtype)
            for g in gathered:
                res["X"][g["xb"]] = g["X"]
        for k in mine.get("per_column", {}):
            res[k] = np.concatenate([g["per_column"][k] for g in gathered])
        np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
