"""Worker of tests/test_gpu_project_start.py: one rank of the column-sharded start projection on cuda:0.  The starts come from argv[1]
(written by the test), every rank takes its own block columns of them; the handle carries a reduce callback, as in a sharded solve, and
the worker counts its calls: the projection is local to a rank and makes no collective.  Rank 0 gathers gamma and X and writes argv[2]."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    src, out, name, prec = sys.argv[1:5]
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert torch.cuda.is_available(), "no GPU: the product has no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from _env_worker import problem      # a golden fixture or a `stencil:` spec
    pr = problem(name)
    given = np.load(src)
    sub, xb, bb = T.shard_columns(pr, world, rank)
    calls = [0]

    def reduce_max(ctx, values, n):
        calls[0] += 1

    with T.Solver() as s:
        s.create_plan(sub)
        nbytes = s.buffer_size(pr.LM, pr.LN, prec)
        s.keep_starts(3)
        s.set_buffer(nbytes=nbytes)
        keep = T.REDUCE_CB(reduce_max)
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, keep, None) == 0
        s.set_matrix("A", given["A"])
        s.set_matrix("B", sub.B)
        for S in given["starts"][::-1]:                   # oldest first: the newest ends up in slot 0
            s.set_matrix("X", S[xb])
            s.push_start()
        got = s.project_start()
        X = s.get_matrix()
    gathered = [None] * world
    dist.all_gather_object(gathered, dict(xb=xb, X=X, first=sub.first_col, n=sub.n_cols, gamma=got["coefficients"], used=got["n_used"], calls=calls[0]))
    if rank == 0:
        Xg = np.zeros((pr.nnzbX, pr.LM, pr.LN), dtype=X.dtype)
        for g in gathered:
            Xg[g["xb"]] = g["X"]
        order = sorted(gathered, key=lambda g: g["first"])
        np.savez(out, X=Xg, gamma=np.concatenate([g["gamma"] for g in order]), used=np.concatenate([g["used"] for g in order]),
                 calls=[g["calls"] for g in gathered], n_cols=[g["n"] for g in order])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
