"""Worker of tests/test_gpu_padding.py: one rank of the column-sharded solve on a PADDED plan (include/tfqmrgpu_ext.h section 18) on
cuda:0, the pattern of tests/_gpu_rank_worker.py: the ranks share the one GPU of the test box, the stopping test is max-reduced through
the host callback.  argv: out, lm, ln, seed, precision, threshold.  Rank 0 gathers the solution and writes argv[1]."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, lm, ln, seed, prec, tol = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], float(sys.argv[6])
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert torch.cuda.is_available(), "no GPU: the product has no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd import problems as PR
    pr = PR.stencil_2d(4, 3, lm, ln, 3, seed=seed)
    sub, xb, bb = T.shard_columns(pr, world, rank)

    def reduce_max(ctx, values, n):
        t = torch.tensor([values[i] for i in range(n)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        for i in range(n):
            values[i] = float(t[i])

    with T.Solver() as s:
        s.create_plan(sub)
        s.allow_padding(True)
        s.set_buffer(nbytes=s.buffer_size(lm, ln, prec))
        shape = s.padded_shape()
        s.set_matrix("A", sub.A)
        s.set_matrix("B", sub.B)
        keep = T.REDUCE_CB(reduce_max)
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, keep, None) == 0
        st = s.solve(tol, 300)
        info, X, hist = s.get_info(), s.get_matrix(), s.bound_history()
    gathered = [None] * world
    dist.all_gather_object(gathered, dict(status=st, iterations=info["iterations"], history=hist, xb=xb, X=X, shape=shape))
    if rank == 0:
        Xg = np.zeros((pr.nnzbX, lm, ln), dtype=X.dtype)
        for g in gathered:
            Xg[g["xb"]] = g["X"]
        np.savez(out, X=Xg, status=[g["status"] for g in gathered], iterations=[g["iterations"] for g in gathered],
                 history=np.array([g["history"] for g in gathered]), shape=np.array([g["shape"] for g in gathered]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
