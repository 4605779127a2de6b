#!/usr/bin/env python3
"""What it costs to move A, B and X from one plan to another (tfqmrgpuExt_carry, include/tfqmrgpu_ext.h section 15), on one GPU
-> profiles/carry.txt

  python scripts/carry.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16, 784 right-hand sides, 'z').  The source plan has
solved; the destination plan has the pattern of X grown by its leak positions (grow_pattern; evenly spaced ones where there are more
than a tenth of X's blocks), so the map has -1 entries and the internal block orders of the two plans differ.  Timed, for the same map:
  (i)   carry('X')                     dst.carry_from(src, 'X', oldBlock): host composition of the list, its upload, one launch
  (ii)  getBlocks + setBlocks          the two-call device route: src.getBlocks of the blocks that have a source into device scratch, then
                                       dst.setBlocks from it (the added blocks are left as they are: it cannot zero them)
  (iii) device-to-device copy          torch's Tensor.copy_ between two device arrays of the size of dst's X (hipMemcpyAsync)
  (iv)  host route                     src.get_matrix, numpy through oldBlock, dst.set_matrix('X')
and also: carry('X') from a 'c' plan of the same problem into the 'z' plan (float -> double, quads -> pairs), carry('A'), carry('B'),
the whole adopt (A, B, X) and the solve_from that follows it.
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the alternatives alternate inside a round, so that they see the same machine.  GB/s: bytes of
dst's X read plus written (2 x) over the time.  The acceptance condition is (i) < (ii); no other target was set in advance.
--small: generate_FD_example 6 24 4 2 -0.25 -- for trying the script out, not for figures.
--revision: written into the file; default `git rev-parse --short HEAD` of this tree."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carry.txt"))
    args = ap.parse_args()
    rev = args.revision or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd.fd_generator import FDExample
    sync = torch.cuda.synchronize
    gen = (6, 24, 4, 2, -0.25, 4) if args.small else (16, 120, 4, 2, -0.25, 4)
    pr = FDExample(*gen).problem()
    tol = 1e-9

    def timed(fn):
        sync(); t0 = time.perf_counter(); out = fn(); sync()
        return (time.perf_counter() - t0) * 1e3, out

    def plan(problem, prec):
        s = T.Solver()
        s.create_plan(problem)
        s.set_buffer(nbytes=s.buffer_size(problem.LM, problem.LN, prec))
        return s

    src, src_c = plan(pr, "z"), plan(pr, "c")
    for s in (src, src_c):
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
    st = src.solve(tol, 2000)
    its = src.get_info()["iterations"]
    src_c.solve(1e-4, 2000)
    n_leak = src.leak_counts()[0]
    take = np.arange(0, n_leak, max(1, (10 * n_leak) // max(1, pr.nnzbX)), dtype=np.uint64)
    rp, ci, old = src.grow_pattern(take)
    grown = T.Problem(pr.rowPtrA, pr.colIndA, pr.A, rp, ci, pr.rowPtrB, pr.colIndB, pr.B, None, pr.tolerance, pr.index_offset)
    dst = plan(grown, "z")
    have = np.flatnonzero(old >= 0).astype(np.int32)
    from_ = old[have].astype(np.int32)
    block_bytes = 2 * pr.LM * pr.LN * 8
    x_bytes = grown.nnzbX * block_bytes
    scratch = torch.empty(len(have) * block_bytes, dtype=torch.uint8, device="cuda")
    a, b = torch.empty(x_bytes, dtype=torch.uint8, device="cuda"), torch.zeros(x_bytes, dtype=torch.uint8, device="cuda")

    def two_calls():
        src.get_blocks_device(scratch.data_ptr(), from_)
        dst.set_blocks_device("X", have, scratch.data_ptr())

    def host_route():
        x = src.get_matrix()
        xm = np.zeros((grown.nnzbX, pr.LM, pr.LN), dtype=np.complex128)
        xm[have] = x[from_]
        dst.set_matrix("X", xm)

    def adopt_and_solve():
        ms_adopt, _ = timed(lambda: dst.adopt(src, old))
        ms_solve, status = timed(lambda: dst.solve_from(tol, 2000))
        return ms_adopt, ms_solve, status, dst.get_info()["iterations"]

    calls = {
        "(i)   carry('X')": lambda: timed(lambda: dst.carry_from(src, "X", old))[0],
        "(ii)  getBlocks + setBlocks": lambda: timed(two_calls)[0],
        "(iii) device-to-device copy": lambda: timed(lambda: a.copy_(b))[0],
        "(iv)  host route": lambda: timed(host_route)[0],
        "carry('X') 'c' -> 'z'": lambda: timed(lambda: dst.carry_from(src_c, "X", old))[0],
        "carry('A')": lambda: timed(lambda: dst.carry_from(src, "A"))[0],
        "carry('B')": lambda: timed(lambda: dst.carry_from(src, "B"))[0],
    }
    ms = {k: [] for k in calls}
    adopt_ms, solve_ms, warm = [], [], None
    for rep in range(2 + args.reps):
        for k, fn in calls.items():
            t = fn()
            if rep >= 2:
                ms[k].append(t)
        t_adopt, t_solve, status, warm_its = adopt_and_solve()
        if rep >= 2:
            adopt_ms.append(t_adopt); solve_ms.append(t_solve); warm = (status, warm_its)
    # what the routes leave behind: (i) against the host route, bit for bit
    dst.carry_from(src, "X", old)
    x_dev = dst.get_matrix(raw=True)
    host_route()
    same = bool(np.array_equal(x_dev.view(np.uint8), dst.get_matrix(raw=True).view(np.uint8)))
    cold_ms, cold_status = timed(lambda: dst.solve(tol, 2000))
    cold_its = dst.get_info()["iterations"]
    for s in (src, src_c, dst):
        s.close()

    med = {k: statistics.median(v) for k, v in ms.items()}
    gbs = lambda t: 2 * x_bytes / (t * 1e-3) / 1e9      # noqa: E731
    lines = [
        "tfqmrgpuExt_carry against the other routes from one plan to another, one MI355X; written by scripts/carry.py (method: its docstring).",
        "revision %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the calls alternating; host clock around the call + device synchronise."
        % (rev, args.reps), "",
        "generate_FD_example %s, %d x %d 'z': nnzbA %d, nnzbB %d, nnzbX %d -> %d on the grown pattern (%d of %d leak positions taken); solve of the old pattern: status %d, %d iterations"
        % (" ".join(str(g) for g in gen[:5]), pr.LM, pr.LN, pr.nnzbA, pr.nnzbB, pr.nnzbX, grown.nnzbX, len(take), n_leak, st, its),
        "X of the grown plan: %.1f MB; A: %.1f MB" % (x_bytes / 1e6, pr.nnzbA * 2 * pr.LM * pr.LM * 8 / 1e6)]
    for k in calls:
        extra = "  %7.1f GB/s read + written" % gbs(med[k]) if "X" in k or "copy" in k or "Blocks" in k or "host" in k else ""
        lines.append("  %-30s %9.3f ms [%.3f .. %.3f]%s" % (k, med[k], min(ms[k]), max(ms[k]), extra))
    lines.append("  %-30s %9.3f ms [%.3f .. %.3f]" % ("adopt (A, B, X)", statistics.median(adopt_ms), min(adopt_ms), max(adopt_ms)))
    lines.append("  %-30s %9.3f ms [%.3f .. %.3f]  status %d, %d iterations" % ("solve_from behind it", statistics.median(solve_ms), min(solve_ms), max(solve_ms), warm[0], warm[1]))
    lines.append("  %-30s %9.3f ms  status %d, %d iterations (once)" % ("cold solve of the grown plan", cold_ms, cold_status, cold_its))
    i, ii, iii = med["(i)   carry('X')"], med["(ii)  getBlocks + setBlocks"], med["(iii) device-to-device copy"]
    lines.append("  (i) / (ii) = %.2f: %s;  (i) / (iii) = %.2f;  X after (i) and after (iv): %s" % (
        i / ii, "the call is faster than the two-call route" if i < ii else "THE CALL IS NOT FASTER THAN THE TWO-CALL ROUTE", i / iii,
        "the same bits" if same else "DIFFERENT BITS"))
    lines.append("")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
