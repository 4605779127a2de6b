#!/usr/bin/env python3
"""What a warm start (tfqmrgpuExt_solveFrom, include/tfqmrgpu_ext.h section 14) costs and saves, on one GPU -> profiles/solve_from.txt

  python scripts/solve_from.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16, 784 right-hand sides, 'z') and on bench.py's
stencil2d_8x8_z (5-point block stencil 256 x 256, 8 x 8 complex<double>, 8 full block columns), on one plan in one process:
  fixed cost            solve_from(1e-30, K) - solve(1e-30, K) for K = 4: the same K iterations, so the difference is the product A X0, the
                        residual pass, the column set-up and the update; in ms and in iterations, one iteration being
                        (solve(1e-30, 12) - solve(1e-30, 4)) / 8
  cold                  solve(threshold, 2000) of A' = A with every diagonal block shifted by 1e-3 (set_blocks('A')): the reference
  (a) energy step       solve_from(threshold, 2000) on A' from the X of the neighbouring energy, the solution of A
  (b) halfway           solve_from(threshold, 2000) on A' from the X of a cold solve stopped at half its iterations
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the calls alternate inside a round -- cold, (a), (b), the fixed-cost solves --, so that they see the
same machine.  X0 is brought back by set_matrix('X') in front of every warm solve; that copy is not timed.  No target was set in
advance.
--small: generate_FD_example 6 24 4 2 -0.25 and a 64 x 64 stencil -- for trying the script out, not for figures.
--revision: written into the file; default `git rev-parse --short HEAD` of this tree."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solve_from.txt"))
    args = ap.parse_args()
    rev = args.revision or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd import problems as PR
    from tfqmrgpu_amd.fd_generator import FDExample
    sync = torch.cuda.synchronize
    gen = (6, 24, 4, 2, -0.25, 4) if args.small else (16, 120, 4, 2, -0.25, 4)
    nx = 64 if args.small else 256
    cases = [("generate_FD_example %s" % " ".join(str(g) for g in gen[:5]), FDExample(*gen).problem(), "z", 1e-9),
             ("5-point block stencil %d x %d, 8 block columns" % (nx, nx), PR.stencil_2d(nx, nx, 8, 8, 8, seed=5), "z", 1e-9)]

    def timed(fn):
        sync(); t0 = time.perf_counter(); out = fn(); sync()
        return (time.perf_counter() - t0) * 1e3, out

    lines = [
        "tfqmrgpuExt_solveFrom against tfqmrgpu_bsrsv_solve on the same plan, one MI355X; written by scripts/solve_from.py (method: its docstring).",
        "revision %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the calls alternating; host clock around the call + device synchronise."
        % (rev, args.reps), ""]
    for name, pr, prec, tol in cases:
        rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
        diag = np.flatnonzero(rows == np.asarray(pr.colIndA, dtype=np.int64) - pr.index_offset)
        with T.Solver() as s:
            s.create_plan(pr)
            s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, prec))
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(tol, 2000)
            its_a = s.get_info()["iterations"]
            x_energy = s.get_matrix()                                # the solution of the neighbouring energy
            s.set_blocks("A", diag, pr.A[diag] + 1e-3 * np.eye(pr.LM))
            stale = s.residual()["worst"]
            s.solve(tol, 2000)
            its_cold = s.get_info()["iterations"]
            assert s.solve(tol, max(1, its_cold // 2)) == 9
            x_half, half = s.get_matrix(), s.residual()["worst"]

            def warm(x0, threshold, max_it):
                s.set_matrix("X", x0)                                # (not timed)
                ms, status = timed(lambda: s.solve_from(threshold, max_it))
                return ms, status, s.get_info()["iterations"]

            def cold(threshold, max_it):
                ms, status = timed(lambda: s.solve(threshold, max_it))
                return ms, status, s.get_info()["iterations"]
            calls = {
                "cold": lambda: cold(tol, 2000),
                "(a) energy step": lambda: warm(x_energy, tol, 2000),
                "(b) halfway": lambda: warm(x_half, tol, 2000),
                "solve(1e-30, %d)" % K: lambda: cold(1e-30, K),
                "solve_from(1e-30, %d)" % K: lambda: warm(x_half, 1e-30, K),
                "solve(1e-30, %d)" % (K + 8): lambda: cold(1e-30, K + 8),
            }
            ms, its, status = {k: [] for k in calls}, {}, {}
            for rep in range(2 + args.reps):
                for k, fn in calls.items():
                    t, status[k], its[k] = fn()
                    if rep >= 2:
                        ms[k].append(t)
            s.set_matrix("X", x_energy)
            s.solve_from(tol, 2000)
            warm_res = s.residual()["worst"]
            s.solve(tol, 2000)
            cold_res = s.residual()["worst"]
        med = {k: statistics.median(v) for k, v in ms.items()}
        per_it = (med["solve(1e-30, %d)" % (K + 8)] - med["solve(1e-30, %d)" % K]) / 8
        fixed = med["solve_from(1e-30, %d)" % K] - med["solve(1e-30, %d)" % K]
        lines.append("%s, %d x %d '%s': nnzbA %d, nnzbX %d; solve of A: status %d, %d iterations; A' = A + 1e-3 on the %d diagonal blocks"
                     % (name, pr.LM, pr.LN, prec, pr.nnzbA, pr.nnzbX, st, its_a, len(diag)))
        lines.append("  relative residual of A' (residual(), double): X of A %.3e | halfway X %.3e | after the cold solve %.3e | after (a) %.3e"
                     % (stale, half, cold_res, warm_res))
        for k in calls:
            lines.append("  %-22s %9.3f ms [%.3f .. %.3f]  status %d, %d iterations" % (k, med[k], min(ms[k]), max(ms[k]), status[k], its[k]))
        lines.append("  one iteration %.3f ms; fixed cost of a warm start %.3f ms = %.2f iterations" % (per_it, fixed, fixed / per_it))
        for k in ("(a) energy step", "(b) halfway"):
            lines.append("  %s / cold: %.2f of the time, %d of %d iterations" % (k, med[k] / med["cold"], its[k], its["cold"]))
        lines.append("")
        print("\n".join(lines[-14:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
