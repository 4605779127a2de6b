#!/usr/bin/env python3
"""What tfqmrgpuExt_dropCost (include/tfqmrgpu_ext.h section 13) costs, on one GPU -> profiles/drop_cost.txt

  python scripts/drop_cost.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16, 784 right-hand sides) as a 'z', a 'c' and an 'm'
plan and on bench.py's stencil2d_8x8_z (5-point block stencil 256 x 256, 8 x 8 complex<double>, 8 full block columns), after one solve
('c': no solve, status -1 in the file -- the float solve of this workload does not reach 1e-4 in 2000 iterations; the X of the 'z' solve
is set instead), on one plan in one process:
  dropCost(cost2)           the C call with cost2 and nProducts (one kernel, one copy of [nnzbX][LN] doubles, one stream synchronise)
  dropCost(weight2)         the C call with weight2 and nProducts: A is not read, no product is formed
  dropCost(both)            the C call with all three outputs: one kernel, two copies
  applyOperator(-N) / N     the plan's own plain multiply, N launches in a row: the same number of block products, in the plan's precision
  residual()                tfqmrgpuExt_residual with all four outputs: the same products in double, [nCols][LN] doubles copied out
  getMatrix('X')            the solution to a host array of the plan's data precision
  shrink (host)             shrinkPattern without every block whose cost is below the median of the blocks without B, and
                            freeGrownPattern: host only
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the calls alternate inside a round, so that they see the same machine.  No target was set in
advance: the call is reported against the three yardsticks of the same plan in the same session, with the size of its records.
--small: generate_FD_example 6 24 4 2 -0.25 and a 64 x 64 stencil -- for trying the script out, not for figures.
--revision: written into the file; default `git rev-parse --short HEAD` of this tree."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_MULTIPLY = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drop_cost.txt"))
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
    fd = FDExample(*gen).problem()
    st8 = PR.stencil_2d(nx, nx, 8, 8, 8, seed=5)
    fd_name = "generate_FD_example %s" % " ".join(str(g) for g in gen[:5])
    cases = [(fd_name, fd, "z", 1e-9), (fd_name, fd, "c", None), (fd_name, fd, "m", 1e-9),
             ("5-point block stencil %d x %d, 8 block columns" % (nx, nx), st8, "z", 1e-9)]

    def timed(fn):
        sync(); t0 = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t0) * 1e3

    lines = [
        "tfqmrgpuExt_dropCost against the plan's plain multiply, tfqmrgpuExt_residual and getMatrix('X'), one MI355X; written by scripts/drop_cost.py (method: its docstring).",
        "revision %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the calls alternating; host clock around the call + device synchronise;"
        % (rev, args.reps),
        "multiply: applyOperator(-%d) / %d." % (N_MULTIPLY, N_MULTIPLY), ""]
    kept_x = None
    for name, pr, prec, tol in cases:
        with T.Solver() as s:
            s.create_plan(pr)
            nbytes = s.buffer_size(pr.LM, pr.LN, prec)
            lib = T.lib
            s.set_buffer(nbytes=nbytes)
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            if tol is None:                                         # 'c': the float solve of this workload does not reach 1e-4 --
                s.set_matrix("X", kept_x)                           # the caller's X: the 'z' solution, rounded to float by the plan
                st, info = -1, dict(iterations=0, residual=float("nan"))
            else:
                st = s.solve(tol, 2000)
                info = s.get_info()
                if kept_x is None:
                    kept_x = s.get_matrix()
            view = s.plan_view()
            n_cols, n_x = int(view["nCols"]), int(view["nnzbX"])
            cost2, weight2 = np.zeros((n_x, pr.LN)), np.zeros((n_x, pr.LN))
            r2, b2 = np.zeros((n_cols, pr.LN)), np.zeros((n_cols, pr.LN))
            columns, worst = np.zeros(n_cols, np.int32), C.c_double(0)
            count = C.c_uint64(0)
            shrunk = T.GrownPattern()
            drop = np.zeros(0, np.int32)
            ptr = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731

            def ok(status):
                assert status == 0, T.error_string(status)

            def shrink():
                ok(lib.tfqmrgpuExt_shrinkPattern(s.plan, len(drop), ptr(drop) if len(drop) else None, C.byref(shrunk)))
                lib.tfqmrgpuExt_freeGrownPattern(C.byref(shrunk))
            calls = {
                "dropCost(cost2)": lambda: ok(lib.tfqmrgpuExt_dropCost(s.handle, s.plan, ptr(cost2), None, C.byref(count))),
                "dropCost(weight2)": lambda: ok(lib.tfqmrgpuExt_dropCost(s.handle, s.plan, None, ptr(weight2), C.byref(count))),
                "dropCost(both)": lambda: ok(lib.tfqmrgpuExt_dropCost(s.handle, s.plan, ptr(cost2), ptr(weight2), C.byref(count))),
                "multiply": lambda: ok(lib.tfqmrgpuExt_applyOperator(s.handle, s.plan, -N_MULTIPLY)),
                "residual()": lambda: ok(lib.tfqmrgpuExt_residual(s.handle, s.plan, ptr(r2), ptr(b2), ptr(columns), C.byref(worst))),
                "getMatrix('X')": lambda: s.get_matrix(raw=True),
                "shrink (host)": shrink,
            }
            first_ms = timed(calls["dropCost(both)"])               # listing + upload + allocation + the call itself
            has_b = np.zeros(n_x, bool)
            has_b[view["subset"]] = True
            total = np.nan_to_num(np.sqrt(cost2), nan=np.inf).max(axis=1)
            free = np.flatnonzero(~has_b)
            drop = np.ascontiguousarray(free[total[free] < np.median(total[free])], dtype=np.int32) if len(free) else drop
            ms = {k: [] for k in calls}
            for rep in range(2 + args.reps):
                for k, fn in calls.items():
                    t = timed(fn) / (N_MULTIPLY if k == "multiply" else 1)
                    if rep >= 2:
                        ms[k].append(t)
            first = (cost2.copy(), weight2.copy())
            calls["dropCost(both)"]()
            same_bits = bool(np.array_equal(first[0], cost2, equal_nan=True) and np.array_equal(first[1], weight2, equal_nan=True))
            not_finite = int((~np.isfinite(cost2)).sum()), int((~np.isfinite(weight2)).sum())
            calls["residual()"]()
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%s, %d x %d '%s': nnzbA %d, nnzbX %d, nCols %d; solve: status %d, %d iterations, residuum_reached %.3e"
                     % (name, pr.LM, pr.LN, prec, pr.nnzbA, pr.nnzbX, n_cols, st, info["iterations"], info["residual"]))
        lines.append("  nProducts %d (%.2f per X block); records [nnzbX][LN] doubles = %.3f MB per array (residual copies out %.3f MB)"
                     % (count.value, count.value / max(1, n_x), n_x * pr.LN * 8e-6, 2 * n_cols * pr.LN * 8e-6))
        lines.append("  sqrt(cost2), largest over j, per block: max %.3e, median %.3e, min %.3e; blocks with cost2 == 0 for all j: %d; worst relative residual %.3e"
                     % (total.max(), np.median(total), total.min(), int((total == 0).sum()), worst.value))
        lines.append("  two calls on the same data: %s; entries that are not finite: cost2 %d, weight2 %d"
                     % ("the same bits" if same_bits else "DIFFERENT BITS", not_finite[0], not_finite[1]))
        for k in calls:
            lines.append("  %-18s %9.3f ms [%.3f .. %.3f]" % (k, med[k], min(ms[k]), max(ms[k])))
        lines.append("  shrink: %d of %d blocks dropped" % (len(drop), n_x))
        lines.append("  first dropCost(both) call %.3f ms = %.3f ms more than a later one (listing, upload, allocation, one synchronise)"
                     % (first_ms, first_ms - med["dropCost(both)"]))
        for k in ("dropCost(cost2)", "dropCost(weight2)", "dropCost(both)"):
            lines.append("  %s / multiply %.2f; / residual() %.2f; / getMatrix('X') %.2f"
                         % (k, med[k] / med["multiply"], med[k] / med["residual()"], med[k] / med["getMatrix('X')"]))
        lines.append("")
        print("\n".join(lines[-18:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
