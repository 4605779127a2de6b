#!/usr/bin/env python3
"""What tfqmrgpuExt_residual (include/tfqmrgpu_ext.h section 10) costs, on one GPU -> profiles/residual_check.txt

  python scripts/residual_check.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16, 784 right-hand sides) as a 'z', a 'c' and an 'm' plan,
and on bench.py's stencil2d_8x8_z (5-point block stencil 256 x 256, 8 x 8 complex<double>, 8 block columns), after one solve, on one plan in
one process:
  residual()                the C call with all four outputs (two kernels, one copy of [nCols][2][LN] doubles, one stream synchronise)
  applyOperator(-N) / N     the plan's own plain multiply, N launches in a row: the yardstick of the kernel
  getMatrix('X')            what a check on the host has to fetch first: the call that residual() replaces
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the three calls alternate inside a round, so that they see the same machine.
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
N_MULTIPLY = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_check.txt"))
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
    cases = [(fd_name, fd, "z", 1e-9), (fd_name, fd, "c", 1e-4), (fd_name, fd, "m", 1e-9),
             ("5-point block stencil %d x %d, 8 block columns" % (nx, nx), st8, "z", 1e-9)]

    def timed(fn):
        sync(); t0 = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t0) * 1e3

    lines = [
        "tfqmrgpuExt_residual against the plan's plain multiply and getMatrix('X'), one MI355X; written by scripts/residual_check.py (method: its docstring).",
        "revision %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the three calls alternating; host clock around the call + device synchronise;"
        % (rev, args.reps),
        "multiply: applyOperator(-%d) / %d." % (N_MULTIPLY, N_MULTIPLY), ""]
    for name, pr, prec, tol in cases:
        with T.Solver() as s:
            s.create_plan(pr)
            s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, prec))
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(tol, 2000)
            info = s.get_info()
            C, lib = T.C, T.lib
            n_cols = int(s.plan_view()["nCols"])
            r2, b2 = np.zeros((n_cols, pr.LN)), np.zeros((n_cols, pr.LN))
            cols, worst = np.zeros(n_cols, np.int32), C.c_double(0)
            dp = s.data_precision
            Xall = np.zeros((pr.nnzbX, pr.LM, pr.LN, 2), dtype=np.float64 if dp == "z" else np.float32)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

            def ok(status):
                assert status == 0, T.error_string(status)
            calls = {
                "residual()": lambda: ok(lib.tfqmrgpuExt_residual(s.handle, s.plan, ptr(r2), ptr(b2), ptr(cols), C.byref(worst))),
                "multiply": lambda: ok(lib.tfqmrgpuExt_applyOperator(s.handle, s.plan, -N_MULTIPLY)),
                "getMatrix('X')": lambda: ok(lib.tfqmrgpu_bsrsv_getMatrix(s.handle, s.plan, b"X", ptr(Xall), dp.encode(), pr.LN, pr.LM, b"n", T.LAYOUT_RIRIRIRI)),
            }
            ms = {k: [] for k in calls}
            for rep in range(2 + args.reps):
                for k, fn in calls.items():
                    t = timed(fn) / (N_MULTIPLY if k == "multiply" else 1)
                    if rep >= 2:
                        ms[k].append(t)
            first = (r2.copy(), b2.copy(), np.float64(worst.value))
            calls["residual()"]()
            again = (r2, b2, np.float64(worst.value))
            same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, again))      # same data, same bits
            if not same or not np.isfinite(r2).all():
                print("%s '%s': status %d, %d entries of residual2 not finite, repeated call %s" % (
                    name, prec, st, int((~np.isfinite(r2)).sum()), "identical" if same else "DIFFERENT: largest |difference| %.3e" % np.nanmax(np.abs(first[0] - r2))), flush=True)
            assert same
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%s, %d x %d '%s': nnzbA %d, nnzbX %d, nCols %d; solve: status %d, %d iterations, residuum_reached %.3e; residual(): worst %.3e"
                     % (name, pr.LM, pr.LN, prec, pr.nnzbA, pr.nnzbX, n_cols, st, info["iterations"], info["residual"], worst.value))
        for k in calls:
            lines.append("  %-16s %9.3f ms [%.3f .. %.3f]" % (k, med[k], min(ms[k]), max(ms[k])))
        lines.append("  residual() / multiply %.2f;  residual() / getMatrix('X') %.3f (%.3f ms less)" % (
            med["residual()"] / med["multiply"], med["residual()"] / med["getMatrix('X')"], med["getMatrix('X')"] - med["residual()"]))
        lines.append("")
        print("\n".join(lines[-7:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
