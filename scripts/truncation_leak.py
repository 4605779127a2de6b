#!/usr/bin/env python3
"""What tfqmrgpuExt_truncationLeak (include/tfqmrgpu_ext.h section 11) costs, on one GPU -> profiles/truncation_leak.txt

  python scripts/truncation_leak.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16 complex<double>, 784 right-hand sides) and on bench.py's
stencil2d_8x8_z (5-point block stencil 256 x 256, 8 x 8 complex<double>, 8 block columns -- cut at 100 grid steps around the sources here:
full columns leak nothing), after one solve, on one plan in one process:
  truncationLeak()          the C call with all four outputs (two kernels, one copy of [nCols][LN] doubles, one stream synchronise)
  residual()                tfqmrgpuExt_residual with all four outputs: the same kernel structure over the plan's own pair list
  applyOperator(-N) / N     the plan's own plain multiply, N launches in a row
  listing                   the FIRST truncationLeak call of a plan (host analysis, upload, one more synchronise) minus a later one;
                            and the host analysis alone: the counts-only call behind a bufferSize that dropped the listing
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the three calls alternate inside a round, so that they see the same machine.
The expectation to hold the result against: residual() scaled by nLeakPairs / nPairs.
--small: generate_FD_example 6 24 4 2 -0.25 and a 64 x 64 stencil cut at 10 grid steps -- for trying the script out, not for figures.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "truncation_leak.txt"))
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
    nx, radius = (64, 10.0) if args.small else (256, 100.0)
    fd = FDExample(*gen).problem()
    st8 = PR.stencil_2d(nx, nx, 8, 8, 8, seed=5, radius=radius)
    cases = [("generate_FD_example %s" % " ".join(str(g) for g in gen[:5]), fd, "z", 1e-9),
             ("5-point block stencil %d x %d, 8 block columns cut at %g grid steps" % (nx, nx, radius), st8, "z", 1e-9)]

    def timed(fn):
        sync(); t0 = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t0) * 1e3

    lines = [
        "tfqmrgpuExt_truncationLeak against tfqmrgpuExt_residual and the plan's plain multiply, one MI355X; written by scripts/truncation_leak.py (method: its docstring).",
        "revision %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the three calls alternating; host clock around the call + device synchronise;"
        % (rev, args.reps),
        "multiply: applyOperator(-%d) / %d." % (N_MULTIPLY, N_MULTIPLY), ""]
    for name, pr, prec, tol in cases:
        with T.Solver() as s:
            s.create_plan(pr)
            nbytes = s.buffer_size(pr.LM, pr.LN, prec)
            lib = T.lib
            nb, npairs = C.c_uint64(0), C.c_uint64(0)
            t0 = time.perf_counter()
            assert 0 == lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, None, None, C.byref(nb), C.byref(npairs))
            host_ms = (time.perf_counter() - t0) * 1e3              # the host analysis alone: no device call
            s.buffer_size(pr.LM, pr.LN, prec)                       # ... dropped again: the first full call below builds and uploads it
            s.set_buffer(nbytes=nbytes)
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(tol, 2000)
            info, view = s.get_info(), s.plan_view()
            n_cols = int(view["nCols"])
            leak2, r2, b2 = np.zeros((n_cols, pr.LN)), np.zeros((n_cols, pr.LN)), np.zeros((n_cols, pr.LN))
            cols, worst = np.zeros(n_cols, np.int32), C.c_double(0)
            ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

            def ok(status):
                assert status == 0, T.error_string(status)
            calls = {
                "truncationLeak()": lambda: ok(lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, ptr(leak2), ptr(cols), C.byref(nb), C.byref(npairs))),
                "residual()": lambda: ok(lib.tfqmrgpuExt_residual(s.handle, s.plan, ptr(r2), ptr(b2), ptr(cols), C.byref(worst))),
                "multiply": lambda: ok(lib.tfqmrgpuExt_applyOperator(s.handle, s.plan, -N_MULTIPLY)),
            }
            first_ms = timed(calls["truncationLeak()"])             # host analysis + upload + the call itself
            ms = {k: [] for k in calls}
            for rep in range(2 + args.reps):
                for k, fn in calls.items():
                    t = timed(fn) / (N_MULTIPLY if k == "multiply" else 1)
                    if rep >= 2:
                        ms[k].append(t)
            first = leak2.copy()
            calls["truncationLeak()"]()
            assert np.array_equal(first, leak2) and np.isfinite(leak2).all()      # same data, same bits
            units = np.zeros(n_cols, np.uint32)
            n_units = lib.tfqmrgpuExt_leakUnits(s.plan, ptr(units))
        med = {k: statistics.median(v) for k, v in ms.items()}
        n_leak, n_in = int(npairs.value), int(view["nPairs"])
        expected = med["residual()"] * n_leak / n_in
        with np.errstate(divide="ignore", invalid="ignore"):
            whole = np.sqrt((r2 + leak2) / b2)
        lines.append("%s, %d x %d '%s': nnzbA %d, nnzbX %d, nCols %d; solve: status %d, %d iterations, residuum_reached %.3e"
                     % (name, pr.LM, pr.LN, prec, pr.nnzbA, pr.nnzbX, n_cols, st, info["iterations"], info["residual"]))
        lines.append("  nPairs %d; nLeakBlocks %d, nLeakPairs %d = %.4f x nPairs, in %d work units (%d ... %d per column)"
                     % (n_in, int(nb.value), n_leak, n_leak / n_in, n_units, int(units.min()), int(units.max())))
        lines.append("  relative residual, largest over the right-hand sides: truncated %.3e, untruncated sqrt((residual2 + leak2) / bnorm2) %.3e"
                     % (worst.value, np.nanmax(whole)))
        for k in calls:
            lines.append("  %-18s %9.3f ms [%.3f .. %.3f]" % (k, med[k], min(ms[k]), max(ms[k])))
        lines.append("  listing: host analysis alone %.3f ms; first call %.3f ms = %.3f ms more than a later one (analysis, upload, one synchronise)"
                     % (host_ms, first_ms, first_ms - med["truncationLeak()"]))
        lines.append("  expected residual() x nLeakPairs / nPairs = %.3f ms; measured / expected = %.2f; truncationLeak() / multiply %.2f"
                     % (expected, med["truncationLeak()"] / expected, med["truncationLeak()"] / med["multiply"]))
        lines.append("")
        print("\n".join(lines[-9:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
