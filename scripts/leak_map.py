#!/usr/bin/env python3
"""What tfqmrgpuExt_leakMap (include/tfqmrgpu_ext.h section 12) costs, on one GPU -> profiles/leak_map.txt

  python scripts/leak_map.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16 complex<double>, 784 right-hand sides) and on bench.py's
stencil2d_8x8_z (5-point block stencil 256 x 256, 8 x 8 complex<double>, 8 block columns -- cut at 100 grid steps around the sources here:
full columns leak nothing), after one solve, on one plan in one process:
  leakMap()                 the C call with all four outputs (one kernel, one copy of [nLeakBlocks][LN] doubles, one stream synchronise)
  truncationLeak()          tfqmrgpuExt_truncationLeak with all four outputs: the same products folded per block column, [nCols][LN] doubles
  applyOperator(-N) / N     the plan's own plain multiply, N launches in a row
  grow                      growPattern with all positions and freeGrownPattern: host only
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the calls alternate inside a round, so that they see the same machine.  No target was set in
advance: the call is reported against truncationLeak() of the same plan in the same session, with the size of its records.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leak_map.txt"))
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
        "tfqmrgpuExt_leakMap against tfqmrgpuExt_truncationLeak and the plan's plain multiply, one MI355X; written by scripts/leak_map.py (method: its docstring).",
        "revision %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the calls alternating; host clock around the call + device synchronise;"
        % (rev, args.reps),
        "multiply: applyOperator(-%d) / %d." % (N_MULTIPLY, N_MULTIPLY), ""]
    for name, pr, prec, tol in cases:
        with T.Solver() as s:
            s.create_plan(pr)
            nbytes = s.buffer_size(pr.LM, pr.LN, prec)
            lib = T.lib
            s.set_buffer(nbytes=nbytes)
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(tol, 2000)
            info, view = s.get_info(), s.plan_view()
            n_cols = int(view["nCols"])
            n_pos, n_pairs = s.leak_counts()
            rows, cols = np.zeros(n_pos, np.int32), np.zeros(n_pos, np.int32)
            pos2, leak2 = np.zeros((n_pos, pr.LN)), np.zeros((n_cols, pr.LN))
            columns = np.zeros(n_cols, np.int32)
            nb, npairs = C.c_uint64(0), C.c_uint64(0)
            grown = T.GrownPattern()
            ptr = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731

            def ok(status):
                assert status == 0, T.error_string(status)

            def grow():
                ok(lib.tfqmrgpuExt_growPattern(s.plan, 0, None, C.byref(grown)))
                lib.tfqmrgpuExt_freeGrownPattern(C.byref(grown))
            calls = {
                "leakMap()": lambda: ok(lib.tfqmrgpuExt_leakMap(s.handle, s.plan, n_pos, ptr(rows), ptr(cols), ptr(pos2), C.byref(nb))),
                "truncationLeak()": lambda: ok(lib.tfqmrgpuExt_truncationLeak(s.handle, s.plan, ptr(leak2), ptr(columns), C.byref(nb), C.byref(npairs))),
                "multiply": lambda: ok(lib.tfqmrgpuExt_applyOperator(s.handle, s.plan, -N_MULTIPLY)),
                "grow (host)": grow,
            }
            first_ms = timed(calls["leakMap()"])                    # host analysis + upload + allocation + the call itself
            ms = {k: [] for k in calls}
            for rep in range(2 + args.reps):
                for k, fn in calls.items():
                    t = timed(fn) / (N_MULTIPLY if k == "multiply" else 1)
                    if rep >= 2:
                        ms[k].append(t)
            first = pos2.copy()
            calls["leakMap()"]()
            assert np.array_equal(first, pos2) and np.isfinite(pos2).all()      # same data, same bits
            sums = np.zeros_like(leak2)
            np.add.at(sums, cols, pos2)
            with np.errstate(divide="ignore", invalid="ignore"):
                rule = np.nanmax(np.where(leak2 > 0, np.abs(sums - leak2) / leak2, 0.0))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%s, %d x %d '%s': nnzbA %d, nnzbX %d, nCols %d; solve: status %d, %d iterations, residuum_reached %.3e"
                     % (name, pr.LM, pr.LN, prec, pr.nnzbA, pr.nnzbX, n_cols, st, info["iterations"], info["residual"]))
        lines.append("  nPairs %d; nLeakBlocks %d, nLeakPairs %d; records [nLeakBlocks][LN] doubles = %.3f MB (truncationLeak copies out %.3f MB)"
                     % (int(view["nPairs"]), n_pos, n_pairs, n_pos * pr.LN * 8e-6, n_cols * pr.LN * 8e-6))
        lines.append("  positions of a column added on the host against leak2: largest relative difference %.2e; largest / smallest pos2 %.3e / %.3e"
                     % (rule, pos2.max() if n_pos else 0.0, pos2.min() if n_pos else 0.0))
        for k in calls:
            lines.append("  %-18s %9.3f ms [%.3f .. %.3f]" % (k, med[k], min(ms[k]), max(ms[k])))
        lines.append("  first leakMap() call %.3f ms = %.3f ms more than a later one (analysis, upload, allocation, one synchronise)"
                     % (first_ms, first_ms - med["leakMap()"]))
        lines.append("  leakMap() / truncationLeak() %.2f; leakMap() / multiply %.2f" % (med["leakMap()"] / med["truncationLeak()"], med["leakMap()"] / med["multiply"]))
        lines.append("")
        print("\n".join(lines[-10:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
