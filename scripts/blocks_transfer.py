#!/usr/bin/env python3
"""Listed blocks (include/tfqmrgpu_ext.h section 8) against the whole-operand calls, on one GPU -> profiles/blocks_transfer.txt

  python scripts/blocks_transfer.py [--reps 9] [--small] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16 complex<double>, 784 right-hand sides), with HOST
arrays, after one solve, four calls on one plan:
  getMatrix('X')            all of X                     getBlocks('X', NULL)         the X blocks on B's pattern
  setMatrix('A')            all of A                     setBlocks('A', diagonal)     the mb diagonal blocks of A
Each is timed as the host clock around the call plus a device synchronise (the device is synchronised before as well), after two
warm-up calls, as the median of --reps calls; the four calls alternate inside one repetition, so that they see the same machine.  The
yardstick of a partial call is the whole-operand call of the same run.  The values that the partial calls move are those already in the
plan, so the plan's A and X are the same after the measurement as before, which the script checks (the blocks read equal the slice of
getMatrix; a solve after the measurement repeats the iterations and the residual of the solve before it).
--small: generate_FD_example 6 24 4 2 -0.25 (what bench.py --small runs) -- for trying the script out, not for figures.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks_transfer.txt"))
    args = ap.parse_args()
    rev = args.revision or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd.fd_generator import FDExample
    gen = (6, 24, 4, 2, -0.25, 4) if args.small else (16, 120, 4, 2, -0.25, 4)
    pr = FDExample(*gen).problem()
    sync = torch.cuda.synchronize

    def timed(fn):
        sync(); t0 = time.perf_counter(); r = fn(); sync()
        return (time.perf_counter() - t0) * 1e3, r

    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    diag = np.flatnonzero(rows == pr.colIndA - pr.index_offset).astype(np.int32)
    assert len(diag) == pr.mb
    Adiag = np.ascontiguousarray(pr.A[diag])
    with T.Solver() as s:
        s.create_plan(pr)
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, "z"))
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        st = s.solve(pr.tolerance, 2000)
        before = s.get_info()
        # the C calls themselves, on host arrays that exist before the clock starts (no allocation or copy of the binding inside a figure)
        C, lib, RIRI = T.C, T.lib, T.LAYOUT_RIRIRIRI
        Xall = np.zeros((pr.nnzbX, pr.LM, pr.LN, 2))
        XonB = np.zeros((pr.nnzbB, pr.LM, pr.LN, 2))
        Aall = np.ascontiguousarray(pr.A, dtype=np.complex128)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

        def ok(status):
            assert status == 0, T.error_string(status)
        calls = {
            "getMatrix('X')": (lambda: ok(lib.tfqmrgpu_bsrsv_getMatrix(s.handle, s.plan, b"X", ptr(Xall), b"z", pr.LN, pr.LM, b"n", RIRI)), Xall.nbytes),
            "getBlocks('X', NULL)": (lambda: ok(lib.tfqmrgpuExt_getBlocks(s.handle, s.plan, b"X", pr.nnzbB, None, ptr(XonB), b"z", b"n", RIRI)), XonB.nbytes),
            "setMatrix('A')": (lambda: ok(lib.tfqmrgpu_bsrsv_setMatrix(s.handle, s.plan, b"A", ptr(Aall), b"z", pr.LM, pr.LM, b"n", RIRI)), Aall.nbytes),
            "setBlocks('A', diagonal)": (lambda: ok(lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, b"A", len(diag), ptr(diag), ptr(Adiag), b"z", b"n", RIRI)), Adiag.nbytes),
        }
        ms = {name: [] for name in calls}
        for rep in range(2 + args.reps):                      # two warm-ups, then the four calls alternating
            for name, (fn, _) in calls.items():
                t = timed(fn)[0]
                if rep >= 2:
                    ms[name].append(t)
        assert np.array_equal(XonB, Xall[s.plan_view()["subset"]]) and np.array_equal(s.get_blocks(None, raw=True), XonB.reshape(pr.nnzbB, -1))
        st2 = s.solve(pr.tolerance, 2000)
        after = s.get_info()
        assert (st2, after["iterations"], after["residual"]) == (st, before["iterations"], before["residual"]), (before, after)

    med = {name: statistics.median(v) for name, v in ms.items()}
    lines = [
        "Listed blocks against whole operands, host arrays, one MI355X; written by scripts/blocks_transfer.py (method: its docstring).",
        "revision %s; generate_FD_example %s: mb %d, nnzbA %d, nnzbX %d, nnzbB %d, %d x %d 'z'; solve: status %d, %d iterations" % (
            rev, " ".join(str(g) for g in gen[:5]), pr.mb, pr.nnzbA, pr.nnzbX, pr.nnzbB, pr.LM, pr.LN, st, before["iterations"]),
        "ms per call: median [min .. max] of %d calls after 2 warm-ups, the four calls alternating; host clock around the call + device synchronise." % args.reps,
        ""]
    for name, (_, nbytes) in calls.items():
        v = ms[name]
        lines.append("  %-26s %10.3f MB  %9.3f ms [%.3f .. %.3f]" % (name, nbytes * 1e-6, med[name], min(v), max(v)))
    lines += ["",
              "  getBlocks('X', NULL) / getMatrix('X')     : time %.5f, bytes %.5f" % (
                  med["getBlocks('X', NULL)"] / med["getMatrix('X')"], calls["getBlocks('X', NULL)"][1] / calls["getMatrix('X')"][1]),
              "  setBlocks('A', diagonal) / setMatrix('A') : time %.5f, bytes %.5f" % (
                  med["setBlocks('A', diagonal)"] / med["setMatrix('A')"], calls["setBlocks('A', diagonal)"][1] / calls["setMatrix('A')"][1]),
              "  (the C calls, through ctypes, on host arrays that exist before the clock starts)"]
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
