#!/usr/bin/env python3
"""An energy loop with the block-Jacobi preconditioner, with and without the kept copy of A (include/tfqmrgpu_ext.h section 9), on one
GPU -> profiles/keep_operator.txt

  python scripts/keep_operator_loop.py [--steps 7] [--small] [--revision REV] [--out FILE]

Two systems, both complex<double> with HOST arrays: the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25) and
configuration 3 (13-point block stencil 64 x 64, 32 x 32 blocks, 2 block columns; bench.py runs it in 'c', here it is 'z').  Along the
loop the diagonal blocks of A change (A_e = A + e * 0.01 * 1 on the diagonal blocks that the variant changes).  Per energy step, three
plans side by side in the same run, one after the other inside a step so that they see the same machine:
  (a) today's loop:   setMatrix('A') whole                        + set-up (inversion, scaling of all of A) + solve
  (b) kept copy:      setBlocks('A', the mb diagonal blocks)      + set-up of what was touched             + solve
  (c) kept copy:      setBlocks('A', three diagonal blocks)       + set-up of what was touched             + solve
The set-up is called on its own through getPreconditioner(NULL, NULL), which performs it so that the solve finds it done: the time
"around the solve" is the set call plus the set-up.  Every figure is the host clock around the call plus a device synchronise (the
device is synchronised before as well), the median over --steps steps after two warm-up steps.  (a) and (b) solve the same matrices:
the script checks at every step that the X blocks on B's pattern are equal bit for bit.
The cost of the copy: the whole set-up after a whole setMatrix('A') on the plan that keeps A against the same on the plan that does not,
alternating, same count.  The extra device memory: the size of the A window, and what the free device memory dropped by at the first
set-up of (b).
--small: generate_FD_example 6 24 4 2 -0.25 and a 16 x 16 grid -- for trying the script out, not for figures."""
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
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_operator.txt"))
    args = ap.parse_args()
    rev = args.revision or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd import problems as PR
    from tfqmrgpu_amd.fd_generator import FDExample
    C, lib, RIRI = T.C, T.lib, T.LAYOUT_RIRIRIRI
    sync = torch.cuda.synchronize
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def timed(fn):
        sync(); t0 = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t0) * 1e3

    def ok(status):
        assert status == 0, T.error_string(status)

    def measure(name, pr):
        rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
        diag = np.flatnonzero(rows == pr.colIndA - pr.index_offset).astype(np.int32)
        assert len(diag) == pr.mb
        three = np.ascontiguousarray(diag[[pr.mb // 7, pr.mb // 2, pr.mb - 2]])
        eye = np.eye(pr.LM)
        Aall = np.ascontiguousarray(pr.A, dtype=np.complex128)            # (a), (b): every diagonal block moves with the energy
        Athree = Aall.copy()                                              # (c): three of them do
        plans = {}
        for v in "abc":
            s = T.Solver()
            s.create_plan(pr)
            nbytes = s.buffer_size(pr.LM, pr.LN, "z")
            s.set_preconditioner(T.PRECOND_BLOCK_JACOBI)
            if v != "a":
                s.keep_operator(True)
            s.set_buffer(nbytes=nbytes)
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            plans[v] = s
        setup = lambda s: ok(lib.tfqmrgpuExt_getPreconditioner(s.handle, s.plan, None, None))   # noqa: E731
        before = torch.cuda.mem_get_info()[0]
        setup(plans["a"])
        mid = torch.cuda.mem_get_info()[0]
        setup(plans["b"])
        after = torch.cuda.mem_get_info()[0]
        extra_measured = (mid - after) - (before - mid)                    # what (b) took beyond M^-1 and the index lists that (a) took too
        setup(plans["c"])
        first = {}
        for v, s in plans.items():
            assert s.solve(pr.tolerance, 2000) == 0
            first[v] = s.get_info()["iterations"]

        ms = {v: dict(set=[], setup=[], solve=[]) for v in "abc"}
        its = {v: [] for v in "abc"}
        for step in range(2 + args.steps):                                # two warm-up steps
            shift = 0.01 * (step + 1) * eye
            Aall[diag] = pr.A[diag] + shift
            Athree[three] = pr.A[three] + shift
            Adiag, A3 = np.ascontiguousarray(Aall[diag]), np.ascontiguousarray(Athree[three])
            sets = {
                "a": lambda s: ok(lib.tfqmrgpu_bsrsv_setMatrix(s.handle, s.plan, b"A", ptr(Aall), b"z", pr.LM, pr.LM, b"n", RIRI)),
                "b": lambda s: ok(lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, b"A", len(diag), ptr(diag), ptr(Adiag), b"z", b"n", RIRI)),
                "c": lambda s: ok(lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, b"A", len(three), ptr(three), ptr(A3), b"z", b"n", RIRI)),
            }
            onB = {}
            for v, s in plans.items():
                t = (timed(lambda: sets[v](s)), timed(lambda: setup(s)),
                     timed(lambda: ok(lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, pr.tolerance, 2000))))
                onB[v] = s.get_blocks(None, raw=True)
                if step >= 2:
                    for k, x in zip(("set", "setup", "solve"), t):
                        ms[v][k].append(x)
                    its[v].append(s.get_info()["iterations"])
            assert np.array_equal(onB["a"], onB["b"]), "step %d: (a) and (b) differ" % step
        # the copy: a whole set-up with and without it
        Aall[diag] = pr.A[diag]
        whole = {"a": [], "b": []}
        for rep in range(2 + args.steps):
            for v in "ab":
                s = plans[v]
                ok(lib.tfqmrgpu_bsrsv_setMatrix(s.handle, s.plan, b"A", ptr(Aall), b"z", pr.LM, pr.LM, b"n", RIRI))
                t = timed(lambda: setup(s))
                if rep >= 2:
                    whole[v].append(t)
        for s in plans.values():
            s.close()

        med = lambda v: statistics.median(v)                               # noqa: E731
        a_bytes = pr.nnzbA * 2 * pr.LM * pr.LM * 8
        out = ["%s: mb %d, nnzbA %d, nnzbX %d, nnzbB %d, %d x %d 'z'; first solve: %s iterations" % (
            name, pr.mb, pr.nnzbA, pr.nnzbX, pr.nnzbB, pr.LM, pr.LN, " | ".join("(%s) %d" % (v, first[v]) for v in "abc")),
            "  ms per energy step, median [min .. max] of %d steps after 2 warm-up steps:" % args.steps,
            "  %-50s %-26s %-26s %-26s %s" % ("", "set call", "set-up", "around the solve", "solve (iterations)")]
        label = {"a": "(a) setMatrix('A') whole, no copy", "b": "(b) setBlocks('A', %d diagonal blocks), copy" % len(diag),
                 "c": "(c) setBlocks('A', 3 diagonal blocks), copy"}
        around = {}
        for v in "abc":
            ar = [x + y for x, y in zip(ms[v]["set"], ms[v]["setup"])]
            around[v] = med(ar)
            cell = lambda x: "%8.3f [%.3f .. %.3f]" % (med(x), min(x), max(x))   # noqa: E731
            out.append("  %-50s %-26s %-26s %-26s %s (%s)" % (label[v], cell(ms[v]["set"]), cell(ms[v]["setup"]), cell(ar), cell(ms[v]["solve"]),
                                                               ",".join(str(i) for i in sorted(set(its[v])))))
        out.append("  around the solve, against (a): (b) %.3f, (c) %.3f%s" % (
            around["b"] / around["a"], around["c"] / around["a"],
            "" if max(around["b"], around["c"]) <= around["a"] else "   <-- ABOVE (a): the expectation of the issue is NOT met"))
        out.append("  (a) and (b): the X blocks on B's pattern equal bit for bit at every step")
        out.append("  whole set-up after a whole setMatrix('A'): without the copy %.3f ms [%.3f .. %.3f], with it %.3f ms [%.3f .. %.3f]: the copy costs %.3f ms" % (
            med(whole["a"]), min(whole["a"]), max(whole["a"]), med(whole["b"]), min(whole["b"]), max(whole["b"]), med(whole["b"]) - med(whole["a"])))
        out.append("  extra device memory of a plan that keeps A: %.3f MB (the A window); free device memory dropped by %.3f MB more at the first set-up of (b) than of (a)" % (
            a_bytes * 1e-6, extra_measured * 1e-6))
        return out

    gen = (6, 24, 4, 2, -0.25, 4) if args.small else (16, 120, 4, 2, -0.25, 4)
    n3 = 16 if args.small else 64
    lines = [
        "Energy loop with block Jacobi: whole setMatrix('A') against setBlocks('A') on a plan that keeps A; host arrays, one MI355X;",
        "written by scripts/keep_operator_loop.py (method: its docstring).  revision %s" % rev, ""]
    lines += measure("headline, generate_FD_example %s" % " ".join(str(g) for g in gen[:5]), FDExample(*gen).problem()) + [""]
    lines += measure("configuration 3 in 'z', 13-point block stencil %d x %d" % (n3, n3), PR.stencil_2d(n3, n3, 32, 32, 2, seed=3, points=13))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
