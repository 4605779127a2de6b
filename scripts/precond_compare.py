#!/usr/bin/env python3
"""Block-Jacobi right preconditioner (include/tfqmrgpu_ext.h section 7) off against on, on one GPU -> profiles/precond_block_jacobi.txt

  python scripts/precond_compare.py [--parent-tree DIR] [--reps 9] [--configs a,b,..] [--out FILE]

For the headline workload of bench.py and the single-GPU BASELINE configurations, in ONE process per configuration, off and on
alternating on two plans that stay alive: iterations, residual, milliseconds per warm solve (median, min and max of --reps solves after
two warm-ups; host clock around solve + device synchronise), and apart from that
  set-up          tfqmrgpuExt_getPreconditioner(NULL, &n) right after setMatrix('A'): inversion of the diagonal blocks, scaling of A,
                  4 bytes read back; host clock, device synchronised before and after (the upload of A is not inside)
  back transform  solve(threshold, 0) -- no iteration, only the start of a solve and, when on, X := M^-1 X -- on minus off
--parent-tree DIR: a built checkout of the parent commit.  The plain solve is then timed in fresh processes, parent and this tree
alternating, twice each: the difference between the two runs of the parent is the run-to-run spread the comparison is held against.
Every measurement runs in a child process of its own (`--measure`), one at a time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    "fd2d_16x16_z": "headline: generate_FD_example 16 120 4 2 -0.25, 16x16 complex<double>, 784 right-hand sides",
    "stencil3d_32x32_c": "BASELINE config 3: 13-point block stencil 64x64, 32x32 complex<float>, 64 right-hand sides, threshold 1e-4",
    "cfg4_shard": "BASELINE config 4, one GPU's shard: 5-point block stencil 128x128, 16x16 complex<double>, 32 block columns",
    "stencil2d_8x8_z": "BASELINE config 5: 5-point block stencil 256x256, 8x8 complex<double>, 8 block columns",
}


def build(name):
    from tfqmrgpu_amd import problems as PR
    from tfqmrgpu_amd.fd_generator import FDExample
    if name == "fd2d_16x16_z":
        return FDExample(16, 120, 4, 2, -0.25, 4).problem(), "z", 1e-9
    if name == "stencil3d_32x32_c":
        return PR.stencil_2d(64, 64, 32, 32, 2, seed=3, points=13), "c", 1e-4
    if name == "cfg4_shard":
        return PR.stencil_2d(128, 128, 16, 16, 32, seed=7), "z", 1e-9
    if name == "stencil2d_8x8_z":
        return PR.stencil_2d(256, 256, 8, 8, 8, seed=5), "z", 1e-9
    raise SystemExit("unknown configuration " + name)


def measure(name, tree, reps, plain_only):
    sys.path.insert(0, tree)
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    pr, prec, tol = build(name)
    sync = torch.cuda.synchronize

    def timed(fn):
        sync(); t0 = time.perf_counter(); r = fn(); sync()
        return (time.perf_counter() - t0) * 1e3, r

    plans = {}
    out = {"config": name, "tree": tree, "mb": pr.mb, "nnzbA": pr.nnzbA, "nnzbX": pr.nnzbX, "LM": pr.LM, "LN": pr.LN, "precision": prec}
    for mode in (["off"] if plain_only else ["off", "on"]):
        s = T.Solver()
        s.create_plan(pr)
        nbytes = s.buffer_size(pr.LM, pr.LN, prec)
        if mode == "on":
            s.set_preconditioner(T.PRECOND_BLOCK_JACOBI)
        s.set_buffer(nbytes=nbytes)
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        rec = {"buffer_bytes": nbytes}
        if mode == "on":
            rec["setup_ms_first"], (_, rec["n_identity"]) = timed(lambda: s.get_preconditioner(values=False))
            setups = []
            for _ in range(max(3, reps // 2)):               # warm: a new A on the same plan, as a caller with a sequence of operators has it
                s.set_matrix("A", pr.A)
                setups.append(timed(lambda: s.get_preconditioner(values=False))[0])
            rec["setup_ms"] = setups
        plans[mode] = (s, rec)
    for mode, (s, rec) in plans.items():
        for _ in range(2):
            st = s.solve(tol, 2000)
        sync()
        info = s.get_info()
        rec.update(status=st, iterations=info["iterations"], residual=info["residual"], flops=info["flops"], solve_ms=[], start_only_ms=[])
    for _ in range(reps):                                      # off and on alternate
        for mode, (s, rec) in plans.items():
            rec["solve_ms"].append(timed(lambda: s.solve(tol, 2000))[0])
    for _ in range(reps):
        for mode, (s, rec) in plans.items():
            rec["start_only_ms"].append(timed(lambda: s.solve(tol, 0))[0])
    for mode, (s, rec) in plans.items():
        out[mode] = rec
        s.close()
    print("PRECOND_COMPARE " + json.dumps(out))


def child(name, tree, reps, plain_only):
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--measure", name, "--tree", tree, "--reps", str(reps)]
    if plain_only:
        cmd.append("--plain-only")
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
    if r.returncode != 0:
        raise SystemExit("measurement of %s in %s ended with %d:\n%s" % (name, tree, r.returncode, (r.stdout + r.stderr)[-3000:]))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("PRECOND_COMPARE ")][-1]
    return json.loads(line[len("PRECOND_COMPARE "):])


def med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precond_block_jacobi.txt"))
    args = ap.parse_args()
    if args.measure:
        return measure(args.measure, args.tree, args.reps, args.plain_only)
    lines = ["Block-Jacobi right preconditioner, off against on, one MI355X; written by scripts/precond_compare.py (method: its docstring).",
             "ms per solve: median [min .. max] of %d warm solves, off and on alternating in one process; host clock around solve + device synchronise." % args.reps, ""]
    for name in args.configs.split(","):
        r = child(name, ROOT, args.reps, False)
        off, on = r["off"], r["on"]
        back = med(on["start_only_ms"]) - med(off["start_only_ms"])
        per_it_off, per_it_on = med(off["solve_ms"]) / max(1, off["iterations"]), (med(on["solve_ms"]) - back) / max(1, on["iterations"])
        lines += [
            "%s -- %s" % (name, CONFIGS[name]),
            "  mb %d, nnzbA %d, nnzbX %d, %d x %d '%s', buffer %.3f GB off | %.3f GB on" % (
                r["mb"], r["nnzbA"], r["nnzbX"], r["LM"], r["LN"], r["precision"], off["buffer_bytes"] * 1e-9, on["buffer_bytes"] * 1e-9),
            "  off: status %d, %3d iterations, residual %.3e, %9.3f ms per solve [%.3f .. %.3f]" % (
                off["status"], off["iterations"], off["residual"], med(off["solve_ms"]), min(off["solve_ms"]), max(off["solve_ms"])),
            "  on : status %d, %3d iterations, residual %.3e, %9.3f ms per solve [%.3f .. %.3f], %d unit rows" % (
                on["status"], on["iterations"], on["residual"], med(on["solve_ms"]), min(on["solve_ms"]), max(on["solve_ms"]), on["n_identity"]),
            "  time per solve on / off = %.3f, iterations on / off = %.3f; ms per iteration off %.3f | on %.3f (back transform taken out)" % (
                med(on["solve_ms"]) / med(off["solve_ms"]), on["iterations"] / max(1, off["iterations"]), per_it_off, per_it_on),
            "  set-up (inversion + scaling of A), once per setMatrix('A'): %.3f ms warm (median of %d; the first one on the plan, with its allocation: %.3f ms)" % (
                med(on["setup_ms"]), len(on["setup_ms"]), on["setup_ms_first"]),
            "  back transform, once per solve: %.3f ms (start-only solve on %.3f - off %.3f ms)" % (back, med(on["start_only_ms"]), med(off["start_only_ms"])),
            "  set-up + back transform = %.2f iterations of the plain solve" % ((med(on["setup_ms"]) + back) / per_it_off), ""]
        if args.parent_tree:
            runs = []
            for k in range(2):
                for tag, tree in (("parent", args.parent_tree), ("this", ROOT)):
                    runs.append((tag, med(child(name, tree, args.reps, True)["off"]["solve_ms"])))
            p, t = [v for tag, v in runs if tag == "parent"], [v for tag, v in runs if tag == "this"]
            spread = abs(p[0] - p[1])
            lines += [
                "  plain solve in fresh processes, alternating: parent commit %.3f, %.3f ms | this tree, preconditioner off %.3f, %.3f ms" % (p[0], p[1], t[0], t[1]),
                "  run-to-run spread of the parent %.3f ms (%.2f %%); this tree - parent (means) %+.3f ms (%+.2f %%)" % (
                    spread, 100 * spread / statistics.mean(p), statistics.mean(t) - statistics.mean(p),
                    100 * (statistics.mean(t) - statistics.mean(p)) / statistics.mean(p)), ""]
        print("\n".join(lines[-12:]), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
