#!/usr/bin/env python3
"""What the two-shape conversions of a padded plan cost (include/tfqmrgpu_ext.h section 18), on one GPU -> profiles/padded_plans.txt

  python scripts/padded_plans.py [--reps 9] [--nx 40] [--ny 30] [--small] [--revision REV] [--out FILE]

On 25 x 25 -> 32 x 32 and 9 x 9 -> 16 x 16, 'z', a 2-D block stencil of nx x ny block rows with 3 dense block columns of X (some thousand
blocks).  Two plans per shape: the PADDED plan of the caller's shape, and the YARDSTICK, a plan of the plan's shape without the switch
that is fed operands padded by hand.  Timed on both, interleaved layout, no transposition:
  setMatrix('X') / getMatrix('X') with host arrays     padded plan: the compact array.  Yardstick: the padded array -- the same call
                                                       on the conversion kernel that existed before --, and next to it what numpy
                                                       takes to pad (set) or to cut out (get) the array on the host
  setMatrix('X') / getMatrix('X') with device arrays   the conversion kernel alone: k_convert_pad against k_convert
  one iteration                                        solve(1e-30, 8) on both plans, per iteration; the same launches on the same
                                                       bytes, so the two must agree within the spread
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median and the spread (min ... max) of --reps rounds; padded plan and yardstick alternate inside a round, so that they see
the same machine.  Record only: no threshold decides anything.
--small: 8 x 6 block rows -- for trying the script out, not for figures.
--revision: written into the file; default `git rev-parse --short HEAD` of this tree."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nx", type=int, default=40)
    ap.add_argument("--ny", type=int, default=30)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "padded_plans.txt"))
    args = ap.parse_args()
    rev = args.revision or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    nx, ny = (8, 6) if args.small else (args.nx, args.ny)

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import pad_ref as PD
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd import problems as PR
    sync = torch.cuda.synchronize

    def timed(fn):
        sync(); t0 = time.perf_counter(); out = fn(); sync()
        return (time.perf_counter() - t0) * 1e3, out

    def fmt(ts):
        return "%9.3f ms  (%.3f ... %.3f)" % (statistics.median(ts), min(ts), max(ts))

    lines = ["padded plans: two-shape conversions against padding by hand (scripts/padded_plans.py), revision %s" % rev,
             "device: %s; 'z', interleaved layout, no transposition; stencil of %d x %d block rows, 3 dense block columns of X" % (torch.cuda.get_device_name(0), nx, ny),
             "median (min ... max) of %d rounds after 2 warm-up rounds; host clock around the call plus a device synchronise" % args.reps, ""]
    for lm, ln in ((25, 25), (9, 9)):
        LM, LN = PD.plan_shape(lm, ln)
        pr = PR.stencil_2d(nx, ny, lm, ln, 3, seed=lm)
        wide = PD.pad_problem(pr, LM, LN)
        rng = np.random.default_rng(lm)
        X = rng.standard_normal((pr.nnzbX, lm, ln)) + 1j * rng.standard_normal((pr.nnzbX, lm, ln))
        p, y = T.Solver(), T.Solver()
        p.create_plan(pr)
        p.allow_padding(True)
        nbytes = p.buffer_size(lm, ln, "z")
        p.set_buffer(nbytes=nbytes)
        y.create_plan(wide); y.set_buffer(nbytes=y.buffer_size(LM, LN, "z"))
        for s, q in ((p, pr), (y, wide)):
            s.set_matrix("A", q.A)
            s.set_matrix("B", q.B)
        Xd, Xwide_d = torch.from_numpy(X).cuda(), torch.from_numpy(PD.pad_blocks(X, LM, LN)).cuda()
        keep = {}

        def host_pad():
            keep["wide"] = PD.pad_blocks(X, LM, LN)

        def host_cut():
            keep["cut"] = np.ascontiguousarray(keep["got"][:, :lm, :ln])

        def y_get():
            keep["got"] = y.get_matrix()

        cases = [
            ("setMatrix('X'), host array,   padded plan", lambda: p.set_matrix("X", X)),
            ("setMatrix('X'), host array,   yardstick  ", lambda: y.set_matrix("X", keep["wide"])),
            ("   numpy pads the array on the host      ", host_pad),
            ("getMatrix('X'), host array,   padded plan", lambda: p.get_matrix()),
            ("getMatrix('X'), host array,   yardstick  ", y_get),
            ("   numpy cuts the inside out on the host ", host_cut),
            ("setMatrix('X'), device array, padded plan", lambda: p.set_matrix_device("X", Xd.data_ptr())),
            ("setMatrix('X'), device array, yardstick  ", lambda: y.set_matrix_device("X", Xwide_d.data_ptr())),
            ("getMatrix('X'), device array, padded plan", lambda: p.get_matrix_device(Xd.data_ptr())),
            ("getMatrix('X'), device array, yardstick  ", lambda: y.get_matrix_device(Xwide_d.data_ptr())),
            ("one iteration (solve(1e-30, 8) / iterations), padded plan", lambda: p.solve(1e-30, 8)),
            ("one iteration (solve(1e-30, 8) / iterations), yardstick  ", lambda: y.solve(1e-30, 8)),
        ]
        host_pad()
        times = {name: [] for name, _ in cases}
        for rnd in range(args.reps + 2):
            for name, fn in cases:
                t, _ = timed(fn)
                if rnd >= 2:
                    its = (p if "padded" in name else y).get_info()["iterations"] if name.startswith("one iteration") else 1
                    times[name].append(t / max(1, its))
            p._keep.clear(); y._keep.clear()
        same = np.array_equal(p.get_matrix(), PD.inside(y.get_matrix(), lm, ln)) and p.get_info()["iterations"] == y.get_info()["iterations"]
        lines.append("%d x %d on %d x %d: %d blocks of X, %.1f MB compact, %.1f MB padded (%.2f x); buffer %.1f MB; X of the two plans equal after the solves: %s"
                     % (lm, ln, LM, LN, pr.nnzbX, X.nbytes / 1e6, X.nbytes / 1e6 * LM * LN / (lm * ln), LM * LN / (lm * ln),
                        nbytes / 1e6, same))
        for name, _ in cases:
            lines.append("  %-52s %s" % (name, fmt(times[name])))
        lines.append("")
        p.close(); y.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
