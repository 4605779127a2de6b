#!/usr/bin/env python3
"""What tfqmrgpuExt_selectDrop and tfqmrgpuExt_selectLeak (include/tfqmrgpu_ext.h section 20) cost against the host route they replace,
on one GPU -> profiles/select.txt

  python scripts/select_calls.py [--reps 9] [--small] [--parent DIR] [--revision REV] [--out FILE]

On the headline workload of bench.py (generate_FD_example 16 120 4 2 -0.25: 16 x 16, 138 229 blocks of X) as a 'z', a 'c' and an 'm' plan,
after one solve ('c': no solve -- the float solve of this workload does not reach 1e-4 in 2000 iterations; the X of the 'z' solve is set
instead), in one process:
  the host route (a)   dropCost(cost2) | residual() | the rule of selectDrop in numpy on what they returned: the list | spent
  the host route (b)   leakMap(pos2) | the rule of selectLeak in numpy: the list | left
  this change          selectDrop and selectLeak, one C call each with room for every index, all three outputs; and the count alone
--parent DIR: the tfqmrgpu_amd package of the parent commit, built (DIR/__init__.py, DIR/lib/libtfQMRgpu.so).  The host route then runs
on THAT library, on a plan of its own with the same A, B and X, in the same process and the same rounds; without it the host route runs
on this tree's library, whose dropCost, residual and leakMap make the launches and copies they made before.
eta: the median over the blocks without B of the smallest eta that lets a block go (the positions: of the largest eta that still takes
one), so that about half are selected; the lists of the two routes are compared entry for entry.
Each figure is the host clock around the call plus a device synchronise (the device is synchronised before as well), after two warm-up
rounds, the median of --reps rounds; the calls alternate inside a round, so that they see the same machine.  The spread of a figure is
its [min .. max] over the rounds.
--small: generate_FD_example 6 24 4 2 -0.25 -- for trying the script out, not for figures."""
import argparse
import ctypes as C
import importlib.util
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
    ap.add_argument("--parent")
    ap.add_argument("--revision")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select.txt"))
    args = ap.parse_args()
    rev = args.revision or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU; there is no CPU fallback"
    torch.cuda.set_device(0)
    import tfqmrgpu_amd as T
    from tfqmrgpu_amd.fd_generator import FDExample
    TP = T
    if args.parent:
        spec = importlib.util.spec_from_file_location("tfqmrgpu_amd_parent", os.path.join(args.parent, "__init__.py"))
        TP = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(TP)
        assert not hasattr(TP.lib, "tfqmrgpuExt_selectDrop"), "--parent names a library that has the new calls"
    sync = torch.cuda.synchronize
    gen = (6, 24, 4, 2, -0.25, 4) if args.small else (16, 120, 4, 2, -0.25, 4)
    pr = FDExample(*gen).problem()
    name = "generate_FD_example %s" % " ".join(str(g) for g in gen[:5])
    ptr = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731

    def timed(fn):
        sync(); t0 = time.perf_counter(); fn(); sync()
        return (time.perf_counter() - t0) * 1e3

    def ok(status):
        assert status == 0, T.error_string(status)

    lines = [
        "tfqmrgpuExt_selectDrop and tfqmrgpuExt_selectLeak against the host route, one MI355X; written by scripts/select_calls.py (method: its docstring).",
        "revision %s; the host route on %s.  ms: median [min .. max] of %d rounds after 2 warm-ups, the calls alternating;"
        % (rev, "the parent commit's library, a plan of its own in the same process" if args.parent else "this tree's library, the same plan", args.reps),
        "host clock around the call + device synchronise.", ""]
    kept_x = None
    for prec, tol in (("z", 1e-9), ("c", None), ("m", 1e-9)):
        with T.Solver.open(pr, prec).load() as s, (TP.Solver.open(pr, prec).load() if args.parent else T.Solver()) as host:
            if tol is None:
                s.set_matrix("X", kept_x)
                st, info = -1, dict(iterations=0, residual=float("nan"))
            else:
                st = s.solve(tol, 2000)
                info = s.get_info()
                if kept_x is None:
                    kept_x = s.get_matrix()
            if args.parent:
                host.set_matrix("X", s.get_matrix())
            else:
                host = s
            hlib = TP.lib
            view = s.plan_view()
            n_cols, n_x, LN = int(view["nCols"]), int(view["nnzbX"]), pr.LN
            n_pos = host.leak_counts()[0]
            cols = np.unique(pr.colIndX, return_inverse=True)[1]
            subset = view["subset"].astype(np.int64)
            pos_cols = host.leak_map(values=False)["cols"].astype(np.int64)
            cost2, pos2 = np.zeros((n_x, LN)), np.zeros((n_pos, LN))
            r2, b2 = np.zeros((n_cols, LN)), np.zeros((n_cols, LN))
            columns, worst = np.zeros(n_cols, np.int32), C.c_double(0)
            count, nb = C.c_uint64(0), C.c_uint64(0)
            blocks, take = np.zeros(n_x, np.int32), np.zeros(max(1, n_pos), np.uint64)
            spent, left = np.zeros((n_cols, LN)), np.zeros((n_cols, LN))
            n_drop, n_take = C.c_uint64(0), C.c_uint64(0)
            out = {}

            def rule_drop(eta):
                with np.errstate(invalid="ignore"):
                    sel = np.all(cost2 <= (np.float64(eta) * np.float64(eta)) * b2[cols], axis=1)
                sel[subset] = False
                out["blocks"] = np.flatnonzero(sel).astype(np.int32)

            def sums_drop():
                out["spent"] = np.zeros((n_cols, LN))
                np.add.at(out["spent"], cols[out["blocks"]], np.sqrt(cost2[out["blocks"]]))

            def rule_leak(eta):
                b = b2[pos_cols]
                with np.errstate(invalid="ignore"):
                    out["hit"] = np.any((b > 0) & (pos2 > (np.float64(eta) * np.float64(eta)) * b), axis=1)
                out["take"] = np.flatnonzero(out["hit"]).astype(np.uint64)

            def sums_leak():
                stay = np.flatnonzero(~out["hit"])
                out["left"] = np.zeros((n_cols, LN))
                np.add.at(out["left"], pos_cols[stay], pos2[stay])

            host_calls = {
                "dropCost(cost2)": lambda: ok(hlib.tfqmrgpuExt_dropCost(host.handle, host.plan, ptr(cost2), None, C.byref(count))),
                "residual()": lambda: ok(hlib.tfqmrgpuExt_residual(host.handle, host.plan, ptr(r2), ptr(b2), ptr(columns), C.byref(worst))),
                "leakMap(pos2)": lambda: ok(hlib.tfqmrgpuExt_leakMap(host.handle, host.plan, n_pos, None, None, ptr(pos2), C.byref(nb))),
            }
            for fn in host_calls.values():
                fn()
            with np.errstate(divide="ignore", invalid="ignore"):
                b = b2[cols]
                need = np.sqrt(np.nanmax(np.where(b > 0, cost2 / b, np.where(cost2 > 0, np.inf, 0.0)), axis=1))
                b = b2[pos_cols]
                reach = np.sqrt(np.nanmax(np.where(b > 0, pos2 / b, 0.0), axis=1)) if n_pos else np.zeros(0)
            free = np.setdiff1d(np.arange(n_x), subset)
            eta_drop = float(np.median(need[free])) * (1 + 1e-9)
            eta_leak = float(np.median(reach)) if n_pos else 0.0
            calls = dict(host_calls)
            calls.update({
                "numpy rule, drop list": lambda: rule_drop(eta_drop),
                "numpy spent": sums_drop,
                "numpy rule, take list": lambda: rule_leak(eta_leak),
                "numpy left": sums_leak,
                "selectDrop": lambda: ok(T.lib.tfqmrgpuExt_selectDrop(s.handle, s.plan, eta_drop, n_x, ptr(blocks), C.byref(n_drop), ptr(spent))),
                "selectDrop, count only": lambda: ok(T.lib.tfqmrgpuExt_selectDrop(s.handle, s.plan, eta_drop, 0, None, C.byref(n_drop), None)),
                "selectLeak": lambda: ok(T.lib.tfqmrgpuExt_selectLeak(s.handle, s.plan, eta_leak, n_pos, ptr(take), C.byref(n_take), ptr(left))),
                "selectLeak, count only": lambda: ok(T.lib.tfqmrgpuExt_selectLeak(s.handle, s.plan, eta_leak, 0, None, C.byref(n_take), None)),
            })
            first = {k: timed(calls[k]) for k in ("selectDrop", "selectLeak")}      # lists, upload, allocation + the call itself
            ms = {k: [] for k in calls}
            for rep in range(2 + args.reps):
                for k, fn in calls.items():
                    t = timed(fn)
                    if rep >= 2:
                        ms[k].append(t)
            calls["selectDrop"](); calls["selectLeak"]()
            same_lists = bool(np.array_equal(blocks[:n_drop.value], out["blocks"]) and np.array_equal(take[:n_take.value], out["take"]))
            with np.errstate(divide="ignore", invalid="ignore"):
                dev_spent = float(np.nanmax(np.where(out["spent"] > 0, np.abs(spent - out["spent"]) / out["spent"], 0.0)))
                dev_left = float(np.nanmax(np.where(out["left"] > 0, np.abs(left - out["left"]) / out["left"], 0.0)))
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%s, %d x %d '%s': nnzbA %d, nnzbX %d, nCols %d, leak positions %d; solve: status %d, %d iterations, residuum_reached %.3e"
                     % (name, pr.LM, pr.LN, prec, pr.nnzbA, n_x, n_cols, n_pos, st, info["iterations"], info["residual"]))
        lines.append("  records: cost2 %.3f MB, pos2 %.3f MB; copied out by selectDrop %.3f MB, by selectLeak %.3f MB"
                     % (n_x * LN * 8e-6, n_pos * LN * 8e-6, (n_x * 4 + n_cols * LN * 8 + 4) * 1e-6, (n_pos * 4 + n_cols * LN * 8 + 4) * 1e-6))
        lines.append("  eta (drop) %.3e: %d of %d blocks without B selected; eta (leak) %.3e: %d of %d positions selected"
                     % (eta_drop, n_drop.value, len(free), eta_leak, n_take.value, n_pos))
        lines.append("  the lists of the two routes: %s; spent, left: largest relative deviation from the numpy sums %.2e, %.2e"
                     % ("the same entries" if same_lists else "DIFFERENT", dev_spent, dev_left))
        for k in calls:
            lines.append("  %-24s %9.3f ms [%.3f .. %.3f]" % (k, med[k], min(ms[k]), max(ms[k])))
        a = med["dropCost(cost2)"] + med["residual()"] + med["numpy rule, drop list"] + med["numpy spent"]
        b = med["leakMap(pos2)"] + med["numpy rule, take list"] + med["numpy left"]
        lines.append("  route (a) dropCost(cost2) + residual() + numpy %.3f ms | selectDrop %.3f ms | selectDrop / dropCost(cost2) alone %.2f"
                     % (a, med["selectDrop"], med["selectDrop"] / med["dropCost(cost2)"]))
        lines.append("  route (b) leakMap(pos2) + numpy %.3f ms (+ residual() for bnorm2) | selectLeak %.3f ms | selectLeak / leakMap(pos2) alone %.2f"
                     % (b, med["selectLeak"], med["selectLeak"] / med["leakMap(pos2)"]))
        lines.append("  first selectDrop call %.3f ms, first selectLeak call %.3f ms (lists, upload, allocation, one more synchronise)"
                     % (first["selectDrop"], first["selectLeak"]))
        lines.append("")
        print("\n".join(lines[-(len(calls) + 9):]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
