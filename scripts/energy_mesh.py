#!/usr/bin/env python
"""Energy mesh (include/tfqmrgpu_ext.h section 19) on the 16 x 16 FD example: a 16-point mesh on a semicircle in the upper half plane,
in 'z' and 'm'.  Records, not thresholds (profiles/energy_mesh.txt):
  - iterations and time per energy for cold solves, for refine_from from the last X (depth 0) and with 1 ... 4 kept starts projected;
  - shift_diagonal against set_blocks('A') of the same diagonal blocks from host arrays;
  - add_to_sum against get_blocks() plus a numpy accumulation.
usage: python scripts/energy_mesh.py [--out profiles/energy_mesh.txt] [--problem tests/golden/fd_16x16_2d.xml]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import tfqmrgpu_amd as T  # noqa: E402
from tfqmrgpu_amd import problems as PR  # noqa: E402

NE, RADIUS, REPS = 16, 5e-3, 50


def mesh_points():
    """sigma_k = R exp(i theta_k), theta_k = pi (k + 1/2) / NE, and the midpoint weights dz_k of the contour integral"""
    theta = np.pi * (np.arange(NE) + 0.5) / NE
    sigma = RADIUS * np.exp(1j * theta)
    return sigma, 1j * sigma * (np.pi / NE)


def opened(pr, prec, depth=0):
    s = T.Solver()
    s.create_plan(pr)
    nbytes = s.buffer_size(pr.LM, pr.LN, prec)
    if depth:
        s.keep_starts(depth)
    s.keep_sum(True)
    s.set_buffer(nbytes=nbytes)
    s.set_matrix("A", pr.A)
    s.set_matrix("B", pr.B)
    return s


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def run_mesh(pr, prec, sigma, weight, mode, depth, thr):
    """the loop of solve_mesh, written out so that every energy can be timed: (iterations, ms) per energy"""
    its, ms = [], []
    with opened(pr, prec, depth) as s:
        for e in range(NE):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.shift_diagonal(sigma[e])
            if mode == "cold" or e == 0:
                s.solve(thr, 2000)
            else:
                if s.start_count() > 0:
                    T._check(T.lib.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None), "tfqmrgpuExt_projectStart")
                s.refine_from(thr, 2000)
            if depth:
                s.push_start()
            s.add_to_sum(weight[e])
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            its.append(s.get_info()["iterations"])
        # the same mesh in one call, from a cold first energy
        s.clear_sum()
        if depth:
            s.keep_starts(0), s.keep_starts(depth)
        t0 = time.perf_counter()
        out = s.solve_mesh(sigma, weight, thr, 2000) if mode != "cold" else None
        torch.cuda.synchronize()
        one_call = (time.perf_counter() - t0) * 1e3 if out is not None else None
    return its, ms, one_call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_mesh.txt"))
    ap.add_argument("--problem", default=os.path.join(ROOT, "tests", "golden", "fd_16x16_2d.xml"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    pr = PR.read_xml(args.problem)
    sigma, weight = mesh_points()
    lines = ["energy mesh on %s: mb %d, nnzbA %d, nnzbX %d, nnzbB %d, blocks %d x %d, threshold %.1e, %s" % (
        os.path.basename(args.problem), pr.mb, pr.nnzbA, pr.nnzbX, pr.nnzbB, pr.LM, pr.LN, pr.tolerance, torch.cuda.get_device_name(0)),
        "mesh: sigma_k = %.1e exp(i pi (k + 1/2) / %d), k = 0 ... %d; weights i sigma_k pi / %d" % (RADIUS, NE, NE - 1, NE)]
    lines += ["  sigma[%2d] = %+.6e %+.6ej" % (k, z.real, z.imag) for k, z in enumerate(sigma)]
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    diag = np.flatnonzero(rows == pr.colIndA.astype(np.int64) - pr.index_offset)
    for prec in "zm":
        lines.append("")
        lines.append("== precision '%s'" % prec)
        for mode, depth in [("cold", 0), ("fromX", 0), ("fromX", 1), ("fromX", 2), ("fromX", 3), ("fromX", 4)]:
            its, ms, one = run_mesh(pr, prec, sigma, weight, mode, depth, pr.tolerance)
            lines.append("%-5s depth %d: iterations %s  sum %d" % (mode, depth, " ".join("%3d" % i for i in its), sum(its)))
            lines.append("               ms/energy %s  sum %.2f%s" % (" ".join("%5.2f" % t for t in ms), sum(ms),
                                                                      "" if one is None else "  | solve_mesh, one call: %.2f ms" % one))
        with opened(pr, prec) as s:
            shifted = pr.A[diag] + sigma[0] * np.eye(pr.LM)
            t_shift = timed(lambda: s.shift_diagonal(sigma[0]))
            t_set = timed(lambda: s.set_blocks("A", diag, shifted))
            t_form = timed(lambda: pr.A[diag] + sigma[0] * np.eye(pr.LM))
            lines.append("shift_diagonal %.4f ms | set_blocks('A') of the %d diagonal blocks from a host array %.4f ms (+ %.4f ms to form them in numpy)" % (
                t_shift, len(diag), t_set, t_form))
            s.solve(pr.tolerance, 2000)
            acc = np.zeros((pr.nnzbB, pr.LM, pr.LN), np.complex128)

            def host_sum():
                nonlocal acc
                acc = acc + weight[0] * s.get_blocks()
            t_add = timed(lambda: s.add_to_sum(weight[0]))
            t_host = timed(host_sum)
            lines.append("add_to_sum %.4f ms | get_blocks() + numpy accumulation of the %d blocks %.4f ms" % (t_add, pr.nnzbB, t_host))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
