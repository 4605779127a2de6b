"""Worker of tests/test_gpu_late_v5.py: the solves of one fixture in a fresh process, written to argv[1].  The library is chosen as
tests/_env_worker.py chooses it: with TFQMRGPU_* tuning switches in the environment the LAB build (libtfQMRgpu_lab.so, tfq_switch.hpp),
without any the product.
argv: out.npz fixture threshold mode[,mode ...]
fixture: a name that _env_worker.problem takes, or `breakdown:<kind:shape>` of tests/breakdown_cases.py (solved with its own shadow vector,
threshold and iteration cap: the mode is `solve`).
modes, each written as `<mode>/status`, `/iterations`, `/residual`, `/history`, `/X`, `/probes`:
  solve   a cold solve to the threshold
  one     a cold solve of one iteration (only the first-iteration kernel instances run)
  from    a cold solve to 1e-3, then tfqmrgpuExt_solveFrom on the same plan to the threshold (the arrays are the warm solve's)
and once per file: `late` (tfqmrgpuExt_getLateV5), `family` (tfqmrgpuExt_getMultiplyKernel), `lib`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def record(out, mode, s, status):
    info = s.get_info()
    out.update({mode + "/status": status, mode + "/iterations": info["iterations"], mode + "/residual": info["residual"],
                mode + "/history": s.bound_history(), mode + "/X": s.get_matrix(), mode + "/probes": s.profile()["probe"][0]})


def main():
    out_path, name, tol, modes = sys.argv[1], sys.argv[2], float(sys.argv[3]), sys.argv[4].split(",")
    import torch
    assert torch.cuda.is_available(), "no GPU: the product has no CPU fallback"
    switches = [k for k in os.environ if k.startswith("TFQMRGPU_") and k != "TFQMRGPU_LIB"]
    if switches and "TFQMRGPU_LIB" not in os.environ:
        os.environ["TFQMRGPU_LIB"] = os.path.join(ROOT, "tfqmrgpu_amd", "lib", "libtfQMRgpu_lab.so")
    import tfqmrgpu_amd as T
    import _env_worker
    import breakdown_cases as BC
    assert os.path.basename(T.LIB_PATH) == ("libtfQMRgpu_lab.so" if switches else "libtfQMRgpu.so"), T.LIB_PATH
    case = BC.by_name(name[len("breakdown:"):]) if name.startswith("breakdown:") else None
    pr = case.pr if case else _env_worker.problem(name)
    out = {"lib": os.path.basename(T.LIB_PATH)}
    with T.Solver.open(pr, "z") as s:
        if case:
            assert T.lib.tfqmrgpuExt_setShadowVector(s.handle, s.plan, T._ptr(case.v3)) == 0
        out["late"], out["family"] = s.late_v5(), s.multiply_kernel()
        s.set_profiling(True)               # events on the solver's stream: the probes that did work are counted, no result moves
        s.load()
        for mode in modes:
            if mode == "solve":
                st = s.solve(BC.THRESHOLD["z"], BC.MAX_ITERATIONS["z"]) if case else s.solve(tol, 300)
            elif mode == "one":
                st = s.solve(tol, 1)
            elif mode == "from":
                assert s.solve(1e-3, 300) == 0
                st = s.solve_from(tol, 300)
            else:
                raise ValueError(mode)
            record(out, mode, s, st)
    np.savez(out_path, **out)


if __name__ == "__main__":
    main()
