"""Writes profiles/warm_families.txt: per case of tests/warm_cases.py and iteration count k the oracle's spread and the allowance of
tests/test_gpu_warm_families.py (CPU oracle alone), and, given the output of that test on a GPU (pytest -s), the deviation it printed as a
fraction of the allowance.

    python scripts/warm_families.py [--gpu-log pytest_output.txt] [--out profiles/warm_families.txt]"""
import argparse
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import warm_cases as WC  # noqa: E402
from oracle import pyoracle  # noqa: E402


def gpu_fractions(path):
    """{(case id, k): worst fraction over the work vectors} from the lines 'warm families <id> k=<k>: ... worst <f> of the allowance'"""
    out = {}
    if path:
        for m in re.finditer(r"warm families (\S+) k=(\d+): .*?worst ([0-9.eE+-]+) of the allowance", open(path).read()):
            out[m.group(1), int(m.group(2))] = float(m.group(3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu-log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_families.txt"))
    a = ap.parse_args()
    pyoracle.lib()
    gpu = gpu_fractions(a.gpu_log)
    lines = ["# tests/warm_cases.py: the oracle's spread under the a-priori rounding bound of R, the allowance of tests/test_gpu_warm_families.py",
             "# (work vectors 4 ... 9 | work vector 1), the largest deviation on an MI355X as a fraction of the allowance, and the oracle seconds",
             "# of the case.  spread is computed at every k of the bound table.  scripts/warm_families.py writes this file.",
             "# %-36s %2s %10s %10s %10s %10s %8s" % ("case", "k", "spread", "allow 4-9", "allow 1", "gpu/allow", "seconds")]
    worst = {}
    for key in WC.EVERY_CASE:
        t0 = time.time()
        prec = WC.precision(key)
        for k in sorted(WC.BOUND[prec]):
            al = WC.allowance(pyoracle, key, k)
            f = gpu.get((WC.case_id(key), k))
            lines.append("%-38s %2d %10.3e %10.3e %10.3e %10s %8.1f" % (WC.case_id(key), k, WC.spread(pyoracle, key, k), al[4], al[1],
                                                                      "-" if f is None else "%.3e" % f, time.time() - t0))
            if f is not None and f > worst.get(prec, (0, None))[0]:
                worst[prec] = (f, "%s k=%d" % (WC.case_id(key), k))
            print(lines[-1], flush=True)
        WC.case.cache_clear(), WC.reference.cache_clear()
    for prec, (f, where) in sorted(worst.items()):
        lines.append("# worst '%s': %.3f of the allowance (%s)" % (prec, f, where))
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
