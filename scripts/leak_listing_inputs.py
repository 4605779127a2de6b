#!/usr/bin/env python3
"""Inputs of scripts/leak_listing_check.cpp: the patterns of the problems of tests/test_gpu_truncation_leak.py (tests 1 and 3) as plain,
zero-based index arrays, with the counts that tests/leak_ref.py expects (Python sets; not the library's listing).

  python scripts/leak_listing_inputs.py <directory>        writes one <name>.txt per problem and prints the file names"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def unit_products(LM, LN):
    return min(64, max(16, 4096 // (LM * LN)))                      # tfq_leak_host.cpp: leak_unit_products


def write(path, pr, max_products):
    import leak_ref as LR
    off = pr.index_offset
    rowsA = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    rowsX = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))
    columns, colsX = np.unique(pr.colIndX, return_inverse=True)
    i2u = np.lexsort((np.arange(pr.nnzbX), rowsX, colsX))           # the internal order: by (column, row), stable
    u2i = np.empty(pr.nnzbX, np.int64)
    u2i[i2u] = np.arange(pr.nnzbX)
    blocks, pairs = LR.counts(pr)
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d\n" % (pr.mb, len(columns), pr.nnzbA, pr.nnzbX, max_products, blocks, pairs))
        for a in (rowsA, pr.colIndA - off, rowsX, colsX, u2i):
            f.write(" ".join(str(int(v)) for v in a) + "\n")


def main():
    from tfqmrgpu_amd import problems as PR
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    cases = {"every_shape_%dx%d" % (LM, LN): (PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN, radius=[None, 1.1, 2.3]), unit_products(LM, LN))
             for LM, LN in ((4, 4), (16, 16), (64, 64))}
    cases["long_shell"] = (PR.stencil_2d(40, 40, 4, 4, ncols=2, seed=40, radius=24.5, points=13), unit_products(4, 4))
    cases["long_shell_units_of_1"] = (cases["long_shell"][0], 1)
    for name, (pr, max_products) in cases.items():
        path = os.path.join(out, name + ".txt")
        write(path, pr, max_products)
        print(path)


if __name__ == "__main__":
    main()
