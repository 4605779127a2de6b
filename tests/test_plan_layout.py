"""The byte count of the work buffer (tfqmrgpu_bsrsv_bufferSize: tfq_plan.cpp, layoutBuffer) for four block patterns, all 15 block
shapes and the three precisions, against the counts recorded from the library before layoutBuffer was split into its steps and the
index windows got one list (tests/golden/plan_layout_sizes.json).  The count is the end of the last window, so a window that moves or
changes its size moves it.  Host code only: bufferSize touches no device.

The recorded table was written by this file's main with the library of the commit in front of that change:
    TFQMRGPU_LIB=<that commit's libtfQMRgpu.so> python tests/test_plan_layout.py"""
import json
import os

import numpy as np

from conftest import GOLDEN, load_problem   # (first: it puts the repository on sys.path when this file runs as a script)
import tfqmrgpu_amd as T
from helpers import first_blocks, index_problem, unordered_pattern

TABLE = os.path.join(GOLDEN, "plan_layout_sizes.json")
PRECISIONS = "zcm"


def shapes():
    n = T.C.c_int32(0)
    arr = (T.C.c_int32 * 64)()
    assert T.lib.tfqmrgpu_bsrsv_allowedBlockSizes(T.C.byref(n), arr, 64) == 0 and n.value == 15
    return [(arr[2 * i], arr[2 * i + 1]) for i in range(15)]


def dense_columns_pattern(mb=512, ncols=8):
    """Identical dense block columns, 512 chunks at 8 x 8 `z` (8 blocks each): more than the 384 up to which a plan folds, so that this
    shape keeps its column batches and their launch order (Plan::colBatch, ChunkTable::orderB)"""
    rpA, ciA = [0], []
    for r in range(mb):
        ciA += [c for c in (r - 1, r, r + 1) if 0 <= c < mb]
        rpA.append(len(ciA))
    rpX, ciX = np.arange(mb + 1) * ncols, np.tile(np.arange(ncols), mb)
    return index_problem(rpA, ciA, rpX, ciX, *first_blocks(mb, rpX, ciX))


def problems():
    return {"fd_16x16_2d": load_problem("fd_16x16_2d"), "fd_8x8_3d": load_problem("fd_8x8_3d"),
            "plan_unordered.14-287-16": unordered_pattern(), "dense_columns_512x8": dense_columns_pattern()}


def buffer_sizes():
    out = {}
    for name, pr in problems().items():
        with T.Solver() as s:
            s.create_plan(pr)
            for lm, ln in shapes():
                for prec in PRECISIONS:
                    out["%s %dx%d %s" % (name, lm, ln, prec)] = s.buffer_size(lm, ln, prec)
    return out


def test_buffer_size_is_the_recorded_one():
    want = json.load(open(TABLE))
    got = buffer_sizes()
    assert len(want) == 4 * 15 * 3 and sorted(got) == sorted(want)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


if __name__ == "__main__":
    with open(TABLE, "w") as f:
        json.dump(buffer_sizes(), f, indent=0, sort_keys=True)
        f.write("\n")
