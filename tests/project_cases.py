"""Planted inputs of tests/test_gpu_project_shapes.py, importable without a GPU; tests/test_project_cases_cpu.py checks on the CPU reference
(tests/project_ref.py) that every one of them is a fair question: no pivot ratio near the threshold, the planted coefficients recovered,
coefficients that no permutation can hide, and a chunk table on the intended side of each edge.

A case needs no solve.  Its starts are arbitrary arrays, S_i = stored(uniform + 1j uniform), and its right-hand side is built from their images:
B = sum_i c_i trunc(A S_i) + 0.05 noise on the FULL pattern of X, with a coefficient c[column, right-hand side, start] of its own for every
triple.  The minimiser gamma is then c up to the noise: a mix-up of right-hand sides, starts, planes or Re / Im is an error of order one, not of
rounding size.  Variants: B on every second X block only ("half": both branches of ld_b_under_x in one chunk; gamma is then no longer c), S_1
equal to S_0 in the odd right-hand sides ("dup": the pivot rule decides differently inside one column), a zero column of B.

The coefficients are not drawn independently: 768 independent points in the annulus 0.5 <= |c| < 1.9 come as close as 4e-3, inside 1000 float
allowances.  They are the points of a hexagonal lattice of spacing 0.1 in that annulus, taken in hashed order: every modulus in [0.5, 1.9), the
phases all over the circle, and any two at least 0.1 apart."""
import functools
from types import SimpleNamespace

import numpy as np

import project_ref as P
import residual_ref as RR
import tfqmrgpu_amd as T
from precond_ref import _product
from tfqmrgpu_amd import problems as PR

SHAPES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64), (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]
SPACING = 0.1            # of the coefficient lattice
NOISE = 0.05
KEPT_RATIO_MIN = 0.25    # every kept pivot ratio of every case
PLANTED_MAX = 0.05       # |gamma_ref - c| on the full pattern


# ---- the plan's chunk rule (tfq_plan.cpp: cutChunks), restated -------------------------------------------------------------------------------
def block_bytes(LM, LN, prec):
    """one block of X in the storage type of the plan's iteration vectors: double for 'z', float for 'c' and 'm'"""
    return 2 * LM * LN * (8 if prec == "z" else 4)


def blocks_per_chunk(pr, prec):
    """CH: a chunk is at most `target` bytes of blocks of one column, target = X / 4096 kept within 8 ... 16 KiB -- 8 KiB for every X below 32 MiB,
    so for every test -- and at least one block; shapes of the MFMA multiply take at least four strips of 16 | 32 rows (tfq_plan.hpp: mfma_units)"""
    real = 8 if prec == "z" else 4
    block = block_bytes(pr.LM, pr.LN, prec)
    target = min(max(pr.nnzbX * block // 4096, 8 * 1024), 16 * 1024)
    CH = max(1, target // block)
    if pr.LM % 16 == 0 and pr.LN % 16 == 0:
        mt = pr.LM // 16
        per_block = mt // (2 if (mt % 2 == 0 and 2 * (pr.LN // 16) * real <= 32) else 1)
        CH = max(CH, -(-4 // per_block))
    return CH


def chunk_lengths(pr, prec):
    """per compressed block column: the blocks of each of its chunks, in order"""
    CH = blocks_per_chunk(pr, prec)
    cols = np.asarray(pr.colIndX, dtype=np.int64) - pr.index_offset
    return [[min(CH, int(n) - b) for b in range(0, int(n), CH)] for n in np.bincount(np.unique(cols, return_inverse=True)[1])]


def items_per_block(LM, LN, prec):
    """vector items per block plane of the projection kernels (tfq_stream.hpp: Geo::IPB): 16 bytes of the type X is HELD in, double for 'm'"""
    return LM * LN // (4 if prec == "c" else 2)


def lanes(LN):
    """tfq_stream.hpp: Geo::T"""
    return (256 // LN) * LN


# ---- values --------------------------------------------------------------------------------------------------------------------------------
def coefficients(seed, shape):
    pts = []
    for r, y in enumerate(np.arange(-1.9, 1.9, SPACING * np.sqrt(3.0) / 2)):
        pts.append(np.arange(-1.9, 1.9, SPACING) + (SPACING / 2 if r % 2 else 0.0) + 1j * y)
    pts = np.concatenate(pts)
    pts = pts[(np.abs(pts) >= 0.5) & (np.abs(pts) < 1.9)]
    n = int(np.prod(shape))
    assert n <= len(pts), (n, len(pts))
    order = np.argsort(PR.hashed_uniform(seed, (len(pts),)), kind="stable")
    return pts[order[:n]].reshape(shape)


def _noise(seed, shape):
    return PR.hashed_uniform(seed, shape) + 1j * PR.hashed_uniform(seed + 1, shape)


def build(oracle, pr0, prec, K, seed, variant="full", zero=None):
    """pr0: A and the pattern of X (its B is ignored).  Returns a namespace: pr (the Problem with the planted B), prec, K, starts (newest first),
    c [nCols, LN, K], A and B as the plan stores them, keep (the X block under each B block), variant"""
    LM, LN, nX = pr0.LM, pr0.LN, pr0.nnzbX
    off = pr0.index_offset
    assert off == 0
    keep = np.arange(0, nX, 2 if variant == "half" else 1)
    rows = np.repeat(np.arange(pr0.mb), np.diff(pr0.rowPtrX))
    rpB = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=pr0.mb))])
    pr = T.Problem(pr0.rowPtrA, pr0.colIndA, pr0.A, pr0.rowPtrX, pr0.colIndX, rpB, pr0.colIndX[keep], np.zeros((len(keep), LM, LN)), None,
                   pr0.tolerance, 0)
    an = oracle.analyse(pr)
    assert an["status"] == 0 and np.array_equal(an["subset"].astype(np.int64), keep)
    col = an["colindx"].astype(np.int64)
    starts = [RR.stored(_noise(seed + 10 * i, (nX, LM, LN)), prec) for i in range(K)]
    if variant == "dup":
        starts[1][:, :, 1::2] = starts[0][:, :, 1::2]
    c = coefficients(seed + 7, (an["nCols"], LN, K))
    A = RR.stored(pr.A, prec)
    Bx = NOISE * _noise(seed + 5, (nX, LM, LN))
    for i, S in enumerate(starts):
        Bx += c[col, :, i][:, None, :] * _product(an, pr, A, S)
    pr.B = np.ascontiguousarray(Bx[keep])
    if zero is not None:
        pr.B[col[keep] == zero[0], :, zero[1]] = 0
    return SimpleNamespace(pr=pr, prec=prec, K=K, starts=starts, c=c, A=A, B=RR.stored(pr.B, prec), keep=keep, variant=variant, zero=zero)


# ---- patterns ------------------------------------------------------------------------------------------------------------------------------
def base_pattern(LM, LN):
    """4 x 4 grid, three block columns of 16, 4 and 8 blocks"""
    return PR.stencil_2d(4, 4, LM, LN, ncols=3, seed=100 * LM + LN, radius=[None, 1.1, 2.3])


PATTERNS = {
    # name: (pattern, what it is there for)
    "long": lambda LM, LN: PR.stencil_2d(40, 40, LM, LN, ncols=2, seed=4040),          # two columns of 1600 blocks
    "long_short_end": lambda LM, LN: PR.stencil_2d(41, 39, LM, LN, ncols=2, seed=4139),   # ... of 1599: a last chunk one block short
    "dense_9x8": lambda LM, LN: PR.stencil_2d(9, 8, LM, LN, ncols=1, seed=908),         # one column of 72 blocks
    "dense_17x8": lambda LM, LN: PR.stencil_2d(17, 8, LM, LN, ncols=1, seed=1708),      # one column of 136 blocks
    "single": lambda LM, LN: PR.stencil_2d(4, 4, LM, LN, ncols=2, seed=404, radius=[None, 0.5]),   # a column of ONE block
}

# a case that misses a condition of tests/test_project_cases_cpu.py gets another seed here, never another condition
SEED_SHIFT = {
    # four starts on a column of ONE 4 x 4 block are four vectors in four dimensions per right-hand side: most seeds give a pivot ratio below 0.25
    ("single", 4, 4, "z", 4, "full"): 422,
}


@functools.lru_cache(maxsize=None)
def case(oracle, pattern, LM, LN, prec, K, variant="full", zero=None):
    """pattern: "base" or a name of PATTERNS.  'm' plans hold A, B and X in double: their case is that of 'z' (the chunk table is not)"""
    store = "z" if prec == "m" else prec
    pr0 = base_pattern(LM, LN) if pattern == "base" else PATTERNS[pattern](LM, LN)
    key = (pattern, LM, LN, store, K, variant)
    seed = 64 * (100 * LM + LN) + 1000003 * SEED_SHIFT.get(key, 0)
    return build(oracle, pr0, store, K, seed, variant, zero)


@functools.lru_cache(maxsize=None)
def reference(oracle, pattern, LM, LN, prec, K, variant="full", zero=None):
    cs = case(oracle, pattern, LM, LN, prec, K, variant, zero)
    return P.project(oracle, cs.pr, cs.A, cs.starts, cs.B, cs.prec)


def allowance(ref, prec):
    """[nCols, LN], absolute: what a gamma of that right-hand side may deviate by (project_ref.gamma_tolerance, relative to the largest |gamma_i|)"""
    return P.gamma_tolerance(ref, prec) * np.abs(ref["gamma"]).max(axis=-1)


# ---- the cases of tests/test_gpu_project_shapes.py ---------------------------------------------------------------------------------------
# (pattern, LM, LN, precision, K, variant)
CASES_A = [("base", LM, LN, prec, K, "full") for LM, LN in SHAPES for prec in "zc" for K in (1, 2, 3, 4)] \
        + [("base", LM, LN, "m", K, "full") for LM, LN in SHAPES for K in (2, 4)]
CASES_B = [("base", LM, LN, prec, 3, "half") for LM, LN, prec in
           [(4, 5, "z"), (4, 5, "c"), (8, 9, "z"), (8, 9, "c"), (8, 10, "z"), (8, 10, "c"), (16, 16, "c"), (64, 64, "z")]]
OFFSET1 = ("base", 8, 9, "c", 3, "half")          # the case of CASES_B that runs on 1-based indices
LONG = [("long", 4, 4, "z"), ("long", 4, 4, "c"), ("long", 4, 4, "m"), ("long_short_end", 4, 4, "z"), ("long_short_end", 4, 4, "c"),
        ("dense_9x8", 16, 64, "z"), ("dense_9x8", 32, 64, "c"), ("dense_9x8", 8, 64, "z"), ("dense_17x8", 8, 64, "c"), ("single", 4, 4, "z")]
CASES_C = [(p, LM, LN, prec, K, "full") for p, LM, LN, prec in LONG for K in (2, 4)]
CASES_D = [("base", 8, 9, "z", 6, "full"), ("base", 4, 32, "c", 6, "full")]          # six starts for the ring, depth 3 and 4
CASES_E = [("base", 8, 10, "z", 3, "dup"), ("base", 4, 5, "c", 3, "dup"), ("base", 16, 16, "m", 3, "dup")]
ZERO_COLUMN = ("base", 8, 9, "z", 3, "full", (1, 4))                                # B = 0 in right-hand side 4 of block column 1
CASES_F = [("base", 8, 9, "c", 3, "full"), ("long", 4, 4, "z", 4, "full")]
EVERY_CASE = sorted(set(CASES_A + CASES_B + CASES_C + CASES_D + CASES_E + CASES_F), key=repr) + [ZERO_COLUMN]


def case_id(k):
    return "%s-%dx%d-%s-K%d-%s" % k[:6] + ("-zero" if len(k) > 6 else "")
