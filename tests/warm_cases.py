"""Planted inputs of tests/test_gpu_warm_families.py, importable without a GPU; tests/test_warm_cases_cpu.py checks on the CPU oracle that
every one of them is a fair question before a GPU sees it.

A case is a problem, a precision and a start X0 = stored(random_x): planted, of order one, so that R = B - trunc(A X0) is of order one and
nothing cancels.  The warm start (include/tfqmrgpu_ext.h section 14) solves the correction problem A D = R from zero and returns X0 + D; the
oracle solves the same problem (tests/warm_ref.py) with R formed in complex128.  The library forms R in the plan's precision, in an order of
its own: element by element the two differ by at most
    E = sqrt(2) (n + 3) eps (|A| |X0| + |B|),      n = LM x the blocks of A in that block row
(plan_paths.rounding_factor, the arithmetic of plan_paths.true_residual).  What the oracle's k-th iterate moves by under such a change of its
right-hand side is measured on the oracle alone: spread(k) is the largest relative move of a work vector between the solve of A D = R and
that of A D = R + sigma E, sigma = hashed signs, one per real and imaginary part (E bounds the modulus of an element's error and so each
of its parts: sigma E is a corner of that box, the full a-priori size), the worse of two draws.  Real rounding is smaller by about sqrt(n),
so no further factor is applied:
    allowance(k) = BOUND[k] + spread(k)            BOUND = helpers.Z_BOUND | helpers.C_BOUND, the cold solve's bounds for identical inputs
and for work vector 1 (X = X0 + D, compared relative to max|D|) eps_storage max|X0| / max|D| more, for the one rounding of the update.
Nothing here is derived from an output of the library."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import family_cases as FC
import helpers as H
import plan_paths as PP
import project_cases as PC
import residual_ref as RR
import tfqmrgpu_amd as T
import warm_ref as WR
from precond_ref import _product
from tfqmrgpu_amd import problems as PR

SHAPES = PC.SHAPES
BOUND = {"z": H.Z_BOUND, "c": H.C_BOUND}
CAP = {"z": 1e-8, "c": 1e-3}              # tests/test_warm_cases_cpu.py: every allowance stays below this; a cap, not a measurement
THRESHOLD = {"z": 1e-9, "c": 1e-4}
TEETH = 100                               # every mutation of R moves the oracle's state by this many allowances or more
VECTORS = (1, 4, 5, 6, 7, 8, 9)

# a case that misses a condition of tests/test_warm_cases_cpu.py gets another seed here, never another condition
SEED_SHIFT = {
}

ROW = {r[0]: r for r in FC.ROWS}


# ---- the case lists ------------------------------------------------------------------------------------------------------------------------
# ("F", row id) | ("S", LM, LN, precision, "full" | "half") | ("E", pattern, LM, LN, precision) | ("M", pattern | "half", LM, LN)
CASES_F = [("F", r[0]) for r in FC.ROWS]
HALF = [(4, 5, "z"), (4, 5, "c"), (8, 9, "z"), (8, 9, "c"), (8, 10, "z"), (8, 10, "c"), (16, 16, "c"), (64, 64, "z")]
CASES_S = [("S", LM, LN, prec, "full") for LM, LN in SHAPES for prec in "zc"] + [("S", LM, LN, prec, "half") for LM, LN, prec in HALF]
OFFSET1 = ("S", 8, 9, "c", "half")          # the half case that runs on 1-based indices
CASES_E = [("E", "long", 4, 4, "z"), ("E", "long", 4, 4, "c"), ("E", "long_short_end", 4, 4, "z"), ("E", "long_short_end", 4, 4, "c"),
           ("E", "dense_9x8", 16, 64, "z"), ("E", "dense_9x8", 8, 64, "z"), ("E", "dense_17x8", 8, 64, "c"), ("E", "single", 4, 4, "z")]
CASES_M = [("M", "long", 4, 4), ("M", "long_short_end", 4, 4), ("M", "dense_9x8", 8, 64), ("M", "half", 8, 9)]
EVERY_CASE = CASES_F + CASES_S + CASES_E
# two calls, same bits: one 'z' unfolded, one 'c' ragged (T = 252 lanes, B under every second block), one segmented
TWICE = [("F", "m4_4x8_z_unfolded"), OFFSET1, ("F", "ilv8w_8x64_z_three_segmented")]
PRECONDITIONED = [("S", 4, 5, "c", "full"), ("S", 8, 9, "z", "full"), ("S", 16, 64, "z", "full"), ("S", 64, 64, "c", "full")]


def case_id(key):
    return {"F": "F-%s", "S": "S-%dx%d-%s-%s", "E": "E-%s-%dx%d-%s", "M": "M-%s-%dx%d"}[key[0]] % key[1:]


def precision(key):
    return {"F": lambda: ROW[key[1]][2], "S": lambda: key[3], "E": lambda: key[4], "M": lambda: "m"}[key[0]]()


# ---- problems ------------------------------------------------------------------------------------------------------------------------------
def half_problem(pr0, seed):
    """B under every second X block (as project_cases.build builds `keep`), values of order one: blocks with and without a B block alternate,
    so both branches of ld_b_under_x meet inside every chunk of two blocks or more"""
    assert pr0.index_offset == 0
    keep = np.arange(0, pr0.nnzbX, 2)
    rows = np.repeat(np.arange(pr0.mb), np.diff(pr0.rowPtrX))
    rpB = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=pr0.mb))])
    shape = (len(keep), pr0.LM, pr0.LN)
    B = PR.hashed_uniform(seed + 5, shape) + 1j * PR.hashed_uniform(seed + 6, shape)
    return T.Problem(pr0.rowPtrA, pr0.colIndA, pr0.A, pr0.rowPtrX, pr0.colIndX, rpB, pr0.colIndX[keep], B, None, pr0.tolerance, 0)


def problem(key):
    if key[0] == "F":
        return ROW[key[1]][1]()
    if key[0] == "S":
        pr = H.stencil(key[1], key[2])
        return half_problem(pr, 100 * key[1] + key[2]) if key[4] == "half" else pr
    if key[0] == "M" and key[1] == "half":
        return half_problem(H.stencil(key[2], key[3]), 100 * key[2] + key[3])
    return PC.PATTERNS[key[1]](key[2], key[3])          # "E" and "M"


def path_of(pr, prec):
    """"fold" | "unfold" | "segmented", as tests/test_gpu_families.py names the paths"""
    ch, seg, folds = PP.plan_paths(pr, prec)
    return "fold" if folds else ("segmented" if max(seg) > 1 else "unfold")


def rounding_bound(an, pr, X0, A, B, prec):
    """E [nnzbX, LM, LN]: |R_plan - R| element by element, on the pattern of X"""
    mag = _product(an, pr, np.abs(A), np.abs(X0))
    mag[an["subset"].astype(np.int64)] += np.abs(B)
    n = pr.LM * np.diff(pr.rowPtrA)[np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))]
    return PP.rounding_factor(n, prec)[:, None, None] * mag


# ---- a case ----------------------------------------------------------------------------------------------------------------------------------
def build(oracle, pr, prec, X0, seed, key=None, v3=None):
    """the case of a start X0 on `pr`; v3: the shadow vector of the solve (default: the library's hashed one)"""
    store = "z" if prec == "m" else prec
    an = oracle.analyse(pr)
    assert an["status"] == 0
    X0 = RR.stored(X0, store)
    A, B = RR.stored(pr.A, store), RR.stored(pr.B, store)
    cp = WR.correction_problem(oracle, pr, X0, A, B)
    row = ROW[key[1]] if key and key[0] == "F" else None
    return SimpleNamespace(key=key, pr=pr, prec=prec, store=store, seed=seed, an=an, X0=X0, A=A, B=B, cp=cp, R=cp.B, an_cp=oracle.analyse(cp),
                           E=rounding_bound(an, pr, X0, A, B, store), v3=T.hash_shadow_vector(pr).reshape(-1) if v3 is None else v3,
                           family=row[3] if row else None, path=row[4] if row else None, three=bool(row[5]) if row else False)


@functools.lru_cache(maxsize=None)
def case(oracle, key):
    """'m' plans hold A, B and X in double: their case is stored as 'z' is"""
    pr = problem(key)
    seed = 1000 + zlib.crc32(repr(key).encode()) % 100000 + 1000003 * SEED_SHIFT.get(key, 0)
    return build(oracle, pr, precision(key), H.random_x(pr, seed), seed, key)


def with_rhs(cp, R):
    return T.Problem(cp.rowPtrA, cp.colIndA, cp.A, cp.rowPtrX, cp.colIndX, cp.rowPtrX, cp.colIndX, R, None, cp.tolerance, cp.index_offset)


def state(oracle, cs, R, k):
    """the oracle's work vectors {1: D, 4 ... 9} after k iterations on A D = R with the library's default shadow vector"""
    st, _, info = oracle.solve(with_rhs(cs.cp, R), cs.store, threshold=1e-30, max_iterations=k, v3=cs.v3, plan=cs.an_cp, dump_iteration=k)
    assert st == 9, (cs.key, k, st)
    return info["vectors"]


def moved(got, want):
    """{w: max|got - want| / max|want|}: the comparison of plan_paths.state_deviation"""
    out = {}
    for w in VECTORS:
        scale = np.abs(want[w]).max()
        assert scale > 0, w
        out[w] = float(np.abs(got[w] - want[w]).max() / scale)
    return out


def spread_of(oracle, cs, k, base):
    worst = 0.0
    for draw in range(2):
        s = cs.seed + 100 + 2 * draw
        sigma = np.where(PR.hashed_uniform(s, cs.R.shape) < 0, -1.0, 1.0) + 1j * np.where(PR.hashed_uniform(s + 1, cs.R.shape) < 0, -1.0, 1.0)
        worst = max(worst, max(moved(state(oracle, cs, cs.R + sigma * cs.E, k), base).values()))
    return worst


def allowance_of(cs, k, sp, base):
    """{work vector: what it may deviate by, relative to max|the oracle's vector|}"""
    a = BOUND[cs.store][k] + sp
    out = {w: a for w in VECTORS}
    out[1] = a + PP.EPS[cs.store] * np.abs(cs.X0).max() / np.abs(base[1]).max()
    return out


@functools.lru_cache(maxsize=None)
def reference(oracle, key, k):
    return state(oracle, case(oracle, key), case(oracle, key).R, k)


@functools.lru_cache(maxsize=None)
def spread(oracle, key, k):
    return spread_of(oracle, case(oracle, key), k, reference(oracle, key, k))


def allowance(oracle, key, k):
    return allowance_of(case(oracle, key), k, spread(oracle, key, k), reference(oracle, key, k))


# ---- teeth -----------------------------------------------------------------------------------------------------------------------------------
def mutations(oracle, key):
    """{name: R as a mistake in front of the correction solve would leave it}
    swap_rhs   two right-hand sides of one block column exchanged
    swap_re_im Re and Im of one block exchanged
    drop_b     the B under one X block left out
    drop_last  the last block of a column's last chunk left at R = -Y.  Where no B lies under that block -- the stencils hold B at one source
               block a column, in the middle of the grid -- this would change nothing; the block is then the last one of that column that has
               a B block under it, in the last chunk that holds one"""
    cs = case(oracle, key)
    sub, col = cs.an["subset"].astype(np.int64), cs.an["colindx"].astype(np.int64)
    out = {}
    R = cs.R.copy()
    blocks = np.flatnonzero(col == 0)
    R[blocks, :, 0], R[blocks, :, cs.pr.LN - 1] = cs.R[blocks, :, cs.pr.LN - 1], cs.R[blocks, :, 0]
    out["swap_rhs"] = R
    R = cs.R.copy()
    q = cs.pr.nnzbX // 2
    R[q] = cs.R[q].imag + 1j * cs.R[q].real
    out["swap_re_im"] = R
    R = cs.R.copy()
    R[sub[0]] -= cs.B[0]
    out["drop_b"] = R
    R = cs.R.copy()
    last_col = np.flatnonzero(col[sub] == col[sub].max())
    R[sub[last_col[-1]]] -= cs.B[last_col[-1]]
    out["drop_last"] = R
    return out


def drop_last_is_the_last_block(oracle, key):
    cs = case(oracle, key)
    sub, col = cs.an["subset"].astype(np.int64), cs.an["colindx"].astype(np.int64)
    c = col[sub].max()
    return sub[np.flatnonzero(col[sub] == c)[-1]] == np.flatnonzero(col == c)[-1]
