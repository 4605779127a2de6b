"""Inputs and a-priori error bounds of the stand-alone multiply's block shapes and precisions (tfqmrgpu_ext.h section 3), shared by
tests/test_multiply_cases_cpu.py and tests/test_gpu_multiply_cases.py.

For a Y element of a block with p block products: n = 2 LM p + 1 terms, env = sum over the products of (|Re A| + |Im A|)^T (|Re X| + |Im X|)
in float64, Y64 = the oracle in float64 on float64 copies of the inputs (for float inputs every product is exact there).
  c | z: |Y - Y64| <= 2 gamma_n env, gamma_n = n u / (1 - n u), u = 2^-24 | 2^-53 (sums in the storage precision)
  m:     |Y - Y64| <= ulp_f32(|Y64|) / 2 + 2 n 2^-53 env (sums in double, one rounding to float)"""
import numpy as np

SOLVER_SHAPES = [(4, 4), (4, 5), (4, 8), (4, 32), (8, 8), (8, 9), (8, 10), (8, 32), (8, 64),
                 (16, 16), (16, 32), (16, 64), (32, 32), (32, 64), (64, 64)]
WIDE_SHAPES = [(48, 48), (96, 96), (128, 128)]                   # the multiply's own shapes on k_spmm_mfma (TFQ_MULTIPLY_SIZES)
PAD_SHAPES = [(6, 6), (12, 12), (24, 24)]                        # shapes of the reference's `bench multi` that do not fill 16 x 16 tiles
ALL_SHAPES = SOLVER_SHAPES + PAD_SHAPES + WIDE_SHAPES            # the 21 shapes of the reference's `bench multi`

NY, NA, NX = 37, 23, 29      # more Y blocks than X blocks
NPROD = 12                   # products per non-empty Y block


def listing(rng, nY=NY, nA=NA, nX=NX, nprod=NPROD):
    """pair list of nY Y blocks: every fifth has no product, every other one nprod products of random A and X blocks"""
    starts, pairs = [0], []
    for y in range(nY):
        for _ in range(0 if y % 5 == 3 else nprod):
            pairs += [int(rng.integers(0, nA)), int(rng.integers(0, nX))]
        starts.append(len(pairs) // 2)
    return np.array(starts, np.uint32), np.array(pairs, np.uint32)


def case(LM, LN, real, seed=0):
    """listing and operands, uniform in [-1, 1]: starts, pairs, A [NA, 2, LM(k), LM(i)], X [NX, 2, LM, LN]"""
    rng = np.random.default_rng(seed)
    starts, pairs = listing(rng)
    A = rng.uniform(-1, 1, (NA, 2, LM, LM)).astype(real)
    X = rng.uniform(-1, 1, (NX, 2, LM, LN)).astype(real)
    return starts, pairs, A, X


def oracle_y(oracle, prec, LM, LN, starts, pairs, A, X):
    """the oracle's product ("z": float64 sums, "c": float32 sums) for nY = len(starts) - 1 Y blocks"""
    nY = len(starts) - 1
    Xp = np.zeros((max(nY, len(X)), 2, LM, LN), X.dtype)        # (the oracle sizes Y like X)
    Xp[:len(X)] = X
    return oracle.spmm(prec, LM, LN, starts, pairs, np.ascontiguousarray(A), Xp)[:nY]


def reference(oracle, LM, LN, starts, pairs, A, X):
    """Y64 [nY, 2, LM, LN], env [nY, 1, LM, LN] and n [nY, 1, 1, 1]"""
    nY = len(starts) - 1
    Y64 = oracle_y(oracle, "z", LM, LN, starts, pairs, A.astype(np.float64), X.astype(np.float64))
    aa = (np.abs(A[:, 0].astype(np.float64)) + np.abs(A[:, 1].astype(np.float64))).transpose(0, 2, 1)   # [i][k]
    xx = np.abs(X[:, 0].astype(np.float64)) + np.abs(X[:, 1].astype(np.float64))
    env = np.zeros((nY, 1, LM, LN))
    for y in range(nY):
        q = np.arange(starts[y], starts[y + 1])
        if len(q):
            env[y, 0] = np.matmul(aa[pairs[2 * q]], xx[pairs[2 * q + 1]]).sum(axis=0)
    n = (2.0 * LM * np.diff(starts.astype(np.int64)) + 1)[:, None, None, None]
    return Y64, env, n


def bound_cz(prec, env, n):
    u = 2.0 ** -24 if prec == "c" else 2.0 ** -53
    return 2 * (n * u / (1 - n * u)) * env


def bound_m(Y64, env, n):
    return 0.5 * np.spacing(np.abs(Y64).astype(np.float32)).astype(np.float64) + 2 * n * 2.0 ** -53 * env
