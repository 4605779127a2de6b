"""Single right-hand sides (RHS) that break down next to healthy ones, in every form of the column operations (tfq_colops.hpp):
folded into the producers' tails, launched on their own, with a column cut into segments, in the several-rank slot, with float and
with double coefficients.  The fixtures (tests/breakdown_cases.py) hit each branch with exact zeros, tests/test_breakdown_cpu.py proves on
the CPU that they do; here the HIP forms are held against the oracle fed with the same shadow vector, and against each other bit for bit.

Against the oracle: the returned status, the iteration count in z, X on the healthy RHS (1e-7 max|X0| in z as the zero-RHS edge test of
tests/test_gpu_parity.py, 1e-3 max|X0| in c as its random ragged systems), on the failed RHS the NaN mask and exact zeros, and the work
vectors x, v4 ... v9 after exactly one and two iterations: within the bounds of tests/test_gpu_families.py on the healthy RHS (a float
trajectory has a bound at k = 1 alone, see there), NaN mask and exact zeros on the failed ones.  The second iteration is where a stale
eta, beta or c67 of a broken RHS shows in v6, v7 or x.  No status can be read per RHS on the device: what is compared is what a caller
sees."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import breakdown_cases as BC
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import ROOT
from plan_paths import gpu_state, plan_paths, state_deviation, true_residual
from helpers import C_BOUND, Z_BOUND

pytestmark = pytest.mark.gpu

X_BOUND = {"z": 1e-7, "c": 1e-3}
FOLD = [(kind, shape, prec) for prec in "zc" for shape in BC.FOLD_SHAPES[prec] for kind in BC.KINDS]
SEGMENTED = [(kind, "8x64seg3" if kind == "column" else "8x64seg", "z") for kind in BC.KINDS]


@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    return BC.case(kind, shape)


@functools.lru_cache(maxsize=None)
def _solve(kind, shape, prec):
    """the product's solve of a fixture (folded, or segmented), once for all tests; nobody changes what it returns"""
    return BC.gpu_solve(_case(kind, shape), prec, residual=True)


def _against_the_oracle(oracle, kind, shape, prec):
    c = _case(kind, shape)
    st, X, info = _solve(kind, shape, prec)
    st0, X0, info0 = BC.oracle_solve(oracle, c, prec)
    dead = np.broadcast_to(c.failed_blocks()[:, None, :], X.shape)
    print("\n%s %s %s: status %d | %d, iterations %d | %d" % (kind, shape, prec, st, st0, info["iterations"], info0["iterations"]))
    assert st == st0 == c.status
    if prec == "z":
        assert info["iterations"] == info0["iterations"]
    assert np.array_equal(np.isnan(X), np.isnan(X0))
    assert np.all(X[dead][X0[dead] == 0] == 0)
    if not dead.all():
        dev, scale = np.abs(X[~dead] - X0[~dead]).max(), np.abs(X0[~dead]).max()
        print("  X on the healthy RHS: %.2e of max|X0| (bound %.0e)" % (dev / scale, X_BOUND[prec]))
        assert dev <= X_BOUND[prec] * scale
    bounds = Z_BOUND if prec == "z" else C_BOUND
    for k in (1, 2):
        if kind == "all" and k > 1:
            break                                            # the solve ends in its first iteration
        want = 6 if kind == "all" else 9
        fam, got = gpu_state(c.pr, prec, k, v3=c.v3, status=want)
        worst = state_deviation(oracle, c.pr, prec, k, got, v3=c.v3, status=want, failed=c.failed_blocks())
        print("  k = %d: %s %s" % (k, fam, {w: "%.1e" % v for w, v in worst.items()}))
        if k in bounds and worst:
            assert max(worst.values()) <= bounds[k], (k, worst)


@pytest.mark.parametrize("kind,shape,prec", FOLD, ids=BC.row_ids(FOLD))
def test_folded_forms_against_the_oracle(oracle, kind, shape, prec):
    ch, seg, folds = plan_paths(_case(kind, shape).pr, prec)
    assert folds is True and len(ch) == 2
    _against_the_oracle(oracle, kind, shape, prec)


@pytest.mark.parametrize("kind,shape,prec", SEGMENTED, ids=BC.row_ids(SEGMENTED))
def test_segmented_columns_against_the_oracle(oracle, kind, shape, prec):
    ch, seg, folds = plan_paths(_case(kind, shape).pr, prec)
    assert seg[0] > 1 and min(seg) > 1 and not folds
    assert 2 * BC.j_star(64) >= 64
    _against_the_oracle(oracle, kind, shape, prec)


def _worker(tmp_path, tag, rows, prec, **env):
    """the fixtures `rows` of one precision in ONE fresh process with the lab build's switches"""
    out = str(tmp_path / (tag + ".npz"))
    name = "breakdown:" + ",".join("%s:%s" % (kind, shape) for kind, shape, _ in rows)
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_env_worker.py"), out, name, prec, "0"],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def _same_bits(got, rows, what):
    for kind, shape, prec in rows:
        st, X, info = _solve(kind, shape, prec)
        key = "%s:%s/" % (kind, shape)
        assert int(got[key + "status"]) == st and int(got[key + "iterations"]) == info["iterations"], (what, key)
        assert np.array_equal(got[key + "history"], info["bound_history"], equal_nan=True), (what, key)
        assert float(got[key + "residual"]) == info["residual"], (what, key)
        assert np.array_equal(got[key + "X"], X, equal_nan=True), (what, key)          # NaN where the other has NaN, the same bits elsewhere


@pytest.mark.parametrize("prec", ["z", "c"])
def test_own_launches_change_no_bit_of_a_folded_solve(tmp_path, prec):
    """the column operations as kernels of their own (lab build, TFQMRGPU_FOLD_MAX=0) on every fold fixture"""
    rows = [r for r in FOLD if r[2] == prec]
    _same_bits(_worker(tmp_path, "own", rows, prec, TFQMRGPU_FOLD_MAX=0), rows, "TFQMRGPU_FOLD_MAX=0")


def test_fold_limit_changes_no_bit_of_a_segmented_column_with_a_broken_rhs(tmp_path):
    """a plan with a segmented column never folds, whatever the limit: the lab build with TFQMRGPU_FOLD_MAX=100000 against the product"""
    _same_bits(_worker(tmp_path, "seg", SEGMENTED, "z", TFQMRGPU_FOLD_MAX=100000), SEGMENTED, "TFQMRGPU_FOLD_MAX=100000")


@pytest.mark.parametrize("kind", BC.KINDS)
def test_reduce_callback_slot_changes_no_bit(kind):
    """the several-rank form of the slot (reduce | callback | decide) on one rank, 16 x 16 z"""
    calls = []
    st, X, info = BC.gpu_solve(_case(kind, "16x16"), "z", reduce_callback=lambda values, n: calls.append(n))
    st0, X0, info0 = _solve(kind, "16x16", "z")
    assert st == st0 == _case(kind, "16x16").status and info["iterations"] == info0["iterations"]
    assert np.array_equal(info["bound_history"], info0["bound_history"], equal_nan=True) and info["residual"] == info0["residual"]
    assert np.array_equal(X, X0, equal_nan=True)
    assert len(calls) >= 1
    if kind != "all":
        assert len(calls) >= info0["iterations"]


def test_mixed_solves_a_zero_right_hand_side_by_zero(oracle):
    """'m' (k_refine_init_col): "a zero right-hand side is solved by x = 0" -- the documented rule, not the oracle's NaN bound"""
    c = _case("zero_rhs", "16x16")
    st, X, info = T.solve_problem(c.pr, "m", threshold=BC.THRESHOLD["m"], max_iterations=BC.MAX_ITERATIONS["m"])
    st0, X0, info0 = oracle.solve(c.pr, "z", threshold=BC.THRESHOLD["m"], max_iterations=BC.MAX_ITERATIONS["m"])
    dead = np.broadcast_to(c.failed_blocks()[:, None, :], X.shape)
    assert st == st0 == 0 and info["residual"] <= BC.THRESHOLD["m"]
    assert not np.isnan(X).any() and not X[dead].any()
    assert np.abs(X[~dead] - X0[~dead]).max() <= 1e-7 * np.abs(X0[~dead]).max()


@pytest.mark.parametrize("kind", ["dec35", "dec34", "column"])
@pytest.mark.parametrize("shape", BC.FOLD_SHAPES["z"])
def test_residual_tells_the_broken_right_hand_sides(oracle, kind, shape):
    """tfqmrgpuExt_residual after a solve that ended with broken RHS: above the threshold exactly there"""
    c = _case(kind, shape)
    st, X, info = _solve(kind, shape, "z")
    got, thr2 = info["per_rhs"], BC.THRESHOLD["z"] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        q = got["residual2"] / got["bnorm2"]
    assert np.all((q[c.failed] > thr2) | np.isnan(q[c.failed])) and np.all(q[~c.failed] < thr2)
    ref = RR.residual(oracle, c.pr, c.pr.A, X)
    for key, bound in (("residual2", "bound_r2"), ("bnorm2", "bound_b2")):
        assert np.all(np.abs(got[key] - ref[key]) <= ref[bound]), key
    res, bound = true_residual(c.pr, X, "z")                 # the solve's own figure: the worst RHS, a broken one
    assert abs(info["residual"] - res) <= bound
