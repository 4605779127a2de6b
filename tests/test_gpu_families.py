"""Every fused multiply family of the solver (tfq_spmm.hip: spmm_select) against the CPU oracle, one iteration at a time.

One table: each row is a problem, a precision, the family the selector must hand the plan's fused multiplies, and the path the row
stands for (the shape, two or four columns per lane, the ragged last column group, the folded tail, an unfolded plan, a segmented
column ...).  Every row
  1. asserts the family first: a change of the selector moves a row to another kernel loudly, not silently;
  2. asserts the plan path from a restatement of the chunk and segment rules (tests/plan_paths.py);
  3. compares the work vectors x, v4 ... v9 after one and two iterations with the oracle's (fed with the same shadow vector):
     v4 and v9 come out of the EPI_XPAY_DOT multiply, v5 and v8 out of EPI_AXPY_NRM_DOT, x, v6 and v7 out of the vector kernels with
     the per-RHS scalars that the column operations computed from the multiplies' chunk records -- a dropped record, a wrong last column
     group or a wrong scalar shows here after one iteration, where the end of a solve would still converge;
  4. solves to the threshold and holds the residual the family's EPI_RESIDUAL epilogue reported against a float64 recomputation from
     the returned X, within the a-priori rounding bound of that epilogue (tests/plan_paths.py: true_residual).
The bounds of 3 are one per precision for every row: z as the state test of tests/test_gpu_hash_mode.py (Z_STATE; 4 x observed
there), c at k = 1 only, 1e-4 relative (a float trajectory's vectors at k = 2 depend on cancellation in the shadow-vector dots, see
STATE_CASES there).  k_spmm_direct (shapes outside the product's list) is covered by tests/test_gpu_operator.py."""
import numpy as np
import pytest

from family_cases import ROWS, load_problem_st16_onecol  # noqa: F401
from helpers import C_BOUND, Z_BOUND
from plan_paths import FOLD_MAX, gpu_state, plan_paths, state_deviation, true_residual
import tfqmrgpu_amd as T

pytestmark = pytest.mark.gpu


def test_every_family_but_direct_has_a_row():
    names = {"k_spmm_" + n for n in ("s4w", "m4", "ilv16", "ilv16f", "ilvf", "ilv8b", "ilv8", "ilv8f", "ilv8w", "mfma", "mfma8", "small4")}
    assert {r[3] for r in ROWS} == names


def _path_of(pr, prec):
    ch, seg, folds = plan_paths(pr, prec)
    if folds:
        return "fold", ch, seg
    return ("segmented" if max(seg) > 1 else "unfold"), ch, seg


@pytest.mark.parametrize("rid,make,prec,family,path,three", ROWS, ids=[r[0] for r in ROWS])
def test_family_against_the_oracle_one_iteration_at_a_time(oracle, rid, make, prec, family, path, three):
    pr = make()
    got_path, ch, seg = _path_of(pr, prec)
    assert got_path == path, (rid, sum(ch), max(ch), max(seg))
    if path == "unfold":
        assert sum(ch) > FOLD_MAX
    if rid.endswith("three_segmented"):
        assert len(ch) == 3 and min(seg) > 1          # every one of the three adjacent columns is cut into segments
    bounds = Z_BOUND if prec == "z" else C_BOUND
    for k in sorted(bounds):
        fam, got = gpu_state(pr, prec, k, three)
        assert fam == family, (rid, fam)
        worst = state_deviation(oracle, pr, prec, k, got)
        assert max(worst.values()) <= bounds[k], (rid, k, worst)

    tol = 1e-9 if prec == "z" else 1e-4
    status, X, info = T.solve_problem(pr, prec, threshold=tol, max_iterations=300, three_products=three)
    assert status == 0 and info["residual"] <= tol, (rid, status, info["residual"])
    res, bound = true_residual(pr, X, prec)
    assert abs(info["residual"] - res) <= bound, (rid, info["residual"], res, bound)
