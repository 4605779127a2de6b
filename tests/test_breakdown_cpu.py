"""Proof, on the CPU oracle, that every fixture of tests/breakdown_cases.py reaches the branch it stands for -- before
tests/test_gpu_breakdown.py holds the HIP forms of the column operations against the oracle on the same fixtures.

Per fixture and precision (z, c), from the per-RHS status that the oracle exports (oracle/pyoracle.py: solve(status=True)):
  - the intended status value arises at the planned (block column, j*) and at no other right-hand side, in the intended iteration
    (the first; `plus_one`: at the first probe);
  - no other right-hand side is ever given any status but 0, and every one of them has converged when the solve ends: its
    |b - A x| / |b|, recomputed in float64 from the returned X, is below the threshold;
  - what the solve returns: 0, or 6 (TFQMRGPU_STATUS_BREAKDOWN) where every right-hand side fails;
  - the plan path: the fold shapes fold, the 8 x 64 z columns are cut into segments.
Run with -s for the table."""
import numpy as np
import pytest

import breakdown_cases as BC
import residual_ref as RR
from plan_paths import FOLD_MAX, plan_paths

FOLD = [(kind, shape, prec) for prec in "zc" for shape in BC.FOLD_SHAPES[prec] for kind in BC.KINDS]
SEGMENTED = [(kind, "8x64seg3" if kind == "column" else "8x64seg", "z") for kind in BC.KINDS]


@pytest.mark.parametrize("kind,shape,prec", FOLD + SEGMENTED, ids=BC.row_ids(FOLD + SEGMENTED))
def test_fixture_reaches_its_branch(oracle, kind, shape, prec):
    c = BC.case(kind, shape)
    st, X, info = BC.oracle_solve(oracle, c, prec, status=True)
    status, when, f = info["status"], info["status_when"], c.failed
    ch, seg, folds = plan_paths(c.pr, prec)
    where = [(int(a), int(b)) for a, b in zip(*np.nonzero(when[c.first]))]
    print("\n%-9s %-8s %s: status %2d first given at (column, j) %s in iteration %s, left as %s; solve returns %d after %d iterations; chunks %s "
          "segments %s folds %s" % (kind, shape, prec, c.first, where if len(where) < 4 else "%d of them" % len(where),
                                    np.unique(when[c.first][f]).tolist(), np.unique(status[f]).tolist(), st, info["iterations"], ch, seg, folds))
    # the path
    if shape.startswith("8x64seg"):
        assert min(seg) > 1 and not folds
    else:
        assert folds and sum(ch) <= FOLD_MAX and len(ch) == 2 and 20 <= c.pr.nnzbX <= 80
    # the planned failures, and only they
    assert f.sum() == {"column": c.pr.LN, "all": f.size}.get(kind, 1)
    assert np.array_equal(when[c.first] != 0, f)
    first_probe = 1 + int(np.argmax(info["bound_history"] <= (100 * BC.THRESHOLD[prec]) ** 2))      # tfqmrgpu_core.hxx:138, 252
    assert np.all(when[c.first][f] == (first_probe if kind == "plus_one" else 1))
    if kind == "dec34":
        assert np.all(when[-1] == 0)                        # z = v3.v5 != 0: dec35 never sees this one
    if kind == "zero_rhs":
        assert np.all(status[f] == -3)
    if kind == "plus_one":
        assert np.all(status[f] == 1) and np.all(when[-3][f] == 1)   # r = 0 exactly after one iteration: tau = 0, then the probe finds it
    for value in (-1, -2, -3, 1):
        assert not when[value][~f].any(), value
    assert not status[~f].any()
    # what the solve returns, and the healthy right-hand sides have converged inside the cap
    assert st == c.status
    assert info["iterations"] <= BC.MAX_ITERATIONS[prec]
    if kind != "all":
        ref = RR.residual(oracle, c.pr, c.pr.A, X)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.sqrt(ref["residual2"] / ref["bnorm2"])
        assert (rel[~f] <= BC.THRESHOLD[prec]).sum() == f.size - f.sum()
        assert not np.isnan(X).any()
    else:
        assert info["iterations"] == BC.MAX_ITERATIONS[prec] and not X.any()      # as the reference leaves iterations_needed (tfqmrgpu_core.hxx:170)


def test_a_broken_right_hand_side_keeps_the_solve_running_to_the_cap(oracle):
    """why the fixtures carry an iteration cap: a RHS that broke down keeps its v5 = b, its tau falls as |b|^2 / (2 it + 1) and no faster, which
    holds the residual bound of the stopping test at 1, so the only probe is the one of the last iteration -- and iterated far past their convergence the healthy RHS break down as well"""
    c = BC.case("dec35", "4x8")
    st, X, info = BC.oracle_solve(oracle, c, "z", status=True)
    assert st == 0 and info["iterations"] == BC.MAX_ITERATIONS["z"] and np.abs(info["bound_history"] - 1).max() <= 1e-14
    st, X, info = oracle.solve(c.pr, "z", threshold=BC.THRESHOLD["z"], max_iterations=300, v3=c.v3.reshape(-1), status=True)
    assert info["iterations"] == 300 and info["status"][~c.failed].all()
