"""Start projection (include/tfqmrgpu_ext.h section 17) on every block shape, depth and chunk edge, against its numpy restatement
(tests/project_ref.py) on planted inputs (tests/project_cases.py; tests/test_project_cases_cpu.py has checked them on the CPU).  No solve
anywhere: set_matrix("X", S); push_start() makes any array a start, so k_project_gram, k_project_solve_col and k_project_combine run on
all 15 shapes x float | double x K = 1 ... 4, on B under half of X, on columns of 18 ... 72 chunks, on a column of one block, on a ring that
has wrapped, and on a pivot rule that decides differently inside one column.

The comparison is that of tests/test_gpu_project_start.py: gamma within project_ref.gamma_tolerance (100 eps_storage / rho relative to the
largest |gamma_i|), X within the bound its _deviations forms, n_used exact.  Worst deviation as a fraction of the allowance, per shape,
precision and K: profiles/project_shapes.txt."""
import numpy as np
import pytest

import project_cases as PC
import project_ref as P
import tfqmrgpu_amd as T
from conftest import offset1
from helpers import deviations, same_bits

pytestmark = pytest.mark.gpu


def _push(s, starts_newest_first):
    """oldest first; returns the starts as read back, newest first"""
    back = []
    for S in starts_newest_first[::-1]:
        s.set_matrix("X", S)
        s.push_start()
        back.insert(0, s.get_matrix())
    return back


def _project(s):
    got = s.project_start()
    return got["coefficients"], got["n_used"], s.get_matrix()


def _run(cs, depth=None, pr=None):
    """(gamma, n_used, X) of a fresh plan that had the starts of the case pushed in plain order"""
    with T.Solver.open(cs.pr if pr is None else pr, cs.prec, keep_starts=cs.K if depth is None else depth).load() as s:
        back = _push(s, cs.starts)
        assert s.start_count() == cs.K and all(np.array_equal(a, b) for a, b in zip(back, cs.starts))      # stored(): nothing left to round
        return _project(s)


def _compare(what, cs, ref, starts, gamma, used, X):
    """the existing comparison; prints before it asserts.  Returns the two deviations as fractions of their allowance"""
    assert np.array_equal(used, ref["n_used"]), what
    assert np.all(np.isfinite(gamma)) and np.all(np.isfinite(X)), what
    dg, bg, dx, bx = deviations(cs.pr, ref, dict(coefficients=gamma), X, starts, cs.prec)
    fg, fx = float((dg / bg).max()), float((dx / bx).max())
    print("project shapes %-34s gamma %.3e of allowed (abs %.2e), X %.3e of allowed (abs %.2e)" % (what, fg, dg.max(), fx, dx.max()))
    assert np.all(dg <= bg), (what, fg)
    assert np.all(dx <= bx), (what, fx)
    return fg, fx


def _case(oracle, key, prec=None):
    """the case under the plan's precision: an 'm' plan holds its operands in double, its case and reference are those of 'z'"""
    cs, ref = PC.case(oracle, *key), PC.reference(oracle, *key)
    if key[3] == "m":
        cs = PC.SimpleNamespace(**dict(vars(cs), prec="m"))
    return cs, ref


# ---- A. every shape and depth ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.CASES_A, ids=PC.case_id)
def test_every_shape_and_depth(oracle, key):
    """the 15 shapes x 'z', 'c' x K = 1 ... 4 and 'm' at K = 2, 4 (the double instances on the float plan's chunk tables), B on the full
    pattern of X: gamma is the planted c up to the noise, |gamma_gpu - c| <= |gamma_ref - c| + allowance, right-hand side by right-hand side.
    MI355X, worst deviation as a fraction of the allowance, gamma or X: 'z' 0.118 (32 x 32, K = 1), 'c' 0.020 (64 x 64, K = 4), 'm' 0.101 (8 x 64,
    K = 4); every shape, precision and K: profiles/project_shapes.txt"""
    cs, ref = _case(oracle, key)
    gamma, used, X = _run(cs)
    assert np.all(used == cs.K)
    _compare(PC.case_id(key), cs, ref, cs.starts, gamma, used, X)
    allowed = PC.allowance(ref, cs.prec)[:, :, None]
    assert np.all(np.abs(gamma - cs.c) <= np.abs(ref["gamma"] - cs.c) + allowed), key


# ---- B. B under half of X ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.CASES_B, ids=PC.case_id)
def test_b_under_every_second_block(oracle, key):
    """both branches of ld_b_under_x inside one chunk; one case on 1-based indices"""
    cs, ref = _case(oracle, key)
    gamma, used, X = _run(cs, pr=offset1(cs.pr) if key == PC.OFFSET1 else None)
    _compare(PC.case_id(key), cs, ref, cs.starts, gamma, used, X)


def test_the_one_based_case_is_among_them():
    assert PC.OFFSET1 in PC.CASES_B


# ---- C. chunk edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.CASES_C, ids=PC.case_id)
def test_chunk_edges(oracle, key):
    """columns of 25 | 50 chunks with and without a short last chunk, two trips a lane on 'm'; a dense column at LN = 64 of 18 chunks (eight
    trips a lane) and of 72 | 68 (the second batch of column_sum<64, 1>); a column of one block, 8 items for 256 lanes.  The chunk tables:
    tests/test_project_cases_cpu.py.  MI355X, worst deviation: 0.334 of the allowance (41 x 39 grid, 'z', K = 4; 50 chunk records a column)"""
    cs, ref = _case(oracle, key)
    gamma, used, X = _run(cs)
    assert np.all(used == cs.K)
    _compare(PC.case_id(key), cs, ref, cs.starts, gamma, used, X)
    allowed = PC.allowance(ref, cs.prec)[:, :, None]
    assert np.all(np.abs(gamma - cs.c) <= np.abs(ref["gamma"] - cs.c) + allowed), key


# ---- D. the ring -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.CASES_D, ids=PC.case_id)
def test_ring_position_does_not_enter_the_arithmetic(oracle, key):
    """depth 3: five pushes (the ring wraps, its head ends in slot 1), keep_starts(4) on that ring and a sixth push, keep_starts(2).  After
    each step gamma, n_used and X are, bit for bit, those of a fresh plan that had exactly the surviving starts pushed in plain order, and
    within the allowance of the reference"""
    cs, _ = _case(oracle, key)
    S = cs.starts[::-1]                                     # six different arrays, in the order in which they are pushed

    def fresh(survivors_oldest_first):
        with T.Solver.open(cs.pr, cs.prec, keep_starts=len(survivors_oldest_first)).load() as t:
            _push(t, survivors_oldest_first[::-1])
            return _project(t)

    def check(step, s, survivors_oldest_first):
        assert s.start_count() == len(survivors_oldest_first)
        got, want = _project(s), fresh(survivors_oldest_first)
        assert all(same_bits(a, b) for a, b in zip(got, want)), (key, step)
        newest_first = survivors_oldest_first[::-1]
        ref = P.project(oracle, cs.pr, cs.A, newest_first, cs.B, cs.prec)
        assert np.all(ref["n_used"] == len(newest_first)) and ref["ratio"].min() >= PC.KEPT_RATIO_MIN
        _compare("%s ring step %d" % (PC.case_id(key), step), cs, ref, newest_first, *got)

    with T.Solver.open(cs.pr, cs.prec, keep_starts=3).load() as s:
        for X in S[:5]:
            s.set_matrix("X", X)
            s.push_start()
        check(1, s, S[2:5])
        assert s.keep_starts(4) == 0 and s.start_count() == 3 and s.start_depth() == 4
        s.set_matrix("X", S[5])
        s.push_start()
        check(2, s, S[2:6])
        assert s.keep_starts(2) == 0 and s.start_depth() == 2
        check(3, s, S[4:6])


# ---- E. the pivot rule, right-hand side by right-hand side -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.CASES_E, ids=PC.case_id)
def test_pivot_rule_decides_per_right_hand_side(oracle, key):
    """S_1 = S_0 in the odd right-hand sides, independent in the even ones: n_used alternates K / K - 1 along j inside every column, the
    dropped gamma_1 is exactly 0, everything is finite, the kept gamma within the allowance"""
    cs, ref = _case(oracle, key)
    gamma, used, X = _run(cs)
    want = np.full(used.shape, cs.K)
    want[:, 1::2] = cs.K - 1
    assert np.array_equal(ref["n_used"], want) and np.array_equal(used, want)
    assert np.all(gamma[:, 1::2, 1] == 0) and np.all(gamma[:, 0::2, 1] != 0) and np.all(gamma[:, :, 0] != 0) and np.all(gamma[:, :, 2] != 0)
    _compare(PC.case_id(key), cs, ref, cs.starts, gamma, used, X)


def test_zero_column_of_b_on_a_ragged_shape(oracle):
    """8 x 9 'z': B = 0 in right-hand side 4 of block column 1: gamma = 0, n_used = 0 and X exactly 0 there and nowhere else"""
    key = PC.ZERO_COLUMN
    cs, ref = _case(oracle, key)
    col, j = cs.zero
    gamma, used, X = _run(cs)
    there = np.zeros(used.shape, bool)
    there[col, j] = True
    assert np.all(used[there] == 0) and np.all(used[~there] == cs.K)
    assert np.all(gamma[there] == 0) and np.all(gamma[~there] != 0)
    in_x = there[ref["an"]["colindx"].astype(np.int64)]                      # [nnzbX, LN]
    assert in_x.any() and np.all(X.transpose(0, 2, 1)[in_x] == 0) and np.all(X.transpose(0, 2, 1)[~in_x] != 0)
    _compare(PC.case_id(key), cs, ref, cs.starts, gamma, used, X)


# ---- F. two calls, same bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.CASES_F, ids=PC.case_id)
def test_two_calls_give_the_same_bits(oracle, key):
    cs, _ = _case(oracle, key)
    with T.Solver.open(cs.pr, cs.prec, keep_starts=cs.K).load() as s:
        _push(s, cs.starts)
        first, second = _project(s), _project(s)
    assert all(same_bits(a, b) for a, b in zip(first, second)), key
    assert all(same_bits(a, b) for a, b in zip(first, _run(cs))), key          # ... and those of another plan
