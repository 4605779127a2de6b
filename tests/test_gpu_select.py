"""tfqmrgpuExt_selectDrop and tfqmrgpuExt_selectLeak (include/tfqmrgpu_ext.h section 20) on the GPU, through the C-ABI.  The index lists
against the numpy rule (tests/select_ref.py) applied to THIS plan's own drop_cost(), leak_map() and residual(): equality is exact, the
records are the same bits.  spent and left against numpy sums of the same records within the bound of a sum of non-negative terms in
another order (select_ref.py); the compaction across tile edges; the round trips through shrink_problem / grow_problem, adopt and
solve_from; that the calls change nothing; and every status in its order.  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import leak_map_ref as MR
import leak_ref as LR
import select_ref as SR
import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import ptr, random_x
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 3, 7, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
TOL = {"z": 1e-9, "c": 1e-4, "m": 1e-9}
HUGE = 1e150                                                         # eta * eta is finite
TILE = 256                                                           # tfq_select.hpp: kSelTile
SENTINEL = -12345.0

# one shape from each record-writing path: multiples of 16 | 8 rows | 4 rows (621 blocks: three compaction tiles, the last one ragged;
# 308 leak positions: two) | a padded plan, 9 x 9 on 16 x 16.  The others fit in a single partial tile
PROBLEMS = {
    "fd_16x16_small": lambda: load_problem("fd_16x16_small"),
    "stencil_8x8": lambda: load_problem("stencil_8x8"),
    "fd_4x4_2d": lambda: load_problem("fd_4x4_2d"),
    "padded_9x9": lambda: PR.stencil_2d(5, 4, 9, 9, 3, seed=99, radius=2.2),
}


def _open(pr, prec, **kw):
    return T.Solver.open(pr, prec, allow_padding=(pr.LM == 9), **kw)


def _pattern(pr):
    """the pattern of X as (block row, the caller's block column index) per block, whatever the index offset"""
    return MR.pattern_set(pr, pr.rowPtrX - pr.index_offset)


def _records(s, pr):
    """the operands of the two rules as this plan's public calls return them"""
    lmap = s.leak_map()
    return dict(cost2=s.drop_cost(weight=False)["cost2"], pos2=lmap["pos2"], pos_cols=lmap["cols"].astype(np.int64),
                bnorm2=s.residual()["bnorm2"], cols=SR.block_columns(pr), carries_b=s.plan_view()["subset"].astype(np.int64))


def _drop_ref(r, eta):
    return SR.select_drop(r["cost2"], r["bnorm2"], r["cols"], r["carries_b"], eta)


def _leak_ref(r, eta):
    return SR.select_leak(r["pos2"], r["bnorm2"], r["pos_cols"], eta)


def _same_drop(s, r, eta, what):
    got, ref = s.select_drop(eta), _drop_ref(r, eta)
    assert got["blocks"].dtype == np.int32 and np.array_equal(got["blocks"], ref["blocks"]), (what, eta, len(got["blocks"]), len(ref["blocks"]))
    dev = np.abs(got["spent"] - ref["spent"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(what, "eta %.3g: %d of %d eligible blocks, spent: largest deviation / bound %.3g" % (
            eta, len(ref["blocks"]), ref["eligible"], np.nanmax(np.where(ref["spent_bound"] > 0, dev / ref["spent_bound"], 0.0))))
    assert got["spent"].shape == ref["spent"].shape and np.all(dev <= ref["spent_bound"]), (what, eta)
    again = s.select_drop(eta)
    assert np.array_equal(again["blocks"], got["blocks"]) and np.array_equal(again["spent"], got["spent"]), (what, eta)      # the same bits
    assert np.array_equal(s.select_drop(eta, spent=False)["blocks"], got["blocks"])
    return got, ref


def _same_leak(s, r, eta, what):
    got, ref = s.select_leak(eta), _leak_ref(r, eta)
    assert got["take"].dtype == np.uint64 and np.array_equal(got["take"], ref["take"]), (what, eta, len(got["take"]), len(ref["take"]))
    dev = np.abs(got["left"] - ref["left"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(what, "eta %.3g: %d of %d positions, left: largest deviation / bound %.3g" % (
            eta, len(ref["take"]), len(r["pos_cols"]), np.nanmax(np.where(ref["left_bound"] > 0, dev / ref["left_bound"], 0.0))))
    assert got["left"].shape == ref["left"].shape and np.all(dev <= ref["left_bound"]), (what, eta)
    again = s.select_leak(eta)
    assert np.array_equal(again["take"], got["take"]) and np.array_equal(again["left"], got["left"]), (what, eta)
    assert np.array_equal(s.select_leak(eta, left=False)["take"], got["take"])
    return got, ref


# ---- 1. the index lists and the sums: every record-writing path, every precision, three values of eta --------------------------------------
@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_lists_and_sums(name, prec):
    pr = PROBLEMS[name]()
    what = "%s %s" % (name, prec)
    with _open(pr, prec).load() as s:
        s.solve(TOL[prec], 300)
        X = s.get_matrix()
        r = _records(s, pr)
        n_pos, free = len(r["pos_cols"]), np.setdiff1d(np.arange(pr.nnzbX), r["carries_b"])
        assert r["cost2"].shape == (pr.nnzbX, s.LN) and n_pos > 0

        # selectDrop: nothing | every eligible block | a share between 10 % and 90 %, chosen on the reference
        with np.errstate(divide="ignore", invalid="ignore"):
            need = np.sqrt(np.nanmax(r["cost2"] / r["bnorm2"][r["cols"]], axis=1))      # (0 / 0 in the padded right-hand sides: ignored)
        nothing, mixed = 0.5 * float(need[free].min()), SR.mixed_eta(r["cost2"], r["bnorm2"], r["cols"], r["carries_b"])
        assert nothing > 0 and mixed is not None
        _, ref = _same_drop(s, r, nothing, what)
        assert len(ref["blocks"]) == 0
        _, ref = _same_drop(s, r, HUGE, what)
        assert np.array_equal(ref["blocks"], free) and len(free) == ref["eligible"] == pr.nnzbX - pr.nnzbB
        _, ref = _same_drop(s, r, mixed, what)
        assert 0.1 * len(free) <= len(ref["blocks"]) <= 0.9 * len(free)

        # selectLeak: nothing | every position that leaks | a share between 10 % and 90 %
        mixed = SR.mixed_eta_leak(r["pos2"], r["bnorm2"], r["pos_cols"])
        assert mixed is not None
        _, ref = _same_leak(s, r, HUGE, what)
        assert len(ref["take"]) == 0
        _, ref = _same_leak(s, r, 0.0, what)
        reached = np.flatnonzero(np.any((r["pos2"] > 0) & (r["bnorm2"][r["pos_cols"]] > 0), axis=1))    # every position that leaks at all
        assert np.array_equal(ref["take"], reached) and len(reached) > 0.9 * n_pos
        got, ref = _same_leak(s, r, mixed, what)
        assert 0.1 * n_pos <= len(ref["take"]) <= 0.9 * n_pos

        # what is left and what is taken add up to truncation_leak(): three orders of sums of the same products, within the a-priori
        # bounds of the two kernels (tests/leak_ref.py, tests/leak_map_ref.py; test_gpu_leak_map.py: _sum_rule) plus that of left
        leak2 = s.truncation_leak()["leak2"]
        take = got["take"].astype(np.int64)
        taken = np.zeros_like(leak2)
        np.add.at(taken, r["pos_cols"][take], r["pos2"][take])
        A_, X_ = LR.stored(pr.A, prec), LR.stored(X, prec)
        ref_map = MR.leak_map(pr, A_, X_)
        tol = np.zeros_like(leak2)
        tol[:, :pr.LN] = LR.leak(pr, A_, X_)["bound"]
        np.add.at(tol[:, :pr.LN], ref_map["cols"], ref_map["bound"])
        tol += ref["left_bound"] + n_pos * SR.EPS * taken
        dev = np.abs(got["left"] + taken - leak2)
        with np.errstate(divide="ignore", invalid="ignore"):
            print(what, "left + taken against truncation_leak: largest deviation / bound %.3g" % np.nanmax(np.where(tol > 0, dev / tol, 0.0)))
        assert np.all(dev <= tol)


# ---- 2. the edges of the compaction ---------------------------------------------------------------------------------------------------------
# (that the fixtures cross these edges: tests/test_select_cpu.py, test_the_fixtures_cover_the_tile_edges)
@pytest.mark.parametrize("pattern", ["every block", "tile edges", "one", "last"])
def test_compaction_across_tile_edges(pattern):
    """records made by hand, not by a solve: X is zero except for chosen blocks, so that eta = 0 selects exactly the OTHER blocks without B --
    whole tiles set, whole tiles empty, the first and last block of every tile, the ragged tail.  4 x 4 blocks, 621 of them"""
    pr = PROBLEMS["fd_4x4_2d"]()
    n = pr.nnzbX
    keep = {"every block": np.arange(n), "tile edges": np.array([k for k in range(n) if k % TILE in (0, TILE - 1)] + [n - 1]),
            "one": np.array([TILE]), "last": np.arange(2 * TILE, n)}[pattern]
    X = np.zeros((n, pr.LM, pr.LN), dtype=np.complex128)
    X[keep] = random_x(pr, 5)[keep]
    with _open(pr, "z").load() as s:
        s.set_matrix("X", X)
        r = _records(s, pr)
        got, ref = _same_drop(s, r, 0.0, "compaction, %s" % pattern)
        want = np.setdiff1d(np.setdiff1d(np.arange(n), keep), r["carries_b"])
        zero_cost = np.setdiff1d(np.flatnonzero(np.all(r["cost2"] == 0, axis=1)), r["carries_b"])
        assert np.array_equal(ref["blocks"], zero_cost) and set(want.tolist()) <= set(zero_cost.tolist())
        if pattern == "every block":
            assert np.all(r["cost2"][np.setdiff1d(np.arange(n), r["carries_b"])].max(axis=1) > 0) and len(got["blocks"]) == 0
        else:
            assert len(got["blocks"]) > 0
        _same_leak(s, r, 0.0, "compaction, %s" % pattern)
        # only the count: no array is needed
        count = C.c_uint64(777)
        assert T.lib.tfqmrgpuExt_selectDrop(s.handle, s.plan, 0.0, 0, None, C.byref(count), None) == 0 and count.value == len(ref["blocks"])


# ---- 3. round trips: the lists go into shrink_problem / grow_problem, a new plan, adopt, solve_from -------------------------------------------
@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("stencil_8x8", "c")])
def test_round_trip_shrink(name, prec):
    pr = PROBLEMS[name]()
    with _open(pr, prec).load() as s:
        assert s.solve(TOL[prec], 300) == 0
        r = _records(s, pr)
        eta = SR.mixed_eta(r["cost2"], r["bnorm2"], r["cols"], r["carries_b"])
        drop = s.select_drop(eta)["blocks"]
        assert 0 < len(drop) < pr.nnzbX - pr.nnzbB
        small = s.shrink_problem(pr, drop)
        old = s.shrink_pattern(drop)[2]
        gone = {_pattern(pr)[n] for n in drop}
        assert small.nnzbX == pr.nnzbX - len(drop) and gone.isdisjoint(_pattern(small)) and len(gone) == len(drop)
        with _open(small, prec) as t:
            assert t.adopt(s, old) == 0
            assert t.solve_from(TOL[prec], 300) == 0
            assert t.residual()["worst"] <= 10 * TOL[prec]


@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("stencil_8x8", "c")])
def test_round_trip_grow(name, prec):
    pr = PROBLEMS[name]()
    with _open(pr, prec).load() as s:
        assert s.solve(TOL[prec], 300) == 0
        r = _records(s, pr)
        take = s.select_leak(SR.mixed_eta_leak(r["pos2"], r["bnorm2"], r["pos_cols"]))["take"]
        assert 0 < len(take) < len(r["pos_cols"])
        grown = s.grow_problem(pr, take)
        old = s.grow_pattern(take)[2]
        lmap = s.leak_map(values=False)
        columns = np.unique(pr.colIndX)
        added = {(int(lmap["rows"][int(p)]), int(columns[lmap["cols"][int(p)]]) ) for p in take}
        assert grown.nnzbX == pr.nnzbX + len(take) and added <= set(_pattern(grown)) and added.isdisjoint(_pattern(pr))
        with _open(grown, prec) as t:
            assert t.adopt(s, old) == 0
            assert t.solve_from(TOL[prec], 300) == 0
            assert t.residual()["worst"] <= 10 * TOL[prec]
            after = t.leak_map(values=False)
            assert added.isdisjoint(zip(after["rows"].tolist(), columns[after["cols"]].tolist()))     # what was taken no longer leaks


# ---- 4. non-destructive, between two solves -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,LM,LN", [("z", 16, 16), ("c", 4, 5), ("z", 8, 32), ("m", 16, 16)])
def test_non_destructive(prec, LM, LN):
    which = () if prec == "m" else (1, 4, 5, 6, 7, 8, 9)             # getWorkVector refuses an 'm' plan: its X is compared through get_matrix
    pr = PR.stencil_2d(5, 4, LM, LN, ncols=3, seed=LM + 2 * LN, radius=2.2)

    def run(with_call):
        with T.Solver.open(pr, prec).load() as s:
            assert s.solve(TOL[prec], 200) == 0
            res, cost, lmap, X = s.residual(), s.drop_cost(), s.leak_map(), s.get_matrix()
            if with_call:
                vectors = [s.get_work_vector(k) for k in which]
                history, info = s.bound_history(), s.get_info()
                for eta in (0.0, 1e-3, HUGE):
                    s.select_drop(eta)
                    s.select_leak(eta)
                for k, v in zip(which, vectors):
                    assert np.array_equal(s.get_work_vector(k), v, equal_nan=True), k
                assert np.array_equal(s.get_matrix(), X)
                assert np.array_equal(s.bound_history(), history) and s.get_info() == info
                res1, cost1, lmap1 = s.residual(), s.drop_cost(), s.leak_map()
                for key in ("residual2", "bnorm2", "columns"):
                    assert np.array_equal(res[key], res1[key]), key
                for key in ("cost2", "weight2"):
                    assert np.array_equal(cost[key], cost1[key]), key
                for key in ("rows", "cols", "pos2"):
                    assert np.array_equal(lmap[key], lmap1[key]), key
            st = s.solve(TOL[prec], 200)
            return st, s.get_info()["iterations"], s.get_matrix(), s.bound_history()

    st0, it0, X0, h0 = run(False)
    st1, it1, X1, h1 = run(True)
    assert (st0, it0) == (st1, it1) and np.array_equal(X0, X1) and np.array_equal(h0, h1)


# ---- 5. statuses, and their order -----------------------------------------------------------------------------------------------------------
def _raw(which, s, n_index, eta=0.5, capacity=None, with_index=True, with_count=True, with_sums=True):
    """(status, index array, count, sums): the arrays start as sentinels"""
    fn = getattr(T.lib, "tfqmrgpuExt_" + which)
    index = np.full(n_index, 77, np.int32 if which == "selectDrop" else np.uint64)
    sums = np.full((int(s.plan_view()["nCols"]), s.LN), SENTINEL)
    count = C.c_uint64(777)
    st = fn(s.handle, s.plan, eta, n_index if capacity is None else capacity, ptr(index) if with_index else None,
            C.byref(count) if with_count else None, ptr(sums) if with_sums else None)
    return st, index, int(count.value), sums


def _untouched(out):
    _, index, count, sums = out
    return bool(np.all(index == 77) and count == 777 and np.all(sums == SENTINEL))


@pytest.mark.parametrize("which", ["selectDrop", "selectLeak"])
def test_statuses_change_nothing(which):
    pr = PR.stencil_2d(4, 4, 4, 5, 2, seed=9, radius=1.5)
    room = 4 * pr.nnzbX
    with T.Solver.open(pr, "z") as s:                                       # a buffer, no A
        s.set_matrix("B", pr.B)
        out = _raw(which, s, room, with_index=False, with_count=False, with_sums=False)
        assert out[0] == NO_INFO_PASSED                             # in front of eta and of everything the operands need
        s.set_operator(lambda *a: 0.0)
        out = _raw(which, s, room, eta=-1.0)
        assert T.decode(out[0])[::2] == (UNDOCUMENTED, ord("E")) and _untouched(out)      # eta comes before the operator ...
        out = _raw(which, s, room)
        assert T.decode(out[0])[::2] == (NO_IMPLEMENTATION, 0) and _untouched(out)        # ... the operator before the missing A
        s.set_operator(None)
        for form in (dict(), dict(with_index=False, with_sums=False)):
            out = _raw(which, s, room, **form)
            assert T.decode(out[0])[::2] == (UNDOCUMENTED, ord("A")) and _untouched(out)
        s.set_matrix("A", pr.A)
        X = random_x(pr, 5)
        X[::3] = 0                                                  # zero blocks: eta = 0 drops them
        s.set_matrix("X", X)
        r = _records(s, pr)
        if which == "selectDrop":
            eta = 0.0
            ref = _drop_ref(r, eta)
            want, want_sums = ref["blocks"], ref["spent"]
        else:
            eta = SR.mixed_eta_leak(r["pos2"], r["bnorm2"], r["pos_cols"])
            ref = _leak_ref(r, eta)
            want, want_sums = ref["take"], ref["left"]
        n = len(want)
        assert n >= 2
        # capacity too small: key 'X', the count filled in, the arrays untouched
        for capacity in (0, n - 1):
            st, index, count, sums = _raw(which, s, room, eta, capacity=capacity)
            assert T.decode(st)[::2] == (UNDOCUMENTED, ord("X")) and count == n
            assert np.all(index == 77) and np.all(sums == SENTINEL)
            out = _raw(which, s, room, eta, capacity=capacity, with_count=False)
            assert T.decode(out[0])[::2] == (UNDOCUMENTED, ord("X")) and _untouched(out)
        # exactly enough room; only the first n entries are written
        st, index, count, sums = _raw(which, s, room, eta, capacity=n)
        assert st == 0 and count == n and np.array_equal(index[:n], want) and np.all(index[n:] == 77)
        assert np.all(np.abs(sums - want_sums) <= ref["spent_bound" if which == "selectDrop" else "left_bound"])
        # only the count | only the sums: capacity is not looked at
        st, index, count, none = _raw(which, s, room, eta, capacity=0, with_index=False, with_sums=False)
        assert st == 0 and count == n and np.all(index == 77) and np.all(none == SENTINEL)
        st, index, count, sums1 = _raw(which, s, room, eta, capacity=0, with_index=False, with_count=False)
        assert st == 0 and count == 777 and np.all(index == 77) and np.array_equal(sums1, sums)      # the same bits as with the list
        # a refusal in between leaves the next call what it was
        out = _raw(which, s, room, eta=float("nan"))
        assert T.decode(out[0])[::2] == (UNDOCUMENTED, ord("E")) and _untouched(out)
        st, index, count, sums2 = _raw(which, s, room, eta)
        assert st == 0 and count == n and np.array_equal(index[:n], want) and np.array_equal(sums2, sums)


@pytest.mark.parametrize("prec,LM", [("z", 8), ("m", 16)])
def test_preconditioned_plan(prec, LM):
    pr = PR.stencil_2d(4, 4, LM, LM, 2, seed=LM, radius=[1.5, 2.1])
    # without the kept copy the caller's A is gone after the first solve: status 19, nothing written
    with T.Solver.open(pr, prec, preconditioner=BJ).load() as s:
        assert s.solve(1e-9, 200) == 0
        for which in ("selectDrop", "selectLeak"):
            out = _raw(which, s, pr.nnzbX)
            assert T.decode(out[0])[::2] == (NO_IMPLEMENTATION, 0) and _untouched(out)
            out = _raw(which, s, pr.nnzbX, with_index=False, with_sums=False)
            assert T.decode(out[0])[::2] == (NO_IMPLEMENTATION, 0) and _untouched(out)
    # with it the calls read the kept copy: the lists are those of this plan's records, which test_gpu_drop_cost.py and
    # test_gpu_leak_map.py compare with the caller's A and the back-transformed X
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True).load() as s:
        assert s.solve(1e-9, 200) == 0
        r = _records(s, pr)
        eta = SR.mixed_eta(r["cost2"], r["bnorm2"], r["cols"], r["carries_b"])
        _, ref = _same_drop(s, r, eta, "kept A %s" % prec)
        assert 0 < len(ref["blocks"]) < ref["eligible"]
        _same_leak(s, r, SR.mixed_eta_leak(r["pos2"], r["bnorm2"], r["pos_cols"]), "kept A %s" % prec)
        # a patch that no set-up has seen yet counts already
        d = np.arange(0, pr.nnzbA, 2, dtype=np.int32)
        s.set_blocks("A", d, pr.A[d] * (1.5 + 0.5j))
        patched = _records(s, pr)
        assert not np.array_equal(patched["cost2"], r["cost2"])
        _same_drop(s, patched, eta, "kept A %s, patched" % prec)
