"""tfqmrgpuExt_selectDrop and tfqmrgpuExt_selectLeak (include/tfqmrgpu_ext.h section 20) without a GPU: the numpy restatement of the two
rules (tests/select_ref.py) on the records of the references drop_cost_ref.py, leak_map_ref.py and residual_ref.py, pinned property by
property; its lists fed to shrinkPattern and growPattern, which are host code; and every status of the two calls that comes before the
first device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import drop_cost_ref as DR
import leak_map_ref as MR
import residual_ref as RR
import select_ref as SR
import tfqmrgpu_amd as T
from helpers import ptr, random_x, stencil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED = 3, 7, 14
HUGE = 1e150                                                         # eta * eta is finite


@pytest.fixture(scope="module")
def graded(oracle):
    """the stencil problem (one full block column, two truncated ones) with an X whose blocks of the last two block rows are zero: the
    records of the three references, computed once and left unchanged"""
    pr = stencil()
    X = random_x(pr, 31)
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrX))
    X[rows >= pr.mb - 2] = 0
    cost = DR.drop_cost(pr, pr.A, X)
    lmap = MR.leak_map(pr, pr.A, X)
    res = RR.residual(oracle, pr, pr.A, X)
    for a in (cost["cost2"], lmap["pos2"], res["bnorm2"]):
        a.setflags(write=False)
    return dict(pr=pr, cost2=cost["cost2"], pos2=lmap["pos2"], pos_cols=lmap["cols"], bnorm2=res["bnorm2"],
                cols=SR.block_columns(pr), carries_b=DR.b_blocks(pr))


def _drop(g, eta, cost2=None, bnorm2=None):
    return SR.select_drop(g["cost2"] if cost2 is None else cost2, g["bnorm2"] if bnorm2 is None else bnorm2, g["cols"], g["carries_b"], eta)


def _leak(g, eta, pos2=None, bnorm2=None):
    return SR.select_leak(g["pos2"] if pos2 is None else pos2, g["bnorm2"] if bnorm2 is None else bnorm2, g["pos_cols"], eta)


# ---- selectDrop ----------------------------------------------------------------------------------------------------------------------------
def test_blocks_that_carry_b_are_never_selected(graded):
    g = graded
    assert len(g["carries_b"]) == g["pr"].nnzbB == 3
    for eta in (0.0, 1e-3, 1.0, HUGE):
        assert set(_drop(g, eta)["blocks"].tolist()).isdisjoint(g["carries_b"])
    # ... also where its record is zero
    cost2 = g["cost2"].copy()
    cost2[g["carries_b"]] = 0
    assert set(_drop(g, 0.0, cost2)["blocks"].tolist()).isdisjoint(g["carries_b"])


def test_eta_zero_selects_exactly_the_zero_records(graded):
    g = graded
    zero = [n for n in np.flatnonzero(np.all(g["cost2"] == 0, axis=1)).tolist() if n not in g["carries_b"]]
    got = _drop(g, 0.0)
    assert got["blocks"].tolist() == zero and 0 < len(zero) < got["eligible"]
    assert got["blocks"].dtype == np.int32 and np.all(got["spent"] == 0)
    # one right-hand side that is not zero keeps the block
    cost2 = g["cost2"].copy()
    cost2[zero[0], 2] = 1e-300
    assert _drop(g, 0.0, cost2)["blocks"].tolist() == zero[1:]


def test_a_huge_eta_selects_every_eligible_block(graded):
    g = graded
    got = _drop(g, HUGE)
    want = [n for n in range(g["pr"].nnzbX) if n not in g["carries_b"]]
    assert got["blocks"].tolist() == want and len(want) == got["eligible"]
    assert np.all(np.diff(got["blocks"]) > 0)
    # spent is then the sum of the square roots over every block without B
    spent = np.zeros_like(g["bnorm2"])
    for n in want:
        spent[g["cols"][n]] += np.sqrt(g["cost2"][n])
    assert np.all(np.abs(got["spent"] - spent) <= got["spent_bound"])


def test_the_rule_is_per_right_hand_side_and_inclusive(graded):
    """a block goes when EVERY right-hand side passes, and a record equal to the limit passes"""
    g = graded
    n = next(k for k in range(g["pr"].nnzbX) if k not in g["carries_b"] and np.all(g["cost2"][k] > 0))
    c, eta = g["cols"][n], 0.25
    lim = (np.float64(eta) * np.float64(eta)) * g["bnorm2"][c]
    cost2 = g["cost2"].copy()
    cost2[n] = lim
    assert n in _drop(g, eta, cost2)["blocks"]
    cost2[n, 3] = np.nextafter(lim[3], np.inf)
    assert n not in _drop(g, eta, cost2)["blocks"]


def test_nan_records_are_rejected(graded):
    g = graded
    free = [n for n in range(g["pr"].nnzbX) if n not in g["carries_b"]]
    cost2 = g["cost2"].copy()
    cost2[free[1], 0] = np.nan
    got = _drop(g, HUGE, cost2)
    assert free[1] not in got["blocks"] and len(got["blocks"]) == len(free) - 1 and np.all(np.isfinite(got["spent"]))
    # a NaN in bnorm2 rejects the blocks of that block column, and no position of it is taken
    bnorm2 = g["bnorm2"].copy()
    bnorm2[1, 2] = np.nan
    assert not np.any(g["cols"][_drop(g, HUGE, bnorm2=bnorm2)["blocks"]] == 1)
    pos2 = g["pos2"].copy()
    pos2[0, :] = np.nan
    assert 0 not in _leak(g, 0.0, pos2)["take"]


def test_padded_right_hand_sides_are_neutral(graded):
    """a padded plan has bnorm2 = 0 and cost2 = pos2 = 0 in the added right-hand sides: the lists do not change"""
    g = graded
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 3))], axis=1)
    for eta in (0.0, 0.05, HUGE):
        assert np.array_equal(_drop(g, eta, pad(g["cost2"]), pad(g["bnorm2"]))["blocks"], _drop(g, eta)["blocks"])
        assert np.array_equal(_leak(g, eta, pad(g["pos2"]), pad(g["bnorm2"]))["take"], _leak(g, eta)["take"])


# ---- selectLeak ----------------------------------------------------------------------------------------------------------------------------
def test_leak_positions(graded):
    g = graded
    n_pos = len(g["pos_cols"])
    assert n_pos > 0 and len(_leak(g, HUGE)["take"]) == 0
    with_leak = np.flatnonzero(np.any(g["pos2"] > 0, axis=1))
    all_of_them = _leak(g, 0.0)
    assert all_of_them["take"].tolist() == with_leak.tolist() and 0 < len(with_leak) < n_pos      # X has zero blocks: some positions get nothing
    assert all_of_them["take"].dtype == np.uint64 and np.all(all_of_them["left"] == 0)
    eta = SR.mixed_eta_leak(g["pos2"], g["bnorm2"], g["pos_cols"])
    mixed = _leak(g, eta)
    assert 0.1 * n_pos <= len(mixed["take"]) <= 0.9 * n_pos
    # what is taken and what is left add up to the leak of the column
    taken = np.zeros_like(g["bnorm2"])
    np.add.at(taken, g["pos_cols"][mixed["take"].astype(np.int64)], g["pos2"][mixed["take"].astype(np.int64)])
    total = np.zeros_like(g["bnorm2"])
    np.add.at(total, g["pos_cols"], g["pos2"])
    assert np.all(np.abs(mixed["left"] + taken - total) <= 4 * n_pos * SR.EPS * total)
    # a right-hand side with b = 0 never takes a position
    bnorm2 = np.zeros_like(g["bnorm2"])
    assert len(_leak(g, 0.0, bnorm2=bnorm2)["take"]) == 0


# ---- the lists go where they are meant to go ------------------------------------------------------------------------------------------------
def test_the_drop_list_is_accepted_by_shrink_pattern(graded):
    g = graded
    pr = g["pr"]
    eta = SR.mixed_eta(g["cost2"], g["bnorm2"], g["cols"], g["carries_b"])
    assert eta is not None
    with T.Solver() as s:
        s.create_plan(pr)
        for e in (0.0, eta, HUGE):
            got = _drop(g, e)
            if e == eta:
                assert 0.1 * got["eligible"] <= len(got["blocks"]) <= 0.9 * got["eligible"]
            rowPtrX, colIndX, old = s.shrink_pattern(got["blocks"])
            for a, b in zip((rowPtrX, colIndX, old), DR.shrunk(pr, got["blocks"])):
                assert np.array_equal(a, b)
            assert len(old) == pr.nnzbX - len(got["blocks"]) and set(g["carries_b"]) <= set(old.tolist())


def test_the_take_list_is_accepted_by_grow_pattern(graded):
    g = graded
    pr = g["pr"]
    positions = MR.positions(pr)
    assert [c for c, _ in positions] == g["pos_cols"].tolist()
    with T.Solver() as s:
        s.create_plan(pr)
        s.buffer_size(pr.LM, pr.LN, "z")
        for e in (0.0, SR.mixed_eta_leak(g["pos2"], g["bnorm2"], g["pos_cols"]), HUGE):
            take = _leak(g, e)["take"]
            rowPtrX, colIndX, old = s.grow_pattern(take)
            assert len(colIndX) == pr.nnzbX + len(take) and int((old < 0).sum()) == len(take)
            new = set(MR.pattern_set(pr, rowPtrX - pr.index_offset, colIndX))
            columns = np.unique(pr.colIndX)
            assert new == set(MR.pattern_set(pr)) | {(positions[int(p)][1], int(columns[positions[int(p)][0]])) for p in take}


def test_the_fixtures_cover_the_tile_edges():
    """what tests/test_gpu_select.py rests on: its 4 x 4 fixture spans three compaction tiles (tfq_select.hpp: kSelTile) with a ragged
    last one, in blocks; two, ragged, in leak positions; its 8 x 8 and 16 x 16 fixtures fit in one partial tile"""
    src = open(os.path.join(ROOT, "tfqmrgpu_amd", "csrc", "tfq_select.hpp")).read()
    tile = int(re.search(r"constexpr uint32_t kSelTile = (\d+);", src).group(1))
    from conftest import load_problem
    big = load_problem("fd_4x4_2d")
    assert big.nnzbX > 2 * tile and big.nnzbX % tile != 0
    n_pos = len(MR.positions(big))
    assert n_pos > tile and n_pos % tile != 0
    for name in ("stencil_8x8", "fd_16x16_small"):
        assert load_problem(name).nnzbX < tile


# ---- symbols and the statuses in front of the first device call ---------------------------------------------------------------------------------
def test_symbols_header_and_binding():
    for name in ("tfqmrgpuExt_selectDrop", "tfqmrgpuExt_selectLeak"):
        assert name in T.EXT_SYMBOLS and hasattr(T.lib, name)
    flat = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_selectDrop(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double eta, uint64_t capacity, "
            "int32_t *blocks, uint64_t *nSelected, double *spent);") in flat
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_selectLeak(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double eta, uint64_t capacity, "
            "uint64_t *take, uint64_t *nSelected, double *left);") in flat
    assert callable(T.Solver.select_drop) and callable(T.Solver.select_leak)


@pytest.mark.parametrize("which", ["selectDrop", "selectLeak"])
def test_argument_checks_in_order_without_a_device(which):
    pr = stencil()
    fn = getattr(T.lib, "tfqmrgpuExt_" + which)
    index = np.full(4 * pr.nnzbX, 77, np.int32 if which == "selectDrop" else np.uint64)
    sums = np.full((3, pr.LN), -12345.0)
    count = C.c_uint64(777)

    def raw(handle, plan, eta=0.5, with_index=True, with_count=True, with_sums=True):
        return fn(handle, plan, eta, len(index), ptr(index) if with_index else None, C.byref(count) if with_count else None,
                  ptr(sums) if with_sums else None)

    assert T.decode(raw(None, None))[::2] == (POINTER_INVALID, 0)
    with T.Solver() as s:
        s.create_plan(pr)
        assert T.decode(raw(None, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(raw(s.handle, None))[::2] == (POINTER_INVALID, 0)
        # no bufferSize yet: before the look at the outputs and at eta
        assert T.decode(raw(s.handle, s.plan))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(raw(s.handle, s.plan, -1.0, False, False, False))[::2] == (UNDOCUMENTED, 0)
        s.buffer_size(pr.LM, pr.LN, "z")
        # all three outputs NULL: before eta
        assert raw(s.handle, s.plan, -1.0, False, False, False) == NO_INFO_PASSED
        # eta: before the missing buffer
        for eta in (-1e-300, -1.0, float("nan"), -float("inf")):
            assert T.decode(raw(s.handle, s.plan, eta))[::2] == (UNDOCUMENTED, ord("E"))
            assert T.decode(raw(s.handle, s.plan, eta, False, True, False))[::2] == (UNDOCUMENTED, ord("E"))
        # no buffer: every form needs one, the count alone as well
        for eta in (0.0, 0.5, float("inf")):
            assert T.decode(raw(s.handle, s.plan, eta))[::2] == (POINTER_INVALID, 0)
            assert T.decode(raw(s.handle, s.plan, eta, False, True, False))[::2] == (POINTER_INVALID, 0)
        with pytest.raises(T.TfqmrError) as e:
            s.select_drop(0.5) if which == "selectDrop" else s.select_leak(0.5)
        assert T.decode(e.value.status)[0] == POINTER_INVALID
    assert np.all(index == 77) and np.all(sums == -12345.0) and count.value == 777       # nothing has been written
