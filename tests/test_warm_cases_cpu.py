"""The inputs of tests/test_gpu_warm_families.py (tests/warm_cases.py) on the CPU oracle, without a GPU: every allowance below its cap, four
mistakes in front of the correction solve each visible at a hundred allowances, and every case on the plan path and the side of the chunk
edge it stands for.  An input that misses a condition gets another seed (warm_cases.SEED_SHIFT), never another condition.  The figures:
profiles/warm_families.txt (scripts/warm_families.py)."""
import numpy as np
import pytest

import family_cases as FC
import plan_paths as PP
import project_cases as PC
import warm_cases as WC


def test_the_lists_hold_what_they_stand_for():
    assert [k[1] for k in WC.CASES_F] == [r[0] for r in FC.ROWS]
    full = {k[1:4] for k in WC.CASES_S if k[4] == "full"}
    assert full == {(LM, LN, prec) for LM, LN in PC.SHAPES for prec in "zc"} and len(PC.SHAPES) == 15
    assert {k[1:4] for k in WC.CASES_S if k[4] == "half"} == {k[1:4] for k in PC.CASES_B} and WC.OFFSET1 in WC.CASES_S and WC.OFFSET1[4] == "half"
    assert {k[1] for k in WC.CASES_E} == set(PC.PATTERNS)
    assert set(WC.TWICE) <= set(WC.EVERY_CASE) and set(WC.PRECONDITIONED) <= set(WC.CASES_S)
    ids = [WC.case_id(k) for k in WC.EVERY_CASE + WC.CASES_M]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("key", WC.EVERY_CASE, ids=WC.case_id)
def test_allowance_stays_below_the_cap(oracle, key):
    """allowance(k) <= 1e-8 'z' | 1e-3 'c' for every k of the bound table and every work vector; X0, R and D are of order one, so that
    the comparison relative to max|D| is not a comparison with rounding noise"""
    cs = WC.case(oracle, key)
    assert np.array_equal(cs.X0, WC.RR.stored(cs.X0, cs.store)) and 0.5 <= np.abs(cs.X0).max() <= 2.2
    assert 0.1 <= np.abs(cs.R).max() <= 10 and np.all(cs.E >= 0) and cs.E.max() <= 1e5 * PP.EPS[cs.store]
    for k in sorted(WC.BOUND[cs.store]):
        al, sp = WC.allowance(oracle, key, k), WC.spread(oracle, key, k)
        D = np.abs(WC.reference(oracle, key, k)[1]).max()
        print("warm case %-34s k=%d: spread %.3e, allowance %.3e (x: %.3e), max|D| %.2e" % (WC.case_id(key), k, sp, al[4], al[1], D))
        assert 0 < sp and max(al.values()) <= WC.CAP[cs.store], (key, k, sp, al)
        assert al[1] >= al[4] == WC.BOUND[cs.store][k] + sp and D >= 0.01


@pytest.mark.parametrize("key", WC.EVERY_CASE, ids=WC.case_id)
def test_mistakes_in_the_right_hand_side_show(oracle, key):
    """two right-hand sides of a block column exchanged, Re and Im of a block exchanged, the B under one X block left out, B dropped for
    the last block of a column (warm_cases.mutations): after ONE iteration of the oracle on the mutated R its state lies 100 allowances or
    more from that of R"""
    cs = WC.case(oracle, key)
    allowed = max(WC.allowance(oracle, key, 1).values())
    base = WC.reference(oracle, key, 1)
    muts = WC.mutations(oracle, key)
    assert sorted(muts) == ["drop_b", "drop_last", "swap_re_im", "swap_rhs"]
    for name, R in muts.items():
        assert R.shape == cs.R.shape and not np.array_equal(R, cs.R), (key, name)
        move = max(WC.moved(WC.state(oracle, cs, R, 1), base).values())
        print("warm case %-34s %-10s moves the state by %.2e = %.1e allowances" % (WC.case_id(key), name, move, move / allowed))
        assert move >= WC.TEETH * allowed, (key, name, move, allowed)


def test_b_under_the_last_block_of_a_column_is_among_the_cases(oracle):
    """drop_last takes the very last block of a column where B lies under it: the half patterns with an even last position and the column
    of one block"""
    hit = [k for k in WC.CASES_S[30:] + [("E", "single", 4, 4, "z")] if WC.drop_last_is_the_last_block(oracle, k)]
    print("B under the last block of the last column:", [WC.case_id(k) for k in hit])
    assert ("E", "single", 4, 4, "z") in hit and any(k[0] == "S" for k in hit)


# ---- plan paths --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,make,prec,family,path,three", FC.ROWS, ids=[r[0] for r in FC.ROWS])
def test_family_rows_take_their_path(rid, make, prec, family, path, three):
    pr = make()
    ch, seg, folds = PP.plan_paths(pr, prec)
    assert WC.path_of(pr, prec) == path, (rid, sum(ch), max(ch), max(seg))
    if path == "unfold":
        assert sum(ch) > PP.FOLD_MAX and max(seg) == 1
    if rid.endswith("three_segmented"):
        assert len(ch) == 3 and min(seg) > 1


def test_shape_cases_are_small_folded_plans_with_short_and_long_chunks():
    """the base pattern: columns of 16, 4 and 8 blocks on every shape, folded; half: B under the even positions"""
    for key in WC.CASES_S:
        pr = WC.problem(key)
        assert sorted(np.bincount(pr.colIndX)) == [4, 8, 16] and WC.path_of(pr, key[3]) == "fold"
        assert pr.nnzbB == (14 if key[4] == "half" else 3)
    assert [PC.lanes(LN) for LN in (5, 9, 10)] == [255, 252, 250]


def _table(key):
    pr, prec = WC.problem(key), WC.precision(key)
    ch = PC.chunk_lengths(pr, prec)
    assert [len(c) for c in ch] == PP.chunks_per_column(pr, prec)
    return pr, ch, PC.items_per_block(pr.LM, pr.LN, prec), PC.lanes(pr.LN)


def test_chunk_edges():
    """the tables of tests/test_project_cases_cpu.py for the cases that run warm: 50 | 25 full chunks a column, the same with a last chunk one
    block short, four blocks a chunk and eight trips a lane on 16 x 64, the second batch of column_sum<64, 1> on 8 x 64, a column of one block"""
    for prec, per_chunk, n_chunks in (("z", 32, 50), ("c", 64, 25)):
        pr, ch, ipb, T = _table(("E", "long", 4, 4, prec))
        assert ch == [[per_chunk] * n_chunks] * 2 and per_chunk * ipb == T == 256
        pr, ch, ipb, T = _table(("E", "long_short_end", 4, 4, prec))
        assert ch == [[per_chunk] * (n_chunks - 1) + [per_chunk - 1]] * 2 and (per_chunk - 1) * ipb < T == per_chunk * ipb
    pr, ch, ipb, T = _table(("E", "dense_9x8", 16, 64, "z"))
    assert ch == [[4] * 18] and 4 * ipb == 8 * T
    batch = PP.col_seg_len(64)
    pr, ch, ipb, T = _table(("E", "dense_9x8", 8, 64, "z"))
    assert ch == [[1] * 72] and batch < 72 < 2 * batch and ipb == T and PP.col_segments(72, 64) == 1
    pr, ch, ipb, T = _table(("E", "dense_17x8", 8, 64, "c"))
    assert ch == [[2] * 68] and batch < 68 < 2 * batch and 2 * ipb == T and PP.col_segments(68, 64) == 1
    pr, ch, ipb, T = _table(("E", "single", 4, 4, "z"))
    assert ch == [[16], [1]] and ipb == 8 and 1 * ipb < T == 256


def test_chunk_tables_of_the_mixed_cases():
    """'m': double items on the float plan's chunk table -- 64 blocks of 4 x 4 are 512 items, two trips a lane; 8 x 64: two blocks a chunk,
    36 chunks; 8 x 9 with B under every second block: 252 lanes"""
    for name, last in (("long", 64), ("long_short_end", 63)):
        pr, ch, ipb, T = _table(("M", name, 4, 4))
        assert ch == [[64] * 24 + [last]] * 2 and 64 * ipb == 2 * T == 512
    pr, ch, ipb, T = _table(("M", "dense_9x8", 8, 64))
    assert ch == [[2] * 36] and 2 * ipb == 2 * T
    pr, ch, ipb, T = _table(("M", "half", 8, 9))
    assert T == 252 and pr.nnzbB == 14 and max(max(c) for c in ch) >= 2
