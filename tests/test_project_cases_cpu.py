"""The inputs of tests/test_gpu_project_shapes.py (tests/project_cases.py) on the CPU reference, without a GPU: every kept pivot ratio far
from the threshold, the planted coefficients recovered, coefficients further apart than any tolerance, the per-right-hand-side duplicate
decided as planted, and the chunk table of every long-column case on the intended side of its edge.  An input that misses a condition gets
another seed (project_cases.SEED_SHIFT), never another condition."""
import numpy as np
import pytest

import plan_paths as PP
import project_cases as PC
import project_ref as P


def _ratios(ref):
    r = ref["ratio"]
    assert np.all(np.isfinite(r[ref["bnorm2"] > 0]))
    return r


@pytest.mark.parametrize("key", PC.EVERY_CASE, ids=PC.case_id)
def test_pivot_ratios_stay_clear_of_the_threshold(oracle, key):
    """every kept ratio >= 0.25; a dropped one (the duplicate) <= threshold / 100, and every kept one >= 100 threshold: the rule of
    tests/test_project_start_cpu.py.  n_used is what the case plants"""
    cs, ref = PC.case(oracle, *key), PC.reference(oracle, *key)
    thr, r = P.pivot_min(cs.prec), _ratios(ref)
    kept = ref["kept"]
    assert np.all(r[kept] >= PC.KEPT_RATIO_MIN), (key, r[kept].min())
    assert np.all(r[kept] >= 100 * thr) and np.all(r[~kept] <= thr / 100), (key, r[~kept])
    want = np.full(ref["n_used"].shape, cs.K, np.int32)
    if cs.variant == "dup":
        want[:, 1::2] = cs.K - 1
        assert not kept[:, 1::2, 1].any() and kept[:, :, 0].all() and kept[:, :, 2:].all() and kept[:, 0::2, 1].all()
    if cs.zero is not None:
        want[cs.zero] = 0
        assert ref["bnorm2"][cs.zero] == 0 and np.count_nonzero(ref["bnorm2"] == 0) == 1
    assert np.array_equal(ref["n_used"], want), key


@pytest.mark.parametrize("key", [k for k in PC.EVERY_CASE if k[5] == "full" and len(k) == 6], ids=PC.case_id)
def test_planted_coefficients_are_recovered_and_apart(oracle, key):
    """on the full pattern |gamma_ref - c| <= 0.05, and any two entries of c lie further apart than 1000 allowances of the case (and than
    twice what the noise moves gamma by): a permutation of right-hand sides, columns or starts cannot hide in the tolerance"""
    cs, ref = PC.case(oracle, *key), PC.reference(oracle, *key)
    c = cs.c
    off = np.abs(ref["gamma"] - c).max()
    allowed = PC.allowance(ref, cs.prec).max()
    flat = c.reshape(-1)
    d = np.abs(flat[:, None] - flat[None, :])
    d[np.diag_indices(len(flat))] = np.inf
    print("%s: |gamma_ref - c| %.2e, smallest pivot ratio %.2f, allowance %.2e, closest coefficients %.3f" % (
        PC.case_id(key), off, ref["ratio"][ref["kept"]].min(), allowed, d.min()))
    assert off <= PC.PLANTED_MAX, (key, off)
    assert np.all((np.abs(c) >= 0.5) & (np.abs(c) < 1.9))
    assert d.min() > 1000 * allowed and d.min() >= PC.SPACING * (1 - 1e-12) and d.min() > 2 * off, (key, d.min(), allowed, off)


@pytest.mark.parametrize("key", PC.CASES_B, ids=PC.case_id)
def test_half_pattern_keeps_every_right_hand_side_in_play(oracle, key):
    """B on every second X block: blocks with and without a B block alternate, so they meet inside every chunk of two blocks or more; gamma
    is no longer c, and stays of order one (the largest |gamma_i| of every right-hand side >= 0.1)"""
    cs, ref = PC.case(oracle, *key), PC.reference(oracle, *key)
    assert np.array_equal(cs.keep, np.arange(0, cs.pr.nnzbX, 2)) and cs.pr.nnzbB == (cs.pr.nnzbX + 1) // 2
    assert np.abs(ref["gamma"]).max(axis=-1).min() >= 0.1
    assert np.abs(ref["gamma"] - cs.c).max() > 0.05


def test_base_pattern():
    for LM, LN in PC.SHAPES:
        pr = PC.base_pattern(LM, LN)
        assert sorted(np.bincount(pr.colIndX)) == [4, 8, 16] and pr.nnzbX == 28


# ---- chunk arithmetic ----------------------------------------------------------------------------------------------------------------------
def _table(pattern, LM, LN, prec):
    pr = PC.PATTERNS[pattern](LM, LN)
    ch = PC.chunk_lengths(pr, prec)
    assert [len(c) for c in ch] == PP.chunks_per_column(pr, prec)          # the two restatements of tfq_plan.cpp: cutChunks agree
    assert pr.nnzbX * 2 * LM * LN * (4 if prec == "c" else 8) < 2 * 1000 * 1000          # X as the plan holds it stays below 2 MB
    return pr, ch, PC.items_per_block(LM, LN, prec), PC.lanes(LN)


def test_every_long_case_is_listed():
    assert {k[:4] for k in PC.CASES_C} == set(PC.LONG)


def test_chunks_of_the_long_columns():
    """40 x 40 block rows of 4 x 4, two dense columns of 1600 blocks.  X is 800 | 400 KiB, far below 32 MiB, so a chunk is 8 KiB of blocks:
    32 blocks of 256 bytes in 'z', 64 of 128 bytes in 'c' and 'm' (whose table is the float plan's): 50 | 25 | 25 chunks a column, 13 or more
    each.  In 'z' and 'c' a chunk is exactly 256 items for 256 lanes; in 'm' the double instances walk the float table: 512 items, two trips"""
    for prec, per_chunk, n_chunks, items in (("z", 32, 50, 256), ("c", 64, 25, 256), ("m", 64, 25, 512)):
        pr, ch, ipb, T = _table("long", 4, 4, prec)
        assert 8 * 1024 // (2 * 4 * 4 * (8 if prec == "z" else 4)) == per_chunk == PC.blocks_per_chunk(pr, prec)
        assert ch == [[per_chunk] * n_chunks] * 2 and 1600 == per_chunk * n_chunks and n_chunks >= 13
        assert per_chunk * ipb == items and T == 256
    # 41 x 39: 1599 blocks a column, so the last chunk is one block short and has fewer items than lanes
    for prec, per_chunk, n_chunks in (("z", 32, 50), ("c", 64, 25)):
        pr, ch, ipb, T = _table("long_short_end", 4, 4, prec)
        assert ch == [[per_chunk] * (n_chunks - 1) + [per_chunk - 1]] * 2 and 1599 == per_chunk * n_chunks - 1
        assert (per_chunk - 1) * ipb < T == per_chunk * ipb


def test_chunks_of_the_dense_columns_at_64_right_hand_sides():
    """column_sum<64, 1> takes 16 records in each of 256 / 64 = 4 lane groups, 64 per batch; the records behind them are a second batch.
    16 x 64 'z' and 32 x 64 'c' (blocks of 16 KiB) are shapes of the MFMA multiply, whose chunks hold four strips or more: four blocks, not
    one, so the 72 blocks of the 9 x 8 grid are 18 chunks of 64 KiB, eight trips a lane.  The second batch is reached on 8 x 64: 'z' blocks of
    8 KiB, one a chunk, 72 chunks; 'c' blocks of 4 KiB, two a chunk, 136 blocks on 17 x 8: 68 chunks"""
    batch = 16 * (256 // 64)
    assert batch == 64 == PP.col_seg_len(64)
    for LM, prec in ((16, "z"), (32, "c")):
        pr, ch, ipb, T = _table("dense_9x8", LM, 64, prec)
        assert PC.block_bytes(LM, 64, prec) == 16 * 1024 and PC.blocks_per_chunk(pr, prec) == 4
        assert ch == [[4] * 18] and 72 == 4 * 18 and 4 * ipb == 8 * T
    pr, ch, ipb, T = _table("dense_9x8", 8, 64, "z")
    assert PC.block_bytes(8, 64, "z") == 8 * 1024 and ch == [[1] * 72] and batch < 72 < 2 * batch and ipb == T
    pr, ch, ipb, T = _table("dense_17x8", 8, 64, "c")
    assert PC.block_bytes(8, 64, "c") == 4 * 1024 and ch == [[2] * 68] and batch < 68 < 2 * batch and 2 * ipb == T
    for n in (72, 68, 18):
        assert PP.col_segments(n, 64) == 1          # one work group sums the column: k_project_solve_col has no shares


def test_chunk_of_a_single_block():
    """4 x 4 'z', radius 0.5: the second column is its source block alone, 16 elements a plane = 8 items for 256 lanes"""
    pr, ch, ipb, T = _table("single", 4, 4, "z")
    assert ch == [[16], [1]] and ipb == 8 and 1 * ipb < T == 256


def test_base_pattern_reaches_the_plane_rounds_on_every_shape():
    """what the base pattern gives each shape: chunks per column, and whether some chunk takes several trips | has fewer items than lanes"""
    seen = set()
    for LM, LN in PC.SHAPES:
        for prec in "zcm":
            pr = PC.base_pattern(LM, LN)
            ch = PC.chunk_lengths(pr, prec)
            items = [n * PC.items_per_block(LM, LN, prec) for c in ch for n in c]
            assert sum(sum(c) for c in ch) == 28 and min(items) >= 1
            seen |= {"short" if min(items) < PC.lanes(LN) else "", "trips" if max(items) > PC.lanes(LN) else "",
                     "chunks" if max(len(c) for c in ch) > 1 else ""}
    assert {"short", "trips", "chunks"} <= seen
    # the three ragged shapes leave lanes idle: T = 255 | 252 | 250
    assert [PC.lanes(LN) for LN in (5, 9, 10)] == [255, 252, 250]
