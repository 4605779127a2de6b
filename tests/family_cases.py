"""The table of tests/test_gpu_families.py, importable without a GPU: each row is a problem, a precision, the family the selector
(tfq_spmm.hip: spmm_select) must hand the plan's fused multiplies, and the path the row stands for (the shape, two or four columns per lane,
the ragged last column group, the folded tail, an unfolded plan, a segmented column ...).  tests/warm_cases.py runs the warm start on the
same rows."""
from tfqmrgpu_amd import problems as PR

st = PR.stencil_2d
# (id, problem, precision, family, path: "fold" | "unfold" | "segmented", three-product multiply)
ROWS = [
    # 4-row blocks
    ("m4_4x8_z", lambda: st(10, 8, 4, 8, 3, seed=31, radius=2.5), "z", "k_spmm_m4", "fold", False),
    ("m4_4x32_z", lambda: st(10, 8, 4, 32, 2, seed=32, radius=3.1), "z", "k_spmm_m4", "fold", False),
    ("m4_4x8_z_unfolded", lambda: st(30, 30, 4, 8, 400, seed=33, radius=1.5), "z", "k_spmm_m4", "unfold", False),
    ("small4_4x5_z", lambda: st(10, 8, 4, 5, 3, seed=34, radius=2.5), "z", "k_spmm_small4", "fold", False),
    ("small4_4x4_c", lambda: st(10, 8, 4, 4, 3, seed=35, radius=2.5), "c", "k_spmm_small4", "fold", False),
    ("small4_4x5_c", lambda: st(9, 7, 4, 5, 3, seed=36, radius=3.3), "c", "k_spmm_small4", "fold", False),
    ("small4_4x5_z_unfolded", lambda: st(30, 30, 4, 5, 400, seed=37, radius=1.5), "z", "k_spmm_small4", "unfold", False),
    ("s4w_4x8_c", lambda: st(10, 8, 4, 8, 3, seed=38, radius=2.5), "c", "k_spmm_s4w", "fold", False),     # two columns per lane (fused launches)
    ("s4w_4x32_c", lambda: st(10, 8, 4, 32, 2, seed=39, radius=3.1), "c", "k_spmm_s4w", "fold", False),   # four
    # 8-row blocks
    ("ilv8f_8x8_c", lambda: st(9, 7, 8, 8, 3, seed=41, radius=3.3), "c", "k_spmm_ilv8f", "fold", False),
    ("ilv8f_8x32_c", lambda: st(8, 6, 8, 32, 2, seed=42, radius=2.5), "c", "k_spmm_ilv8f", "fold", False),
    ("ilv8f_8x64_c", lambda: st(8, 6, 8, 64, 2, seed=43, radius=2.5), "c", "k_spmm_ilv8f", "fold", False),
    ("mfma8_8x9_c", lambda: st(9, 7, 8, 9, 3, seed=44, radius=3.3), "c", "k_spmm_mfma8", "fold", False),
    ("mfma8_8x10_c", lambda: st(9, 7, 8, 10, 3, seed=45, radius=3.3), "c", "k_spmm_mfma8", "fold", False),
    ("ilv8w_8x9_z", lambda: st(9, 7, 8, 9, 3, seed=46, radius=3.3), "z", "k_spmm_ilv8w", "fold", False),   # the ragged second column group
    ("ilv8w_8x10_z", lambda: st(9, 7, 8, 10, 3, seed=47, radius=3.3), "z", "k_spmm_ilv8w", "fold", False),
    ("ilv8w_8x64_z", lambda: st(8, 6, 8, 64, 2, seed=48, radius=2.5), "z", "k_spmm_ilv8w", "fold", False),
    ("ilv8w_8x64_z_unfolded", lambda: st(24, 20, 8, 64, 4, seed=49, radius=6.0), "z", "k_spmm_ilv8w", "unfold", False),
    ("ilv8_8x8_z", lambda: st(9, 7, 8, 8, 3, seed=40, radius=3.3), "z", "k_spmm_ilv8", "fold", False),
    ("ilv8b_8x8_z", lambda: st(60, 60, 8, 8, 2, seed=3), "z", "k_spmm_ilv8b", "unfold", False),          # column batches: identical dense columns
    # three adjacent long columns at LN = 64 (one block per chunk): several columns' shares in colPart at once (col_part_slot)
    ("ilv8w_8x64_z_three_segmented", lambda: st(20, 15, 8, 64, 3, seed=50), "z", "k_spmm_ilv8w", "segmented", False),
    # 16 | 32 | 64-row blocks
    ("mfma_16x64_z", lambda: st(8, 6, 16, 64, 2, seed=51, radius=2.5), "z", "k_spmm_mfma", "fold", False),
    ("mfma_64x64_z", lambda: st(6, 5, 64, 64, 2, seed=52, radius=2.0), "z", "k_spmm_mfma", "fold", False),
    ("mfma_32x64_z_three", lambda: st(7, 5, 32, 64, 2, seed=53, radius=2.5), "z", "k_spmm_mfma", "fold", True),
    ("mfma_16x64_z_unfolded", lambda: st(20, 20, 16, 64, 4, seed=54), "z", "k_spmm_mfma", "unfold", False),
    ("ilvf_16x64_c", lambda: st(8, 6, 16, 64, 2, seed=55, radius=2.5), "c", "k_spmm_ilvf", "fold", False),
    ("ilvf_64x64_c", lambda: st(6, 5, 64, 64, 2, seed=56, radius=2.0), "c", "k_spmm_ilvf", "fold", False),
    ("ilv16_onecol_z", lambda: load_problem_st16_onecol(), "z", "k_spmm_ilv16", "fold", False),        # one block column: A streamed past the caches
    ("ilv16f_onecol_c", lambda: load_problem_st16_onecol(), "c", "k_spmm_ilv16f", "fold", False),
    ("ilv16_16x16_z_unfolded", lambda: st(40, 40, 16, 16, 1, seed=57), "z", "k_spmm_ilv16", "unfold", False),
    ("ilv16_16x16_z_segmented", lambda: st(70, 60, 16, 16, 1, seed=58), "z", "k_spmm_ilv16", "segmented", False),   # > 1024 chunks at LN = 16
]


def load_problem_st16_onecol():
    return st(12, 12, 16, 16, 1, seed=7)     # tests/test_gpu_hash_mode.py: st16x16_onecol
