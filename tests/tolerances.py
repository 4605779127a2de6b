"""Per-fixture tolerances of the GPU-against-oracle comparisons (tests/test_gpu_parity.py), kept in a module of their own so
that tests/test_oracle_sensitivity.py can hold them against the fixtures' own rounding sensitivity without a GPU."""

# Rounding differences (MFMA summation order, FMA contraction, other reduction order) are amplified by the tfQMR
# recurrences; how fast depends on the conditioning.  The tolerances below are 2 x the deviation OBSERVED on MI355X
# against the oracle with the same (glibc) shadow vector (tests/parity_report.py -> profiles/r02_parity_report.txt; the
# largest of the values seen with the arithmetic variants the library has had: round-1 and round-2 multiply kernels,
# compiler-contracted and explicit fused multiply-adds),
# per fixture: hist = whole per-iteration bound history (relative), half = its first half, res = final residual
# (relative).  The north star's "residuals matching to 1e-6 relative" holds on every fixture whose final residual sits
# at the threshold (1e-10 .. 1e-9: the 16x16 FD systems that bench.py times, the stencils, the dense system); where the
# solve ends in rounding noise (julia_kat: 5e-15; 3-D Poisson at energy 0, fd_8x8_3d: the last iterations shed 8 digits
# per step) or the blocks are 4x4 (longer sums in another order) the END of the trajectory differs more and the table
# says by how much; the first half of the history agrees to 1e-7 everywhere.
Z_TOL = {
    "fd_16x16_2d":       dict(hist=3e-10, half=4e-11, res=3e-7),    # observed 1.3e-10 / 2.0e-11 / 1.1e-7
    "fd_16x16_small":    dict(hist=3e-10, half=3e-11, res=3e-7),    # 1.4e-10 / 1.1e-11 / 1.4e-7
    "dense_random":      dict(hist=3e-10, half=2e-12, res=5e-6),    # 1.1e-10 / 6.8e-13 / 2.3e-6
    "stencil_8x8":       dict(hist=1e-11, half=1e-12, res=2e-6),    # 9.5e-13 / 1.7e-13 / 1.0e-6
    "stencil_8x32":      dict(hist=1e-10, half=1e-12, res=3e-7),    # 4.3e-11 / 2.6e-13 / 1.3e-7
    "dense_random_rect": dict(hist=1e-10, half=1e-12, res=8e-6,     # 4.5e-11 / 2.4e-13 / 3.7e-6 (residual 2e-11: noise floor; r04, k_spmm_m4 --
                              hist_floor=1e-18),                    # one running MFMA sum over the products of a Y block: 4.5e-10 in the LAST entry, 1.2e-20,
                                                                    # below hist_floor: entries under it are compared absolutely, to hist x hist_floor)
    "fd_4x4_2d":         dict(hist=2e-5,  half=1e-10, res=8e-5),    # 9.2e-6  / 2.0e-11 / 3.8e-5
    "fd_8x8_3d":         dict(hist=1.7,   half=1.4e-7, res=0.52),   # 8.5e-1  / 7.0e-8  / 2.6e-1 (both below the threshold)
    "julia_kat":         dict(hist=1.3,   half=1e-14, res=0.5),     # 6.5e-1  / 2.2e-15 / 2.4e-1 (converges to 5e-15)
}
# complex<float>: the trajectories separate after a few iterations (every product is rounded to 24 bits in another order).
# it = allowed difference of the iteration count, x = max|X - X0| / max|X0|; observed: equal counts everywhere but on the
# 3-D Poisson fixture at its float floor (tol 1e-2: 26 against 21 iterations, both converged, X within 0.6 * tol).
C_TOL = {
    "fd_8x8_3d": dict(it=10, x=1.2e-2), "fd_16x16_2d": dict(it=0, x=1.1e-4), "fd_16x16_small": dict(it=0, x=2.2e-4),
    "julia_kat": dict(it=0, x=4e-6), "dense_random": dict(it=0, x=6e-7), "stencil_8x8": dict(it=0, x=4e-7),
}
