"""The DEFAULT shadow vector (counter-based hash) is what bench.py times: for 16 x 16 blocks the fused multiply kernels
do not even read it, they recompute it in registers (k_spmm_mfma<..., HASH = true>, tfq_spmm_mfma.hip).  These tests pin
that variant to the CPU oracle the same way the glibc-mode tests pin the other one: the oracle is fed with the very
same vector (numpy restatement of tfq_device.hpp: shadow_key / shadow_value) and must take the same iterations
with the same bound history (reference algorithm: tfqmrgpu_core.hxx:189-304).  Needs an MI355X (`pytest -m gpu`)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tfqmrgpu_amd as T
from conftest import ROOT, load_problem, offset1
from solve_helpers import HASH_CASES as CASES
from solve_helpers import STATE_CASES, STATE_ITERATIONS
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("name", sorted(CASES))
def test_device_shadow_vector_is_the_documented_hash(name):
    pr = CASES[name]()
    for p in (pr, offset1(pr)):                       # Fortran indices must give the same vector (original column - offset)
        for prec in "zc":
            with T.Solver() as s:
                s.create_plan(p)
                s.set_buffer(nbytes=s.buffer_size(p.LM, p.LN, prec))
                got = s.get_shadow_vector()
            want = T.hash_shadow_vector(p)
            assert got.dtype == want.dtype == np.float32 and np.array_equal(got, want), (name, prec)
            assert want.min() > 0 and want.max() <= 1


# Tolerances = 2 x the deviation observed on MI355X (tests/parity_report.py -> profiles/r02_parity_report.txt) between
# the HIP path and the oracle fed with the same vector: (whole bound history, its first half, final residual), relative.
# How far rounding differences are amplified depends on the shadow vector; each entry is the larger of the values seen
# with the arithmetic variants this library has had (one hash per real until mid round 2 | one per four reals; compiler-contracted |
# explicit fused multiply-adds in the epilogues and vector kernels).
# Everything that ends at the threshold agrees to about 1e-6 (a residual of 1e-10 |b| is itself only known to ~1e-6: eps |A||x| / |r|);
# the 3-D Poisson system at energy 0 (fd_8x8_3d) sheds 8 digits per iteration at the end, there the first half of the
# history is what can be compared tightly.
Z_TOL = {
    "fd_16x16_2d": (2e-10, 3e-11, 1.3e-6),    # observed 6.5e-11 / 1.2e-11 / 6.2e-7
    "fd_16x16_small": (3e-10, 1e-10, 2e-6),   # 1.1e-10 / 4.8e-11 / 7.6e-7
    "dense_random": (1e-10, 2e-12, 1e-4),     # 4.4e-11 / 6.9e-13 / 4.6e-5 (the residual 4e-12 is rounding noise)
    "stencil_8x8": (1e-10, 2e-12, 1e-6),      # 9.7e-12 / 6.6e-13 / 4.3e-7
    "stencil_8x32": (1e-10, 2e-11, 1e-5),     # 1.1e-11 / 5.8e-12 / 4.8e-6
    "st16x16": (2e-10, 2e-12, 3e-6),          # 5.2e-11 / 9.7e-13 / 1.1e-6
    "st16x16_ragged": (1e-11, 1e-12, 1e-7),   # 1.8e-12 / 1.2e-13 / 3.8e-8
    "st16x16_onecol": (2e-11, 1e-12, 1e-7),   # 9.4e-12 / 2.3e-13 / 2.3e-8
    "st32x32": (2e-11, 1e-12, 1e-6),          # 7.3e-12 / 5.6e-14 / 4.5e-7
    "fd_8x8_3d": (1.2, 2e-8, 0.55),           # 5.7e-1 / 6.6e-9 / 2.6e-1
    "fd_4x4_2d": (8e-6, 2e-9, 1.2e-5),        # 3.7e-6 / 6.2e-10 / 6.0e-6
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hash_mode_takes_the_oracles_trajectory_z(oracle, name):
    pr = CASES[name]()
    tol = {"dense_random": 1e-10}.get(name, pr.tolerance)
    st, X, info = T.solve_problem(pr, "z", threshold=tol, max_iterations=300)
    st0, X0, info0 = oracle.solve(pr, "z", threshold=tol, max_iterations=300, v3=T.hash_shadow_vector(pr).reshape(-1))
    assert st == st0 == 0
    assert info["iterations"] == info0["iterations"], "same shadow vector, same decisions (tfqmrgpu_core.hxx:239-298)"
    assert info["flops"] == info0["flops"]
    h, h0 = info["bound_history"], info0["bound_history"]
    htol, half_tol, rtol = Z_TOL[name]
    half = (len(h0) + 1) // 2
    assert len(h) == len(h0) and np.allclose(h, h0, rtol=htol, atol=0), np.abs(h / h0 - 1).max()
    assert np.allclose(h[:half], h0[:half], rtol=half_tol, atol=0), np.abs(h[:half] / h0[:half] - 1).max()
    assert abs(info["residual"] - info0["residual"]) <= rtol * info0["residual"], info["residual"] / info0["residual"] - 1   # (not pytest.approx: abs 1e-12)
    assert np.abs(X - X0).max() <= 1e-7 * np.abs(X0).max()


# the complex<double> shapes with 32 and 64 columns (k_spmm_mfma on the native order), four-product form | three-product form (opt-in);
# observed on MI355X (scripts/zwide_report.py): history within 2e-10, its first half 2e-12, residual 8e-6, solution 4e-15 of the oracle's
Z_WIDE = {"st16x32": lambda: PR.stencil_2d(7, 6, 16, 32, 2, seed=13), "st16x64": lambda: PR.stencil_2d(6, 5, 16, 64, 2, seed=5),
          "st32x64": lambda: PR.stencil_2d(5, 5, 32, 64, 2, seed=6), "st64x64": lambda: PR.stencil_2d(4, 4, 64, 64, 2, seed=8),
          "st32x32_ragged": lambda: PR.stencil_2d(6, 5, 32, 32, 3, seed=17, radius=2.4)}
Z_WIDE_TOL = (1e-9, 1e-11, 4e-5, 1e-13)    # history, its first half, residual, solution


@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("name", sorted(Z_WIDE))
def test_wide_z_shapes_take_the_oracles_trajectory(oracle, name, three):
    pr = Z_WIDE[name]()
    st, X, info = T.solve_problem(pr, "z", threshold=pr.tolerance, max_iterations=300, three_products=three)
    st0, X0, info0 = oracle.solve(pr, "z", threshold=pr.tolerance, max_iterations=300, v3=T.hash_shadow_vector(pr).reshape(-1))
    assert st == st0 == 0 and info["iterations"] == info0["iterations"]
    h, h0 = info["bound_history"], info0["bound_history"]
    htol, half_tol, rtol, xtol = Z_WIDE_TOL
    half = (len(h0) + 1) // 2
    assert len(h) == len(h0) and np.allclose(h, h0, rtol=htol, atol=0), np.abs(h / h0 - 1).max()
    assert np.allclose(h[:half], h0[:half], rtol=half_tol, atol=0), np.abs(h[:half] / h0[:half] - 1).max()
    assert abs(info["residual"] - info0["residual"]) <= rtol * info0["residual"], info["residual"] / info0["residual"] - 1
    assert np.abs(X - X0).max() <= xtol * np.abs(X0).max()


# 64 columns in complex<float>: k_spmm_ilvf on column halves (r03; two waves of a work group per half, their own record sums)
C_WIDE = {"st16x64": lambda: PR.stencil_2d(6, 5, 16, 64, 2, seed=5), "st32x64": lambda: PR.stencil_2d(5, 5, 32, 64, 2, seed=6),
          "st64x64": lambda: PR.stencil_2d(4, 4, 64, 64, 2, seed=8), "st32x64_ragged": lambda: PR.stencil_2d(5, 4, 32, 64, 3, seed=11, radius=2.2)}


@pytest.mark.parametrize("name", ["fd_16x16_2d", "fd_16x16_small", "st16x16", "st16x16_ragged", "st16x16_onecol", "st32x32", "stencil_8x8"] + sorted(C_WIDE))
def test_hash_mode_against_the_oracle_c(oracle, name):
    # complex<float>: both sides round every product to 24 bits in a different order, the trajectories separate after a
    # few iterations: the first two bounds agree to 1e-3, the count to within one iteration, both converge
    pr = {**CASES, **C_WIDE}[name]()
    tol = 1e-4
    st, X, info = T.solve_problem(pr, "c", threshold=tol, max_iterations=300)
    st0, X0, info0 = oracle.solve(pr, "c", threshold=tol, max_iterations=300, v3=T.hash_shadow_vector(pr).reshape(-1))
    assert st == st0 == 0
    assert abs(info["iterations"] - info0["iterations"]) <= 1, (info["iterations"], info0["iterations"])
    # (st64x64 sheds five digits of bound^2 per iteration: its second bound, 1.3e-4 of the first, is already within 1.2e-3 of float rounding)
    assert np.allclose(info["bound_history"][:2], info0["bound_history"][:2], rtol=3e-3 if "st64x64" == name else 1e-3, atol=0)
    assert np.allclose(info["bound_history"][:1], info0["bound_history"][:1], rtol=1e-4, atol=0)
    assert info["residual"] <= tol and np.abs(X - X0).max() <= 1e-3 * np.abs(X0).max()


def _worker(tmp_path, tag, name, prec, tol, **env):
    out = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_env_worker.py"), out, name, prec, repr(tol)],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("name,prec,tol", [("fd_16x16_2d", "z", 1e-9), ("fd_16x16_2d", "c", 1e-4),
                                           ("stencil:12:12:16:16:4:7:5", "z", 1e-9)])
def test_recomputing_the_shadow_vector_changes_no_bit(tmp_path, name, prec, tol):
    # TFQMRGPU_HASHV3=0 makes the 16 x 16 multiply kernels READ v3 (HASH = false, the variant the glibc-mode tests cover)
    a = _worker(tmp_path, "recompute", name, prec, tol, TFQMRGPU_HASHV3=1)
    b = _worker(tmp_path, "read", name, prec, tol, TFQMRGPU_HASHV3=0)
    assert int(a["status"]) == int(b["status"]) == 0 and int(a["iterations"]) == int(b["iterations"])
    assert np.array_equal(a["history"], b["history"]) and float(a["residual"]) == float(b["residual"])
    assert np.array_equal(a["X"], b["X"])


SWITCHES = [dict(TFQMRGPU_3M=1), dict(TFQMRGPU_3M=2), dict(TFQMRGPU_EPI_PREFETCH=0), dict(TFQMRGPU_ORDER=0),
            dict(TFQMRGPU_DEPTH=1), dict(TFQMRGPU_DEPTH=4), dict(TFQMRGPU_CHUNK_KIB=64), dict(TFQMRGPU_ORDER_G=8),
            dict(TFQMRGPU_ILV=0),     # ILV=0: 16 x 16 and 8 x 8 z plans keep the native element order (k_spmm_mfma / k_spmm_mfma8)
            dict(TFQMRGPU_A_STREAM=0), dict(TFQMRGPU_CLAMP=0),
            dict(TFQMRGPU_FOLD_MAX=0),   # the column operations as launches of their own (plans of at most 384 chunks fold them into the producers' tails)
            dict(TFQMRGPU_FOLD_MAX=100000)]   # ... and folded where the product does not (the first fixture below has 256 chunks)


@pytest.mark.parametrize("name,prec,tol", [("stencil:16:16:16:16:4:7:5", "z", 1e-9), ("stencil:8:8:32:32:2:3:13", "z", 1e-9),
                                           ("stencil:12:12:8:8:4:5:5", "z", 1e-9), ("stencil:12:12:16:16:1:7:5", "z", 1e-9)])   # one block column: A streamed past the caches
def test_tuning_switches_change_code_paths_not_results(tmp_path, name, prec, tol):
    """every non-default value of the tuning switches (read by the LAB build only, the product has them frozen):
    same status and iteration count, the solution within rounding (a switch may change the order of a sum: chunk length,
    three-product form).  The base line is the PRODUCT, so the lab build with every switch at its default is checked against it too."""
    base = _worker(tmp_path, "default", name, prec, tol)
    lab = _worker(tmp_path, "lab_default", name, prec, tol, TFQMRGPU_DEPTH=0)      # (0 = default) loads the lab build
    assert np.array_equal(lab["X"], base["X"]) and np.array_equal(lab["history"], base["history"])
    assert int(base["status"]) == 0
    for n, sw in enumerate(SWITCHES):
        got = _worker(tmp_path, "sw%d" % n, name, prec, tol, **sw)
        assert int(got["status"]) == 0 and int(got["iterations"]) == int(base["iterations"]), sw
        assert np.allclose(got["history"], base["history"], rtol=1e-6, atol=0), sw
        assert np.abs(got["X"] - base["X"]).max() <= 1e-9 * np.abs(base["X"]).max(), sw
        if "TFQMRGPU_DEPTH" in sw or "TFQMRGPU_ORDER" in sw or "TFQMRGPU_ORDER_G" in sw or "TFQMRGPU_A_STREAM" in sw or "TFQMRGPU_FOLD_MAX" in sw:
            assert np.array_equal(got["X"], base["X"]), sw   # these change WHEN things run, never what is added to what


# Long columns: the column kernels sum a column of more than 4 x col_seg_len(LN) chunks in col_segments shares (several work groups, then the
# shares in order), so a plan with such a column must never fold its column operations into the multiplies' tails, where one work group
# sums the whole column in another order.  Each fixture proves the path it stands for with the restated chunk and segment rules.
FOLD_LIMIT_CASES = [("stencil:20:15:8:64:1:5:5", 300, True),      # 8 x 64 z (k_spmm_ilv8w), one block per chunk: 300 chunks, 5 segments, <= 384
                    ("stencil:40:30:16:64:1:5:5", 300, True),     # 16 x 64 z (k_spmm_mfma), 4 blocks per chunk: the same column of 300 chunks
                    ("stencil:70:60:16:16:1:7:5", 1050, False)]   # 16 x 16 z (k_spmm_ilv16): 1050 chunks (5 segments at LN = 16), past kFoldMax


@pytest.mark.parametrize("name,chunks,small", FOLD_LIMIT_CASES)
def test_fold_limit_changes_no_bit_of_a_segmented_column(tmp_path, name, chunks, small):
    """the product, the lab build with TFQMRGPU_FOLD_MAX=0 (never fold) and with 100000 (fold every plan the rule allows): the order of every
    column sum depends on (chunks of the column, LN) alone, so the solve must not differ in a single bit"""
    import _env_worker
    from plan_paths import FOLD_MAX, plan_paths
    pr = _env_worker.problem(name)
    ch, seg, folds = plan_paths(pr, "z")
    assert ch == [chunks] and seg[0] > 1 and (sum(ch) <= FOLD_MAX) == small and not folds
    base = _worker(tmp_path, "default", name, "z", 1e-9)
    assert int(base["status"]) == 0
    for n, sw in enumerate([dict(TFQMRGPU_FOLD_MAX=0), dict(TFQMRGPU_FOLD_MAX=100000)]):
        got = _worker(tmp_path, "fold%d" % n, name, "z", 1e-9, **sw)
        assert int(got["status"]) == 0 and int(got["iterations"]) == int(base["iterations"]), sw
        assert np.array_equal(got["history"], base["history"]) and float(got["residual"]) == float(base["residual"]), sw
        assert np.array_equal(got["X"], base["X"]), sw


@pytest.mark.parametrize("name", ["stencil:40:40:8:8:5:7:5", "stencil:60:60:8:8:2:3:5", "stencil:64:40:8:8:3:11:5"])   # batches (2, 2, 1) | (2) | (2, 1) of block columns; 500 | 450 | 480 chunks (plans of at most 384 fold their column operations instead)
def test_column_batches_change_no_bit(tmp_path, name):
    """8 x 8 complex<double>: block columns with identical row patterns are multiplied two at a time (k_spmm_ilv8b: one A fetch for both, plans of more
    than 384 chunks; profiles/r03_column_batches.txt).  Chunks, records and every sum are those of the one-column kernel: against the lab build with
    TFQMRGPU_BATCH=1 (batches off) the solve must not differ in a single bit -- iteration count, bound history, residual, solution."""
    on = _worker(tmp_path, "batched", name, "z", 1e-9)
    off = _worker(tmp_path, "single", name, "z", 1e-9, TFQMRGPU_BATCH=1)
    assert int(on["status"]) == int(off["status"]) == 0 and int(on["iterations"]) == int(off["iterations"])
    assert np.array_equal(on["history"], off["history"]) and float(on["residual"]) == float(off["residual"])
    assert np.array_equal(on["X"], off["X"])


def test_plain_mode_xcd_mapping(tmp_path):
    """lab switch TFQMRGPU_PLAIN_XCD (native-API multiply: contiguous eighths of the caller's Y blocks per XCD instead of round-robin work
    groups; profiles/r03_native_multiply.txt): which work group computes a Y block changes, the product does not -- on BASELINE config 1's plan."""
    got = {}
    for tag, env in (("product", {}), ("lab", dict(TFQMRGPU_PLAIN_XCD=0)), ("eighths", dict(TFQMRGPU_PLAIN_XCD=1))):
        out = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_multiply_worker.py"), out],
                           env=dict(os.environ, **{k: str(v) for k, v in env.items()}), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        got[tag] = np.load(out)
    assert str(got["product"]["lib"]) == "libtfQMRgpu.so" and str(got["eighths"]["lib"]) == "libtfQMRgpu_lab.so"
    assert np.abs(got["product"]["Y"]).max() > 1
    assert np.array_equal(got["product"]["Y"], got["lab"]["Y"]) and np.array_equal(got["product"]["Y"], got["eighths"]["Y"])


@pytest.mark.parametrize("name,prec,tol,switch,xtol", [
    ("stencil:40:40:4:4:3:5:5", "z", 1e-9, dict(TFQMRGPU_M4=0), 1e-9), ("stencil:40:40:4:8:3:5:5", "z", 1e-9, dict(TFQMRGPU_M4=0), 1e-9),
    ("stencil:24:24:4:32:2:5:5", "z", 1e-9, dict(TFQMRGPU_M4=0), 1e-9),       # k_spmm_m4 against k_spmm_small4 | the tile of k_spmm_mfma8 (one running sum per Y block)
    ("stencil:40:40:4:8:3:5:5", "c", 1e-4, dict(TFQMRGPU_S4W=0), 2e-4), ("stencil:24:24:4:32:2:5:5", "c", 1e-4, dict(TFQMRGPU_S4W=0), 2e-4),   # k_spmm_s4w against k_spmm_small4
    ("stencil:40:40:4:4:3:5:5", "c", 1e-4, dict(TFQMRGPU_S4W=2), 2e-4)])      # ... and fused on 4 x 4 c, where the product keeps k_spmm_small4
def test_four_row_kernels_against_the_kernels_they_replaced(tmp_path, name, prec, tol, switch, xtol):
    """r04: the 4-row shapes moved to new multiply kernels; the ones they replaced stay reachable in the lab build (TFQMRGPU_M4=0, TFQMRGPU_S4W=0): same status and
    iteration count, the solution within rounding (the sums of a chunk's records are grouped differently; k_spmm_m4 adds the products of a Y block in one running sum)"""
    new = _worker(tmp_path, "new", name, prec, tol)
    old = _worker(tmp_path, "old", name, prec, tol, **switch)
    assert int(new["status"]) == int(old["status"]) == 0 and int(new["iterations"]) == int(old["iterations"])
    assert np.allclose(new["history"][: (len(new["history"]) + 1) // 2], old["history"][: (len(old["history"]) + 1) // 2], rtol=1e-6 if prec == "z" else 2e-2, atol=0)
    assert np.abs(new["X"] - old["X"]).max() <= xtol * np.abs(old["X"]).max()


def test_native_16x16_multiply_through_the_lds_patch_changes_no_bit(tmp_path):
    """k_spmm_n16 (r04: the stand-alone 16 x 16 multiply on the caller's planes with its operands through a wave-private LDS patch as 16-byte accesses; float ships,
    double is a lab option) against k_spmm_mfma (4 | 8-byte operand loads, lab switch TFQMRGPU_N16=0): same k-steps, same order of the four real products --
    not a bit of the product on BASELINE config 1's plan may differ, in either precision."""
    def run(tag, prec, **env):
        out = str(tmp_path / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_multiply_worker.py"), out, prec],
                           env=dict(os.environ, **{k: str(v) for k, v in env.items()}), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return np.load(out)
    c_product, c_direct, c_patch = run("c_product", "c"), run("c_direct", "c", TFQMRGPU_N16=0), run("c_patch", "c", TFQMRGPU_N16=1)
    assert str(c_product["lib"]) == "libtfQMRgpu.so" and str(c_direct["lib"]) == "libtfQMRgpu_lab.so"
    assert np.abs(c_product["Y"]).max() > 1 and c_product["Y"].dtype == np.float32
    assert np.array_equal(c_product["Y"], c_direct["Y"]) and np.array_equal(c_product["Y"], c_patch["Y"])
    z_direct, z_patch = run("z_direct", "z", TFQMRGPU_N16=0), run("z_patch", "z", TFQMRGPU_N16=3)
    assert np.array_equal(z_direct["Y"], z_patch["Y"])


# ---- kernel-level state parity (axpy/xpay, dotp/nrm2, dec35/dec34/decT) ----------------------------
# After exactly k iterations every work vector is the output of one kernel of the slot (x, v6, v7: k_x_v6_v7; v4, v9:
# the EPI_XPAY_DOT multiply; v5, v8: the EPI_AXPY_NRM_DOT multiply and k_v5_nrm), computed with the per-RHS scalars of
# the decision kernels.  tfqmrgpuExt_getWorkVector hands them out; the oracle (fed with the same shadow vector) dumps
# its own at the end of the same iteration (tfqmrgpu_core.hxx:189-233).  A bug in a fused kernel that cancelled over an
# iteration would show here in the vector it writes.  Bounds per k = 4 x the worst deviation observed on MI355X
# (tests/parity_report.py -> profiles/r02_parity_report.txt, both hash definitions): after one iteration every vector agrees to
# 14 digits (5 in float); later the recurrences amplify the rounding differences while the vectors themselves shrink with the residual
# (st32x32 converges by two digits per iteration: in float its vectors are rounding noise at k = 5, not compared).
# (the table itself: tests/solve_helpers.py, shared with tests/parity_report.py)


@pytest.mark.parametrize("name,prec,bounds", STATE_CASES)
@pytest.mark.parametrize("k", STATE_ITERATIONS)
def test_work_vectors_after_k_iterations_match_the_oracle(oracle, name, prec, bounds, k):
    if k not in bounds:
        pytest.skip("rounding noise at this iteration (see the table above)")
    pr = CASES[name]()
    v3 = T.hash_shadow_vector(pr).reshape(-1)
    st0, X0, info0 = oracle.solve(pr, prec, threshold=1e-30, max_iterations=k, v3=v3, dump_iteration=k)
    with T.Solver() as s:
        s.create_plan(pr)
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, prec))
        s.set_matrix("A", pr.A, "n")
        s.set_matrix("B", pr.B, "n")
        st = s.solve(1e-30, k)
        got = {w: s.get_work_vector(w) for w in (1, 4, 5, 6, 7, 8, 9)}
        X = s.get_matrix()
    assert st == st0 == 9                                     # out of iterations on both sides (tfqmrgpu_core.hxx:258)
    assert np.array_equal(got[1], X)                          # the getter and getMatrix('X') agree
    worst = {}
    for w, want in info0["vectors"].items():
        scale = np.abs(want).max()
        assert scale > 0, w
        worst[w] = np.abs(got[w] - want).max() / scale
    assert max(worst.values()) <= bounds[k], worst


def test_work_vector_getter_refuses_what_it_cannot_give():
    pr = CASES["fd_16x16_2d"]()
    with T.Solver() as s:
        s.create_plan(pr)
        out = np.zeros((pr.nnzbX, 2, pr.LM, pr.LN))
        st = T.lib.tfqmrgpuExt_getWorkVector(s.handle, s.plan, 4, T._ptr(out))
        assert T.decode(st)[0] == 7                                   # no buffer registered yet: TFQMRGPU_POINTER_INVALID
        s.set_buffer(nbytes=s.buffer_size(pr.LM, pr.LN, "z"))
        for which in (0, 2, 3, 10, -1):                                # v2 (= B) and v3 (float) are not X-shaped work vectors of this getter
            st = T.lib.tfqmrgpuExt_getWorkVector(s.handle, s.plan, which, T._ptr(out))
            assert T.decode(st)[0] == 18, which                        # TFQMRGPU_VARIABLENAME_UNKNOWN
        assert T.lib.tfqmrgpuExt_getWorkVector(s.handle, s.plan, 4, None) % 1000 == 7


# ---- a solve does not depend on what the work buffer held before -----------------------------------------------------------
# The first iteration treats v4, v6, v7, v8 and x as the zeros they are by definition (tfqmrgpu_core.hxx:125,147-151) without
# reading them, and the start of a solve clears only v5 (DevPlan::first): a buffer full of NaN bit patterns must give the very
# bits of a buffer full of zeros -- for every multiply kernel family (interleaved, MFMA tiles, 8-row tiles, 4-row, operator path).
POISON_CASES = [("fd_16x16_2d", "z"), ("fd_16x16_2d", "c"), ("stencil_8x8", "z"), ("st32x32", "c"), ("st32x32", "z"), ("stencil_8x32", "c"),
                ("fd_4x4_2d", "z"), ("st16x16_onecol", "z")]


@pytest.mark.parametrize("name,prec", POISON_CASES)
def test_solve_does_not_depend_on_the_previous_buffer_content(name, prec):
    import torch
    pr = CASES[name]()
    tol = pr.tolerance if prec == "z" else 1e-4
    out = {}
    for fill in (0x00, 0xFF):                                   # 0xFF bytes: NaN in float and double
        with T.Solver() as s:
            s.create_plan(pr)
            nbytes = s.buffer_size(pr.LM, pr.LN, prec)
            buf = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
            s.set_buffer(device_ptr=buf.data_ptr())
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(tol, 300)
            info = s.get_info()
            X = s.get_matrix()
            st1 = s.solve(tol, 1)                               # and a solve of one iteration on the used buffer
            X1 = s.get_matrix()
            st0 = s.solve(tol, 0)                               # no iteration at all: X is the initial guess, zero
            X0 = s.get_matrix()
        out[fill] = (st, info["iterations"], info["residual"], X, st1, X1)
        assert st0 == 9 and not X0.any()
        assert np.isfinite(X).all() and np.isfinite(X1).all()
    a, b = out[0x00], out[0xFF]
    assert a[:3] == b[:3] and a[4] == b[4]
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[5], b[5])
