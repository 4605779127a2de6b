"""The "late v5" form of the iteration slot (DevPlan::lateV5; tfq_solve.hpp: late_v5): on plans whose fused multiplies run on k_spmm_ilv16
and that do not fold, k_v5_nrm sums |v5 + alfa v9|^2 without storing v5 and the second fused multiply applies that half step in its epilogue,
in front of its own -- the same two fused multiply-adds on the same operands.  So the slot in which k_v5_nrm stores v5 (lab build,
TFQMRGPU_LATE_V5=0) and the new one must agree in every bit: status, iteration count, residual, the whole bound history and X.  Every
setting of the switch runs in a child process of its own (tests/_late_v5_worker.py), as the fold switch does in tests/test_gpu_hash_mode.py.
Needs an MI355X (`pytest -m gpu`)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _env_worker
import tfqmrgpu_amd as T
from conftest import ROOT
from helpers import same_typed_bits
from plan_paths import FOLD_MAX, plan_paths

pytestmark = pytest.mark.gpu

# 16 x 16 z, three dense block columns of 23 x 23 = 529 blocks: four blocks per chunk (one per wave), so 133 chunks per column with a ragged last
# one (one block), 399 chunks in all -- past the fold limit of 384 on its own
RAGGED = "stencil:23:23:16:16:3:7:5"
GOLDEN = "fd_16x16_2d"        # 1017 blocks, 261 chunks: folds unless the lab build is told not to
PROBES_TOL = 1e-12            # RAGGED to this threshold: the first probe does not end the solve
BIG_8X8 = "stencil:40:40:8:8:5:7:5"   # 8 x 8 z, 500 chunks: unfolded, on k_spmm_ilv8 | k_spmm_ilv8b


def run(tmp_path, tag, name, tol, modes, **env):
    out = str(tmp_path / (tag + ".npz"))
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_late_v5_worker.py"), out, name, repr(tol), modes],
                       env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def assert_same_solve(a, b, mode, what):
    for key in ("status", "iterations", "probes"):
        assert int(a[mode + "/" + key]) == int(b[mode + "/" + key]), (what, mode, key, int(a[mode + "/" + key]), int(b[mode + "/" + key]))
    assert same_typed_bits(a[mode + "/residual"], b[mode + "/residual"]), (what, mode, float(a[mode + "/residual"]), float(b[mode + "/residual"]))
    assert same_typed_bits(a[mode + "/history"], b[mode + "/history"]), (what, mode, a[mode + "/history"], b[mode + "/history"])
    assert same_typed_bits(a[mode + "/X"], b[mode + "/X"]), (what, mode, np.abs(a[mode + "/X"] - b[mode + "/X"]).max())


def test_ragged_unfolded_plan_old_and_new_slot_agree_bit_for_bit(tmp_path):
    """the product (new slot) against the lab build with the old and with the new slot: a solve to the threshold, a solve of one iteration
    (the first-iteration instances alone), and a warm start on the same plan (the right-hand side is the X-shaped R)"""
    ch, seg, folds = plan_paths(_env_worker.problem(RAGGED), "z")
    assert ch == [133, 133, 133] and sum(ch) > FOLD_MAX and not folds     # 529 blocks per column, four per chunk: the last chunk holds one
    modes = "solve,one,from"
    new = run(tmp_path, "product", RAGGED, 1e-9, modes)
    old = run(tmp_path, "old", RAGGED, 1e-9, modes, TFQMRGPU_LATE_V5=0)
    lab = run(tmp_path, "lab", RAGGED, 1e-9, modes, TFQMRGPU_LATE_V5=1)
    assert str(new["lib"]) == "libtfQMRgpu.so" and str(old["lib"]) == str(lab["lib"]) == "libtfQMRgpu_lab.so"
    assert str(new["family"]) == str(old["family"]) == "k_spmm_ilv16"
    assert bool(new["late"]) and bool(lab["late"]) and not bool(old["late"])
    assert int(old["solve/status"]) == 0 and int(old["solve/iterations"]) >= 2
    assert int(old["one/status"]) == 9 and int(old["one/iterations"]) == 1
    assert int(old["from/status"]) == 0 and int(old["from/iterations"]) >= 2
    for mode in modes.split(","):
        assert np.isfinite(old[mode + "/X"]).all() and np.abs(old[mode + "/X"]).max() > 0
        assert_same_solve(new, old, mode, "product")
        assert_same_solve(lab, old, mode, "lab")


def test_golden_plan_with_folding_off_agrees_bit_for_bit(tmp_path):
    """the golden 16 x 16 system (1017 blocks, 261 chunks) folds on its own; with the fold limit at 0 it runs the unfolded slot, old and new"""
    modes = "solve,one"
    old = run(tmp_path, "old", GOLDEN, 1e-9, modes, TFQMRGPU_FOLD_MAX=0, TFQMRGPU_LATE_V5=0)
    new = run(tmp_path, "new", GOLDEN, 1e-9, modes, TFQMRGPU_FOLD_MAX=0, TFQMRGPU_LATE_V5=1)
    assert bool(new["late"]) and not bool(old["late"]) and str(new["family"]) == "k_spmm_ilv16"
    assert int(old["solve/status"]) == 0 and int(old["solve/iterations"]) >= 2 and int(old["solve/probes"]) >= 2   # 13 iterations, two probes
    for mode in modes.split(","):
        assert_same_solve(new, old, mode, GOLDEN)


@pytest.mark.parametrize("case", ["zero_rhs:16x16", "dec34:16x16"])
def test_breakdown_cases_agree_bit_for_bit(tmp_path, case):
    """a right-hand side that is zero (tau = 0, and z = 0 half a step earlier) and one that breaks down in dec34 (alfa = 0 from then on: both half
    steps leave v5 as it is), next to healthy neighbours; the fixtures are small and fold, so the fold limit is 0 on both sides"""
    old = run(tmp_path, "old", "breakdown:" + case, 1e-9, "solve", TFQMRGPU_FOLD_MAX=0, TFQMRGPU_LATE_V5=0)
    new = run(tmp_path, "new", "breakdown:" + case, 1e-9, "solve", TFQMRGPU_FOLD_MAX=0, TFQMRGPU_LATE_V5=1)
    assert bool(new["late"]) and not bool(old["late"])
    assert int(old["solve/iterations"]) >= 2
    assert_same_solve(new, old, "solve", case)


def test_which_plans_take_the_late_slot():
    """on: an unfolded 16 x 16 z plan with the built-in operator.  Off: the same plan with a user-defined operator, a plan that folds, an 8 x 8 z
    plan (another multiply family), a 16 x 16 c plan (the float family)"""
    with T.Solver.open(_env_worker.problem(RAGGED), "z") as s:
        assert s.multiply_kernel() == "k_spmm_ilv16" and s.late_v5()
        s.set_operator(lambda *a: 0.)
        assert not s.late_v5()
        s.set_operator(None)
        assert s.late_v5()
    with T.Solver.open(_env_worker.problem(GOLDEN), "z") as s:
        assert s.multiply_kernel() == "k_spmm_ilv16" and not s.late_v5()
    pr = _env_worker.problem(BIG_8X8)
    assert not plan_paths(pr, "z")[2]
    with T.Solver.open(pr, "z") as s:
        assert s.multiply_kernel().startswith("k_spmm_ilv8") and not s.late_v5()
    with T.Solver.open(_env_worker.problem(RAGGED), "c") as s:
        assert s.multiply_kernel() == "k_spmm_ilv16f" and not s.late_v5()
    on = T.C.c_int32(0)
    with T.Solver() as s:
        s.create_plan(_env_worker.problem(GOLDEN))
        s.buffer_size(16, 16, "z")
        assert T.decode(T.lib.tfqmrgpuExt_getLateV5(s.plan, T.C.byref(on)))[0] == 7      # no buffer yet: TFQMRGPU_POINTER_INVALID
        assert T.decode(T.lib.tfqmrgpuExt_getLateV5(None, T.C.byref(on)))[0] == 7


def test_a_solve_of_several_probes_agrees_bit_for_bit(tmp_path):
    """a probe reads x and runs the multiply with the residual epilogue between two slots: a threshold at which the first probe does not
    end the solve, so that iterations follow a probe"""
    old = run(tmp_path, "old", RAGGED, PROBES_TOL, "solve", TFQMRGPU_LATE_V5=0)
    new = run(tmp_path, "new", RAGGED, PROBES_TOL, "solve")
    assert bool(new["late"]) and not bool(old["late"])
    assert int(old["solve/probes"]) >= 2, int(old["solve/probes"])
    assert_same_solve(new, old, "solve", "probes")


def test_two_ranks_old_and_new_slot_agree_bit_for_bit(tmp_path, monkeypatch):
    """several ranks: no plan folds, a max-reduction through the host sits in front of every decision, and the golden system's shards take the late
    slot (tests/rank_worker.py, two ranks on one device, each in the lab build)"""
    from helpers import run_ranks
    monkeypatch.setenv("TFQMRGPU_LIB", T.LAB_LIB_PATH)
    got = {}
    for late in (0, 1):
        monkeypatch.setenv("TFQMRGPU_LATE_V5", str(late))
        got[late] = run_ranks(2, "solve", str(tmp_path / ("ranks%d.npz" % late)), GOLDEN, "z", 1e-9, timeout=300)
    old, new = got[0], got[1]
    assert list(old["status"]) == [0, 0] and int(old["iterations"][0]) >= 2 and np.abs(old["X"]).max() > 0
    for key in ("status", "iterations", "calls"):
        assert np.array_equal(old[key], new[key]), (key, old[key], new[key])
    for key in ("residual", "history", "X"):
        assert same_typed_bits(old[key], new[key]), key
