"""Start projection (include/tfqmrgpu_ext.h section 17) without a GPU: the four calls are declared, exported and bound; the statuses that
are decided before the first device call come in the header's order; and the inputs of the GPU tests (tests/project_ref.py: FIXTURES,
SHIFT_SETS) are checked on the CPU reference -- no pivot ratio near the threshold, and a projection that beats the newest start."""
import os
import re
import subprocess

import numpy as np
import pytest

import project_ref as P
import residual_ref as RR
import tfqmrgpu_amd as T
from conftest import load_problem
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTER_INVALID, UNDOCUMENTED = 7, 14
NAMES = ["tfqmrgpuExt_keepStarts", "tfqmrgpuExt_pushStart", "tfqmrgpuExt_startCount", "tfqmrgpuExt_startDepth", "tfqmrgpuExt_projectStart"]
LM, LN = 4, 5


def test_symbols_are_exported_and_listed():
    for path in (T.LIB_PATH, T.LAB_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert name in T.EXT_SYMBOLS
            assert re.search(r"\bT %s\b" % name, out), (path, name)


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "tfqmrgpuStatus_t tfqmrgpuExt_keepStarts(tfqmrgpuBsrsvPlan_t plan, int depth);" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_pushStart(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan);" in flat
    assert "int32_t tfqmrgpuExt_startCount(tfqmrgpuBsrsvPlan_t plan);" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_projectStart(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double *coefficients , int32_t *nUsed );" in flat
    assert "(17) start projection" in text
    # the two constants, in the header and in the CPU reference
    m = dict(re.findall(r"#define (TFQMRGPU_PROJECT_PIVOT_\w+)\s+([0-9.e+-]+)", text))
    assert float(m["TFQMRGPU_PROJECT_PIVOT_DOUBLE"]) == P.PIVOT_DOUBLE == 2.0 ** -26
    assert float(m["TFQMRGPU_PROJECT_PIVOT_FLOAT"]) == P.PIVOT_FLOAT == 2.0 ** -12


def test_python_binding_is_complete():
    for name in ("keep_starts", "push_start", "start_count", "start_depth", "project_start"):
        assert callable(getattr(T.Solver, name))
    C = T.C
    assert T.lib.tfqmrgpuExt_keepStarts.argtypes == [C.c_void_p, C.c_int]
    assert T.lib.tfqmrgpuExt_pushStart.argtypes == [C.c_void_p, C.c_void_p]
    assert T.lib.tfqmrgpuExt_startCount.argtypes == [C.c_void_p] and T.lib.tfqmrgpuExt_startCount.restype is C.c_int32
    assert T.lib.tfqmrgpuExt_projectStart.argtypes == [C.c_void_p] * 4


def test_statuses_in_order_without_a_device():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    L = T.lib
    code = lambda st: T.decode(st)[::2]      # noqa: E731
    assert code(L.tfqmrgpuExt_keepStarts(None, 2)) == (POINTER_INVALID, 0)
    assert code(L.tfqmrgpuExt_pushStart(None, None)) == (POINTER_INVALID, 0)
    assert code(L.tfqmrgpuExt_projectStart(None, None, None, None)) == (POINTER_INVALID, 0)
    assert L.tfqmrgpuExt_startCount(None) == 0
    with T.Solver() as s:
        s.create_plan(pr)
        assert code(L.tfqmrgpuExt_pushStart(None, s.plan)) == (POINTER_INVALID, 0)
        assert code(L.tfqmrgpuExt_pushStart(s.handle, None)) == (POINTER_INVALID, 0)
        assert code(L.tfqmrgpuExt_projectStart(None, s.plan, None, None)) == (POINTER_INVALID, 0)
        assert code(L.tfqmrgpuExt_projectStart(s.handle, None, None, None)) == (POINTER_INVALID, 0)
        # no bufferSize yet
        assert code(L.tfqmrgpuExt_pushStart(s.handle, s.plan)) == (UNDOCUMENTED, 0)
        assert code(L.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None)) == (UNDOCUMENTED, 0)
        before = s.get_info()
        for prec in "zcm":
            s.buffer_size(LM, LN, prec)
            # a depth outside 0 ... 4
            for depth in (-1, 5, 100):
                assert code(L.tfqmrgpuExt_keepStarts(s.plan, depth)) == (UNDOCUMENTED, ord("X")), depth
            # depth 0: pushStart says so before it looks at the buffer; projectStart looks at the buffer first
            assert s.keep_starts(0) == 0
            assert code(L.tfqmrgpuExt_pushStart(s.handle, s.plan)) == (UNDOCUMENTED, ord("X")), prec
            assert code(L.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None)) == (POINTER_INVALID, 0), prec
            for depth in (1, 4, 2):
                assert s.keep_starts(depth) == 0 and s.start_count() == 0 and s.start_depth() == depth
                assert code(L.tfqmrgpuExt_pushStart(s.handle, s.plan)) == (POINTER_INVALID, 0), prec      # no buffer
                assert code(L.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None)) == (POINTER_INVALID, 0), prec
                assert s.start_count() == 0
            # the depth survives bufferSize; no buffer comes before the user-defined operator
            s.buffer_size(LM, LN, prec)
            s.set_operator(lambda *a: 0.0)
            assert code(L.tfqmrgpuExt_pushStart(s.handle, s.plan)) == (POINTER_INVALID, 0), prec
            assert code(L.tfqmrgpuExt_projectStart(s.handle, s.plan, None, None)) == (POINTER_INVALID, 0), prec
            s.set_operator(None)
            with pytest.raises(T.TfqmrError) as e:
                s.project_start()
            assert T.decode(e.value.status)[0] == POINTER_INVALID
            assert s.keep_starts(0) == 0
        assert s.get_info() == before and len(s.bound_history()) == 0


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------------------
def _oracle_starts(oracle, pr, sigmas, prec):
    starts = []
    for sigma in sigmas:
        q = T.Problem(pr.rowPtrA, pr.colIndA, P.shifted(pr, sigma), pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, pr.B, None,
                      pr.tolerance, pr.index_offset)
        st, X, _ = oracle.solve(q, "c" if prec == "c" else "z", threshold=1e-4 if prec == "c" else 1e-9, max_iterations=500)
        assert st == 0, sigma
        starts.insert(0, RR.stored(X, prec))            # newest first
    return starts


@pytest.mark.parametrize("prec", ["z", "c"])
@pytest.mark.parametrize("name,fifth", [(n, False) for n in P.FIXTURES] + [("stencil_8x32", True)])
def test_inputs_of_the_gpu_tests_stay_clear_of_the_threshold(oracle, name, fifth, prec):
    """('m' stores doubles and has the threshold of 'z'.)  Every pivot ratio lies a factor 100 away from the threshold, on either side, so
    that the device and the reference keep the same starts; and the projection beats the newest start on every right-hand side"""
    pr = load_problem(name)
    sig = P.shifts(pr, name, fifth)
    starts = _oracle_starts(oracle, pr, sig[:-1], prec)
    A, B = RR.stored(P.shifted(pr, sig[-1]), prec), RR.stored(pr.B, prec)
    ref = P.project(oracle, pr, A, starts, B, prec)
    thr, r = P.pivot_min(prec), ref["ratio"]
    print("%s %s: pivot ratios per start, min %s, max %s" % (name, prec, np.nanmin(r, axis=(0, 1)), np.nanmax(r, axis=(0, 1))))
    assert np.all(np.isfinite(r))
    assert not np.any((r > thr / 100) & (r < thr * 100))
    assert np.all(r[ref["kept"]] > 100 * thr) and np.all(ref["n_used"] == len(starts))
    r0 = RR.residual(oracle, pr, A, starts[0], B)
    rp = RR.residual(oracle, pr, A, ref["X"], B)
    nz = r0["bnorm2"] > 0
    assert nz.any() and np.all(rp["residual2"][nz] < r0["residual2"][nz])
    assert np.all(rp["residual2"][nz] <= r0["bnorm2"][nz])
