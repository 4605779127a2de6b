"""tfqmrgpuExt_refineFrom (include/tfqmrgpu_ext.h section 16) without a GPU: the call is declared, exported from both libraries and bound,
and the statuses that are decided before the first device call -- plan / handle pointers, no bufferSize yet, no buffer, for every precision
and with a user-defined operator or a preconditioner asked for -- are those of the header, in its order, and change nothing that getInfo
and getBoundHistory report.  Mirrors tests/test_solve_from_cpu.py."""
import os
import re
import subprocess

import tfqmrgpu_amd as T
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTER_INVALID, UNDOCUMENTED = 7, 14
LM, LN = 4, 5


def _raw(handle, plan, threshold=1e-9, max_iterations=50):
    return T.lib.tfqmrgpuExt_refineFrom(handle, plan, threshold, max_iterations)


def test_symbol_is_exported_and_listed():
    assert "tfqmrgpuExt_refineFrom" in T.EXT_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tfqmrgpuExt_refineFrom\b", out)
    lab = subprocess.run(["nm", "-D", "--defined-only", T.LAB_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tfqmrgpuExt_refineFrom\b", lab)


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_refineFrom(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, "
            "double threshold, int maxIterations);") in flat
    assert "(16) mixed-precision warm start" in text
    # the contract's corner stones: what X0 is, what the history starts with, what the call must not write
    assert "getRefinementHistory: residual[0] is |B - A X0| / |B|" in text
    assert "does NOT write it" in text
    assert text.index("(15) carry") < text.index("(16) mixed-precision warm start")


def test_python_binding_has_the_call():
    assert callable(getattr(T.Solver, "refine_from"))
    args = T.lib.tfqmrgpuExt_refineFrom.argtypes
    assert args is not None and len(args) == 4 and args[2] is T.C.c_double and args[3] is T.C.c_int


def test_statuses_in_order_without_a_device():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    # no plan, no handle
    assert T.decode(_raw(None, None))[::2] == (POINTER_INVALID, 0)
    with T.Solver() as s:
        s.create_plan(pr)
        assert T.decode(_raw(None, s.plan))[::2] == (POINTER_INVALID, 0)
        assert T.decode(_raw(s.handle, None))[::2] == (POINTER_INVALID, 0)
        # no bufferSize yet: before the look at the buffer, whatever maxIterations says
        assert T.decode(_raw(s.handle, s.plan))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(_raw(s.handle, s.plan, 1e-9, 0))[::2] == (UNDOCUMENTED, 0)
        before = s.get_info()
        for prec in "zcm":
            s.buffer_size(LM, LN, prec)
            # no buffer comes first: before the operator, A and the preconditioner are looked at, and before maxIterations <= 0
            assert T.decode(_raw(s.handle, s.plan))[::2] == (POINTER_INVALID, 0), prec
            assert T.decode(_raw(s.handle, s.plan, 1e-9, 0))[::2] == (POINTER_INVALID, 0), prec
            assert T.decode(_raw(s.handle, s.plan, 1e-9, -3))[::2] == (POINTER_INVALID, 0), prec
            s.set_preconditioner(T.PRECOND_BLOCK_JACOBI)
            assert T.decode(_raw(s.handle, s.plan))[::2] == (POINTER_INVALID, 0), prec
            s.set_preconditioner(T.PRECOND_NONE)
            s.set_operator(lambda *a: 0.0)
            assert T.decode(_raw(s.handle, s.plan))[::2] == (POINTER_INVALID, 0), prec
            s.set_operator(None)
            if prec in "zc":   # the same words as solveFrom, line for line: the call forwards
                assert _raw(s.handle, s.plan) == T.lib.tfqmrgpuExt_solveFrom(s.handle, s.plan, 1e-9, 50), prec
            try:
                s.refine_from(1e-9, 50)
            except T.TfqmrError as e:
                assert T.decode(e.status)[0] == POINTER_INVALID
            else:
                raise AssertionError("Solver.refine_from() on a plan without a buffer must raise")
        # a refusal leaves the results of the last solve (here: of no solve) as they were
        assert s.get_info() == before and len(s.bound_history()) == 0
