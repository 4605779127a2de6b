"""tfqmrgpuExt_residual (include/tfqmrgpu_ext.h section 10) without a GPU: the call is declared, exported and bound, and the argument
checks that come before the first device call -- a plan with createPlan + bufferSize and NO buffer reaches four of them -- return the
statuses of the header, in its order, and leave the caller's arrays alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import tfqmrgpu_amd as T
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_INFO_PASSED, POINTER_INVALID, UNDOCUMENTED = 3, 7, 14
LM, LN = 4, 5
SENTINEL = -12345.0


def _outputs(n_cols):
    r2, b2 = np.full((n_cols, LN), SENTINEL), np.full((n_cols, LN), SENTINEL)
    return r2, b2, np.full(n_cols, -77, np.int32), C.c_double(SENTINEL)


def _raw(handle, plan, r2=None, b2=None, cols=None, worst=None):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return T.lib.tfqmrgpuExt_residual(handle, plan, ptr(r2), ptr(b2), ptr(cols), None if worst is None else C.byref(worst))


def _untouched(r2, b2, cols, worst):
    return bool((r2 == SENTINEL).all() and (b2 == SENTINEL).all() and (cols == -77).all() and worst.value == SENTINEL)


def test_symbol_is_exported_and_listed():
    assert "tfqmrgpuExt_residual" in T.EXT_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tfqmrgpuExt_residual\b", out)


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_residual(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, "
            "double *residual2, double *bnorm2, int32_t *columns, double *worst);") in flat
    assert "(10) per-right-hand-side residual" in text
    assert "the caller's A is gone" in text and "keepOperator" in text


def test_python_binding_has_the_call():
    assert callable(getattr(T.Solver, "residual"))
    assert T.lib.tfqmrgpuExt_residual.argtypes is not None and len(T.lib.tfqmrgpuExt_residual.argtypes) == 6


def test_argument_checks_in_order_without_a_device():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    out = _outputs(3)
    # no plan, no handle
    assert T.decode(_raw(None, None, *out))[::2] == (POINTER_INVALID, 0)
    with T.Solver() as s:
        s.create_plan(pr)
        assert T.decode(_raw(None, s.plan, *out))[::2] == (POINTER_INVALID, 0)
        assert T.decode(_raw(s.handle, None, *out))[::2] == (POINTER_INVALID, 0)
        # no bufferSize yet: before the look at the outputs
        assert T.decode(_raw(s.handle, s.plan, *out))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(_raw(s.handle, s.plan))[::2] == (UNDOCUMENTED, 0)
        s.buffer_size(LM, LN, "z")
        # all four outputs NULL: before the look at the buffer
        assert _raw(s.handle, s.plan) == NO_INFO_PASSED
        # no buffer; one output is enough to pass the check before it
        assert T.decode(_raw(s.handle, s.plan, *out))[::2] == (POINTER_INVALID, 0)
        for k in range(4):
            one = [None] * 4
            one[k] = out[k]
            assert T.decode(_raw(s.handle, s.plan, *one))[::2] == (POINTER_INVALID, 0)
        try:
            s.residual()
        except T.TfqmrError as e:
            assert T.decode(e.status)[0] == POINTER_INVALID
        else:
            raise AssertionError("Solver.residual() on a plan without a buffer must raise")
    assert _untouched(*out)
