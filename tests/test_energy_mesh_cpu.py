"""The energy mesh (include/tfqmrgpu_ext.h section 19) without a GPU: the six calls are declared, exported and bound, and the statuses
that are decided before the first device call are those of the header, in its order.  What needs a registered buffer and a whole A to be
reached -- "A never set whole", the missing diagonal block (key 'D'), "scaled and no copy kept" -- stands behind "no buffer" in that order
and is pinned in tests/test_gpu_energy_mesh.py; here the pattern without block (1, 1) shows that its refusal does not come early."""
import contextlib
import ctypes as C
import os
import re
import subprocess

import numpy as np

import tfqmrgpu_amd as T
from mesh_ref import no_diagonal_problem
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 14, 19
LM, LN = 4, 5
NAMES = ["tfqmrgpuExt_shiftDiagonal", "tfqmrgpuExt_keepSum", "tfqmrgpuExt_addToSum", "tfqmrgpuExt_getSum", "tfqmrgpuExt_clearSum",
         "tfqmrgpuExt_solveMesh"]
L = T.lib


def _code_key(status):
    return T.decode(status)[::2]


def _mesh(handle, plan, nE=2, sigma=True, n_done=None):
    sg = np.zeros(2 * max(nE, 1))
    return L.tfqmrgpuExt_solveMesh(handle, plan, nE, T._ptr(sg) if sigma else None, None, 1e-9, 10, 0, None, None, None, n_done)


def test_symbols_are_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lab = subprocess.run(["nm", "-D", "--defined-only", T.LAB_LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert name in T.EXT_SYMBOLS and hasattr(L, name)
        assert re.search(r"\bT %s\b" % name, out) and re.search(r"\bT %s\b" % name, lab), name


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "(19) energy mesh" in text
    assert "tfqmrgpuStatus_t tfqmrgpuExt_shiftDiagonal(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double sigmaRe, double sigmaIm);" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_keepSum(tfqmrgpuBsrsvPlan_t plan, int on);" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_addToSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double wRe, double wIm);" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_getSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double *values , int32_t *nTerms );" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_clearSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan);" in flat
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_solveMesh(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int32_t nE, double const *sigma , "
            "double const *weight , double threshold, int maxIterations, int fromX, int32_t *iterations, double *residual, "
            "tfqmrgpuStatus_t *status , int32_t *nDone );") in flat


def test_python_binding_has_the_calls():
    for name in ("shift_diagonal", "keep_sum", "add_to_sum", "get_sum", "clear_sum", "solve_mesh"):
        assert callable(getattr(T.Solver, name)), name
    assert L.tfqmrgpuExt_shiftDiagonal.argtypes[2:] == [C.c_double, C.c_double]
    assert L.tfqmrgpuExt_addToSum.argtypes[2:] == [C.c_double, C.c_double]
    assert len(L.tfqmrgpuExt_solveMesh.argtypes) == 12 and len(L.tfqmrgpuExt_getSum.argtypes) == 4


def test_shift_diagonal_statuses_in_order():
    shift = lambda h, p: L.tfqmrgpuExt_shiftDiagonal(h, p, 1e-3, 5e-4)      # noqa: E731
    assert _code_key(shift(None, None)) == (POINTER_INVALID, 0)
    for pr in (PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6), no_diagonal_problem()):
        with T.Solver() as s:
            s.create_plan(pr)
            assert _code_key(shift(None, s.plan)) == (POINTER_INVALID, 0)
            assert _code_key(shift(s.handle, None)) == (POINTER_INVALID, 0)
            assert _code_key(shift(s.handle, s.plan)) == (UNDOCUMENTED, 0)             # no bufferSize yet
            for prec in "zcm":
                s.buffer_size(LM, LN, prec)
                assert _code_key(shift(s.handle, s.plan)) == (POINTER_INVALID, 0), prec  # no buffer: before A and the pattern are looked at
                s.set_operator(lambda *a: 0.0)
                assert _code_key(shift(s.handle, s.plan)) == (NO_IMPLEMENTATION, 0), prec   # the operator comes before the buffer
                s.set_operator(None)
                s.set_preconditioner(T.PRECOND_BLOCK_JACOBI)
                assert _code_key(shift(s.handle, s.plan)) == (POINTER_INVALID, 0), prec
                s.set_preconditioner(T.PRECOND_NONE)
            try:
                s.shift_diagonal(1e-3 + 5e-4j)
            except T.TfqmrError as e:
                assert T.decode(e.status)[0] == POINTER_INVALID
            else:
                raise AssertionError("Solver.shift_diagonal() on a plan without a buffer must raise")


def test_sum_statuses_in_order():
    n = C.c_int32(-1)
    vals = np.full(8, 7.0)
    calls = {
        "addToSum": lambda h, p: L.tfqmrgpuExt_addToSum(h, p, 0.5, -0.25),
        "getSum": lambda h, p: L.tfqmrgpuExt_getSum(h, p, T._ptr(vals), C.byref(n)),
        "clearSum": lambda h, p: L.tfqmrgpuExt_clearSum(h, p),
    }
    assert _code_key(L.tfqmrgpuExt_keepSum(None, 1)) == (POINTER_INVALID, 0)
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    with T.Solver() as s:
        s.create_plan(pr)
        for name, call in calls.items():
            assert _code_key(call(None, None)) == (POINTER_INVALID, 0), name
            assert _code_key(call(None, s.plan)) == (POINTER_INVALID, 0), name
            assert _code_key(call(s.handle, None)) == (POINTER_INVALID, 0), name
            assert _code_key(call(s.handle, s.plan)) == (UNDOCUMENTED, 0), name        # no bufferSize yet
        for prec in "zcm":
            s.buffer_size(LM, LN, prec)
            for name, call in calls.items():
                assert _code_key(call(s.handle, s.plan)) == (UNDOCUMENTED, ord("X")), (name, prec)   # keepSum is off: before the buffer
            assert s.keep_sum(True) == 0
            for name, call in calls.items():
                assert _code_key(call(s.handle, s.plan)) == (POINTER_INVALID, 0), (name, prec)       # no buffer
            s.set_operator(lambda *a: 0.0)                                             # accepted: the sum only reads X
            assert _code_key(calls["addToSum"](s.handle, s.plan)) == (POINTER_INVALID, 0)
            s.set_operator(None)
            s.buffer_size(LM, LN, prec)                                                # the switch survives bufferSize
            assert _code_key(calls["addToSum"](s.handle, s.plan)) == (POINTER_INVALID, 0)
            assert s.keep_sum(False) == 0
            assert _code_key(calls["addToSum"](s.handle, s.plan)) == (UNDOCUMENTED, ord("X"))
    assert n.value == -1 and np.all(vals == 7.0)                                       # a refusal writes nothing


def test_solve_mesh_statuses_in_order():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    done = C.c_int32(5)
    assert _code_key(_mesh(None, None, n_done=C.byref(done))) == (POINTER_INVALID, 0) and done.value == 5
    with T.Solver() as s:
        s.create_plan(pr)
        assert _code_key(_mesh(None, s.plan)) == (POINTER_INVALID, 0)
        assert _code_key(_mesh(s.handle, None)) == (POINTER_INVALID, 0)
        assert _code_key(_mesh(s.handle, s.plan, sigma=False, n_done=C.byref(done))) == (POINTER_INVALID, 0) and done.value == 0
        assert _code_key(_mesh(s.handle, s.plan, nE=0, sigma=False)) == (POINTER_INVALID, 0)        # sigma comes before nE
        for nE in (0, -3):
            assert _code_key(_mesh(s.handle, s.plan, nE=nE)) == (UNDOCUMENTED, ord("E"))
        # then those of shiftDiagonal, by the call itself
        assert _code_key(_mesh(s.handle, s.plan)) == (UNDOCUMENTED, 0)                 # no bufferSize yet
        s.buffer_size(LM, LN, "z")
        done.value = 5
        assert _code_key(_mesh(s.handle, s.plan, n_done=C.byref(done))) == (POINTER_INVALID, 0) and done.value == 0   # no buffer
        # a user-defined operator: refused in front of the loop
        s.set_operator(lambda *a: 0.0)
        assert _code_key(_mesh(s.handle, s.plan)) == (NO_IMPLEMENTATION, 0)
        # several ranks (a reduce callback makes the handle one of several): refused from the handle alone, before the operator is looked
        # at, without a collective -- the callback is never called
        calls = []
        with contextlib.suppress(T.TfqmrError):                        # (its vote buffer needs a device; the callback is registered first)
            s.set_reduce_callback(lambda values, k: calls.append(k))
        assert _code_key(_mesh(s.handle, s.plan)) == (NO_IMPLEMENTATION, 0)
        s.set_operator(None)
        assert _code_key(_mesh(s.handle, s.plan)) == (NO_IMPLEMENTATION, 0)
        assert _code_key(_mesh(s.handle, s.plan, nE=0)) == (UNDOCUMENTED, ord("E"))    # the argument checks come first
        assert calls == []
        s.set_reduce_callback(None)
        assert _code_key(_mesh(s.handle, s.plan)) == (POINTER_INVALID, 0)              # one rank again: no buffer
        before = s.get_info()
        try:
            s.solve_mesh([0.0, 1e-3], None, 1e-9, 10)
        except T.TfqmrError as e:
            assert T.decode(e.status)[0] == POINTER_INVALID
        else:
            raise AssertionError("Solver.solve_mesh() on a plan without a buffer must raise")
        assert s.get_info() == before and len(s.bound_history()) == 0
