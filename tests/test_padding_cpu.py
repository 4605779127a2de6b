"""Padded plans (include/tfqmrgpu_ext.h section 18) without a GPU: the two calls are declared, exported and bound; the shape rule of
bufferSize on every (lm, ln) in 1 ... 64 x 1 ... 64 against its numpy restatement (tests/pad_ref.py); a plan without the switch returns
what it always returned; and the operand calls on a padded plan without a buffer return the statuses of a plan that is not padded --
every check is host code in front of the first device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pad_ref as PD
import tfqmrgpu_amd as T
from conftest import ROOT
from tfqmrgpu_amd import problems as PR

POINTER_INVALID, BLOCKSIZE_MISSING, UNDOCUMENTED = 7, 12, 14
LAYOUTS = (T.LAYOUT_RRRRIIII, T.LAYOUT_RRIIRRII, T.LAYOUT_RIRIRIRI)


@pytest.fixture(scope="module")
def pattern():
    return PR.stencil_2d(4, 3, 4, 4, 3, seed=18, radius=1.6)


def _plan(pattern, padding=None):
    s = T.Solver()
    s.create_plan(pattern)
    if padding is not None:
        s.allow_padding(padding)
    return s


def _buffer_size(s, lm, ln, prec=b"z", blockDim=None, rhsDim=None, out=True, handle=True):
    n = C.c_size_t(12345)
    st = T.lib.tfqmrgpu_bsrsv_bufferSize(s.handle if handle else None, s.plan, lm, lm if blockDim is None else blockDim, ln,
                                         ln if rhsDim is None else rhsDim, prec, C.byref(n) if out else None)
    return st, n.value


def _shape(s):
    v = [C.c_int32(-1) for _ in range(4)]
    st = T.lib.tfqmrgpuExt_paddedShape(s.plan, *[C.byref(x) for x in v])
    return st, tuple(x.value for x in v)


def test_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert "tfqmrgpuStatus_t tfqmrgpuExt_allowPadding(tfqmrgpuBsrsvPlan_t plan, int on);" in flat
    assert "tfqmrgpuStatus_t tfqmrgpuExt_paddedShape(tfqmrgpuBsrsvPlan_t plan, int32_t *lm, int32_t *ln, int32_t *LM, int32_t *LN);" in flat
    for lib in (T.LIB_PATH, T.LAB_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in ("tfqmrgpuExt_allowPadding", "tfqmrgpuExt_paddedShape"):
            assert re.search(r"\bT %s\b" % name, exported), (lib, name)
            assert name in T.EXT_SYMBOLS and hasattr(T.lib, name)
    assert T.decode(T.lib.tfqmrgpuExt_allowPadding(None, 1))[0] == POINTER_INVALID
    assert T.decode(T.lib.tfqmrgpuExt_paddedShape(None, None, None, None, None))[0] == POINTER_INVALID


def test_the_listed_shapes_are_the_librarys():
    n, sizes = C.c_int32(0), np.zeros(64, np.int32)
    assert T.lib.tfqmrgpu_bsrsv_allowedBlockSizes(C.byref(n), sizes.ctypes.data_as(C.POINTER(C.c_int32)), 64) == 0
    assert [tuple(p) for p in sizes[:2 * n.value].reshape(-1, 2)] == PD.LISTED


def test_shape_rule_on_every_shape(pattern):
    """1 ... 64 x 1 ... 64 on ONE plan: the pick, the caller's shape that paddedShape gives back, and the buffer size, which is that of a
    plan of the plan's shape without the switch"""
    listed_bytes = {}
    with _plan(pattern) as plain:
        for LM, LN in PD.LISTED:
            st, listed_bytes[LM, LN] = _buffer_size(plain, LM, LN)
            assert st == 0
    with _plan(pattern, True) as s:
        for lm in range(1, 65):
            for ln in range(1, 65):
                st, nbytes = _buffer_size(s, lm, ln)
                want = PD.plan_shape(lm, ln)
                assert want is not None and st == 0, (lm, ln, st)
                assert _shape(s) == (0, (lm, ln) + want), (lm, ln)
                assert nbytes == listed_bytes[want], (lm, ln)
                if (lm, ln) in PD.LISTED:
                    assert want == (lm, ln)
        view = s.plan_view()
        assert s.padded_shape() == (64, 64, 64, 64) and view["nCols"] == 3


@pytest.mark.parametrize("lm,ln,want", [(3, 3, (4, 4)), (4, 6, (4, 8)), (4, 33, (8, 64)), (5, 5, (8, 8)), (9, 9, (16, 16)), (16, 1, (16, 16)),
                                        (25, 25, (32, 32)), (33, 40, (64, 64))])
def test_spot_values(pattern, lm, ln, want):
    assert PD.plan_shape(lm, ln) == want
    with _plan(pattern, True) as s:
        for prec in (b"z", b"c", b"m"):
            assert _buffer_size(s, lm, ln, prec)[0] == 0
            assert _shape(s) == (0, (lm, ln) + want)
        v = T.PlanView()
        assert T.lib.tfqmrgpuExt_planView(s.plan, C.byref(v)) == 0
        assert (v.LM, v.LN) == want                                  # everything behind the pick sees the plan's shape


@pytest.mark.parametrize("lm,ln", [(65, 65), (64, 65), (65, 1), (1, 65), (100, 200)])
def test_above_64_is_missing_with_the_callers_shape(pattern, lm, ln):
    assert PD.plan_shape(lm, ln) is None
    with _plan(pattern, True) as s:
        st, nbytes = _buffer_size(s, lm, ln)
        assert T.decode(st) == (BLOCKSIZE_MISSING, ln, lm)
        assert st == T.lib.tfqmrgpu_bsrsv_blockSizeMissing(lm, ln) and nbytes == 12345


def test_checks_of_buffer_size_with_padding_on(pattern):
    with _plan(pattern, True) as s:
        assert T.decode(_buffer_size(s, 5, 5, blockDim=6)[0])[0] == UNDOCUMENTED       # ldA != blockDim
        assert T.decode(_buffer_size(s, 5, 5, rhsDim=4)[0])[0] == UNDOCUMENTED         # ldB != RhsBlockDim
        assert T.decode(_buffer_size(s, 5, 5, handle=False)[0])[0] == POINTER_INVALID
        assert T.decode(_buffer_size(s, 5, 5, out=False)[0])[0] == POINTER_INVALID
        for lm, ln in ((0, 4), (4, 0), (-1, 4), (4, -3), (0, 0)):
            assert T.decode(_buffer_size(s, lm, ln)[0])[0] == UNDOCUMENTED, (lm, ln)
        assert T.decode(_shape(s)[0])[0] == UNDOCUMENTED             # none of them has laid a buffer out
        assert _buffer_size(s, 9, 2)[0] == 0                         # fewer right-hand sides than rows
        assert _shape(s) == (0, (9, 2, 16, 16))
        # the switch survives bufferSize; switched off, the next bufferSize refuses again
        assert _buffer_size(s, 5, 5)[0] == 0
        s.allow_padding(False)
        assert T.decode(_buffer_size(s, 5, 5)[0]) == (BLOCKSIZE_MISSING, 5, 5)


@pytest.mark.parametrize("padding", [None, False])
def test_padding_off_is_the_plan_it_was(pattern, padding):
    """every unlisted shape returns the status of today, lm > ln today's error, a listed shape its size; paddedShape gives equal pairs"""
    with _plan(pattern, padding) as s:
        assert T.decode(_shape(s)[0])[0] == UNDOCUMENTED             # before bufferSize
        for lm in range(0, 67):
            for ln in range(0, 67):
                st, nbytes = _buffer_size(s, lm, ln)
                if lm > ln:
                    assert T.decode(st)[0] == UNDOCUMENTED and T.decode(st)[2] == 0, (lm, ln)
                elif (lm, ln) in PD.LISTED:
                    assert st == 0 and _shape(s) == (0, (lm, ln, lm, ln))
                else:
                    assert T.decode(st) == (BLOCKSIZE_MISSING, ln, lm), (lm, ln)
                    assert nbytes == 12345


def test_padded_shape_before_buffer_size_and_null_pointers(pattern):
    with _plan(pattern, True) as s:
        st, v = _shape(s)
        assert T.decode(st)[0] == UNDOCUMENTED and v == (-1, -1, -1, -1)
        assert _buffer_size(s, 25, 25)[0] == 0
        assert T.lib.tfqmrgpuExt_paddedShape(s.plan, None, None, None, None) == 0
        LM = C.c_int32(0)
        assert T.lib.tfqmrgpuExt_paddedShape(s.plan, None, None, C.byref(LM), None) == 0 and LM.value == 32


def _operand_statuses(s, lm, ln):
    """the statuses of the operand calls on a plan without a buffer, in the order of their checks"""
    vals = np.zeros(64 * 2 * 64 * 64)
    ptr = vals.ctypes.data_as(C.c_void_p)
    idx = np.array([1, 0], np.int32)
    iptr = idx.ctypes.data_as(C.c_void_p)
    L = T.LAYOUT_RIRIRIRI
    out = []
    for var in b"ABXQ":
        v = bytes([var])
        out.append(T.lib.tfqmrgpu_bsrsv_setMatrix(s.handle, s.plan, v, ptr, b"z", ln, lm, b"n", L))
        out.append(T.lib.tfqmrgpu_bsrsv_getMatrix(s.handle, s.plan, v, ptr, b"z", ln, lm, b"n", L))
        out.append(T.lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, v, 2, iptr, ptr, b"z", b"t", L))
        out.append(T.lib.tfqmrgpuExt_getBlocks(s.handle, s.plan, v, 2, iptr, ptr, b"z", b"c", L))
        out.append(T.lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, v, 2, np.array([0, 0], np.int32).ctypes.data_as(C.c_void_p), ptr, b"z", b"n", L))
        out.append(T.lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, v, 1, np.array([9999], np.int32).ctypes.data_as(C.c_void_p), ptr, b"z", b"n", L))
        out.append(T.lib.tfqmrgpuExt_setBlocks(s.handle, s.plan, v, -1, iptr, ptr, b"z", b"n", L))
    out.append(T.lib.tfqmrgpu_bsrsv_setMatrix(s.handle, s.plan, b"A", ptr, b"z", lm, lm, b"n", 0x77))       # an unknown layout
    out.append(T.lib.tfqmrgpu_bsrsv_setMatrix(s.handle, s.plan, b"A", ptr, b"z", lm, lm, b"q", L))          # an unknown transposition
    out.append(T.lib.tfqmrgpuExt_getBlocks(s.handle, s.plan, b"X", s.problem.nnzbB, None, ptr, b"z", b"n", L))   # B's pattern
    out.append(T.lib.tfqmrgpuExt_getBlocks(s.handle, s.plan, b"X", 1, None, ptr, b"z", b"n", L))                 # ... with a wrong count
    return [T.decode(st)[::2] for st in out]                         # (code, key): the line is the source line of the check


@pytest.mark.parametrize("lm,ln", [(5, 7), (25, 25), (16, 1)])
def test_operand_calls_without_a_buffer_return_what_a_plain_plan_returns(pattern, lm, ln):
    LM, LN = PD.plan_shape(lm, ln)
    with _plan(pattern, True) as padded, _plan(pattern) as plain:
        for prec in (b"z", b"c", b"m"):
            assert _buffer_size(padded, lm, ln, prec)[0] == 0 and _buffer_size(plain, LM, LN, prec)[0] == 0
            got, want = _operand_statuses(padded, lm, ln), _operand_statuses(plain, LM, LN)
            assert got == want
            assert (POINTER_INVALID, 0) in got and (UNDOCUMENTED, ord("A")) in got     # the list checks and the missing buffer are among them


def test_carry_requires_equal_callers_shapes(pattern):
    """two padded plans of one plan shape and different caller's shapes: the status of unequal block shapes, key 'L'; no buffer is looked at"""
    with _plan(pattern, True) as a, _plan(pattern, True) as b, _plan(pattern) as c:
        assert _buffer_size(a, 5, 5)[0] == 0 and _buffer_size(b, 6, 6)[0] == 0 and _buffer_size(c, 8, 8)[0] == 0
        assert _shape(a)[1][2:] == _shape(b)[1][2:] == _shape(c)[1][2:] == (8, 8)
        for dst, src in ((a, b), (b, a), (a, c), (c, a)):
            st = T.lib.tfqmrgpuExt_carry(dst.handle, dst.plan, src.plan, b"X", pattern.nnzbX, None)
            assert T.decode(st)[::2] == (UNDOCUMENTED, ord("L"))
        assert _buffer_size(b, 5, 5)[0] == 0                         # equal now: the call goes on to the missing buffers
        st = T.lib.tfqmrgpuExt_carry(a.handle, a.plan, b.plan, b"X", pattern.nnzbX, None)
        assert T.decode(st)[::2] == (POINTER_INVALID, 0)


def test_python_solver_keeps_both_shapes(pattern):
    with _plan(pattern, True) as s:
        s.buffer_size(9, 10, "z")
        assert (s.lm, s.ln, s.LM, s.LN) == (9, 10, 16, 16) == s.padded_shape()
    with _plan(pattern) as s:
        s.buffer_size(8, 9, "c")
        assert (s.lm, s.ln, s.LM, s.LN) == (8, 9, 8, 9)
        with pytest.raises(T.TfqmrError) as e:
            s.buffer_size(9, 10, "z")
        assert T.decode(e.value.status) == (BLOCKSIZE_MISSING, 10, 9)


@pytest.mark.parametrize("lm,ln,tol", [(5, 5, 1e-10), (25, 25, 1e-10)])
def test_the_padded_problem_solves_the_callers_system(oracle, lm, ln, tol):
    """The inputs of the truth test of tests/test_gpu_padding.py, through the CPU oracle: the padded problem, solved as a problem of the
    plan's shape, gives inside the solution of the caller's system (dense LAPACK on the caller's blocks) to 1e-8 of its largest
    element, and exact zeros in the padding"""
    pr = PR.stencil_2d(4, 3, lm, ln, 3, seed=100 * lm + ln)
    LM, LN = PD.plan_shape(lm, ln)
    st, X, info = oracle.solve(PD.pad_problem(pr, LM, LN), "z", threshold=tol, max_iterations=300)
    Xd = PR.dense_reference_solution(pr)
    dev = np.abs(PD.inside(X, lm, ln) - Xd).max() / np.abs(Xd).max()
    print("%dx%d on %dx%d: status %d, %d iterations, deviation of the inside from the dense solution %.3g" % (lm, ln, LM, LN, st, info["iterations"], dev))
    assert st == 0 and dev <= 1e-8
    pad = X.copy()
    pad[:, :lm, :ln] = 0
    assert not pad.any()
