"""tfqmrgpuExt_setBlocks / tfqmrgpuExt_getBlocks (include/tfqmrgpu_ext.h section 8) without a GPU: every check of the arguments and of
the list is host code that comes before the first device call, so a plan with createPlan + bufferSize and NO buffer reaches all of them.
A list that passes ends at the missing buffer (TFQMRGPU_POINTER_INVALID)."""
import ctypes as C

import numpy as np
import pytest

import tfqmrgpu_amd as T
from tfqmrgpu_amd import problems as PR

POINTER_INVALID, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 14, 19
LM, LN = 4, 5


@pytest.fixture()
def solver():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    with T.Solver() as s:
        s.create_plan(pr)
        s.buffer_size(LM, LN, "z")
        yield s


VALUES = np.zeros(64 * 2 * LN * LN)


def _call(fn, s, var, blocks, n=None, values=VALUES, precision=b"z", trans=b"n", layout=T.LAYOUT_RIRIRIRI):
    idx = None if blocks is None else np.ascontiguousarray(blocks, dtype=np.int32)
    n = (0 if idx is None else len(idx)) if n is None else n
    ptr = None if idx is None else idx.ctypes.data_as(C.c_void_p)      # (also for an empty list: a valid pointer, nothing behind it)
    vals = None if values is None else values.ctypes.data_as(C.c_void_p)
    return fn(s.handle, s.plan, var, n, ptr, vals, precision, trans, layout)


def _set(s, var, blocks, **kw):
    return _call(T.lib.tfqmrgpuExt_setBlocks, s, var, blocks, **kw)


def _get(s, var, blocks, **kw):
    return _call(T.lib.tfqmrgpuExt_getBlocks, s, var, blocks, **kw)


def _nnzb(s, var):
    return {"A": s.problem.nnzbA, "B": s.problem.nnzbB, "X": s.problem.nnzbX}[var]


@pytest.mark.parametrize("var", "ABX")
def test_index_out_of_range_carries_the_variable(solver, var):
    n = _nnzb(solver, var)
    assert n >= 3
    for bad in (-1, n):
        for blocks in ([bad], [0, bad], [bad, n - 1], [0, 1, bad, 2]):
            st = _set(solver, var.encode(), blocks)
            assert T.decode(st)[::2] == (UNDOCUMENTED, ord(var)), (var, blocks, st)
            st = _set(solver, var.lower().encode(), blocks)
            assert T.decode(st)[::2] == (UNDOCUMENTED, ord(var.lower()))
    for bad in (-1, solver.problem.nnzbX):
        assert T.decode(_get(solver, b"X", [0, bad]))[::2] == (UNDOCUMENTED, ord("X"))


@pytest.mark.parametrize("var", "ABX")
def test_repeated_index(solver, var):
    n = _nnzb(solver, var)
    for blocks in ([0, 0], [n - 1, 1, n - 1], [2, 0, 1, 0]):
        assert T.decode(_set(solver, var.encode(), blocks))[::2] == (UNDOCUMENTED, ord(var)), blocks
    # reading a block twice is allowed: the list passes and the call ends at the missing buffer
    assert T.decode(_get(solver, b"X", [0, 0, solver.problem.nnzbX - 1, 0]))[0] == POINTER_INVALID
    assert T.decode(_get(solver, b"X", [0, 0]))[2] == 0


@pytest.mark.parametrize("var", "ABX")
def test_valid_list_reaches_the_buffer_check(solver, var):
    n = _nnzb(solver, var)
    for blocks in ([0], [n - 1], list(range(n))[::-1], [n - 1, 0, 1]):
        assert T.decode(_set(solver, var.encode(), blocks))[::2] == (POINTER_INVALID, 0), blocks
    assert T.decode(_get(solver, b"X", [solver.problem.nnzbX - 1, 0]))[::2] == (POINTER_INVALID, 0)
    # B's pattern with the right count passes the list check as well
    assert T.decode(_get(solver, b"X", None, n=solver.problem.nnzbB))[::2] == (POINTER_INVALID, 0)


def test_get_blocks_reads_x_only(solver):
    a = VALUES.ctypes.data_as(C.c_void_p)
    for var in (b"A", b"B", b"a", b"Q"):
        want = T.lib.tfqmrgpu_bsrsv_getMatrix(solver.handle, solver.plan, var, a, b"z", LN, LM, b"n", T.LAYOUT_RIRIRIRI)
        assert want != 0 and T.decode(want)[::2] == (UNDOCUMENTED, ord(var))
        assert _get(solver, var, [0]) == want
        assert _get(solver, var, [-1]) == want            # `var` comes before the list
    assert T.decode(_set(solver, b"Q", [0]))[::2] == (18, ord("Q"))   # TFQMRGPU_VARIABLENAME_UNKNOWN, as setMatrix


def test_null_list(solver):
    nB = solver.problem.nnzbB
    for n in (0, 1, nB - 1, nB + 1, -1):
        assert T.decode(_get(solver, b"X", None, n=n))[::2] == (POINTER_INVALID, 0), n
    for var in (b"A", b"B", b"X"):
        for n in (1, nB):
            assert T.decode(_set(solver, var, None, n=n))[::2] == (POINTER_INVALID, 0)


def test_empty_list_succeeds(solver):
    empty = np.zeros(0, np.int32)
    for var in (b"A", b"B", b"X"):
        assert _set(solver, var, empty) == 0
        assert _set(solver, var, empty, values=None) == 0
    assert _get(solver, b"X", empty) == 0
    assert _set(solver, b"A", None, n=0) == 0


def test_before_buffer_size():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    with T.Solver() as s:
        s.create_plan(pr)
        for fn in (_set, _get):
            assert T.decode(fn(s, b"X", [0]))[::2] == (UNDOCUMENTED, 0)
            assert T.decode(fn(s, b"X", np.zeros(0, np.int32)))[::2] == (UNDOCUMENTED, 0)
        assert T.decode(_get(s, b"X", None, n=pr.nnzbB))[::2] == (UNDOCUMENTED, 0)
    for fn in (T.lib.tfqmrgpuExt_setBlocks, T.lib.tfqmrgpuExt_getBlocks):   # no plan, no handle
        assert T.decode(fn(None, None, b"X", 0, None, None, b"z", b"n", T.LAYOUT_RIRIRIRI))[0] == POINTER_INVALID


def test_layout_and_trans_as_set_matrix(solver):
    a = VALUES.ctypes.data_as(C.c_void_p)
    for fn, whole in ((_set, T.lib.tfqmrgpu_bsrsv_setMatrix), (_get, T.lib.tfqmrgpu_bsrsv_getMatrix)):
        want = whole(solver.handle, solver.plan, b"X", a, b"z", LN, LM, b"n", 0x77)
        assert T.decode(want) == (15, 0x77, 0)
        assert fn(solver, b"X", [0], layout=0x77) == want
        assert fn(solver, b"X", [-1], layout=0x77) == want           # the layout comes first
        want = whole(solver.handle, solver.plan, b"X", a, b"z", LN, LM, b"q", T.LAYOUT_RIRIRIRI)
        assert T.decode(want)[::2] == (17, ord("q"))
        assert fn(solver, b"X", [0], trans=b"q") == want
        assert fn(solver, b"Q", [-1], trans=b"q") == want
        for tr in (b"n", b"t", b"c", b"h", b"*", b"N", b"T"):        # every known one passes on to the buffer check
            assert T.decode(fn(solver, b"X", [0], trans=tr))[0] == POINTER_INVALID


def test_python_binding_has_the_calls():
    for name in ("set_blocks", "get_blocks", "set_blocks_device", "get_blocks_device"):
        assert callable(getattr(T.Solver, name))
    assert "tfqmrgpuExt_setBlocks" in T.EXT_SYMBOLS and "tfqmrgpuExt_getBlocks" in T.EXT_SYMBOLS
