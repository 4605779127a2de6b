"""tfqmrgpuExt_carry (include/tfqmrgpu_ext.h section 15) without a GPU: the call is declared, exported and bound, and the statuses that
are decided before the first device call -- pointers, no bufferSize yet, the operand's name, the block shape, the block map, no buffer --
are those of the header, in its order, for 'z', 'c' and 'm' on either side, and change nothing that getInfo and getBoundHistory report."""
import itertools
import os
import re
import subprocess

import numpy as np

import tfqmrgpu_amd as T
from tfqmrgpu_amd import problems as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTER_INVALID, UNDOCUMENTED, VARIABLENAME_UNKNOWN = 7, 14, 18
LM, LN = 4, 5


def _raw(handle, dst, src, var, n, old):
    idx = None if old is None else np.ascontiguousarray(old, dtype=np.int32)
    return T.lib.tfqmrgpuExt_carry(handle, dst, src, var.encode(), n, None if idx is None else T.C.c_void_p(idx.ctypes.data))


def _status(*a):
    return T.decode(_raw(*a))[::2]


def test_symbol_is_exported_and_listed():
    assert "tfqmrgpuExt_carry" in T.EXT_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", T.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tfqmrgpuExt_carry\b", out)
    lab = subprocess.run(["nm", "-D", "--defined-only", T.LAB_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tfqmrgpuExt_carry\b", lab)


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tfqmrgpu_ext.h")).read()
    flat = re.sub(r"\s+", " ", text)
    assert ("tfqmrgpuStatus_t tfqmrgpuExt_carry(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t dst, tfqmrgpuBsrsvPlan_t src, "
            "char var /* 'A', 'B', 'X' */, int32_t nBlocks, int32_t const *oldBlock /* HOST [nBlocks], or NULL */);") in flat
    assert "(15) carry A, B and X" in text
    assert "oldBlock[n] == -1" in text and "rounds to nearest, once" in text


def test_python_binding_has_the_call():
    assert callable(getattr(T.Solver, "carry_from")) and callable(getattr(T.Solver, "adopt"))
    args = T.lib.tfqmrgpuExt_carry.argtypes
    assert args is not None and len(args) == 6 and args[3] is T.C.c_char and args[4] is T.C.c_int32


def test_the_same_status_word_as_set_matrix_for_an_unknown_operand():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    with T.Solver() as d, T.Solver() as s:
        for q in (d, s):
            q.create_plan(pr)
            q.buffer_size(LM, LN, "z")
        for var in "QyZ":
            mine = T.decode(_raw(d.handle, d.plan, s.plan, var, 0, None))
            dummy = np.zeros(4)
            theirs = T.decode(T.lib.tfqmrgpu_bsrsv_setMatrix(d.handle, d.plan, var.encode(), T.C.c_void_p(dummy.ctypes.data), b"z", LN, LM, b"n",
                                                             T.LAYOUT_RIRIRIRI))
            assert mine[::2] == theirs[::2] == (VARIABLENAME_UNKNOWN, ord(var))


def test_statuses_in_order_without_a_device():
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    other = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=2.4)      # the same A and B patterns, more blocks of X
    assert other.nnzbX > pr.nnzbX and other.nnzbA == pr.nnzbA and other.nnzbB == pr.nnzbB
    counts = {"A": (pr.nnzbA, other.nnzbA), "B": (pr.nnzbB, other.nnzbB), "X": (pr.nnzbX, other.nnzbX)}
    assert _status(None, None, None, "X", 0, None) == (POINTER_INVALID, 0)
    for pd, ps in itertools.product("zcm", repeat=2):
        with T.Solver() as d, T.Solver() as s:
            d.create_plan(pr)
            s.create_plan(other)
            state = lambda: (d.get_info(), s.get_info(), len(d.bound_history()), len(s.bound_history()))      # noqa: E731
            before = state()
            nX, nXs = counts["X"]
            ident = np.arange(nX)
            # 1. pointers: before bufferSize is looked at, before the operand's name, before the map
            for h, a, b in ((None, d.plan, s.plan), (d.handle, None, s.plan), (d.handle, d.plan, None), (d.handle, d.plan, d.plan),
                            (d.handle, s.plan, s.plan)):
                assert _status(h, a, b, "?", -5, None) == (POINTER_INVALID, 0)
            # 2. no bufferSize yet, on either side: before the operand's name and the map
            assert _status(d.handle, d.plan, s.plan, "?", -5, None) == (UNDOCUMENTED, 0)
            d.buffer_size(LM, LN, pd)
            assert _status(d.handle, d.plan, s.plan, "?", -5, None) == (UNDOCUMENTED, 0)
            s.buffer_size(LM, 8, ps)
            # 3. the operand's name: before the block shape
            assert _status(d.handle, d.plan, s.plan, "?", -5, None) == (VARIABLENAME_UNKNOWN, ord("?"))
            # 4. the block shape: before the map
            for var in "ABXabx":
                assert _status(d.handle, d.plan, s.plan, var, -5, None) == (UNDOCUMENTED, ord("L")), var
            s.buffer_size(LM, LN, ps)
            # 5. the map, with the key character var; before the look at the buffers
            for var in "ABX":
                n, ns = counts[var]
                good = np.arange(n) % ns
                assert _status(d.handle, d.plan, s.plan, var, n - 1, good) == (UNDOCUMENTED, ord(var))
                assert _status(d.handle, d.plan, s.plan, var, n + 1, good) == (UNDOCUMENTED, ord(var))
                assert _status(d.handle, d.plan, s.plan, var, 0, None) == (UNDOCUMENTED, ord(var))
                assert _status(d.handle, d.plan, s.plan, var.lower(), -1, good) == (UNDOCUMENTED, ord(var.lower()))
                for bad in (-2, ns, ns + 7, -2**31, 2**31 - 1):
                    for at in (0, n - 1):
                        m = good.copy()
                        m[at] = bad
                        assert _status(d.handle, d.plan, s.plan, var, n, m) == (UNDOCUMENTED, ord(var)), (var, bad, at)
            assert _status(d.handle, d.plan, s.plan, "X", nX, None) == (UNDOCUMENTED, ord("X"))       # no list: the counts differ
            assert _status(s.handle, s.plan, d.plan, "X", nXs, None) == (UNDOCUMENTED, ord("X"))
            # 6. no buffer (a good map, -1 entries and repeats included): the last thing that needs no device
            m = ident % 3
            m[::2] = -1
            for var, n, old in (("X", nX, m), ("X", nX, ident), ("A", counts["A"][0], None), ("B", counts["B"][0], None),
                                ("A", counts["A"][0], np.zeros(counts["A"][0], int)), ("B", counts["B"][0], -np.ones(counts["B"][0], int))):
                assert _status(d.handle, d.plan, s.plan, var, n, old) == (POINTER_INVALID, 0), (var, pd, ps)
            try:
                d.adopt(s, ident)
            except T.TfqmrError as e:
                assert T.decode(e.status)[0] == POINTER_INVALID
            else:
                raise AssertionError("Solver.adopt() on plans without buffers must raise")
            # a refusal leaves the results of the last solve (here: of no solve) as they were, on both plans
            assert state() == before


def test_a_count_of_zero_is_not_the_operands_own_count():
    """nBlocks == 0 is a success only where the operand has no block; createPlan admits no such plan of this problem, so here it is
    refused like every other wrong count, with or without a list"""
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)
    with T.Solver() as d, T.Solver() as s:
        for q in (d, s):
            q.create_plan(pr)
            q.buffer_size(LM, LN, "z")
        for var in "ABX":
            assert _status(d.handle, d.plan, s.plan, var, 0, None) == (UNDOCUMENTED, ord(var))
            assert _status(d.handle, d.plan, s.plan, var, 0, np.zeros(1, np.int32)) == (UNDOCUMENTED, ord(var))
