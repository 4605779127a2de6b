"""The transitions of a plan's host state that no other test walks, through the C-ABI on the GPU: a second bufferSize with another block
shape, a second setBuffer, keepOperator(0) after patches, block lists that grow, a user-operator plan that changes its shape, the prepared
multiply orders, and destroyPlan / DestroyHandle in every one of these states.  The yardstick is a FRESH plan that is given the same final
inputs: status, iteration count, bound history, residual, X, M^-1 and the number of unit matrices are the same bits (np.array_equal).
Fixture: tests/golden/fd_4x4_2d (109 block rows of 4 x 4 blocks, 849 blocks of A).  Needs an MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_keep_operator as KO
import test_gpu_operator as TO
import tfqmrgpu_amd as T
from conftest import load_problem
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

BJ = T.PRECOND_BLOCK_JACOBI
PRECISIONS = ["z", "m"]      # 'm': the plan has a float A beside the double one


@pytest.fixture(scope="module")
def system():
    """(problem with 4 x 4 right-hand-side blocks, the same with 4 x 8 blocks, A with every diagonal block changed)"""
    pr = load_problem("fd_4x4_2d")
    assert (pr.LM, pr.LN) == (4, 4) and pr.nnzbA > pr.mb
    B8 = np.concatenate([pr.B, pr.B[:, :, ::-1] * (0.5 - 0.25j)], axis=2)     # the data of the other allowed shape: LN = 8
    pr8 = T.Problem(pr.rowPtrA, pr.colIndA, pr.A, pr.rowPtrX, pr.colIndX, pr.rowPtrB, pr.colIndB, B8, None, pr.tolerance, pr.index_offset)
    diag = KO._diagonal(pr)
    assert len(diag) == pr.mb
    return pr, pr8, diag, KO._changed(pr, pr.A, diag, seed=11)


class _Plan(T.Solver):
    """a Solver whose workspaces are created one by one (a second setBuffer), and whose close() checks the statuses"""

    def new_buffer(self, nbytes):
        buf = C.c_void_p(None)
        assert T.lib.tfqmrgpuCreateWorkspace(C.byref(buf), nbytes, b"d") == 0
        self.workspaces = getattr(self, "workspaces", []) + [buf]
        self.set_buffer(device_ptr=buf.value)

    def close(self):
        if self.plan:
            assert T.lib.tfqmrgpu_bsrsv_destroyPlan(self.handle, self.plan) == 0
            self.plan = C.c_void_p(None)
        for buf in getattr(self, "workspaces", []):
            assert T.lib.tfqmrgpuDestroyWorkspace(buf) == 0
        self.workspaces = []
        if self.handle:
            assert T.lib.tfqmrgpuDestroyHandle(self.handle) == 0
            self.handle = C.c_void_p(None)


def _kept_patched_plan(s, pr, diag, A1, prec):
    """preconditioned, kept, solved, patched, solved again: every piece of library-owned memory of a plan exists"""
    s.create_plan(pr)
    nbytes = s.buffer_size(pr.LM, pr.LN, prec)
    s.set_preconditioner(BJ)
    s.keep_operator(True)
    s.new_buffer(nbytes)
    s.set_matrix("A", pr.A)
    s.set_matrix("B", pr.B)
    KO._solve(s, prec)
    KO._set_blocks(s, diag, A1)
    return KO._solve(s, prec), nbytes


@pytest.fixture(scope="module")
def fresh(system):
    """the yardsticks, each computed once: (precision, LN, which A) -> what a fresh plan's solve leaves behind"""
    pr, pr8, diag, A1 = system
    cache = {}

    def get(prec, LN=4, A=None):
        key = (prec, LN, None if A is None else hash(A.tobytes()))
        if key not in cache:
            cache[key] = KO._fresh(pr8 if 8 == LN else pr, pr.A if A is None else A, prec)
        return cache[key]
    return get


# ---- 1. a second bufferSize with another allowed shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_second_buffer_size_with_another_shape(system, fresh, prec):
    pr, pr8, diag, A1 = system
    with _Plan() as s:
        second, _ = _kept_patched_plan(s, pr, diag, A1, prec)
        KO._same(second, fresh(prec, 4, A1))
        s.new_buffer(s.buffer_size(4, 8, prec))                          # 4 x 4 -> 4 x 8: M^-1, the kept copy and the dirty marks are the old shape's
        s.set_matrix("A", A1)
        s.set_matrix("B", pr8.B)
        KO._same(KO._solve(s, prec), fresh(prec, 8, A1))
        KO._set_blocks(s, diag, pr.A)                                    # the plan still keeps: a copy of the new shape takes the patch
        KO._same(KO._solve(s, prec), fresh(prec, 8))


# ---- 2. a second setBuffer without a new bufferSize ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_second_set_buffer_on_a_new_workspace(system, fresh, prec):
    pr, _, diag, A1 = system
    with _Plan() as s:
        _, nbytes = _kept_patched_plan(s, pr, diag, A1, prec)
        s.new_buffer(nbytes)
        # the new buffer holds no A: the set-up has nothing to scale (status 14, key 'A'), and nothing to patch
        assert T.decode(T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, KO.TOL[prec], KO.MAXIT))[::2] == (14, ord("A"))
        s.set_matrix("A", A1)
        s.set_matrix("B", pr.B)
        KO._same(KO._solve(s, prec), fresh(prec, 4, A1))
        KO._set_blocks(s, diag, pr.A)
        KO._same(KO._solve(s, prec), fresh(prec, 4))


# ---- 3. keepOperator(0) after patches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_keep_operator_off_after_patches(system, fresh, prec):
    pr, _, diag, A1 = system
    with _Plan() as s:
        _kept_patched_plan(s, pr, diag, A1, prec)
        KO._set_blocks(s, diag[:3], pr.A)                                # marks that no set-up has seen go with the copy
        s.keep_operator(False)
        with pytest.raises(T.TfqmrError) as e:                           # as on a plan that never kept: A M^-1 cannot be patched
            s.set_blocks("A", diag[:1], pr.A[diag[:1]])
        assert T.decode(e.value.status)[0] == 19
        s.set_matrix("A", pr.A)
        KO._same(KO._solve(s, prec), fresh(prec, 4))


# ---- 4. lists that grow -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_block_list_and_dirty_list_grow(system, fresh, prec):
    pr, _, diag, A1 = system
    every = np.arange(pr.nnzbA, dtype=np.int32)
    one = KO._changed(pr, pr.A, diag[5:6], seed=23)
    with _Plan() as s:
        s.create_plan(pr)
        nbytes = s.buffer_size(pr.LM, pr.LN, prec)
        s.set_preconditioner(BJ)
        s.keep_operator(True)
        s.new_buffer(nbytes)
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        KO._same(KO._solve(s, prec), fresh(prec, 4))
        KO._set_blocks(s, diag[5:6], one)                                # a list of one block; the set-up redoes one row and one column
        KO._same(KO._solve(s, prec), fresh(prec, 4, one))
        KO._set_blocks(s, every, A1)                                     # every block: both device lists are longer than before
        KO._same(KO._solve(s, prec), fresh(prec, 4, A1))
        assert np.array_equal(s.get_blocks(np.arange(pr.nnzbX, dtype=np.int32)), s.get_matrix())


# ---- 5. a user-operator plan changes its shape ------------------------------------------------------------------------------------------------
def _operator_solve(torch, s, pr, prec="z"):
    s.set_matrix("A", 0 * pr.A)
    s.set_matrix("B", pr.B)
    s.set_operator(TO._builtin_as_operator(torch, s, pr, prec, s.plan_view(), []))
    st = s.solve(pr.tolerance, KO.MAXIT)
    return dict(status=st, iterations=s.get_info()["iterations"], bounds=s.bound_history(), X=s.get_matrix())


def test_operator_plan_changes_its_shape(system):
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU; there is no CPU fallback"
    pr, pr8, _, _ = system
    with _Plan() as s:
        s.create_plan(pr)
        s.new_buffer(s.buffer_size(4, 4, "z"))
        first = _operator_solve(torch, s, pr)
        s.new_buffer(s.buffer_size(4, 8, "z"))                           # the scratch in the caller's block order is twice as large now
        second = _operator_solve(torch, s, pr8)
    for got, p in ((first, pr), (second, pr8)):
        with _Plan() as f:
            f.create_plan(p)
            f.new_buffer(f.buffer_size(p.LM, p.LN, "z"))
            KO._same(got, _operator_solve(torch, f, p))
    assert second["X"].shape[2] == 8 and first["X"].shape[2] == 4


# ---- 6. prepared multiply orders ------------------------------------------------------------------------------------------------------------
def test_multiply_order_life_cycle():
    import torch
    assert torch.cuda.is_available(), "the gpu tests need a GPU; there is no CPU fallback"
    pr = PR.stencil_2d(4, 4, 16, 16, 2, seed=7)
    with _Plan() as s:
        s.create_plan(pr)
        view = s.plan_view()
        nY = pr.nnzbX
        dS = torch.from_numpy(view["starts"].view(np.int32)).cuda()
        dP = torch.from_numpy(view["pairs"].view(np.int32)).cuda()
        dA = TO._native_A(torch, pr, "z")
        dX = torch.from_numpy(PR.hashed_uniform(3, (nY, 2, 16, 16))).cuda()
        dY, dZ = torch.zeros_like(dX), torch.zeros_like(dX)
        args = (b"z", 16, 16, nY, dS.data_ptr(), dP.data_ptr())
        assert T.lib.tfqmrgpuExt_multiply(s.handle, *args, dA.data_ptr(), dX.data_ptr(), dY.data_ptr()) == 0
        orders = []
        for mode in (1, 4):
            order = C.c_void_p(None)
            assert T.lib.tfqmrgpuExt_multiplyPrepare(s.handle, *args, mode, C.byref(order)) == 0 and order.value
            orders.append(order)
        for order in orders:                                             # two orders alive at once, each its own device list
            dZ.zero_()
            assert T.lib.tfqmrgpuExt_multiplyOrdered(s.handle, *args, dA.data_ptr(), dX.data_ptr(), dZ.data_ptr(), order) == 0
            torch.cuda.synchronize()
            assert torch.equal(dZ, dY)
        for order in orders:
            assert T.lib.tfqmrgpuExt_multiplyRelease(order) == 0
        assert T.lib.tfqmrgpuExt_multiplyRelease(None) == 0
        foreign = C.create_string_buffer(32)                             # not an order: refused and left alone
        assert T.decode(T.lib.tfqmrgpuExt_multiplyRelease(C.cast(foreign, C.c_void_p)))[0] == 7
        assert foreign.raw == bytes(32)
        nothing = C.c_void_p(None)                                       # mode 0: nothing to prepare, a null order is the caller's order
        assert T.lib.tfqmrgpuExt_multiplyPrepare(s.handle, *args, 0, C.byref(nothing)) == 0 and not nothing.value


# ---- 7. destroying a plan and a handle in the states in between ---------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", range(6))
def test_destroy_in_every_state(system, steps):
    """_Plan.close() asserts the statuses of destroyPlan, DestroyWorkspace and DestroyHandle"""
    pr, _, diag, A1 = system
    with _Plan() as s:
        s.create_plan(pr)                                                # 0: a plan and nothing else
        if steps >= 1:
            nbytes = s.buffer_size(pr.LM, pr.LN, "m")                    # 1: laid out, no buffer
            s.set_preconditioner(BJ)
            s.keep_operator(True)
        if steps >= 2:
            s.new_buffer(nbytes)                                         # 2: a buffer, no operand
        if steps >= 3:
            s.set_matrix("A", pr.A)                                      # 3: operands, no set-up
            s.set_matrix("B", pr.B)
            KO._set_blocks(s, diag[:2], A1)                              # (not scaled yet: the patch goes into the buffer; a block list exists)
        if steps >= 4:
            s.get_preconditioner(values=False)                           # 4: set up and kept, never solved
        if steps >= 5:
            KO._set_blocks(s, diag[2:4], A1)                             # 5: solved, with marks that no set-up has seen
            s.solve(1e-9, 5)
            KO._set_blocks(s, diag[4:6], A1)


def test_destroy_a_handle_with_a_vote_buffer():
    with _Plan() as s:                                                   # the device buffer of the ranks' vote comes with the callback
        cb = T.REDUCE_CB(lambda ctx, v, n: None)
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, cb, None) == 0
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, cb, None) == 0
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, T.REDUCE_CB(0), None) == 0
