"""The transitions of a plan's host state that no other test walks, through the C-ABI on the GPU: a second bufferSize with another block
shape, a second setBuffer, keepOperator(0) after patches, block lists that grow, a user-operator plan that changes its shape, the prepared
multiply orders, destroyPlan / DestroyHandle in every one of these states, and (8) a second bufferSize and a second setBuffer while
everything that tfqmrgpu_ext.h sections 10 to 17 keep in a plan is alive.  The yardstick is a FRESH plan that is given the same final
inputs: status, iteration count, bound history, residual, X, M^-1 and the number of unit matrices are the same bits (np.array_equal).
Fixture: tests/golden/fd_4x4_2d (109 block rows of 4 x 4 blocks, 849 blocks of A); 8: a truncated stencil of 16 block rows.  Needs an
MI355X (`pytest -m gpu`)."""
import ctypes as C

import numpy as np
import pytest

import solve_helpers as SH
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
    diag = SH.present_diagonal(pr)
    assert len(diag) == pr.mb
    return pr, pr8, diag, SH.changed(pr, pr.A, diag, seed=11)


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
    SH.solve_record(s, prec)
    SH.patch_blocks(s, diag, A1)
    return SH.solve_record(s, prec), nbytes


@pytest.fixture(scope="module")
def fresh(system):
    """the yardsticks, each computed once: (precision, LN, which A) -> what a fresh plan's solve leaves behind"""
    pr, pr8, diag, A1 = system
    cache = {}

    def get(prec, LN=4, A=None):
        key = (prec, LN, None if A is None else hash(A.tobytes()))
        if key not in cache:
            cache[key] = SH.fresh_solve(pr8 if 8 == LN else pr, pr.A if A is None else A, prec)
        return cache[key]
    return get


# ---- 1. a second bufferSize with another allowed shape ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_second_buffer_size_with_another_shape(system, fresh, prec):
    pr, pr8, diag, A1 = system
    with _Plan() as s:
        second, _ = _kept_patched_plan(s, pr, diag, A1, prec)
        SH.same_record(second, fresh(prec, 4, A1))
        s.new_buffer(s.buffer_size(4, 8, prec))                          # 4 x 4 -> 4 x 8: M^-1, the kept copy and the dirty marks are the old shape's
        s.set_matrix("A", A1)
        s.set_matrix("B", pr8.B)
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 8, A1))
        SH.patch_blocks(s, diag, pr.A)                                    # the plan still keeps: a copy of the new shape takes the patch
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 8))


# ---- 2. a second setBuffer without a new bufferSize ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_second_set_buffer_on_a_new_workspace(system, fresh, prec):
    pr, _, diag, A1 = system
    with _Plan() as s:
        _, nbytes = _kept_patched_plan(s, pr, diag, A1, prec)
        s.new_buffer(nbytes)
        # the new buffer holds no A: the set-up has nothing to scale (status 14, key 'A'), and nothing to patch
        assert T.decode(T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, SH.TOL[prec], SH.MAXIT))[::2] == (14, ord("A"))
        s.set_matrix("A", A1)
        s.set_matrix("B", pr.B)
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 4, A1))
        SH.patch_blocks(s, diag, pr.A)
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 4))


# ---- 3. keepOperator(0) after patches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_keep_operator_off_after_patches(system, fresh, prec):
    pr, _, diag, A1 = system
    with _Plan() as s:
        _kept_patched_plan(s, pr, diag, A1, prec)
        SH.patch_blocks(s, diag[:3], pr.A)                                # marks that no set-up has seen go with the copy
        s.keep_operator(False)
        with pytest.raises(T.TfqmrError) as e:                           # as on a plan that never kept: A M^-1 cannot be patched
            s.set_blocks("A", diag[:1], pr.A[diag[:1]])
        assert T.decode(e.value.status)[0] == 19
        s.set_matrix("A", pr.A)
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 4))


# ---- 4. lists that grow -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
def test_block_list_and_dirty_list_grow(system, fresh, prec):
    pr, _, diag, A1 = system
    every = np.arange(pr.nnzbA, dtype=np.int32)
    one = SH.changed(pr, pr.A, diag[5:6], seed=23)
    with _Plan() as s:
        s.create_plan(pr)
        nbytes = s.buffer_size(pr.LM, pr.LN, prec)
        s.set_preconditioner(BJ)
        s.keep_operator(True)
        s.new_buffer(nbytes)
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 4))
        SH.patch_blocks(s, diag[5:6], one)                                # a list of one block; the set-up redoes one row and one column
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 4, one))
        SH.patch_blocks(s, every, A1)                                     # every block: both device lists are longer than before
        SH.same_record(SH.solve_record(s, prec), fresh(prec, 4, A1))
        assert np.array_equal(s.get_blocks(np.arange(pr.nnzbX, dtype=np.int32)), s.get_matrix())


# ---- 5. a user-operator plan changes its shape ------------------------------------------------------------------------------------------------
def _operator_solve(torch, s, pr, prec="z"):
    s.set_matrix("A", 0 * pr.A)
    s.set_matrix("B", pr.B)
    s.set_operator(SH.builtin_as_operator(torch, s, pr, prec, s.plan_view(), []))
    st = s.solve(pr.tolerance, SH.MAXIT)
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
            SH.same_record(got, _operator_solve(torch, f, p))
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
        dA = SH.native_A(torch, pr, "z")
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
            SH.patch_blocks(s, diag[:2], A1)                              # (not scaled yet: the patch goes into the buffer; a block list exists)
        if steps >= 4:
            s.get_preconditioner(values=False)                           # 4: set up and kept, never solved
        if steps >= 5:
            SH.patch_blocks(s, diag[2:4], A1)                             # 5: solved, with marks that no set-up has seen
            s.solve(1e-9, 5)
            SH.patch_blocks(s, diag[4:6], A1)


def test_destroy_a_handle_with_a_vote_buffer():
    with _Plan() as s:                                                   # the device buffer of the ranks' vote comes with the callback
        cb = T.REDUCE_CB(lambda ctx, v, n: None)
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, cb, None) == 0
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, cb, None) == 0
        assert T.lib.tfqmrgpuExt_setReduceCallback(s.handle, T.REDUCE_CB(0), None) == 0


# ---- 8. a second bufferSize and a second setBuffer with everything of sections 10 to 17 alive ---------------------------------------------------
# What a plan keeps for these calls is sized or cut by the layout (the scratch of the residual, the leak listing and its device copy, the
# records of the leak map and of the drop cost, M^-1) or holds values of one buffer (X0 and R of a warm solve, the kept starts and the scratch
# of their projection, the kept A).  Each of them is built by its first call and found there by every later one: one that outlived its
# layout would be read and written with the new shape.
WARM_MAXIT = 8


@pytest.fixture(scope="module")
def stencils():
    """{LN: the small truncated stencil of test_gpu_truncation_leak.py with 4 x LN right-hand-side blocks}: 16 block rows, one full block
    column and two with leak positions.  The patterns do not depend on LN: one plan serves both"""
    prs = {LN: PR.stencil_2d(4, 4, 4, LN, ncols=3, seed=404, radius=[None, 1.1, 2.3]) for LN in (4, 8)}
    for name in ("rowPtrA", "colIndA", "rowPtrX", "colIndX", "rowPtrB", "colIndB"):
        assert np.array_equal(getattr(prs[4], name), getattr(prs[8], name)), name
    assert prs[4].mb == 16 and np.array_equal(prs[4].A, prs[8].A)
    return prs


def _lay_out(s, LN, prec, kept):
    """bufferSize, what the caller asks for (it outlives every later bufferSize), a new workspace"""
    nbytes = s.buffer_size(4, LN, prec)
    if kept:                                                             # M^-1 and the kept copy of the caller's A exist as well
        s.set_preconditioner(BJ)
        s.keep_operator(True)
    s.new_buffer(nbytes)
    return nbytes


def _left(s, status, prec):
    info = s.get_info()
    out = dict(status=status, iterations=info["iterations"], residual=info["residual"], flops=info["flops"], bounds=s.bound_history(),
               X=s.get_matrix())
    if prec == "m":
        out["refinement"], out["cycle_iterations"] = s.refinement_history(with_iterations=True)
    return out


def _warm(s, prec):
    return (s.refine_from if prec == "m" else s.solve_from)(SH.TOL[prec], WARM_MAXIT)


def _everything_alive(s, pr, prec, kept):
    """on a laid-out plan with a buffer: every call of sections 10 to 17 once, so that each library-owned piece exists; all results"""
    out = {}
    cplx = lambda seed, shape: PR.hashed_uniform(seed, shape) - 0.5 + 1j * (PR.hashed_uniform(seed + 1, shape) - 0.5)   # noqa: E731
    s.set_matrix("A", pr.A)
    s.set_matrix("B", pr.B)
    out["solve"] = _left(s, s.solve(SH.TOL[prec], WARM_MAXIT), prec)
    if kept:
        out["Minv"], out["n_identity"] = s.get_preconditioner()
    out["residual"], out["leak"], out["map"], out["drop"] = s.residual(), s.truncation_leak(), s.leak_map(), s.drop_cost()
    s.keep_starts(2)
    s.push_start()
    s.set_matrix("B", pr.B[:, :, ::-1] * (0.5 - 0.25j))
    out["solve2"] = _left(s, s.solve(SH.TOL[prec], WARM_MAXIT), prec)
    s.push_start()
    out["starts"] = (s.start_count(), s.start_depth())
    s.set_matrix("B", pr.B + 0.3 * cplx(51, pr.B.shape))                # not in the span of the two: the warm solve has work to do
    out["project"] = s.project_start()
    out["projected"] = s.get_matrix()
    out["warm"] = _left(s, _warm(s, prec), prec)
    listed = np.arange(0, pr.nnzbX, 3, dtype=np.int32)
    s.set_blocks("X", listed, cplx(31, (len(listed), pr.LM, pr.LN)))
    out["listed"] = s.get_matrix()
    # X from a second, smaller plan of the same block shape: every block of this plan takes a block of that one, every fifth is zero
    small = PR.stencil_2d(4, 4, pr.LM, pr.LN, ncols=3, seed=405, radius=[None, 1.1, 1.1])
    assert small.nnzbX < pr.nnzbX
    old = (np.arange(pr.nnzbX, dtype=np.int32) * 7) % small.nnzbX
    old[::5] = -1
    with _Plan() as src:
        src.create_plan(small)
        src.new_buffer(src.buffer_size(pr.LM, pr.LN, "z"))
        src.set_matrix("X", cplx(41, (small.nnzbX, pr.LM, pr.LN)))
        s.carry_from(src, "X", old)
        out["carried"] = s.get_matrix()
    return out


def _flat(d, prefix=""):
    out = {}
    for k, v in d.items():
        out.update(_flat(v, prefix + k + ".") if isinstance(v, dict) else {prefix + k: v})
    return out


def _same_entries(got, want):
    got, want = _flat(got), _flat(want)
    print("everything alive:", {k: got[k] for k in got if k.split(".")[-1] in ("status", "iterations", "starts", "n_leak_blocks", "n_leak_pairs", "worst")})
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert want["starts"] == (2, 2) and min(want["solve.iterations"], want["warm.iterations"]) >= 1 and want["leak.n_leak_blocks"] > 0


@pytest.fixture(scope="module")
def alive_fresh(stencils):
    """the yardsticks, each computed once: (LN, precision, kept) -> what a plan that only ever saw this layout leaves behind"""
    cache = {}

    def get(LN, prec, kept):
        if (LN, prec, kept) not in cache:
            with _Plan() as s:
                s.create_plan(stencils[LN])
                _lay_out(s, LN, prec, kept)
                cache[LN, prec, kept] = _everything_alive(s, stencils[LN], prec, kept)
        return cache[LN, prec, kept]
    return get


# each group of the plan's state grows and shrinks, and the storage type changes under it
STEPS = [((4, "z"), (8, "z")), ((8, "z"), (4, "c")), ((4, "c"), (8, "m")), ((8, "m"), (4, "z"))]


@pytest.mark.parametrize("kept", [False, True], ids=["plain", "kept"])
@pytest.mark.parametrize("before,after", STEPS, ids=["4z-8z", "8z-4c", "4c-8m", "8m-4z"])
def test_second_buffer_size_with_everything_alive(stencils, alive_fresh, before, after, kept):
    (LN0, prec0), (LN1, prec1) = before, after
    want = alive_fresh(LN1, prec1, kept)
    with _Plan() as s:
        s.create_plan(stencils[LN0])
        _lay_out(s, LN0, prec0, kept)
        _same_entries(_everything_alive(s, stencils[LN0], prec0, kept), alive_fresh(LN0, prec0, kept))
        nbytes = s.buffer_size(4, LN1, prec1)
        assert (s.start_count(), s.start_depth()) == (0, 2)              # the starts go with their buffer, the depth is the caller's
        assert T.lib.tfqmrgpuExt_leakUnits(s.plan, None) == 0            # the listing of the old shape is gone ...
        assert s.leak_counts() == (want["leak"]["n_leak_blocks"], want["leak"]["n_leak_pairs"])   # ... and is built again on demand
        s.new_buffer(nbytes)
        _same_entries(_everything_alive(s, stencils[LN1], prec1, kept), want)


@pytest.mark.parametrize("kept", [False, True], ids=["plain", "kept"])
@pytest.mark.parametrize("prec", ["z", "c", "m"])
def test_second_set_buffer_with_everything_alive(stencils, alive_fresh, prec, kept):
    pr = stencils[4]
    want = alive_fresh(4, prec, kept)
    warm = T.lib.tfqmrgpuExt_refineFrom if prec == "m" else T.lib.tfqmrgpuExt_solveFrom
    with _Plan() as never:                                               # a plan whose A was never set
        never.create_plan(pr)
        _lay_out(never, 4, prec, kept)
        refused = warm(never.handle, never.plan, SH.TOL[prec], WARM_MAXIT)
    assert T.decode(refused)[::2] == (14, ord("A"))
    with _Plan() as s:
        s.create_plan(pr)
        nbytes = _lay_out(s, 4, prec, kept)
        _same_entries(_everything_alive(s, pr, prec, kept), want)
        s.new_buffer(nbytes)
        assert (s.start_count(), s.start_depth()) == (0, 2)
        assert warm(s.handle, s.plan, SH.TOL[prec], WARM_MAXIT) == refused   # the new buffer holds no A, and no X0 of the old one
        _same_entries(_everything_alive(s, pr, prec, kept), want)
