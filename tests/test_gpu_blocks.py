"""tfqmrgpuExt_setBlocks / tfqmrgpuExt_getBlocks (include/tfqmrgpu_ext.h section 8) on the GPU, through the C-ABI: listed blocks against
the whole-operand calls.  A conversion moves numbers and never computes with them, so every comparison is exact (np.array_equal): a
get is a slice of getMatrix, a set changes the listed blocks and nothing else, and a solve after a partial update is the solve after the
whole update bit for bit.  B has no getter (getMatrix hands out X only), so B is read back through what a solve makes of it.
Needs an MI355X (`pytest -m gpu`)."""
import numpy as np
import pytest

import tfqmrgpu_amd as T
from conftest import offset1
from helpers import exact_random_blocks, real_dtype, torch_cuda, user_array  # noqa: F401  (torch_cuda: a fixture)
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

LAYOUTS = (T.LAYOUT_RIRIRIRI, T.LAYOUT_RRRRIIII, T.LAYOUT_RRIIRRII)
TRANS = "nt*c"
# one shape per element order / kernel class: 16 x 16 and 8 x 8 (rows interleaved in 'z'), 4 x 5 (ragged, never interleaved), 8 x 32
# (rectangular: a transposition that is wrong shows), 32 x 32 (interleaved in 'c')
SHAPES = [(16, 16), (8, 8), (4, 5), (8, 32), (32, 32)]
TOL = {"z": 1e-9, "c": 1e-4, "m": 1e-9}
MAXIT = 500


def _small(LM, LN):
    return PR.stencil_2d(4, 3, LM, LN, 3, seed=12, radius=1.6)   # the plans of test_set_get_matrix_layouts


def _half_list(rng, n, twice):
    """about half of the blocks 0 ... n - 1 in a shuffled order, the first and the last among them; twice: one of them a second time"""
    inner = rng.permutation(np.arange(1, n - 1))[: max(1, n // 2 - 2)]
    idx = rng.permutation(np.concatenate([[0, n - 1], inner]))
    if np.all(np.diff(idx) > 0):
        idx = idx[::-1]
    if twice:
        idx = np.insert(idx, len(idx) // 2, idx[0])
    return idx.astype(np.int32)


def _plan(s, pr, prec, kind=None):
    s.create_plan(pr)
    nbytes = s.buffer_size(pr.LM, pr.LN, prec)
    if kind is not None:
        s.set_preconditioner(kind)
    s.set_buffer(nbytes=nbytes)


def _diagonal(pr):
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    return np.flatnonzero(rows == pr.colIndA - pr.index_offset).astype(np.int32)


def _other_diagonal(pr, seed=77):
    """A with every diagonal block changed, still block diagonally dominant"""
    diag = _diagonal(pr)
    assert len(diag) == pr.mb
    A1 = pr.A.copy()
    A1[diag] += 0.5 * np.eye(pr.LM) + 0.05 * (PR.hashed_uniform(seed, A1[diag].shape) + 1j * PR.hashed_uniform(seed + 1, A1[diag].shape))
    return diag, A1


def _solve(s, prec):
    """everything a solve leaves behind, for exact comparison"""
    st = s.solve(TOL[prec], MAXIT)
    info = s.get_info()
    out = dict(status=st, iterations=info["iterations"], residual=info["residual"], bounds=s.bound_history(), X=s.get_matrix())
    if prec == "m":
        out["refinement"], out["cycle_iterations"] = s.refinement_history(with_iterations=True)
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["iterations"] >= 1 and len(a["bounds"]) >= 1 and np.all(np.isfinite(a["X"]))


# ---- 1. get is a slice of getMatrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
@pytest.mark.parametrize("shape", SHAPES)
def test_get_blocks_is_a_slice_of_get_matrix(prec, shape):
    LM, LN = shape
    pr = _small(LM, LN)
    rng = np.random.default_rng(100 * LM + LN)
    idx = _half_list(rng, pr.nnzbX, twice=True)
    assert len(set(idx)) == len(idx) - 1 and {0, pr.nnzbX - 1} <= set(idx) and np.any(np.diff(idx) < 0)
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("X", exact_random_blocks(rng, pr.nnzbX, LM, LN, prec))
        for layout in LAYOUTS:
            for tr in TRANS:
                whole = s.get_matrix(trans=tr, layout=layout, raw=True)
                got = s.get_blocks(idx, trans=tr, layout=layout, raw=True)
                assert got.dtype == whole.dtype and np.array_equal(got, whole[idx]), (layout, tr)
        # the shapes of the unpacked form follow get_matrix
        assert np.array_equal(s.get_blocks(idx), s.get_matrix()[idx]) and s.get_blocks(idx).shape == (len(idx), LM, LN)
        assert np.array_equal(s.get_blocks(idx, trans="t"), s.get_matrix(trans="t")[idx]) and s.get_blocks(idx, trans="t").shape == (len(idx), LN, LM)


# ---- 2. set changes the listed blocks and nothing else ------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
@pytest.mark.parametrize("shape", SHAPES)
def test_set_blocks_changes_the_listed_blocks_of_x_only(prec, shape):
    LM, LN = shape
    pr = _small(LM, LN)
    rng = np.random.default_rng(200 * LM + LN)
    idx = _half_list(rng, pr.nnzbX, twice=False)
    X0, V = exact_random_blocks(rng, pr.nnzbX, LM, LN, prec), exact_random_blocks(rng, len(idx), LM, LN, prec)
    want = X0.copy()
    want[idx] = V
    with T.Solver.open(pr, prec) as s:
        for layout in LAYOUTS:
            for tr in TRANS:
                s.set_matrix("X", X0)
                s.set_blocks("X", idx, user_array(V, layout, tr).astype(real_dtype(prec)), tr, layout)
                assert np.array_equal(s.get_matrix(), want), (layout, tr)


@pytest.mark.parametrize("prec", ["z", "c"])
@pytest.mark.parametrize("shape", SHAPES)
def test_set_blocks_of_b_is_set_matrix_of_b(prec, shape):
    """B is read back through a solve: the same B in the buffer gives the same iterations, bounds and X bit for bit.  A partial list in every
    layout and transposition against setMatrix of the patched B, and all blocks in reversed order against setMatrix of the same data"""
    LM, LN = shape
    pr = _small(LM, LN)
    rng = np.random.default_rng(300 * LM + LN)
    assert pr.nnzbB == 3
    some = np.array([2, 0], np.int32)
    V = exact_random_blocks(rng, len(some), LM, LN, prec)
    B1 = pr.B.copy()
    B1[some] = V
    every = np.arange(pr.nnzbB, dtype=np.int32)[::-1]
    with T.Solver() as q, T.Solver() as s:
        _plan(q, pr, prec)
        q.set_matrix("A", pr.A)
        q.set_matrix("B", B1)
        patched = _solve(q, prec)
        q.set_matrix("B", pr.B)
        plain = _solve(q, prec)
        assert not np.array_equal(plain["X"], patched["X"])
        _plan(s, pr, prec)
        s.set_matrix("A", pr.A)
        for layout in LAYOUTS:
            for tr in TRANS:
                s.set_matrix("B", pr.B)
                s.set_blocks("B", some, user_array(V, layout, tr).astype(real_dtype(prec)), tr, layout)
                _same(_solve(s, prec), patched)
        s.set_matrix("B", B1)
        s.set_blocks("B", every, pr.B[every])
        _same(_solve(s, prec), plain)


# ---- 3. a partial update of A is the whole update -----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,shape", [("z", (16, 16)), ("c", (8, 8)), ("m", (16, 16))])
def test_diagonal_update_of_a_is_the_whole_update(prec, shape):
    LM, LN = shape
    pr = _small(LM, LN)
    diag, A1 = _other_diagonal(pr)
    with T.Solver.open(pr, prec) as q:
        q.set_matrix("A", A1)
        q.set_matrix("B", pr.B)
        want = _solve(q, prec)
        q.set_matrix("A", pr.A)
        assert not np.array_equal(_solve(q, prec)["X"], want["X"])      # the diagonal matters
    assert want["status"] == 0 and want["iterations"] <= 20
    for tr in "nt":
        with T.Solver.open(pr, prec) as s:
            s.set_matrix("A", pr.A)
            s.set_blocks("A", diag, A1[diag] if tr == "n" else A1[diag].transpose(0, 2, 1), tr)
            s.set_matrix("B", pr.B)
            _same(_solve(s, prec), want)      # 'm': the refinement history pins the float copy of A as well


# ---- 4. B's pattern -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("prec,shape", [("z", (16, 16)), ("c", (4, 8))])
def test_blocks_on_the_pattern_of_b(prec, shape, off):
    pr = _small(*shape)
    pr = offset1(pr) if off else pr
    with T.Solver.open(pr, prec) as s:
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(TOL[prec], MAXIT) == 0
        subset = s.plan_view()["subset"]
        assert len(subset) == pr.nnzbB and len(set(subset)) == pr.nnzbB
        X = s.get_matrix()
        assert np.array_equal(s.get_blocks(None), X[subset]) and np.abs(X[subset]).max(axis=(1, 2)).min() > 0
        assert np.array_equal(s.get_blocks(), s.get_blocks(subset))
        for layout in LAYOUTS:
            assert np.array_equal(s.get_blocks(None, "c", layout, raw=True), s.get_matrix(trans="c", layout=layout, raw=True)[subset])


# ---- 5. more blocks than the stage holds --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "m"])
def test_a_list_longer_than_one_batch(prec):
    """64 blocks of A through a stage of 6 nnzbX = 48 blocks ('m' fed double data: float-sized vectors, 24 blocks), in reversed order"""
    pr = PR.dense_random(mb=8, LM=8, LN=8, ncols=1, seed=5)
    assert pr.nnzbA == 64 and 6 * pr.nnzbX == 48
    every = np.arange(pr.nnzbA, dtype=np.int32)[::-1]
    with T.Solver() as q, T.Solver() as s:
        _plan(q, pr, prec)
        q.set_matrix("A", pr.A)
        q.set_matrix("B", pr.B)
        want = _solve(q, prec)
        _plan(s, pr, prec)
        assert s.data_precision == "z"
        s.set_blocks("A", every, pr.A[every])
        s.set_matrix("B", pr.B)
        _same(_solve(s, prec), want)
    assert want["status"] == 0


# ---- 6. values in device memory -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["z", "c"])
def test_device_arrays_give_the_bytes_of_the_host_path(torch_cuda, prec):
    torch = torch_cuda
    LM = LN = 16
    pr = _small(LM, LN)
    rng = np.random.default_rng(6)
    ctype = np.complex64 if prec == "c" else np.complex128
    idx = _half_list(rng, pr.nnzbX, twice=False)
    X0, V = exact_random_blocks(rng, pr.nnzbX, LM, LN, prec), exact_random_blocks(rng, len(idx), LM, LN, prec)
    with T.Solver.open(pr, prec) as s:
        for tr in "nc":
            s.set_matrix("X", X0)
            s.set_blocks("X", idx, V, tr)
            host = s.get_matrix()
            s.set_matrix("X", X0)
            dV = torch.from_numpy(V.astype(ctype)).cuda()
            s.set_blocks_device("X", idx, dV.data_ptr(), tr)
            torch.cuda.synchronize()
            assert np.array_equal(s.get_matrix(), host) and not np.array_equal(host, X0)
        twice = np.append(idx, idx[:2])
        for blocks, n in ((twice, len(twice)), (None, pr.nnzbB)):
            for tr in "nt":
                dOut = torch.zeros((n, LM, LN), dtype=dV.dtype, device="cuda")
                s.get_blocks_device(dOut.data_ptr(), blocks, tr)
                torch.cuda.synchronize()
                assert np.array_equal(dOut.cpu().numpy().reshape(n, -1), s.get_blocks(blocks, tr).astype(ctype).reshape(n, -1))


# ---- 7. with the block-Jacobi preconditioner ----------------------------------------------------------------------------------------
def test_preconditioned_plan():
    prec, BJ = "z", T.PRECOND_BLOCK_JACOBI
    pr = _small(16, 16)
    diag, A1 = _other_diagonal(pr)
    with T.Solver() as q, T.Solver() as s:
        _plan(q, pr, prec, BJ)
        q.set_matrix("A", A1)
        q.set_matrix("B", pr.B)
        want = _solve(q, prec)
        assert want["status"] == 0
        # between setMatrix('A') and the first solve: A is not scaled yet, the solve inverts and scales what is then in the buffer
        _plan(s, pr, prec, BJ)
        s.set_matrix("A", pr.A)
        s.set_blocks("A", diag, A1[diag])
        s.set_matrix("B", pr.B)
        _same(_solve(s, prec), want)
        # now the buffer holds A M^-1: refused, and nothing written
        with pytest.raises(T.TfqmrError) as e:
            s.set_blocks("A", diag, pr.A[diag])
        assert T.decode(e.value.status)[0] == 19      # TFQMRGPU_NO_IMPLEMENTATION
        _same(_solve(s, prec), want)
        X = s.get_matrix()
        assert np.array_equal(s.get_blocks(None), X[s.plan_view()["subset"]])   # X, not Y: the back-transformed solution
        # a whole setMatrix('A') makes partial updates possible again
        s.set_matrix("A", pr.A)
        s.set_blocks("A", diag[::-1], A1[diag[::-1]])
        _same(_solve(s, prec), want)


# ---- 8. a plan that calls nothing of this ---------------------------------------------------------------------------------------------
def test_plans_that_do_not_call_it_see_nothing():
    pr = _small(16, 16)
    runs = []
    for calls in (False, True):
        with T.Solver.open(pr, "z") as s:
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            assert s.solve(TOL["z"], MAXIT) == 0
            if calls:
                assert s.get_blocks(None).shape == (pr.nnzbB, 16, 16) and s.get_blocks([0, 3, 0]).shape == (3, 16, 16)
            runs.append((s.get_matrix(), s.bound_history()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert len(runs[0][1]) >= 1
