"""The energy mesh (include/tfqmrgpu_ext.h section 19) on the GPU.  Every numerical claim is bit for bit against calls the library already
has: shift_diagonal against set_blocks('A') of the diagonal blocks formed on the host (tests/mesh_ref.py), the sum against its restatement
in real numpy arithmetic on get_blocks(), solve_mesh against the same loop written with the public Python calls on a twin plan.  No
tolerance anywhere but the meaning that `threshold` already has."""
import ctypes as C

import numpy as np
import pytest

import mesh_ref as MR
import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import bits, same_typed_bits
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

POINTER_INVALID, BREAKDOWN, MAX_ITERATIONS, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 6, 9, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
# the smallest shapes at which each block order can go wrong (tests/test_gpu_solve_from.py)
FIXTURES = ["fd_4x4_2d", "fd_16x16_small", "fd_8x8_3d", "stencil_8x32", "dense_random_rect"]
PRECISIONS = ["z", "c", "m"]
SIGMA = 1e-3 * (1 + 0.5j)
W1, W2 = 0.75 - 0.5j, -0.3 + 1.25j


def _stored(A, prec):
    a = np.asarray(A, dtype=np.complex128)
    return (a.astype(np.complex64).astype(np.complex128) if prec == "c" else a).copy()


def _x0(pr, seed=5):
    """an X that every storage precision holds exactly"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((pr.nnzbX, pr.LM, pr.LN)) + 1j * rng.standard_normal((pr.nnzbX, pr.LM, pr.LN))
    return v.astype(np.complex64).astype(np.complex128)


def _product(s, X0):
    """A X0 by the plan's own multiply: it reads every element of A in plan order"""
    s.set_matrix("X", X0)
    s.apply_operator()
    return s.get_matrix()


def _solved(s, iterations=3):
    assert s.solve(1e-30, iterations) == MAX_ITERATIONS
    return s.get_matrix(), s.bound_history()


def _same_operator(p, q, X0):
    """the same product, and the same three iterations: the second reads the float A of an 'm' plan as well"""
    assert same_typed_bits(_product(p, X0), _product(q, X0))
    (xp, hp), (xq, hq) = _solved(p), _solved(q)
    assert same_typed_bits(xp, xq) and same_typed_bits(hp, hq)


def _padded_problem():
    return PR.stencil_2d(4, 3, 9, 9, 3, seed=909)      # 9 x 9 on 16 x 16, cut as tests/test_gpu_padding.py cuts its problems


# ---- 1. shift ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", FIXTURES)
def test_shift_is_set_blocks_of_the_diagonal(name, prec):
    """P: shift_diagonal(sigma).  Q, a twin: set_blocks('A') of every diagonal block with stored(A) + sigma 1 formed on the host in the
    storage precision ('m': 'z' data).  U, a third: never shifted.  shift(sigma), shift(2 sigma), shift(0) on P gives U's bits back"""
    pr = load_problem(name)
    diag, X0 = MR.diagonal_blocks(pr), _x0(pr)
    assert len(diag) == pr.mb
    with T.Solver.open(pr, prec).load() as p, T.Solver.open(pr, prec).load() as q, T.Solver.open(pr, prec).load() as u:
        assert p.shift_diagonal(SIGMA) == 0
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, SIGMA))
        _same_operator(p, q, X0)
        assert not same_typed_bits(_product(p, X0), _product(u, X0))          # and it is another operator than before
        # shifts do not accumulate
        for sigma in (SIGMA, 2 * SIGMA, 0.0):
            assert p.shift_diagonal(sigma) == 0
        _same_operator(p, u, X0)
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, 2 * SIGMA))
        assert p.shift_diagonal(2 * SIGMA) == 0
        _same_operator(p, q, X0)


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", ["fd_16x16_small", "stencil_8x32"])
def test_shift_on_a_preconditioned_plan_that_keeps_a(name, prec):
    """block-Jacobi and keepOperator, after a first solve: the shift goes into the kept copy and marks every block row and column, the next
    set-up redoes them through the partial set-up: M^-1 and the solve have the bits of the twin that got set_blocks('A')"""
    pr = load_problem(name)
    diag = MR.diagonal_blocks(pr)
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True).load() as p, T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True).load() as q:
        (xp, _), (xq, _) = _solved(p), _solved(q)
        assert same_typed_bits(xp, xq)
        assert p.shift_diagonal(SIGMA) == 0
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, SIGMA))
        (mp, ip), (mq, iq) = p.get_preconditioner(), q.get_preconditioner()
        assert ip == iq == 0 and same_typed_bits(mp, mq)
        (xp2, hp), (xq2, hq) = _solved(p), _solved(q)
        assert same_typed_bits(xp2, xq2) and same_typed_bits(hp, hq) and not same_typed_bits(xp2, xp)
        # and a second shift builds on the caller's diagonal, not on the shifted one
        assert p.shift_diagonal(2 * SIGMA) == 0
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, 2 * SIGMA))
        assert same_typed_bits(p.get_preconditioner()[0], q.get_preconditioner()[0])
        assert same_typed_bits(_solved(p)[0], _solved(q)[0])


def test_shift_on_a_scaled_plan_without_a_copy_is_refused():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "z", preconditioner=BJ).load() as s:
        x, h = _solved(s)
        m = s.get_preconditioner()[0]
        assert T.decode(T.lib.tfqmrgpuExt_shiftDiagonal(s.handle, s.plan, SIGMA.real, SIGMA.imag))[::2] == (NO_IMPLEMENTATION, 0)
        x2, h2 = _solved(s)                                              # nothing has been written: the same operator, the same M^-1
        assert same_typed_bits(x, x2) and same_typed_bits(h, h2) and same_typed_bits(m, s.get_preconditioner()[0])


@pytest.mark.parametrize("prec", PRECISIONS)
def test_shift_builds_on_the_base_that_the_last_write_left(prec):
    """set_blocks('A') of one diagonal block, a whole set_matrix('A') and carry_from(.., 'A') each call the captured diagonal stale"""
    pr = load_problem("fd_16x16_small")
    diag, X0 = MR.diagonal_blocks(pr), _x0(pr)
    rng = np.random.default_rng(11)
    patch = (rng.standard_normal((1, pr.LM, pr.LM)) + 1j * rng.standard_normal((1, pr.LM, pr.LM))).astype(np.complex64).astype(np.complex128)
    patched = _stored(pr.A, prec)
    patched[diag[1]] = patch[0]
    other = _stored(pr.A, prec)
    other[diag] *= 1.25
    with T.Solver.open(pr, prec).load() as p, T.Solver.open(pr, prec).load() as q, T.Solver.open(pr, prec).load() as src:
        assert p.shift_diagonal(SIGMA) == 0                              # captures the diagonal of pr.A
        p.set_blocks("A", diag[1:2], patch)
        assert p.shift_diagonal(2 * SIGMA) == 0
        q.set_blocks("A", diag[1:2], patch)
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(patched, diag, prec, 2 * SIGMA))
        _same_operator(p, q, X0)
        # a whole new A
        p.set_matrix("A", other)
        assert p.shift_diagonal(SIGMA) == 0
        q.set_matrix("A", other)
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(other, diag, prec, SIGMA))
        _same_operator(p, q, X0)
        # A carried from another plan
        p.carry_from(src, "A")
        assert p.shift_diagonal(SIGMA) == 0
        q.set_matrix("A", pr.A)
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, SIGMA))
        _same_operator(p, q, X0)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_shifts_do_not_accumulate_through_patches_and_refused_writes(prec):
    """Two sequences that leave a shifted A in the plan while something looks like a write of A.  (1) An impurity loop: the same diagonal
    block set mb + 1 times between two shifts.  (2) A set_matrix('A') that is refused behind its naming of A -- the wrong precision, no
    values.  Neither may make the next shift take base + sigma for the base: the twin gets set_blocks('A') of the true A + sigma2 1"""
    pr = load_problem("fd_4x4_2d")
    diag, X0 = MR.diagonal_blocks(pr), _x0(pr)
    rng = np.random.default_rng(12)
    patch = (rng.standard_normal((1, pr.LM, pr.LM)) + 1j * rng.standard_normal((1, pr.LM, pr.LM))).astype(np.complex64).astype(np.complex128)
    patch += 8 * np.eye(pr.LM)
    patched = _stored(pr.A, prec)
    patched[diag[2]] = patch[0]
    with T.Solver.open(pr, prec).load() as p, T.Solver.open(pr, prec).load() as q:
        assert p.shift_diagonal(SIGMA) == 0
        for _ in range(pr.mb + 1):
            p.set_blocks("A", diag[2:3], patch)
        assert p.shift_diagonal(3 * SIGMA) == 0
        q.set_blocks("A", diag[2:3], patch)
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(patched, diag, prec, 3 * SIGMA))
        _same_operator(p, q, X0)
    with T.Solver.open(pr, prec).load() as p, T.Solver.open(pr, prec).load() as q:
        assert p.shift_diagonal(SIGMA) == 0
        raw = np.zeros((pr.nnzbA, pr.LM, pr.LM, 2), np.float64)
        wrong = b"z" if prec == "c" else b"c"
        refusals = [T.lib.tfqmrgpu_bsrsv_setMatrix(p.handle, p.plan, b"A", None, p.data_precision.encode(), pr.LM, pr.LM, b"n", T.LAYOUT_RIRIRIRI)]
        if prec != "m":                                                  # (an 'm' plan takes both precisions)
            refusals.append(T.lib.tfqmrgpu_bsrsv_setMatrix(p.handle, p.plan, b"A", T._ptr(raw), wrong, pr.LM, pr.LM, b"n", T.LAYOUT_RIRIRIRI))
        assert [T.decode(st)[0] for st in refusals] == [POINTER_INVALID, 16][:len(refusals)]
        assert p.shift_diagonal(2 * SIGMA) == 0
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, 2 * SIGMA))
        _same_operator(p, q, X0)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_shift_on_a_padded_plan(prec):
    """9 x 9 on 16 x 16: only the first 9 diagonal elements move; M^-1 keeps 1 on the padded diagonal"""
    pr = _padded_problem()
    diag, X0 = MR.diagonal_blocks(pr), _x0(pr)
    assert len(diag) == pr.mb
    with T.Solver.open(pr, prec, allow_padding=True).load() as p, T.Solver.open(pr, prec, allow_padding=True).load() as q:
        assert p.padded_shape() == (9, 9, 16, 16)
        assert p.shift_diagonal(SIGMA) == 0
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, SIGMA))
        _same_operator(p, q, X0)
    with T.Solver.open(pr, prec, allow_padding=True, preconditioner=BJ, keep_operator=True).load() as p, T.Solver.open(pr, prec, allow_padding=True, preconditioner=BJ, keep_operator=True).load() as q:
        _solved(p), _solved(q)
        assert p.shift_diagonal(SIGMA) == 0
        q.set_blocks("A", diag, MR.shifted_diagonal_blocks(pr.A, diag, prec, SIGMA))
        (mp, ip), (mq, _) = p.get_preconditioner(), q.get_preconditioner()
        assert ip == 0 and same_typed_bits(mp, mq) and mp.shape == (pr.mb, 16, 16)
        assert np.all(mp[:, 9:, 9:] == np.eye(7)) and np.all(mp[:, 9:, :9] == 0) and np.all(mp[:, :9, 9:] == 0)
        assert same_typed_bits(_solved(p)[0], _solved(q)[0])


def test_shift_statuses_that_need_a_device():
    raw = lambda s: T.decode(T.lib.tfqmrgpuExt_shiftDiagonal(s.handle, s.plan, SIGMA.real, SIGMA.imag))[::2]      # noqa: E731
    pr = load_problem("fd_4x4_2d")
    with T.Solver.open(pr, "z") as s:                                            # A has never been set whole on this buffer
        s.set_matrix("B", pr.B)
        assert raw(s) == (UNDOCUMENTED, ord("A"))
        s.set_blocks("A", [0], pr.A[:1])                                 # a patch makes no whole A
        assert raw(s) == (UNDOCUMENTED, ord("A"))
    # a block row without a diagonal block: A + sigma 1 cannot be represented; nothing is written
    nd = MR.no_diagonal_problem()
    X0 = _x0(nd)
    for prec in PRECISIONS:
        with T.Solver.open(nd, prec).load() as s, T.Solver.open(nd, prec).load() as u:
            assert raw(s) == (UNDOCUMENTED, ord("D"))
            assert same_typed_bits(_product(s, X0), _product(u, X0))
            s.set_operator(lambda *a: 0.0)                               # the operator is looked at first
            assert raw(s) == (NO_IMPLEMENTATION, 0)


# ---- 2. sum -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", FIXTURES)
def test_sum_is_its_restatement_in_real_arithmetic(name, prec):
    pr = load_problem(name)
    import torch
    with T.Solver.open(pr, prec, keep_sum=True, buffer=False) as s:
        s.torch_buffer = torch.zeros(s.buffer_bytes, dtype=torch.uint8, device="cuda")      # a buffer of the test's own: it can be looked at, byte for byte
        s.set_buffer(device_ptr=s.torch_buffer.data_ptr())
        s.load()
        S, n = s.get_sum()
        assert n == 0 and S.shape == (pr.nnzbB, pr.LM, pr.LN) and not S.any()       # no term yet: zeros, and nothing allocated
        terms = []
        for w, its in ((W1, 2), (W2, 3)):
            assert s.solve(1e-30, its) == MAX_ITERATIONS
            # the work vectors through their getter, which serves 'z' and 'c' plans only (an 'm' plan's are refused with
            # PRECISION_MISSMATCH); and, for every precision, the whole buffer byte for byte -- 'm': the float vectors and the double side
            before = {v: s.get_work_vector(v) for v in (4, 5, 6, 7, 8, 9)} if prec != "m" else {}
            h, info = s.bound_history(), s.get_info()
            torch.cuda.synchronize()
            snapshot = s.torch_buffer.clone()
            assert s.add_to_sum(w) == 0
            torch.cuda.synchronize()
            assert torch.equal(snapshot, s.torch_buffer)                 # the buffer is untouched
            for v in before:
                assert same_typed_bits(before[v], s.get_work_vector(v)), v
            assert same_typed_bits(h, s.bound_history()) and s.get_info() == info
            terms.append((w, s.get_blocks()))                            # (get_blocks stages through the work vectors: behind the check)
        S, n = s.get_sum()
        want = MR.weighted_sum(terms, S.shape)
        assert n == 2 and S.dtype == np.complex128 and same_typed_bits(S, want)
        assert np.abs(S).max() > 0
        assert s.clear_sum() == 0
        S, n = s.get_sum()
        assert n == 0 and not S.any()
        assert s.add_to_sum(W2) == 0                                     # and it sums again from zero
        assert same_typed_bits(s.get_sum()[0], MR.weighted_sum(terms[1:], S.shape))
        assert s.keep_sum(True) == 0 and s.get_sum()[1] == 0 and not s.get_sum()[0].any()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_sum_on_a_padded_and_on_a_preconditioned_plan(prec):
    pr = _padded_problem()
    with T.Solver.open(pr, prec, allow_padding=True, keep_sum=True).load() as s:                # the caller's compact shape
        terms = []
        for w, its in ((W1, 2), (W2, 3)):
            assert s.solve(1e-30, its) == MAX_ITERATIONS
            s.add_to_sum(w)
            terms.append((w, s.get_blocks()))
        S, n = s.get_sum()
        assert n == 2 and S.shape == (pr.nnzbB, 9, 9) and same_typed_bits(S, MR.weighted_sum(terms, S.shape)) and np.abs(S).max() > 0
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_sum=True).load() as s:                 # the back-transformed X, as get_blocks returns it
        assert s.solve(1e-30, 3) == MAX_ITERATIONS
        s.add_to_sum(W1)
        S, n = s.get_sum()
        assert n == 1 and same_typed_bits(S, MR.weighted_sum([(W1, s.get_blocks())], S.shape))
    with T.Solver.open(pr, prec).load() as s:                                         # keepSum is off: refused, as pushStart without a depth
        assert T.decode(T.lib.tfqmrgpuExt_addToSum(s.handle, s.plan, 1.0, 0.0))[::2] == (UNDOCUMENTED, ord("X"))


# ---- 3. mesh ----------------------------------------------------------------------------------------------------------------------------
NE = 4
SIGMAS = [e * SIGMA for e in range(NE)]
WEIGHTS = [0.5 + 0.25j, -0.25 + 1j, 1.5 - 0.75j, 0.125 + 2j]


def _loop(q, sigmas, weights, threshold, max_iterations, from_x):
    """solve_mesh written with the public calls"""
    its, res, sts = [], [], []
    for e, sigma in enumerate(sigmas):
        q.shift_diagonal(sigma)
        if e == 0 and not from_x:
            st = q.solve(threshold, max_iterations)
        else:
            if q.start_count() > 0:
                q.project_start()
            st = q.refine_from(threshold, max_iterations)
        info = q.get_info()
        its.append(info["iterations"]), res.append(info["residual"]), sts.append(st)
        if st not in (0, MAX_ITERATIONS):
            break
        if q.start_depth() > 0:
            q.push_start()
        if weights is not None:
            q.add_to_sum(weights[e])
    return np.array(its, np.int32), np.array(res, np.float64), np.array(sts, np.int32)


@pytest.mark.parametrize("from_x", [0, 1])
@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("prec", ["z", "m"])
@pytest.mark.parametrize("name", ["fd_16x16_small", "fd_4x4_2d"])
def test_mesh_is_the_loop_of_the_public_calls(name, prec, depth, from_x):
    pr = load_problem(name)
    with T.Solver.open(pr, prec, keep_starts=depth or None, keep_sum=True).load() as p, T.Solver.open(pr, prec, keep_starts=depth or None, keep_sum=True).load() as q:
        if from_x:                                                       # an X to start from: the same on both
            _solved(p, 2), _solved(q, 2)
        out = p.solve_mesh(SIGMAS, WEIGHTS, 1e-30, 3, from_x=from_x)
        its, res, sts = _loop(q, SIGMAS, WEIGHTS, 1e-30, 3, from_x)
        assert out["status"] == MAX_ITERATIONS and out["n_done"] == NE and np.all(out["statuses"] == MAX_ITERATIONS)
        assert np.array_equal(out["statuses"], sts) and np.array_equal(out["iterations"], its) and same_typed_bits(out["residual"], res)
        assert same_typed_bits(p.get_matrix(), q.get_matrix())
        (sp, np_), (sq, nq) = p.get_sum(), q.get_sum()
        assert np_ == nq == NE and same_typed_bits(sp, sq) and np.abs(sp).max() > 0
        assert p.start_count() == q.start_count() == min(depth, NE)
        assert same_typed_bits(p.bound_history(), q.bound_history())


def test_mesh_converges_on_a_preconditioned_plan():
    """the fixture's own threshold, block-Jacobi with a kept A, two kept starts: every energy returns SUCCESS and the last X solves the
    last system to `threshold` -- residual() reads the caller's A, the kept copy"""
    pr = load_problem("fd_16x16_small")
    thr = pr.tolerance
    with T.Solver.open(pr, "z", preconditioner=BJ, keep_operator=True, keep_starts=2, keep_sum=True).load() as p, T.Solver.open(pr, "z", preconditioner=BJ, keep_operator=True, keep_starts=2, keep_sum=True).load() as q:
        out = p.solve_mesh(SIGMAS, WEIGHTS, thr, 500)
        its, res, sts = _loop(q, SIGMAS, WEIGHTS, thr, 500, 0)
        print("mesh, fd_16x16_small z block-Jacobi depth 2: iterations %s, residual %s" % (list(out["iterations"]), list(out["residual"])))
        assert out["status"] == 0 and out["n_done"] == NE and np.all(out["statuses"] == 0)
        assert np.array_equal(out["iterations"], its) and same_typed_bits(out["residual"], res) and np.all(out["residual"] <= thr)
        worst = p.residual()["worst"]
        print("mesh: residual()['worst'] of the last energy %.3e, threshold %.1e" % (worst, thr))
        assert worst <= thr
        assert same_typed_bits(p.get_matrix(), q.get_matrix()) and same_typed_bits(p.get_sum()[0], q.get_sum()[0])


def _raw_mesh(p, threshold, max_iterations):
    done = C.c_int32(-1)
    sg = np.ascontiguousarray(np.array(SIGMAS, np.complex128)).view(np.float64)
    wt = np.ascontiguousarray(np.array(WEIGHTS, np.complex128)).view(np.float64)
    its, res, sts = np.full(NE, -7, np.int32), np.full(NE, -7.0), np.full(NE, -7, np.int32)
    got = T.lib.tfqmrgpuExt_solveMesh(p.handle, p.plan, NE, T._ptr(sg), T._ptr(wt), threshold, max_iterations, 0, T._ptr(its), T._ptr(res),
                                      T._ptr(sts), C.byref(done))
    return got, done.value, its, res, sts


def test_mesh_stops_at_the_first_energy_that_fails():
    """A = 0 and sigma_0 = 0: v3.(A v6) = 0 for every right-hand side, the solve of the first energy returns BREAKDOWN
    (tests/test_gpu_parity.py).  The mesh leaves at e = 0 with the status and the X that solve gives on a twin plan; nothing of the later
    energies is written, and steps 4 and 5 of that energy do not run"""
    pr = load_problem("fd_16x16_small")
    pr.A[:] = 0
    with T.Solver.open(pr, "z", keep_starts=2, keep_sum=True).load() as p, T.Solver.open(pr, "z").load() as q:
        want = T.lib.tfqmrgpu_bsrsv_solve(q.handle, q.plan, 1e-9, 50)
        assert want == BREAKDOWN
        got, done, its, res, sts = _raw_mesh(p, 1e-9, 50)
        assert got == want and done == 1 and sts[0] == want and np.all(sts[1:] == -7) and np.all(its[1:] == -7) and np.all(res[1:] == -7.0)
        info = q.get_info()
        assert its[0] == info["iterations"] and same_typed_bits(res[:1], np.array([info["residual"]]))
        assert same_typed_bits(p.get_matrix(), q.get_matrix())
        assert p.start_count() == 0 and p.get_sum()[1] == 0


@pytest.mark.parametrize("prec", ["z", "m"])
def test_mesh_with_an_entry_of_b_that_is_not_finite(prec):
    """B with one NaN.  Measured on an MI355X: solve gives up that right-hand side alone and returns SUCCESS ('z' and 'm'), so the first
    energy is no failure and the stopping rule lets the mesh run on.  Whichever status solve returns, the mesh is the loop of the public
    calls, which leaves behind the first status that is neither SUCCESS nor MAX_ITERATIONS: the first energy has the status and the X
    that solve gives for that B on a twin plan, and everything behind it has the twin's bits, the NaNs included"""
    pr = load_problem("fd_16x16_small")
    pr.B[0, 1, 2] = np.nan
    with T.Solver.open(pr, prec, keep_sum=True).load() as p, T.Solver.open(pr, prec, keep_sum=True).load() as q, T.Solver.open(pr, prec).load() as cold:
        want = T.lib.tfqmrgpu_bsrsv_solve(cold.handle, cold.plan, 1e-9, 50)
        got, done, its, res, sts = _raw_mesh(p, 1e-9, 50)
        its_q, res_q, sts_q = _loop(q, SIGMAS, WEIGHTS, 1e-9, 50, 0)
        print("NaN in B, %s: solve returns %d; the mesh returns %d after %d energies, statuses %s" % (prec, want, got, done, list(sts[:done])))
        assert sts[0] == want and its[0] == cold.get_info()["iterations"]
        assert done == len(sts_q) and np.array_equal(sts[:done], sts_q) and np.array_equal(its[:done], its_q) and same_typed_bits(res[:done], res_q)
        if want not in (0, MAX_ITERATIONS):
            assert got == want and done == 1 and same_typed_bits(p.get_matrix(), cold.get_matrix())
        assert same_typed_bits(p.get_matrix(), q.get_matrix()) and same_typed_bits(p.get_sum()[0], q.get_sum()[0]) and p.get_sum()[1] == q.get_sum()[1]
