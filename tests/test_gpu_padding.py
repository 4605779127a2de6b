"""Padded plans (include/tfqmrgpu_ext.h section 18) on the GPU, through the C-ABI.  The yardstick throughout is a SECOND plan of the plan's
shape that is fed the padded problem (tests/pad_ref.py: pad_problem) through the calls that existed before.  The buffers of the two plans
then hold the same bytes by construction, the same launches run on them, and every comparison is exact (np.array_equal), not a tolerance.
Only the last section compares with the truth: the residual of the caller's system and the dense solution of it.
Needs an MI355X (`pytest -m gpu`)."""
import numpy as np
import pytest

import pad_ref as PD
import tfqmrgpu_amd as T
from helpers import exact_random_blocks, real_dtype, run_ranks, torch_cuda  # noqa: F401  (torch_cuda: a fixture)
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

LAYOUTS = (T.LAYOUT_RIRIRIRI, T.LAYOUT_RRRRIIII, T.LAYOUT_RRIIRRII)
TRANS = "nt*c"
TRANSFER_SHAPES = [(3, 3), (4, 6), (5, 7), (9, 10), (17, 20), (25, 25), (33, 40), (16, 1)]
SOLVE_SHAPES = [(5, 5), (9, 9), (25, 25), (16, 1)]
# (plan precision, precision of the caller's data): an 'm' plan takes both
PRECISIONS = [("z", "z"), ("c", "c"), ("m", "z"), ("m", "c")]
TOL = {"z": 1e-9, "c": 1e-4, "m": 1e-9}
MAXIT = 300
NO_IMPLEMENTATION = 19
BJ = T.PRECOND_BLOCK_JACOBI


def _problem(lm, ln, radius=None):
    return PR.stencil_2d(4, 3, lm, ln, 3, seed=100 * lm + ln, radius=radius)


def _user(blocks, layout, trans, data, pad=None, unit=None):
    """what a caller hands over for complex blocks [n, r, c] in that layout and transposition.  pad = (R, C): the
    blocks are first padded to R x C -- the yardstick's input: zeros around, 1 on the padded diagonal of the blocks that `unit` flags.  A
    conjugating transfer negates the imaginary plane, so the padded zeros of that plane are handed over as -0.0: the yardstick then stores
    +0.0, as the padded plan does, and the two buffers can be compared byte by byte"""
    conj = trans in "*c"
    re, im = blocks.real.copy(), (-blocks.imag if conj else blocks.imag.copy())
    if pad is not None:
        (R, Cn), (n, r, c) = pad, blocks.shape
        re2, im2 = np.zeros((n, R, Cn)), np.full((n, R, Cn), -0.0 if conj else 0.0)
        re2[:, :r, :c], im2[:, :r, :c] = re, im
        if unit is not None:
            for k in range(min(r, c), min(R, Cn)):
                re2[unit, k, k] = 1.0
        re, im = re2, im2
    if trans in "tc":
        re, im = re.transpose(0, 2, 1), im.transpose(0, 2, 1)
    axis = {T.LAYOUT_RIRIRIRI: -1, T.LAYOUT_RRRRIIII: 1, T.LAYOUT_RRIIRRII: 2}[layout]
    return np.ascontiguousarray(np.stack([re, im], axis=axis).reshape(len(blocks), -1), dtype=real_dtype(data))


class Pair:
    """the padded plan `p` of the caller's problem and the yardstick `y`: a plan of the plan's shape without the switch"""

    def __init__(self, pr, prec, data=None, kind=None, keep=False, torch=None, fill=None):
        self.pr, self.prec, self.data = pr, prec, data or ("c" if prec == "c" else "z")
        self.lm, self.ln = pr.LM, pr.LN
        self.LM, self.LN = PD.plan_shape(pr.LM, pr.LN)
        self.unit = PD.diagonal_flags(pr)
        self.p, self.y, self.buffers = T.Solver(), T.Solver(), []
        for s, padded in ((self.p, True), (self.y, False)):
            s.create_plan(pr)
            if padded:
                s.allow_padding(True)
            nbytes = s.buffer_size(*((self.lm, self.ln) if padded else (self.LM, self.LN)), prec)
            s.data_precision = self.data
            if kind is not None:
                s.set_preconditioner(kind)
            if keep:
                s.keep_operator(True)
            if torch is None:
                s.set_buffer(nbytes=nbytes)
            else:                                                    # a buffer of the test's own, pre-filled: it can be looked at
                buf = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
                self.buffers.append(buf)
                s.set_buffer(device_ptr=buf.data_ptr())
        assert self.p.padded_shape() == (self.lm, self.ln, self.LM, self.LN)
        assert self.y.padded_shape() == (self.LM, self.LN, self.LM, self.LN)
        assert len({b.numel() for b in self.buffers}) <= 1            # the buffer of the plan's shape on both

    def set(self, var, blocks):
        self.p.set_matrix(var, blocks)
        self.y.set_matrix(var, PD.pad_blocks(blocks, self.LM, self.LM if var == "A" else self.LN, self.unit if var == "A" else None))

    def set_blocks(self, var, idx, blocks):
        self.p.set_blocks(var, idx, blocks)
        unit = self.unit[np.asarray(idx)] if var == "A" else None
        self.y.set_blocks(var, idx, PD.pad_blocks(blocks, self.LM, self.LM if var == "A" else self.LN, unit))

    def inside(self, blocks):
        return PD.inside(blocks, self.lm, self.ln)

    def same_x(self, what=""):
        """getMatrix of the padded plan is the inside of the yardstick's, whose padding is exactly zero"""
        Xp, Xy = self.p.get_matrix(), self.y.get_matrix()
        assert Xp.shape == (self.pr.nnzbX, self.lm, self.ln) and Xy.shape == (self.pr.nnzbX, self.LM, self.LN)
        assert np.array_equal(Xp, self.inside(Xy)), what
        rest = Xy.copy()
        rest[:, :self.lm, :self.ln] = 0
        assert not rest.any(), what
        return Xp

    def same_work_vectors(self, which=(1,), what=""):
        if self.prec == "m":                                         # (getWorkVector is for 'z' and 'c' plans)
            return
        for k in which:
            vp, vy = self.p.get_work_vector(k), self.y.get_work_vector(k)
            assert vp.shape == (self.pr.nnzbX, self.LM, self.LN)      # the plan's shape on both
            assert np.array_equal(vp, vy, equal_nan=True), (what, k)

    def close(self):
        self.p.close()
        self.y.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _outcome(s, prec, st):
    info = s.get_info()
    out = dict(status=st, iterations=info["iterations"], residual=info["residual"], flops=info["flops"], bounds=s.bound_history())
    if prec == "m":
        out["refinement"], out["cycle_iterations"] = s.refinement_history(with_iterations=True)
    return out


def _both(pair, call, what="", vectors=(1,)):
    """the same solve call on both plans: status, iterations, residual, flop count, bound history and X bit for bit; and the work vectors
    `vectors`, read before getMatrix with a host array stages its blocks in v4 ... v9"""
    sp, sy = call(pair.p), call(pair.y)
    pair.same_work_vectors(vectors, what)
    a, b = _outcome(pair.p, pair.prec, sp), _outcome(pair.y, pair.prec, sy)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])
    X = pair.same_x(what)
    assert np.all(np.isfinite(X)), what                              # (an 'm' refinement from a converged X runs no float solve: no bound history)
    return a, X


def _diagonal(pr):
    return np.flatnonzero(PD.diagonal_flags(pr)).astype(np.int32)


def _patched(pr, seed, data):
    """A with every diagonal block changed, still block diagonally dominant, in values that the caller's precision holds"""
    diag = _diagonal(pr)
    assert len(diag) == pr.mb
    A1 = pr.A.copy()
    A1[diag] += 0.3 * np.eye(pr.LM) + 0.02 * (PR.hashed_uniform(seed, A1[diag].shape) + 1j * PR.hashed_uniform(seed + 1, A1[diag].shape))
    return diag, (A1.astype(np.complex64).astype(np.complex128) if data == "c" else A1)


# ---- 1. transfers, without a solve ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,data", PRECISIONS)
@pytest.mark.parametrize("lm,ln", TRANSFER_SHAPES)
def test_transfers(torch_cuda, lm, ln, prec, data):
    """setMatrix('A' | 'B' | 'X') in every layout and transposition, with device and with host arrays, on two buffers pre-filled with NaN
    bytes.  Device arrays first: they are converted in place, no staging, so after every set the two buffers differ in exactly the bytes
    they differed in after setBuffer (the device pointers of the plan's own copy) -- A, B and X windows are equal byte for byte, 'm' plans'
    float A included, and nothing of the NaN fill is left in a block that was set.  Host arrays are staged in the work vectors, which then
    hold different raw bytes: there the comparison is X by getWorkVector, A by applyOperator on that X, and getMatrix."""
    torch = torch_cuda
    pr = _problem(lm, ln)
    rng = np.random.default_rng(1000 * lm + ln)
    with Pair(pr, prec, data, torch=torch, fill=0xFF) as pair:
        LM, LN, p, y = pair.LM, pair.LN, pair.p, pair.y
        bufP, bufY = pair.buffers
        torch.cuda.synchronize()
        differ0 = bufP != bufY
        assert int(differ0.sum()) <= 1024                            # the plan's device copy of its own pointers (window wSelf)
        real = torch.float64 if data == "z" else torch.float32

        def get_device(s, rows, cols, tr="n", layout=T.LAYOUT_RIRIRIRI):
            out = torch.full((pr.nnzbX * 2 * rows * cols,), 7.0, dtype=real, device="cuda")
            s.get_matrix_device(out.data_ptr(), tr, layout)
            torch.cuda.synchronize()
            return out.cpu().numpy().reshape(pr.nnzbX, -1)

        def as_complex(raw, rows, cols):
            v = raw.reshape(pr.nnzbX, rows, cols, 2).astype(np.float64)
            return v[..., 0] + 1j * v[..., 1]

        for device in (True, False):                                 # (the device pass touches no host array of values: nothing is staged)
            for layout in LAYOUTS:
                for tr in TRANS:
                    what = (lm, ln, prec, data, device, hex(layout), tr)
                    vals = dict(A=exact_random_blocks(rng, pr.nnzbA, lm, lm, data), B=exact_random_blocks(rng, pr.nnzbB, lm, ln, data),
                                X=exact_random_blocks(rng, pr.nnzbX, lm, ln, data))
                    alive = []
                    for var, blocks in vals.items():
                        cols = lm if var == "A" else ln
                        up = _user(blocks, layout, tr, data)
                        uy = _user(blocks, layout, tr, data, pad=(LM, LM if var == "A" else LN), unit=pair.unit if var == "A" else None)
                        assert up.shape == (len(blocks), 2 * lm * cols)
                        if device:
                            dp, dy = torch.from_numpy(up).cuda(), torch.from_numpy(uy).cuda()
                            alive += [dp, dy]
                            p.set_matrix_device(var, dp.data_ptr(), tr, layout)
                            y.set_matrix_device(var, dy.data_ptr(), tr, layout)
                        else:
                            p.set_matrix(var, up, tr, layout)
                            y.set_matrix(var, uy, tr, layout)
                    pair.same_work_vectors((1,), what)               # X as the plans hold it (the getter brings its own staging)
                    if device:
                        torch.cuda.synchronize()
                        assert torch.equal(bufP != bufY, differ0), what
                        assert np.array_equal(get_device(p, lm, ln, tr, layout), _user(vals["X"], layout, tr, data)), what
                    else:
                        assert np.array_equal(pair.same_x(what), vals["X"]), what
                        assert np.array_equal(p.get_matrix(trans=tr, layout=layout, raw=True), _user(vals["X"], layout, tr, data)), what
                    # A: X := A X gives the same bits on both plans, finite everywhere -- no NaN is left in A, and the padding stays 0
                    p.apply_operator()
                    y.apply_operator()
                    pair.same_work_vectors((1,), what)
                    if device:
                        torch.cuda.synchronize()
                        assert torch.equal(bufP != bufY, differ0), what
                        AX, wide = as_complex(get_device(p, lm, ln), lm, ln), as_complex(get_device(y, LM, LN), LM, LN)
                        assert np.array_equal(AX, pair.inside(wide)), what
                        wide[:, :lm, :ln] = 0
                        assert not wide.any(), what
                    else:
                        AX = pair.same_x(what)
                    assert np.all(np.isfinite(AX)) and np.abs(AX).max() > 0, what
        # B, and everything together: two iterations on the caller's A and the last B leave the same bits in every work vector
        pair.set("A", pr.A.astype(np.complex64).astype(np.complex128) if data == "c" else pr.A)
        _both(pair, lambda s: s.solve(1e-30, 2), "two iterations", vectors=(1, 4, 5, 6, 7, 8, 9))


# ---- 2. listed blocks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, BJ])
@pytest.mark.parametrize("prec,data", [("z", "z"), ("c", "c"), ("m", "z")])
@pytest.mark.parametrize("lm,ln", [(5, 7), (9, 10), (25, 25)])
def test_listed_blocks(torch_cuda, lm, ln, prec, data, kind):
    """setBlocks('A') of the diagonal blocks, setBlocks('B' | 'X') of a scattered list, getBlocks with a list that names a block twice and
    with NULL (B's pattern); host and device values; on a preconditioned plan with keepOperator behind its first solve as well"""
    torch = torch_cuda
    pr = _problem(lm, ln, radius=1.6)
    rng = np.random.default_rng(10 * lm + ln)
    with Pair(pr, prec, data, kind=kind, keep=kind is not None) as pair:
        LM, LN, p, y = pair.LM, pair.LN, pair.p, pair.y
        pair.set("A", pr.A)
        pair.set("B", pr.B)
        _both(pair, lambda s: s.solve(TOL[prec], MAXIT), "first solve")
        if kind is not None:
            assert p.get_preconditioner(values=False)[1] == y.get_preconditioner(values=False)[1] == 0
        # A: the diagonal blocks (into the kept copy on the preconditioned plan), then the same solve on both
        diag, A1 = _patched(pr, 31, data)
        pair.set_blocks("A", diag, A1[diag])
        _both(pair, lambda s: s.solve(TOL[prec], MAXIT), "after setBlocks('A')")
        # B and X: a scattered list, out of order; device values for X
        ib = rng.permutation(pr.nnzbB)[:2].astype(np.int32)
        pair.set_blocks("B", ib, exact_random_blocks(rng, len(ib), lm, ln, data))
        ix = rng.permutation(pr.nnzbX)[: pr.nnzbX // 2].astype(np.int32)
        Xnew = exact_random_blocks(rng, len(ix), lm, ln, data)
        before = pair.same_x()
        for layout, tr in ((T.LAYOUT_RRRRIIII, "t"), (T.LAYOUT_RRIIRRII, "c")):
            dp = torch.from_numpy(_user(Xnew, layout, tr, data)).cuda()
            dy = torch.from_numpy(_user(Xnew, layout, tr, data, pad=(LM, LN))).cuda()
            p.set_blocks_device("X", ix, dp.data_ptr(), tr, layout)
            y.set_blocks_device("X", ix, dy.data_ptr(), tr, layout)
            torch.cuda.synchronize()
            after = pair.same_x((layout, tr))
            want = before.copy()
            want[ix] = Xnew
            assert np.array_equal(after, want)                       # the listed blocks and nothing else
            pair.same_work_vectors((1,))
        # getBlocks: a block twice, and B's pattern
        twice = np.concatenate([ix[:3], ix[:1], [0, pr.nnzbX - 1]]).astype(np.int32)
        for layout in LAYOUTS:
            for tr in TRANS:
                got = p.get_blocks(twice, trans=tr, layout=layout, raw=True)
                assert np.array_equal(got, _user(after[twice], layout, tr, data)), (hex(layout), tr)
        assert np.array_equal(p.get_blocks(twice), pair.inside(y.get_blocks(twice)))
        onB = p.get_blocks(None)
        assert onB.shape == (pr.nnzbB, lm, ln) and np.array_equal(onB, pair.inside(y.get_blocks(None)))
        out = torch.full((len(twice) * 2 * lm * ln,), 7.0, dtype=torch.float64 if data == "z" else torch.float32, device="cuda")
        p.get_blocks_device(out.data_ptr(), twice, "t", T.LAYOUT_RRRRIIII)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(len(twice), -1), _user(after[twice], T.LAYOUT_RRRRIIII, "t", data))
        _both(pair, lambda s: s.solve(TOL[prec], MAXIT), "after setBlocks('B')")


# ---- 3. solves, and the loop of sections 10 to 17 --------------------------------------------------------------------------------------
def test_no_diagonal_block_of_the_inputs_is_singular():
    """what nIdentity == 0 below rests on (CPU): every diagonal block of every input is well conditioned, so A_ii (+) 1 is inverted"""
    for lm, ln in SOLVE_SHAPES:
        for radius in (None, 1.6):
            pr = _problem(lm, ln, radius)
            diag = _diagonal(pr)
            assert len(diag) == pr.mb and np.linalg.cond(pr.A[diag]).max() < 10.0


@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("lm,ln", SOLVE_SHAPES)
def test_solve(lm, ln, prec):
    pr = _problem(lm, ln)
    with Pair(pr, prec) as pair:
        pair.set("A", pr.A)
        pair.set("B", pr.B)
        out, X = _both(pair, lambda s: s.solve(TOL[prec], MAXIT), vectors=(1, 4, 5, 6, 7, 8, 9))
        assert out["status"] == 0 and out["iterations"] >= 2
        assert pair.p.multiply_kernel() == pair.y.multiply_kernel()
        if prec != "m":
            x = pair.p.get_work_vector(1)                            # the plan's shape: the padding is exactly 0
            x[:, :lm, :ln] = 0
            assert not x.any()


@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("lm,ln", SOLVE_SHAPES)
def test_preconditioned_solve(lm, ln, prec):
    pr = _problem(lm, ln)
    with Pair(pr, prec, kind=BJ) as pair:
        pair.set("A", pr.A)
        pair.set("B", pr.B)
        Mp, nP = pair.p.get_preconditioner()
        My, nY = pair.y.get_preconditioner()
        assert nP == nY == 0
        assert Mp.shape == (pr.mb, pair.LM, pair.LM) and np.array_equal(Mp, My)      # the plan's shape: A_ii^-1 (+) 1
        assert np.allclose(Mp[:, lm:, lm:], np.eye(pair.LM - lm)) and np.abs(Mp[:, :lm, :lm]).max() > 0
        out, _ = _both(pair, lambda s: s.solve(TOL[prec], MAXIT))
        assert out["status"] == 0
        assert pair.p.get_preconditioner(values=False)[1] == pair.y.get_preconditioner(values=False)[1] == 0


def _same_dict(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("lm,ln", SOLVE_SHAPES)
def test_energy_loop(lm, ln, prec):
    """solve, keep the start, patch the diagonal, warm start; residual, truncation leak, projection of two starts, carry into a second
    padded plan: each call gives on the padded plan what it gives on the yardstick, bit for bit.  The per-right-hand-side arrays have the
    plan's shape [nCols][LN]; the padded right-hand sides are zero columns of B"""
    pr = _problem(lm, ln, radius=1.6)
    data = "c" if prec == "c" else "z"
    with Pair(pr, prec) as pair:
        p, y, LN = pair.p, pair.y, pair.LN
        pair.set("A", pr.A)
        pair.set("B", pr.B)
        _both(pair, lambda s: s.solve(TOL[prec], MAXIT), "solve")
        for s in (p, y):
            s.keep_starts(2)
            s.push_start()
        diag, A1 = _patched(pr, 41, data)
        pair.set_blocks("A", diag, A1[diag])
        _both(pair, lambda s: s.refine_from(TOL[prec], MAXIT), "warm start")
        for s in (p, y):
            s.push_start()
        diag, A2 = _patched(pr, 43, data)
        pair.set_blocks("A", diag, A2[diag])
        rp, ry = p.residual(), y.residual()                          # the old X on the new A
        assert rp["residual2"].shape == (3, LN)
        _same_dict(rp, ry, ("residual2", "bnorm2", "columns", "relative", "worst"), "residual")
        assert not rp["bnorm2"][:, ln:].any() and not rp["residual2"][:, ln:].any() and np.all(rp["bnorm2"][:, :ln] > 0)
        assert np.isfinite(rp["worst"]) and rp["worst"] > 0          # the padded right-hand sides (0 / 0) are left out
        lp, ly = p.truncation_leak(), y.truncation_leak()
        _same_dict(lp, ly, ("leak2", "columns", "n_leak_blocks", "n_leak_pairs", "units"), "truncation leak")
        assert lp["leak2"].shape == (3, LN) and lp["n_leak_blocks"] > 0 and np.all(lp["leak2"][:, :ln] > 0) and not lp["leak2"][:, ln:].any()
        gp, gy = p.project_start(), y.project_start()
        _same_dict(gp, gy, ("coefficients", "n_used"), "projection")
        assert gp["n_used"].shape == (3, LN) and not gp["n_used"][:, ln:].any() and np.all(gp["n_used"][:, :ln] >= 1)
        pair.same_x("projected start")
        _both(pair, lambda s: s.refine_from(TOL[prec], MAXIT), "warm start from the projection")
        # carry into a second pair of plans of the same shapes, and go on there
        with Pair(pr, prec) as second:
            second.p.adopt(p)
            second.y.adopt(y)
            second.same_x("carried X")
            second.same_work_vectors((1,), "carried X")
            _both(second, lambda s: s.refine_from(TOL[prec], MAXIT), "warm start on the second plan")
        # a padded plan of another caller's shape on the same plan shape is refused, as unequal block shapes are
        if (lm, ln) == (5, 5):
            with T.Solver() as other:
                other.create_plan(pr)
                other.allow_padding(True)
                other.set_buffer(nbytes=other.buffer_size(6, 6, prec))
                st = T.lib.tfqmrgpuExt_carry(other.handle, other.plan, p.plan, b"X", pr.nnzbX, None)
                assert T.decode(st)[::2] == (14, ord("L"))


# ---- 4. truth -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm,ln", [(5, 5), (25, 25)])
def test_truth(lm, ln):
    """The padded plan solves the CALLER's system.  residual()'s worst is at or below the solve's threshold -- the comparison of
    tests/test_gpu_residual.py on a plan that is not padded (worst <= threshold, no margin).  X's inside agrees with the dense solution of
    the caller's problem to 1e-8 of its largest element at a threshold of 1e-10: the bound that tests/test_gpu_parity.py holds the solver
    to against the same reference, and tighter than every stencil entry of tests/tolerances.py (3e-7 the smallest), whichever of them is
    read as "the plan's shape".  That the yardstick -- the padded problem solved as a problem of the plan's shape -- meets it on these
    inputs is verified through the CPU oracle in tests/test_padding_cpu.py (test_the_padded_problem_solves_the_callers_system)."""
    pr = _problem(lm, ln)
    tol = 1e-10
    with T.Solver() as s:
        s.create_plan(pr)
        s.allow_padding(True)
        s.set_buffer(nbytes=s.buffer_size(lm, ln, "z"))
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        assert s.solve(tol, MAXIT) == 0
        X, graded, info = s.get_matrix(), s.residual(), s.get_info()
    Xd = PR.dense_reference_solution(pr)
    dev = np.abs(X - Xd).max() / np.abs(Xd).max()
    print("%dx%d: %d iterations, worst residual %.3e (threshold %.0e), deviation from the dense solution %.3e"
          % (lm, ln, info["iterations"], graded["worst"], tol, dev))
    assert graded["worst"] <= tol
    assert dev <= 1e-8
    # one call: the same through solve_problem
    st, X1, info1 = T.solve_problem(pr, "z", threshold=tol, max_iterations=MAXIT, allow_padding=True)
    assert st == 0 and np.array_equal(X1, X) and info1["padded_shape"] == (lm, ln) + PD.plan_shape(lm, ln)


# ---- 5. what is refused, and what does not change ----------------------------------------------------------------------------------------
def test_user_defined_operator_on_a_padded_plan_is_refused():
    pr = _problem(5, 5)
    with T.Solver() as s:
        s.create_plan(pr)
        s.allow_padding(True)
        s.set_buffer(nbytes=s.buffer_size(5, 5, "z"))
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        calls = []
        s.set_operator(lambda *a: calls.append(1) or 0.0)
        st = T.lib.tfqmrgpu_bsrsv_solve(s.handle, s.plan, 1e-9, 50)
        assert T.decode(st)[::2] == (NO_IMPLEMENTATION, 0) and not calls
        s.set_operator(None)                                         # ... and the plan solves again
        assert s.solve(1e-9, MAXIT) == 0


@pytest.mark.parametrize("prec", ["z", "c", "m"])
@pytest.mark.parametrize("LM,LN", [(4, 5), (8, 8), (16, 16), (8, 32)])
def test_a_listed_shape_with_padding_on_is_the_plan_without(LM, LN, prec):
    pr = PR.stencil_2d(4, 3, LM, LN, 3, seed=5, radius=1.6)
    runs = []
    for padding in (False, True):
        with T.Solver() as s:
            s.create_plan(pr)
            if padding:
                s.allow_padding(True)
            nbytes = s.buffer_size(LM, LN, prec)
            assert s.padded_shape() == (LM, LN, LM, LN)
            s.set_buffer(nbytes=nbytes)
            s.set_matrix("A", pr.A)
            s.set_matrix("B", pr.B)
            st = s.solve(TOL[prec], MAXIT)
            out = _outcome(s, prec, st)
            out.update(X=s.get_matrix(), kernel=s.multiply_kernel(), nbytes=nbytes)
            runs.append(out)
    assert runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert runs[0]["status"] == 0


# ---- 6. two ranks on one GPU --------------------------------------------------------------------------------------------------------------
def test_two_ranks_on_a_padded_plan(tmp_path):
    """block columns sharded over 2 ranks that share cuda:0 (3 processes with this one): every rank pads alike, and the gathered X is
    the X of one rank bit for bit"""
    lm, ln, prec, tol = 9, 9, "z", 1e-9
    g = run_ranks(2, "solve", str(tmp_path / "sharded.npz"), "stencil:4:3:%d:%d:3:%d:5" % (lm, ln, 100 * lm + ln), prec, tol, "pad", timeout=300)
    pr = _problem(lm, ln)
    with T.Solver() as s:
        s.create_plan(pr)
        s.allow_padding(True)
        s.set_buffer(nbytes=s.buffer_size(lm, ln, prec))
        s.set_matrix("A", pr.A)
        s.set_matrix("B", pr.B)
        st = s.solve(tol, 300)
        info, X, hist = s.get_info(), s.get_matrix(), s.bound_history()
    assert st == 0 and list(g["status"]) == [0, 0]
    assert [tuple(v) for v in g["shape"]] == [(9, 9, 16, 16)] * 2
    assert list(g["iterations"]) == [info["iterations"]] * 2
    for h in g["history"]:
        assert np.array_equal(h, hist)
    assert np.array_equal(g["X"], X)
