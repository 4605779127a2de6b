"""tfqmrgpuExt_carry (include/tfqmrgpu_ext.h section 15) on the GPU: an operand of one plan into another, device to device, through a
block map.  Everything is a copy (or one rounding), so every comparison is bit for bit: against numpy's indexing of what the source
plan returns, and against a twin plan that was loaded from the host."""
import numpy as np
import pytest

import tfqmrgpu_amd as T
from conftest import load_problem
from helpers import same_typed_bits, with_a
from tfqmrgpu_amd import problems as PR

pytestmark = pytest.mark.gpu

POINTER_INVALID, MAX_ITERATIONS, UNDOCUMENTED, NO_IMPLEMENTATION = 7, 9, 14, 19
BJ = T.PRECOND_BLOCK_JACOBI
# plain element order (4 x 4, 8 x 32 z, 4 x 8), pairs (16 x 16 z, 8 x 8 z), quads (16 x 16 c, 8 x 8 c, 8 x 32 c), LM != LN
FIXTURES = ["fd_4x4_2d", "fd_16x16_small", "fd_8x8_3d", "stencil_8x32", "dense_random_rect"]
REAL = {"z": np.float64, "m": np.float64, "c": np.float32}


def _with_x(pr, rowPtrX, colIndX):
    return T.Problem(pr.rowPtrA, pr.colIndA, pr.A, rowPtrX, colIndX, pr.rowPtrB, pr.colIndB, pr.B, None, pr.tolerance, pr.index_offset)


def _raw_x(s):
    """X as the plan stores it and getMatrix returns it: real [nnzbX, LM * LN * 2], the plan's storage type"""
    x = s.get_matrix(raw=True)
    assert x.dtype == REAL[s.precision]
    return x


def _mapped(x, old, dtype):
    """numpy's side of the map: block n := block old[n], zeros at -1, converted once"""
    old = np.asarray(old)
    want = np.zeros((len(old), x.shape[1]), dtype=dtype)
    want[old >= 0] = x[old[old >= 0]].astype(dtype)
    return want


def _droppable(s, pr):
    """every other block of X that carries no block of B (shrink_pattern refuses those)"""
    has_b = np.zeros(pr.nnzbX, bool)
    has_b[s.plan_view()["subset"]] = True
    return np.flatnonzero(~has_b)[::2]


def _carried_x(src, pattern, old, prec):
    """a fresh plan of `pattern` in precision `prec`, its X filled with ones, then carried into from src: what it returns"""
    with T.Solver.open(pattern, prec) as d:
        d.set_matrix("X", np.ones((pattern.nnzbX, pattern.LM, pattern.LN), dtype=complex))       # the zero blocks must be WRITTEN
        assert d.carry_from(src, "X", old) == 0
        return _raw_x(d)


def _patterns(src, pr):
    """[(what, problem with that pattern of X, oldBlock)]: grown by every leak position, shrunk by every other droppable block, the same
    pattern under a random map with repeats, and under a map of -1 alone"""
    out = []
    rp, ci, old = src.grow_pattern(None)
    out.append(("grown", _with_x(pr, rp, ci), old))
    drop = _droppable(src, pr)
    if len(drop):
        rp, ci, old = src.shrink_pattern(drop)
        assert len(old) == pr.nnzbX - len(drop)
        out.append(("shrunk", _with_x(pr, rp, ci), old))
    rng = np.random.RandomState(pr.nnzbX)
    out.append(("repeats", pr, rng.randint(0, pr.nnzbX, pr.nnzbX).astype(np.int32)))
    out.append(("zeros", pr, np.full(pr.nnzbX, -1, np.int32)))
    return out


# ---- 1. X, same precision: bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [(n, p) for n in FIXTURES for p in "zc"] + [("fd_16x16_small", "m"), ("fd_4x4_2d", "m")])
def test_x_same_precision_bit_for_bit(name, prec):
    pr = load_problem(name)
    with T.Solver.open(pr, prec).load() as src:
        src.solve(1e-30, 3)
        xs = _raw_x(src)
        assert np.abs(xs).max() > 0
        for what, pattern, old in _patterns(src, pr):
            got = _carried_x(src, pattern, old, prec)
            assert same_typed_bits(got, _mapped(xs, old, REAL[prec])), (name, prec, what)
        # no list: the identity, through the internal orders of both plans
        with T.Solver.open(pr, prec) as d:
            assert d.carry_from(src, "X") == 0
            assert same_typed_bits(_raw_x(d), xs)


# ---- 2. X across precisions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ps,pd", [("c", "z"), ("z", "c"), ("m", "z"), ("z", "m"), ("c", "m"), ("m", "c")])
@pytest.mark.parametrize("name", ["fd_16x16_small", "fd_8x8_3d", "fd_4x4_2d"])
def test_x_across_precisions(name, ps, pd):
    """float -> double is exact, double -> float rounds to nearest once (numpy's astype); 'm' stores X in double, as 'z' does.  The element
    order inside a block changes with the precision (16 x 16: quads in float, pairs in double)"""
    pr = load_problem(name)
    with T.Solver.open(pr, ps).load() as src:
        src.solve(1e-30, 3)
        xs = _raw_x(src)
        for what, pattern, old in _patterns(src, pr)[:2]:
            got = _carried_x(src, pattern, old, pd)
            assert same_typed_bits(got, _mapped(xs, old, REAL[pd])), (name, ps, pd, what)


# ---- 3. A and B ------------------------------------------------------------------------------------------------------------------------------
def _solve_record(s, pr, maxit=9):
    st = s.solve(pr.tolerance, maxit)
    info = s.get_info()
    del info["flops_all"]                                       # (the sum over all solves of the plan: not a property of this one)
    out = dict(status=st, X=_raw_x(s), bounds=s.bound_history(), info=info)
    if s.precision == "m":
        out["refinement"], out["cycles"] = s.refinement_history(with_iterations=True)
    else:
        out.update({"v%d" % w: s.get_work_vector(w) for w in (4, 5, 6, 7, 8, 9)})
    return out


def _same_record(got, want):
    assert got.keys() == want.keys()
    for k in want:
        if k in ("status", "info"):
            assert got[k] == want[k], k
        else:
            assert same_typed_bits(got[k], want[k]), k
    assert len(want["bounds"]) >= 1


@pytest.mark.parametrize("name,ps,pd", [("fd_16x16_small", "z", "z"), ("fd_16x16_small", "c", "c"), ("fd_16x16_small", "m", "m"),
                                        ("fd_16x16_small", "z", "m"), ("fd_16x16_small", "c", "z"), ("fd_8x8_3d", "z", "c"),
                                        ("dense_random_rect", "z", "z"), ("stencil_8x32", "c", "c")])
def test_a_and_b_solve_as_a_twin_loaded_from_the_host(name, ps, pd):
    """dst takes A and B from src; its twin takes the values src stores (rounded to float where src is 'c') through set_matrix.  z -> m
    writes both copies of A: the float one drives the inner solves, the double one the refinement history"""
    pr = load_problem(name)
    stored = (lambda a: a.astype(np.complex64).astype(np.complex128)) if ps == "c" else (lambda a: a)
    with T.Solver.open(pr, ps).load() as src, T.Solver.open(pr, pd) as dst, T.Solver.open(pr, pd) as twin:
        assert dst.carry_from(src, "A") == 0
        assert dst.carry_from(src, "B") == 0
        twin.set_matrix("A", stored(pr.A))
        twin.set_matrix("B", stored(pr.B))
        _same_record(_solve_record(dst, pr), _solve_record(twin, pr))


# ---- 4. the source A on a preconditioned plan ----------------------------------------------------------------------------------------------------
def _patched(pr):
    rows = np.repeat(np.arange(pr.mb), np.diff(pr.rowPtrA))
    diag = np.flatnonzero(rows == np.asarray(pr.colIndA, dtype=np.int64) - pr.index_offset).astype(np.int32)
    A1 = pr.A.copy()
    A1[diag] += 0.3 * np.eye(pr.LM) * (1 + 0.5j)
    return diag, A1


@pytest.mark.parametrize("prec", ["z", "m"])
def test_source_a_of_a_preconditioned_plan_that_keeps_it(prec):
    """src has solved with the block-Jacobi preconditioner (its buffer holds A M^-1) and has a patch of set_blocks('A') that no set-up
    has seen: the carried A is the caller's patched A"""
    pr = load_problem("fd_16x16_small")
    diag, A1 = _patched(pr)
    with T.Solver.open(pr, prec, preconditioner=BJ, keep_operator=True).load() as src, T.Solver.open(pr, prec) as dst, T.Solver.open(with_a(pr, A1), prec).load() as twin:
        assert src.solve(pr.tolerance, 200) in (0, MAX_ITERATIONS)
        assert src.set_blocks("A", diag, A1[diag]) == 0
        assert dst.carry_from(src, "A") == 0
        assert dst.carry_from(src, "B") == 0
        _same_record(_solve_record(dst, pr), _solve_record(twin, pr))


def test_source_a_scaled_and_not_kept_is_refused():
    pr = load_problem("fd_16x16_small")
    with T.Solver.open(pr, "z", preconditioner=BJ).load() as src, T.Solver.open(pr, "z").load() as dst:
        assert src.solve(pr.tolerance, 200) == 0
        want = _solve_record(dst, pr)
        before = (dst.get_info(), src.get_info())
        status = T.lib.tfqmrgpuExt_carry(dst.handle, dst.plan, src.plan, b"A", pr.nnzbA, None)
        assert T.decode(status)[::2] == (NO_IMPLEMENTATION, 0)
        assert (dst.get_info(), src.get_info()) == before and same_typed_bits(_raw_x(dst), want["X"])
        _same_record(_solve_record(dst, pr), want)              # dst still holds its A
        # B and X need no A of src
        assert dst.carry_from(src, "B") == 0 and dst.carry_from(src, "X") == 0
        assert same_typed_bits(_raw_x(dst), _raw_x(src))
    # A never set whole on src: key character 'A'; a user-defined operator on src: refused before that
    with T.Solver.open(pr, "z") as src, T.Solver.open(pr, "z").load() as dst:
        raw = lambda: T.decode(T.lib.tfqmrgpuExt_carry(dst.handle, dst.plan, src.plan, b"A", pr.nnzbA, None))[::2]      # noqa: E731
        assert raw() == (UNDOCUMENTED, ord("A"))
        src.set_operator(lambda *a: 0.0)
        assert raw() == (NO_IMPLEMENTATION, 0)
        src.set_operator(None)
        assert dst.solve(pr.tolerance, 9) in (0, MAX_ITERATIONS)


def test_preconditioned_destination_sets_up_again():
    """a carried A makes M^-1 stale, as set_matrix('A') does: the next solve inverts the new diagonal blocks"""
    pr = load_problem("fd_16x16_small")
    _, A1 = _patched(pr)

    def record(s):
        out = _solve_record(s, pr)
        out["Minv"], n_identity = s.get_preconditioner()
        out["info"] = dict(out["info"], n_identity=n_identity)
        return out
    with T.Solver.open(with_a(pr, A1), "z").load() as src, T.Solver.open(pr, "z", preconditioner=BJ).load() as dst, T.Solver.open(with_a(pr, A1), "z", preconditioner=BJ).load() as twin:
        first = record(dst)
        assert dst.carry_from(src, "A") == 0
        got, want = record(dst), record(twin)
        _same_record(got, want)
        assert not same_typed_bits(got["Minv"], first["Minv"])


# ---- 5. the loop end to end, with no host values ----------------------------------------------------------------------------------------------------
def _chain():
    """the 1-D chain of tests/test_gpu_solve_from.py::test_grown_pattern_end_to_end"""
    mb, LM, LN = 4, 4, 4
    rpA, ciA = [0], []
    for r in range(mb):
        ciA += [c for c in (r - 1, r, r + 1) if 0 <= c < mb]
        rpA.append(len(ciA))
    A = (PR.hashed_uniform(1, (len(ciA), LM, LM)) + 1j * PR.hashed_uniform(2, (len(ciA), LM, LM))) / (3 * LM)
    for q, (r, c) in enumerate(zip(np.repeat(np.arange(mb), np.diff(rpA)), ciA)):
        if r == c:
            A[q] += 2.0 * np.eye(LM)
    B = PR.hashed_uniform(3, (1, LM, LN)) + 1j * PR.hashed_uniform(4, (1, LM, LN))
    return T.Problem(rpA, ciA, A, [0, 1, 2, 3, 3], [0, 0, 0], [0, 0, 1, 1, 1], [0], B)


def test_the_loop_end_to_end_without_host_values():
    pr = _chain()
    with T.Solver.open(pr, "z").load() as src:
        assert src.solve(1e-9, 200) == 0
        pr.X = src.get_matrix()
        grown = src.grow_problem(pr, [0])
        rp, ci, old = src.grow_pattern([0])
        assert grown.nnzbX == 4 and list(old) == [0, 1, 2, -1]
        # the host route of the existing test
        with T.Solver.open(grown, "z").load() as host:
            host.set_matrix("X", grown.X)
            assert host.solve_from(1e-9, 200) == 0
            want = dict(X=_raw_x(host), info=host.get_info(), bounds=host.bound_history(), residual2=host.residual()["residual2"])
        # the device route: no values cross the bus
        with T.Solver.open(grown, "z") as dev:
            assert dev.adopt(src, old) == 0
            assert dev.solve_from(1e-9, 200) == 0
            assert same_typed_bits(_raw_x(dev), want["X"]) and dev.get_info() == want["info"] and same_typed_bits(dev.bound_history(), want["bounds"])
            assert same_typed_bits(dev.residual()["residual2"], want["residual2"])
            assert np.all(dev.truncation_leak()["leak2"] == 0.0)
            assert dev.residual()["worst"] <= 1.01e-9


# ---- 6. nothing else moves ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("fd_16x16_small", "z"), ("fd_8x8_3d", "c")])
def test_nothing_else_moves(name, prec):
    pr = load_problem(name)
    with T.Solver.open(pr, prec).load() as src, T.Solver.open(pr, prec).load() as bystander, T.Solver.open(pr, prec) as dst:
        cold = _solve_record(src, pr)
        rp, ci, old = src.grow_pattern(None)
        with T.Solver.open(_with_x(pr, rp, ci), prec) as grown:
            assert grown.adopt(src, old) == 0
            first = _raw_x(grown)
            assert grown.carry_from(src, "X", old) == 0          # two carries: the same bits
            assert same_typed_bits(_raw_x(grown), first)
        assert dst.adopt(src) == 0
        # src is as the solve left it: X and the work vectors, and its next cold solve is the one before
        assert same_typed_bits(_raw_x(src), cold["X"])
        for w in (4, 5, 6, 7, 8, 9):
            assert same_typed_bits(src.get_work_vector(w), cold["v%d" % w]), w
        _same_record(_solve_record(src, pr), cold)
        # a plan that never made or served the call solves the same bits, and so does the one that was carried into
        _same_record(_solve_record(bystander, pr), cold)
        _same_record(_solve_record(dst, pr), cold)
