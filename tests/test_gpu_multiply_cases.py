"""The stand-alone multiply (tfqmrgpuExt_multiply) on the further shapes and the precision `m` of the reference's `bench multi`
(bench_tfqmrgpu.cu:520-547): 6 x 6, 12 x 12, 24 x 24, 48 x 48, 96 x 96 and 128 x 128 in `c` and `z`, and `m` -- float data, sums in
double, one rounding to float (gemmNxNf<float, ..., double>) -- on all 21 shapes.  Bounds: tests/multiply_cases.py, derived a
priori.  Also the two drivers' `multi` mode in these cases."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import multiply_cases as MC
import tfqmrgpu_amd as T
from conftest import GOLDEN, ROOT
from helpers import torch_cuda  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

PLAN = os.path.join(GOLDEN, "plan_unordered.14-287-16.gz")
BENCH = os.path.join(ROOT, "tfqmrgpu_amd", "lib", "bench_tfqmrgpu")


def _run(torch, s, prec, LM, LN, starts, pairs, dA, dX, nY, fill, order=None):
    dS, dP = torch.from_numpy(starts.view(np.int32)).cuda(), torch.from_numpy(pairs.view(np.int32)).cuda()
    dY = torch.full((nY, 2, LM, LN), fill, dtype=dA.dtype, device="cuda")
    if order is None:
        st = T.lib.tfqmrgpuExt_multiply(s.handle, prec.encode(), LM, LN, nY, dS.data_ptr(), dP.data_ptr(), dA.data_ptr(), dX.data_ptr(), dY.data_ptr())
    else:
        st = T.lib.tfqmrgpuExt_multiplyOrdered(s.handle, prec.encode(), LM, LN, nY, dS.data_ptr(), dP.data_ptr(), dA.data_ptr(), dX.data_ptr(),
                                               dY.data_ptr(), order)
    assert st == 0, T.decode(st)
    torch.cuda.synchronize()
    return dY.cpu().numpy()


def _orders_agree(torch, s, prec, LM, LN, starts, pairs, dA, dX, nY, got):
    """every prepared order (modes 1-4) gives the bits of the caller's order; an order exactly for multiples of 16"""
    dS, dP = torch.from_numpy(starts.view(np.int32)).cuda(), torch.from_numpy(pairs.view(np.int32)).cuda()
    for mode in (1, 2, 3, 4):
        order = C.c_void_p(None)
        assert T.lib.tfqmrgpuExt_multiplyPrepare(s.handle, prec.encode(), LM, LN, nY, dS.data_ptr(), dP.data_ptr(), mode, C.byref(order)) == 0
        assert bool(order.value) == (LM % 16 == 0 and LN % 16 == 0), (LM, LN, prec, mode)
        again = _run(torch, s, prec, LM, LN, starts, pairs, dA, dX, nY, 5.0, order)
        assert T.lib.tfqmrgpuExt_multiplyRelease(order) == 0
        assert np.array_equal(again, got), (LM, LN, prec, mode)


@pytest.mark.parametrize("prec", ["c", "z"])
@pytest.mark.parametrize("shape", MC.PAD_SHAPES + MC.WIDE_SHAPES)
def test_new_shapes_within_bound(torch_cuda, oracle, prec, shape):
    torch = torch_cuda
    LM, LN = shape
    real = np.float64 if prec == "z" else np.float32
    starts, pairs, A, X = MC.case(LM, LN, real)
    nY = len(starts) - 1
    Y64, env, n = MC.reference(oracle, LM, LN, starts, pairs, A, X)
    bound = MC.bound_cz(prec, env, n)
    dA, dX = torch.from_numpy(A).cuda(), torch.from_numpy(X).cuda()
    with T.Solver() as s:
        got = _run(torch, s, prec, LM, LN, starts, pairs, dA, dX, nY, 7.0)        # (7: a sentinel in every element of Y)
        _orders_agree(torch, s, prec, LM, LN, starts, pairs, dA, dX, nY, got)
    err = np.abs(got.astype(np.float64) - Y64)
    print("%d x %d %s: max |Y - Y64| %.3e, max of |Y - Y64| / bound %.3f" % (LM, LN, prec, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound), (shape, prec, err.max())


@pytest.mark.parametrize("shape", MC.ALL_SHAPES)
def test_m_sums_in_double(torch_cuda, oracle, shape):
    torch = torch_cuda
    LM, LN = shape
    starts, pairs, A, X = MC.case(LM, LN, np.float32)
    nY = len(starts) - 1
    Y64, env, n = MC.reference(oracle, LM, LN, starts, pairs, A, X)
    bound = MC.bound_m(Y64, env, n)
    dA, dX = torch.from_numpy(A).cuda(), torch.from_numpy(X).cuda()
    with T.Solver() as s:
        got = _run(torch, s, "m", LM, LN, starts, pairs, dA, dX, nY, 7.0)
        assert got.dtype == np.float32
        assert np.array_equal(_run(torch, s, "m", LM, LN, starts, pairs, dA, dX, nY, 3.0), got), "two calls, other bits"
        _orders_agree(torch, s, "m", LM, LN, starts, pairs, dA, dX, nY, got)
    err = np.abs(got.astype(np.float64) - Y64)
    print("%d x %d m: max |Y - Y64| %.3e, elements outside the bound %d" % (LM, LN, err.max(), int((err > bound).sum())))
    assert np.all(err <= bound), (shape, err.max())


def _plan_file():
    with gzip.open(PLAN, "rt") as f:           # "#nnzb_for_Y_A_X= nY nA nX", then iY iA iX beta; a group = run of equal iY
        head = f.readline().split()
        rows = np.loadtxt(f, dtype=np.int64)
    nY, nA, nX = int(head[1]), int(head[2]), int(head[3])
    starts = np.concatenate([[0], np.flatnonzero(np.diff(rows[:, 0])) + 1, [len(rows)]]).astype(np.uint32)
    assert len(starts) == nY + 1
    return nY, nA, nX, starts, np.ascontiguousarray(rows[:, 1:3].reshape(-1).astype(np.uint32))


def test_m_reference_plan_file(torch_cuda, oracle):
    """16 x 16 `m` with the reference's cos/sin fill (bench_tfqmrgpu.cu:274-287): |Y| < 32, so half an ulp of float is 9.537e-7 and the double
    sums add less than 1e-11; float sums miss by 2.5e-5"""
    torch = torch_cuda
    nY, nA, nX, starts, pairs = _plan_file()
    LM = LN = 16

    def fill(nb):
        arg = np.arange(nb * LM * LN, dtype=np.float64).reshape(nb, LM, LN)
        return np.stack([np.cos(arg), np.sin(arg)], axis=1).astype(np.float32)
    A, X = fill(nA), fill(nX)
    Y64 = MC.oracle_y(oracle, "z", LM, LN, starts, pairs, A.astype(np.float64), X.astype(np.float64))
    dA, dX = torch.from_numpy(A).cuda(), torch.from_numpy(X).cuda()
    with T.Solver() as s:
        got = _run(torch, s, "m", LM, LN, starts, pairs, dA, dX, nY, 0.0)
    dev = np.abs(got.astype(np.float64) - Y64).max()
    print("plan file 16 x 16 m: max |Y - Y64| = %.4e (max |Y64| %.2f)" % (dev, np.abs(Y64).max()))
    assert dev <= 9.6e-7, dev


def _maxdev(out):
    m = re.search(r"^# GPU maxdev (\S+)$", out, re.M)
    assert m, out[-2000:]
    return float(m.group(1))


def _bench(args, timeout):
    r = subprocess.run([BENCH, "multi", PLAN] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-1500:])
    return r


def test_driver_multi_m():
    r = _bench(["m", 3, 2], 600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _maxdev(r.stdout) <= 9.6e-7
    assert re.search(r"^# GPU performed \S+ Tflop in", r.stdout, re.M) and re.search(r"Gflop/sec$", r.stdout, re.M), r.stdout
    assert re.search(r"^# MI355X roofline: .* of the 78\.6 Tflop/s matrix peak", r.stdout, re.M), r.stdout


@pytest.mark.parametrize("L", [6, 12, 24, 48, 96, 128])
def test_driver_multi_z_new_shapes(L):
    r = _bench(["z", 1, 1, L], 900)            # (the host check at 128 is 8.5e11 flops in double)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _maxdev(r.stdout) <= 1e-4


@pytest.mark.parametrize("prec,L", [("m", 16), ("z", 6)])
def test_python_driver_prints_the_compiled_maxdev(prec, L):
    line = re.compile(r"^# GPU maxdev .*$", re.M)
    c = _bench([prec, 1, 1, L], 600)
    assert c.returncode == 0, c.stderr[-2000:]
    p = subprocess.run([sys.executable, "-m", "tfqmrgpu_amd.bench_tfqmrgpu", "multi", PLAN, prec, "1", "1", str(L)], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    print(p.stdout[-1500:])
    assert p.returncode == 0, p.stderr[-2000:]
    assert line.search(p.stdout).group(0) == line.search(c.stdout).group(0)
