"""Python binding of the MI355X-native libtfQMRgpu.so (C-ABI in include/tfqmrgpu.h).

This is plumbing for tests and bench.py, not a second implementation: every call goes through
ctypes into the HIP library.  There is no CPU fallback -- if the shared library is missing the
import fails loudly (build it with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C tfqmrgpu_amd/csrc``).

The function names and argument order mirror the reference interface
(real-space/tfQMRgpu tfQMRgpu/include/tfqmrgpu.h:16-156) the way its own ctypes example binds it
(example/tfqmrgpu_python_example.py:40-67).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFQMRGPU_LIB", os.path.join(_HERE, "lib", "libtfQMRgpu.so"))   # override for A/B builds
LAB_LIB_PATH = os.path.join(_HERE, "lib", "libtfQMRgpu_lab.so")   # the same sources with -DTFQ_LAB: reads the TFQMRGPU_* tuning switches

LAYOUT_RRRRIIII, LAYOUT_RRIIRRII, LAYOUT_RIRIRIRI = 0x0F, 0x33, 0x55
SHADOW_HASH, SHADOW_GLIBC_RAND = 0, 1
PRECOND_NONE, PRECOND_BLOCK_JACOBI = 0, 1
CODE_LINE, CODE_CHAR = 1000, 10000 * 1000

EXPORTED_SYMBOLS = [  # include/tfqmrgpu.h
    "tfqmrgpuPrintError", "tfqmrgpuGetErrorString", "tfqmrgpuCreateHandle", "tfqmrgpuDestroyHandle",
    "tfqmrgpuSetStream", "tfqmrgpuGetStream", "tfqmrgpuCreateWorkspace", "tfqmrgpuDestroyWorkspace",
    "tfqmrgpu_bsrsv_allowedBlockSizes", "tfqmrgpu_bsrsv_blockSizeMissing", "tfqmrgpu_bsrsv_createPlan",
    "tfqmrgpu_bsrsv_destroyPlan", "tfqmrgpu_bsrsv_bufferSize", "tfqmrgpu_bsrsv_setBuffer",
    "tfqmrgpu_bsrsv_getBuffer", "tfqmrgpu_bsrsv_setMatrix", "tfqmrgpu_bsrsv_getMatrix",
    "tfqmrgpu_bsrsv_solve", "tfqmrgpu_bsrsv_getInfo", "tfqmrgpu_bsrsv_z", "tfqmrgpu_bsrsv_c",
]
EXT_SYMBOLS = [  # include/tfqmrgpu_ext.h
    "tfqmrgpuExt_planView", "tfqmrgpuExt_getBoundHistory", "tfqmrgpuExt_setProfiling", "tfqmrgpuExt_getProfile",
    "tfqmrgpuExt_getProfileGated", "tfqmrgpuExt_getProfileFirst", "tfqmrgpuExt_getMultiplyKernel", "tfqmrgpuExt_getLateV5",
    "tfqmrgpuExt_setShadowMode",
    "tfqmrgpuExt_setShadowVector", "tfqmrgpuExt_getShadowVector", "tfqmrgpuExt_getWorkVector", "tfqmrgpuExt_multiply", "tfqmrgpuExt_multiplyPrepare", "tfqmrgpuExt_multiplyOrdered", "tfqmrgpuExt_multiplyRelease", "tfqmrgpuExt_applyOperator", "tfqmrgpuExt_shardColumns",
    "tfqmrgpuExt_freeShard", "tfqmrgpuExt_commUniqueId", "tfqmrgpuExt_commInit",
    "tfqmrgpuExt_commDestroy", "tfqmrgpuExt_setReduceCallback", "tfqmrgpuExt_setOperator",
    "tfqmrgpuExt_getRefinementHistory", "tfqmrgpuExt_setThreeProductMultiply",
    "tfqmrgpuExt_setPreconditioner", "tfqmrgpuExt_getPreconditioner", "tfqmrgpuExt_setBlocks", "tfqmrgpuExt_getBlocks",
    "tfqmrgpuExt_keepOperator", "tfqmrgpuExt_residual", "tfqmrgpuExt_truncationLeak", "tfqmrgpuExt_leakUnits",
    "tfqmrgpuExt_leakMap", "tfqmrgpuExt_growPattern", "tfqmrgpuExt_freeGrownPattern",
    "tfqmrgpuExt_dropCost", "tfqmrgpuExt_shrinkPattern", "tfqmrgpuExt_solveFrom", "tfqmrgpuExt_carry",
    "tfqmrgpuExt_refineFrom",
    "tfqmrgpuExt_keepStarts", "tfqmrgpuExt_pushStart", "tfqmrgpuExt_startCount", "tfqmrgpuExt_startDepth", "tfqmrgpuExt_projectStart",
    "tfqmrgpuExt_allowPadding", "tfqmrgpuExt_paddedShape",
    "tfqmrgpuExt_shiftDiagonal", "tfqmrgpuExt_keepSum", "tfqmrgpuExt_addToSum", "tfqmrgpuExt_getSum", "tfqmrgpuExt_clearSum",
    "tfqmrgpuExt_solveMesh",
    "tfqmrgpuExt_selectDrop", "tfqmrgpuExt_selectLeak",
]
FORTRAN_SYMBOLS = [  # tfqmrgpu_amd/csrc/tfq_fortran.c
    "tfqmrgpuprinterror_", "tfqmrgpucreatehandle_", "tfqmrgpudestroyhandle_", "tfqmrgpusetstream_",
    "tfqmrgpugetstream_", "tfqmrgpu_bsrsv_createplan_", "tfqmrgpu_bsrsv_destroyplan_",
    "tfqmrgpu_bsrsv_buffersize_", "tfqmrgpucreateworkspace_", "tfqmrgpudestroyworkspace_",
    "tfqmrgpu_bsrsv_setbuffer_", "tfqmrgpu_bsrsv_getbuffer_", "tfqmrgpu_bsrsv_setmatrix_c_",
    "tfqmrgpu_bsrsv_setmatrix_z_", "tfqmrgpu_bsrsv_getmatrix_c_", "tfqmrgpu_bsrsv_getmatrix_z_",
    "tfqmrgpu_bsrsv_solve_", "tfqmrgpu_bsrsv_getinfo_",
]


class PlanView(C.Structure):
    _fields_ = [("nRows", C.c_uint32), ("nCols", C.c_uint32), ("nnzbA", C.c_uint32), ("nnzbX", C.c_uint32),
                ("nnzbB", C.c_uint32), ("nPairs", C.c_uint64), ("pairs", C.POINTER(C.c_uint32)),
                ("starts", C.POINTER(C.c_uint32)), ("subset", C.POINTER(C.c_uint32)),
                ("colindx", C.POINTER(C.c_uint16)), ("original_bsrColIndX", C.POINTER(C.c_int32)),
                ("LM", C.c_int32), ("LN", C.c_int32), ("precision", C.c_char)]


class Shard(C.Structure):
    _fields_ = [("mb", C.c_int32), ("nnzbX", C.c_int32), ("nnzbB", C.c_int32),
                ("rowPtrX", C.POINTER(C.c_int32)), ("colIndX", C.POINTER(C.c_int32)),
                ("rowPtrB", C.POINTER(C.c_int32)), ("colIndB", C.POINTER(C.c_int32)),
                ("xBlocks", C.POINTER(C.c_int32)), ("bBlocks", C.POINTER(C.c_int32)),
                ("firstCol", C.c_int32), ("nCols", C.c_int32)]


class GrownPattern(C.Structure):
    _fields_ = [("mb", C.c_int32), ("nnzbX", C.c_int32), ("rowPtrX", C.POINTER(C.c_int32)), ("colIndX", C.POINTER(C.c_int32)),
                ("oldBlock", C.POINTER(C.c_int32))]


REDUCE_CB = C.CFUNCTYPE(None,C.c_void_p, C.POINTER(C.c_double), C.c_int)
# tfqmrgpuOperator_t: (ctx, Y_d, X_d, colindx_d, nnzbX, nCols, lm, ln, precision, stream, *flops) -> status
OPERATOR_CB = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                          C.c_int, C.c_int, C.c_char, C.c_void_p, C.POINTER(C.c_double))


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            "tfqmrgpu_amd: %s is missing -- the HIP library has not been built; there is no CPU fallback. "
            "Run __graft_entry__.build() or `make -C tfqmrgpu_amd/csrc`." % path)
    # PyTorch ships its own libamdhip64.so.7 (same soname as /opt/rocm's).  A process must run ONE HIP
    # runtime: when torch is going to be used (bench.py, tests: device memory, streams, torch.distributed)
    # it has to be loaded first, then this library binds to the runtime that is already there.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    I, P = C.c_int, C.c_void_p
    lib.tfqmrgpuGetErrorString.restype = C.c_char_p
    lib.tfqmrgpuGetErrorString.argtypes = [C.c_int32]
    lib.tfqmrgpuCreateHandle.argtypes = [C.POINTER(P)]
    lib.tfqmrgpuDestroyHandle.argtypes = [P]
    lib.tfqmrgpuSetStream.argtypes = [P, P]
    lib.tfqmrgpuGetStream.argtypes = [P, C.POINTER(P)]
    lib.tfqmrgpuCreateWorkspace.argtypes = [C.POINTER(P), C.c_size_t, C.c_char]
    lib.tfqmrgpuDestroyWorkspace.argtypes = [P]
    lib.tfqmrgpu_bsrsv_allowedBlockSizes.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), I]
    lib.tfqmrgpu_bsrsv_blockSizeMissing.argtypes = [I, I]
    lib.tfqmrgpu_bsrsv_createPlan.argtypes = [P, C.POINTER(P), I, P, I, P, P, I, P, P, I, P, I, I]
    lib.tfqmrgpu_bsrsv_destroyPlan.argtypes = [P, P]
    lib.tfqmrgpu_bsrsv_bufferSize.argtypes = [P, P, I, I, I, I, C.c_char, C.POINTER(C.c_size_t)]
    lib.tfqmrgpu_bsrsv_setBuffer.argtypes = [P, P, P]
    lib.tfqmrgpu_bsrsv_getBuffer.argtypes = [P, P, C.POINTER(P)]
    lib.tfqmrgpu_bsrsv_setMatrix.argtypes = [P, P, C.c_char, P, C.c_char, I, I, C.c_char, I]
    lib.tfqmrgpu_bsrsv_getMatrix.argtypes = [P, P, C.c_char, P, C.c_char, I, I, C.c_char, I]
    lib.tfqmrgpu_bsrsv_solve.argtypes = [P, P, C.c_double, I]
    lib.tfqmrgpu_bsrsv_getInfo.argtypes = [P, P, C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_double), C.POINTER(C.c_double)]
    onecall = [I, I, I, P, I, P, P, C.c_char, P, I, P, P, C.c_char, P, I, P, P, C.c_char,
               C.POINTER(C.c_int32), C.POINTER(C.c_float), I, I]
    lib.tfqmrgpu_bsrsv_z.argtypes = onecall
    lib.tfqmrgpu_bsrsv_c.argtypes = onecall
    lib.tfqmrgpuExt_planView.argtypes = [P, C.POINTER(PlanView)]
    lib.tfqmrgpuExt_getBoundHistory.argtypes = [P, P, C.c_int32]
    lib.tfqmrgpuExt_setProfiling.argtypes = [P, I]
    lib.tfqmrgpuExt_getProfile.argtypes = [P, P, P]
    lib.tfqmrgpuExt_getProfileGated.argtypes = [P, P, P]
    lib.tfqmrgpuExt_getProfileFirst.argtypes = [P, P, P]
    lib.tfqmrgpuExt_getMultiplyKernel.argtypes = [P, P, C.c_int32]
    lib.tfqmrgpuExt_getLateV5.argtypes = [P, C.POINTER(C.c_int32)]
    lib.tfqmrgpuExt_setShadowMode.argtypes = [P, I]
    lib.tfqmrgpuExt_setShadowVector.argtypes = [P, P, P]
    lib.tfqmrgpuExt_getShadowVector.argtypes = [P, P, P]
    lib.tfqmrgpuExt_getWorkVector.argtypes = [P, P, C.c_int, P]
    lib.tfqmrgpuExt_multiply.argtypes = [P, C.c_char, I, I, C.c_uint32, P, P, P, P, P]
    lib.tfqmrgpuExt_multiplyPrepare.argtypes = [P, C.c_char, I, I, C.c_uint32, P, P, I, C.POINTER(C.c_void_p)]
    lib.tfqmrgpuExt_multiplyOrdered.argtypes = [P, C.c_char, I, I, C.c_uint32, P, P, P, P, P, P]
    lib.tfqmrgpuExt_multiplyRelease.argtypes = [P]
    lib.tfqmrgpuExt_applyOperator.argtypes = [P, P, I]
    lib.tfqmrgpuExt_shardColumns.argtypes = [I, P, I, P, P, I, P, I, I, I, C.POINTER(Shard)]
    lib.tfqmrgpuExt_freeShard.argtypes = [C.POINTER(Shard)]
    lib.tfqmrgpuExt_freeShard.restype = None
    lib.tfqmrgpuExt_commUniqueId.argtypes = [P]
    lib.tfqmrgpuExt_commInit.argtypes = [P, I, I, P]
    lib.tfqmrgpuExt_commDestroy.argtypes = [P]
    lib.tfqmrgpuExt_setReduceCallback.argtypes = [P, REDUCE_CB, P]
    lib.tfqmrgpuExt_setOperator.argtypes = [P, OPERATOR_CB, P]
    lib.tfqmrgpuExt_getRefinementHistory.argtypes = [P, P, P, C.c_int32]
    lib.tfqmrgpuExt_setThreeProductMultiply.argtypes = [P, I]
    lib.tfqmrgpuExt_setPreconditioner.argtypes = [P, I]
    lib.tfqmrgpuExt_getPreconditioner.argtypes = [P, P, P, C.POINTER(C.c_int32)]
    lib.tfqmrgpuExt_setBlocks.argtypes = [P, P, C.c_char, C.c_int32, P, P, C.c_char, C.c_char, I]
    lib.tfqmrgpuExt_getBlocks.argtypes = [P, P, C.c_char, C.c_int32, P, P, C.c_char, C.c_char, I]
    lib.tfqmrgpuExt_keepOperator.argtypes = [P, I]
    lib.tfqmrgpuExt_residual.argtypes = [P, P, P, P, P, C.POINTER(C.c_double)]
    lib.tfqmrgpuExt_truncationLeak.argtypes = [P, P, P, P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.tfqmrgpuExt_leakUnits.argtypes = [P, P]
    lib.tfqmrgpuExt_leakUnits.restype = C.c_int64
    lib.tfqmrgpuExt_leakMap.argtypes = [P, P, C.c_uint64, P, P, P, C.POINTER(C.c_uint64)]
    lib.tfqmrgpuExt_growPattern.argtypes = [P, C.c_uint64, P, C.POINTER(GrownPattern)]
    lib.tfqmrgpuExt_freeGrownPattern.argtypes = [C.POINTER(GrownPattern)]
    lib.tfqmrgpuExt_dropCost.argtypes = [P, P, P, P, C.POINTER(C.c_uint64)]
    lib.tfqmrgpuExt_shrinkPattern.argtypes = [P, C.c_uint64, P, C.POINTER(GrownPattern)]
    lib.tfqmrgpuExt_freeGrownPattern.restype = None
    lib.tfqmrgpuExt_solveFrom.argtypes = [P, P, C.c_double, I]
    lib.tfqmrgpuExt_carry.argtypes = [P, P, P, C.c_char, C.c_int32, P]
    lib.tfqmrgpuExt_refineFrom.argtypes = [P, P, C.c_double, I]
    lib.tfqmrgpuExt_keepStarts.argtypes = [P, I]
    lib.tfqmrgpuExt_pushStart.argtypes = [P, P]
    lib.tfqmrgpuExt_startCount.argtypes = [P]
    lib.tfqmrgpuExt_startCount.restype = C.c_int32
    lib.tfqmrgpuExt_startDepth.argtypes = [P]
    lib.tfqmrgpuExt_startDepth.restype = C.c_int32
    lib.tfqmrgpuExt_projectStart.argtypes = [P, P, P, P]
    lib.tfqmrgpuExt_allowPadding.argtypes = [P, I]
    lib.tfqmrgpuExt_paddedShape.argtypes = [P] + [C.POINTER(C.c_int32)] * 4
    lib.tfqmrgpuExt_shiftDiagonal.argtypes = [P, P, C.c_double, C.c_double]
    lib.tfqmrgpuExt_keepSum.argtypes = [P, I]
    lib.tfqmrgpuExt_addToSum.argtypes = [P, P, C.c_double, C.c_double]
    lib.tfqmrgpuExt_getSum.argtypes = [P, P, P, C.POINTER(C.c_int32)]
    lib.tfqmrgpuExt_clearSum.argtypes = [P, P]
    lib.tfqmrgpuExt_solveMesh.argtypes = [P, P, C.c_int32, P, P, C.c_double, I, I, P, P, P, C.POINTER(C.c_int32)]
    lib.tfqmrgpuExt_selectDrop.argtypes = [P, P, C.c_double, C.c_uint64, P, C.POINTER(C.c_uint64), P]
    lib.tfqmrgpuExt_selectLeak.argtypes = [P, P, C.c_double, C.c_uint64, P, C.POINTER(C.c_uint64), P]
    return lib


lib = load_library()


def decode(status):
    """(code, line, char) of a status word (include/tfqmrgpu.h)."""
    key = status // CODE_CHAR
    rest = status - key * CODE_CHAR
    return rest % CODE_LINE, rest // CODE_LINE, key


def error_string(status):
    return lib.tfqmrgpuGetErrorString(status).decode()


class TfqmrError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        super().__init__("%s returned %d: %s" % (where, status, error_string(status)))


def _check(status, where, allowed=(0,)):
    if status not in allowed:
        raise TfqmrError(status, where)
    return status


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def _addr(a):
    """the address of `a` even where it has no entries (_ptr would make that NULL, which means "not asked for"); None stays NULL"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _copied(p, n):
    """a host copy of the n int32 that the library's pointer p shows"""
    return np.ctypeslib.as_array(p, (n,)).copy() if n else np.zeros(0, np.int32)


class Problem:
    """A*X==B in BSR form: index arrays plus complex block values (C row-major blocks
    A[nnzbA, LM, LM], B[nnzbB, LM, LN]); the shape the reference's readers produce (bsr.hxx:10-24)."""

    def __init__(self, rowPtrA, colIndA, A, rowPtrX, colIndX, rowPtrB, colIndB, B, X=None, tolerance=1e-9, index_offset=0):
        self.rowPtrA, self.colIndA = _i32(rowPtrA), _i32(colIndA)
        self.rowPtrX, self.colIndX = _i32(rowPtrX), _i32(colIndX)
        self.rowPtrB, self.colIndB = _i32(rowPtrB), _i32(colIndB)
        self.A = np.ascontiguousarray(A, dtype=np.complex128)
        self.B = np.ascontiguousarray(B, dtype=np.complex128)
        self.X = None if X is None else np.ascontiguousarray(X, dtype=np.complex128)
        self.tolerance = float(tolerance)
        self.index_offset = int(index_offset)
        self.mb = len(self.rowPtrA) - 1
        self.LM = self.A.shape[1]
        self.LN = self.B.shape[2]
        self.nnzbA, self.nnzbX, self.nnzbB = len(self.colIndA), len(self.colIndX), len(self.colIndB)


class Solver:
    """Staged use of the C-ABI: createHandle, setStream, createPlan, bufferSize, (workspace), setBuffer,
    setMatrix, solve, getInfo, getMatrix -- the call sequence of the reference's benchmark driver
    (bench_tfqmrgpu.cu:64-217)."""

    def __init__(self, stream=None):
        self.handle = C.c_void_p(None)
        _check(lib.tfqmrgpuCreateHandle(C.byref(self.handle)), "tfqmrgpuCreateHandle")
        _check(lib.tfqmrgpuSetStream(self.handle, C.c_void_p(stream or 0)), "tfqmrgpuSetStream")
        self.plan = C.c_void_p(None)
        self.buffer = C.c_void_p(None)
        self._own_buffer = False
        self._keep = []
        self._reduce = None

    @classmethod
    def open(cls, pr, precision, *, preconditioner=None, keep_operator=False, keep_starts=None, keep_sum=False, allow_padding=False,
             three_products=False, shadow_mode=None, data_precision=None, buffer=True, stream=None):
        """a Solver with a plan for `pr`; the calls below stand in the one order the plan's options take.  An option left at its default
        makes no library call; buffer=False leaves set_buffer to the caller (self.buffer_bytes has the size); a step that raises closes"""
        s = cls(stream)
        try:
            s.create_plan(pr)
            if allow_padding:
                s.allow_padding(True)
            s.buffer_size(pr.LM, pr.LN, precision)
            if data_precision:
                s.data_precision = data_precision
            if three_products:
                s.set_three_product_multiply(True)
            if preconditioner is not None:
                s.set_preconditioner(preconditioner)
            if keep_operator:
                s.keep_operator(True)
            if keep_starts is not None:
                s.keep_starts(keep_starts)
            if keep_sum:
                s.keep_sum(True)
            if shadow_mode is not None:
                s.set_shadow_mode(shadow_mode)
            if buffer:
                s.set_buffer(nbytes=s.buffer_bytes)
        except BaseException:
            s.close()
            raise
        return s

    def load(self, A=None, B=None):
        """set_matrix('A') and set_matrix('B'), from the plan's problem where not given; returns self"""
        self.set_matrix("A", self.problem.A if A is None else A)
        self.set_matrix("B", self.problem.B if B is None else B)
        return self

    # -- plan ------------------------------------------------------------------------------------------
    def create_plan(self, pr, echo=0):
        self.problem = pr
        st = lib.tfqmrgpu_bsrsv_createPlan(self.handle, C.byref(self.plan), pr.mb,
                                           _ptr(pr.rowPtrA), pr.nnzbA, _ptr(pr.colIndA),
                                           _ptr(pr.rowPtrX), pr.nnzbX, _ptr(pr.colIndX),
                                           _ptr(pr.rowPtrB), pr.nnzbB, _ptr(pr.colIndB), pr.index_offset, echo)
        return _check(st, "tfqmrgpu_bsrsv_createPlan")

    def plan_view(self):
        v = PlanView()
        _check(lib.tfqmrgpuExt_planView(self.plan, C.byref(v)), "tfqmrgpuExt_planView")
        n = int(v.nPairs)
        return dict(nRows=v.nRows, nCols=v.nCols, nnzbA=v.nnzbA, nnzbX=v.nnzbX, nnzbB=v.nnzbB, nPairs=n,
                    pairs=np.ctypeslib.as_array(v.pairs, (2 * n,)).copy() if n else np.zeros(0, np.uint32),
                    starts=np.ctypeslib.as_array(v.starts, (v.nnzbX + 1,)).copy(),
                    subset=np.ctypeslib.as_array(v.subset, (v.nnzbB,)).copy() if v.nnzbB else np.zeros(0, np.uint32),
                    colindx=np.ctypeslib.as_array(v.colindx, (v.nnzbX,)).copy(),
                    original_bsrColIndX=np.ctypeslib.as_array(v.original_bsrColIndX, (v.nCols,)).copy())

    def allow_padding(self, on=True):
        """tfqmrgpu_ext.h section 18: buffer_size may pick the smallest listed block shape that holds the caller's; call after
        create_plan and before buffer_size"""
        return _check(lib.tfqmrgpuExt_allowPadding(self.plan, int(bool(on))), "tfqmrgpuExt_allowPadding")

    def padded_shape(self):
        """(lm, ln, LM, LN): the caller's block shape as given to buffer_size, and the plan's -- equal unless the plan is padded"""
        v = [C.c_int32(0) for _ in range(4)]
        _check(lib.tfqmrgpuExt_paddedShape(self.plan, *[C.byref(x) for x in v]), "tfqmrgpuExt_paddedShape")
        return tuple(int(x.value) for x in v)

    def buffer_size(self, LM, LN, precision):
        """LM, LN: the caller's block shape.  Afterwards self.lm, self.ln hold it -- the shape of the arrays of set_matrix, get_matrix,
        set_blocks and get_blocks -- and self.LM, self.LN the plan's shape, which sizes everything else; they differ on a padded plan only"""
        n = C.c_size_t(0)
        _check(lib.tfqmrgpu_bsrsv_bufferSize(self.handle, self.plan, LM, LM, LN, LN, precision.encode(), C.byref(n)),
               "tfqmrgpu_bsrsv_bufferSize")
        self.lm, self.ln, self.LM, self.LN = self.padded_shape()
        self.precision = precision
        # precision of the host arrays handed to set_matrix / returned by get_matrix: the plan's, for a mixed-precision plan ('m',
        # which takes both) double unless the caller sets data_precision = "c"
        self.data_precision = "z" if precision in "zm" else "c"
        self.buffer_bytes = n.value
        return n.value

    def set_shadow_mode(self, mode):
        _check(lib.tfqmrgpuExt_setShadowMode(self.plan, mode), "tfqmrgpuExt_setShadowMode")

    def set_buffer(self, device_ptr=None, nbytes=None):
        if device_ptr is None:
            _check(lib.tfqmrgpuCreateWorkspace(C.byref(self.buffer), nbytes, b"d"), "tfqmrgpuCreateWorkspace")
            self._own_buffer = True
        else:
            self.buffer = C.c_void_p(device_ptr)
        _check(lib.tfqmrgpu_bsrsv_setBuffer(self.handle, self.plan, self.buffer), "tfqmrgpu_bsrsv_setBuffer")

    def get_shadow_vector(self):
        """the shadow vector v3 in use: float [nnzbX, 2, LM, LN], caller's block order"""
        v3 = np.zeros((self.problem.nnzbX, 2, self.LM, self.LN), dtype=np.float32)
        _check(lib.tfqmrgpuExt_getShadowVector(self.handle, self.plan, _ptr(v3)), "tfqmrgpuExt_getShadowVector")
        return v3

    def get_work_vector(self, which):
        """work vector `which` (1: X, 4 ... 9: v4 ... v9, tfqmrgpu_core.hxx:52-59) as the last solve left it: complex [nnzbX, LM, LN]"""
        v = np.zeros((self.problem.nnzbX, 2, self.LM, self.LN), dtype=self._real_dtype())
        _check(lib.tfqmrgpuExt_getWorkVector(self.handle, self.plan, which, _ptr(v)), "tfqmrgpuExt_getWorkVector")
        return v[:, 0].astype(np.float64) + 1j * v[:, 1]

    # -- values ----------------------------------------------------------------------------------------
    def _real_dtype(self):
        return np.float64 if self.data_precision == "z" else np.float32

    def _values(self, blocks):
        """the caller's values in data_precision, contiguous: complex stays complex, anything else is taken as raw reals"""
        a = np.asarray(blocks)
        if np.iscomplexobj(a):
            return np.ascontiguousarray(a.astype(np.complex128 if self.data_precision == "z" else np.complex64))
        return np.ascontiguousarray(a, dtype=self._real_dtype())

    def _blocks_out(self, out, trans, layout, raw):
        """what get_matrix and get_blocks return from out[n, lm, ln, 2]: complex blocks, reshaped if transposed; raw reals otherwise"""
        n = out.shape[0]
        if raw or layout != LAYOUT_RIRIRIRI:
            return out.reshape(n, -1)
        c = out[..., 0] + 1j * out[..., 1]
        return c if trans in "n*" else c.reshape(n, self.ln, self.lm)

    def set_matrix(self, var, blocks, trans="n", layout=LAYOUT_RIRIRIRI):
        """blocks: complex array [nnzb, rows, cols] (interleaved layout) or a raw real array for other layouts"""
        a = self._values(blocks)
        self._keep.append(a)
        st = lib.tfqmrgpu_bsrsv_setMatrix(self.handle, self.plan, var.encode(), _ptr(a), self.data_precision.encode(),
                                          self.ln if var in "XBxb" else self.lm, self.lm, trans.encode(), layout)
        return _check(st, "tfqmrgpu_bsrsv_setMatrix('%s')" % var)

    def set_matrix_device(self, var, device_ptr, trans="n", layout=LAYOUT_RIRIRIRI):
        """the same call with an array that lives in DEVICE memory (data_precision says float or double): the library converts
        straight from it, asynchronously on the handle's stream"""
        st = lib.tfqmrgpu_bsrsv_setMatrix(self.handle, self.plan, var.encode(), C.c_void_p(device_ptr), self.data_precision.encode(),
                                          self.ln if var in "XBxb" else self.lm, self.lm, trans.encode(), layout)
        return _check(st, "tfqmrgpu_bsrsv_setMatrix('%s', device array)" % var)

    def get_matrix_device(self, device_ptr, trans="n", layout=LAYOUT_RIRIRIRI):
        st = lib.tfqmrgpu_bsrsv_getMatrix(self.handle, self.plan, b"X", C.c_void_p(device_ptr), self.data_precision.encode(),
                                          self.ln, self.lm, trans.encode(), layout)
        return _check(st, "tfqmrgpu_bsrsv_getMatrix(device array)")

    def get_matrix(self, nnzb=None, trans="n", layout=LAYOUT_RIRIRIRI, raw=False):
        nnzb = self.problem.nnzbX if nnzb is None else nnzb
        out = np.zeros((nnzb, self.lm, self.ln, 2), dtype=self._real_dtype())
        st = lib.tfqmrgpu_bsrsv_getMatrix(self.handle, self.plan, b"X", _ptr(out), self.data_precision.encode(),
                                          self.ln, self.lm, trans.encode(), layout)
        _check(st, "tfqmrgpu_bsrsv_getMatrix")
        return self._blocks_out(out, trans, layout, raw)

    # -- listed blocks (tfqmrgpu_ext.h section 8) -------------------------------------------------------
    def set_blocks(self, var, blocks, values, trans="n", layout=LAYOUT_RIRIRIRI):
        """set the blocks of operand `var` that `blocks` lists (positions in the caller's block order) from `values`, compact: complex
        [len(blocks), rows, cols] (interleaved layout) or a raw real array for other layouts, as set_matrix; returns the raw status"""
        idx = _i32(blocks)
        a = self._values(values)
        st = lib.tfqmrgpuExt_setBlocks(self.handle, self.plan, var.encode(), len(idx), _ptr(idx), _ptr(a), self.data_precision.encode(),
                                       trans.encode(), layout)
        return _check(st, "tfqmrgpuExt_setBlocks('%s')" % var)

    def set_blocks_device(self, var, blocks, device_ptr, trans="n", layout=LAYOUT_RIRIRIRI):
        """the same with values in DEVICE memory (data_precision says float or double); the list stays a host array"""
        idx = _i32(blocks)
        st = lib.tfqmrgpuExt_setBlocks(self.handle, self.plan, var.encode(), len(idx), _ptr(idx), C.c_void_p(device_ptr),
                                       self.data_precision.encode(), trans.encode(), layout)
        return _check(st, "tfqmrgpuExt_setBlocks('%s', device array)" % var)

    def _block_list(self, blocks):
        """(host list or None, its length): None means the X blocks on B's pattern, in B's block order"""
        if blocks is None:
            return None, self.problem.nnzbB
        idx = _i32(blocks)
        return idx, len(idx)

    def get_blocks(self, blocks=None, trans="n", layout=LAYOUT_RIRIRIRI, raw=False):
        """the X blocks that `blocks` lists (None: those on B's pattern, in B's block order); shapes as get_matrix"""
        idx, n = self._block_list(blocks)
        out = np.zeros((n, self.lm, self.ln, 2), dtype=self._real_dtype())
        st = lib.tfqmrgpuExt_getBlocks(self.handle, self.plan, b"X", n, None if idx is None else _ptr(idx), _ptr(out),
                                       self.data_precision.encode(), trans.encode(), layout)
        _check(st, "tfqmrgpuExt_getBlocks")
        return self._blocks_out(out, trans, layout, raw)

    def get_blocks_device(self, device_ptr, blocks=None, trans="n", layout=LAYOUT_RIRIRIRI):
        idx, n = self._block_list(blocks)
        st = lib.tfqmrgpuExt_getBlocks(self.handle, self.plan, b"X", n, None if idx is None else _ptr(idx), C.c_void_p(device_ptr),
                                       self.data_precision.encode(), trans.encode(), layout)
        return _check(st, "tfqmrgpuExt_getBlocks(device array)")

    def apply_operator(self, repetitions=1):
        """X := A*X on the plan's data (tfqmrgpuExt_applyOperator)"""
        return _check(lib.tfqmrgpuExt_applyOperator(self.handle, self.plan, repetitions), "tfqmrgpuExt_applyOperator")

    # -- solve -----------------------------------------------------------------------------------------
    def solve(self, threshold, max_iterations):
        """returns the raw status: 0 converged, 9 max iterations, 6 breakdown (tfqmrgpu_core.hxx:170,258,297)"""
        st = lib.tfqmrgpu_bsrsv_solve(self.handle, self.plan, threshold, max_iterations)
        return _check(st, "tfqmrgpu_bsrsv_solve", allowed=(0, 6, 9))

    def solve_from(self, threshold, max_iterations):
        """tfqmrgpu_ext.h section 14: the same solve started from the X in the plan -- the last solution, or what set_matrix('X') /
        set_blocks('X') brought -- where solve() ignores it and starts from zero.  threshold and get_info stay relative to |B|.
        Returns the raw status as solve does"""
        st = lib.tfqmrgpuExt_solveFrom(self.handle, self.plan, threshold, max_iterations)
        return _check(st, "tfqmrgpuExt_solveFrom", allowed=(0, 6, 9))

    def refine_from(self, threshold, max_iterations):
        """tfqmrgpu_ext.h section 16: on a mixed-precision plan ('m') the refinement started from the X in the plan -- the float solves
        work on the correction to it, refinement_history()[0] is the residual of that X instead of 1; on a 'z' or 'c' plan it is
        solve_from.  Returns the raw status as solve does"""
        st = lib.tfqmrgpuExt_refineFrom(self.handle, self.plan, threshold, max_iterations)
        return _check(st, "tfqmrgpuExt_refineFrom", allowed=(0, 6, 9))

    # -- start projection (tfqmrgpu_ext.h section 17) ---------------------------------------------------
    def keep_starts(self, depth):
        """keep the `depth` newest starts in the plan, 0 (off) ... 4; call after buffer_size.  A smaller depth drops the oldest starts"""
        return _check(lib.tfqmrgpuExt_keepStarts(self.plan, int(depth)), "tfqmrgpuExt_keepStarts")

    def push_start(self):
        """the X that get_matrix would return now becomes the newest start; with `depth` starts held the oldest leaves"""
        return _check(lib.tfqmrgpuExt_pushStart(self.handle, self.plan), "tfqmrgpuExt_pushStart")

    def start_count(self):
        return int(lib.tfqmrgpuExt_startCount(self.plan))

    def start_depth(self):
        return int(lib.tfqmrgpuExt_startDepth(self.plan))

    def project_start(self):
        """X := per (block column, right-hand side) the combination of the kept starts that minimises |B - A X| for the caller's A as it
        is now; what precedes solve_from / refine_from in an energy loop.  Returns a dict: coefficients, complex [nCols, LN, depth]
        (newest start first, zeros for dropped and absent starts), and n_used, int32 [nCols, LN], the starts kept per right-hand side"""
        n, depth = int(self.plan_view()["nCols"]), self.start_depth()      # the plan's own depth sizes the array the library fills
        g = np.zeros((n, self.LN, max(depth, 1), 2), np.float64)
        used = np.zeros((n, self.LN), np.int32)
        _check(lib.tfqmrgpuExt_projectStart(self.handle, self.plan, _ptr(g), _ptr(used)), "tfqmrgpuExt_projectStart")
        return dict(coefficients=(g[..., 0] + 1j * g[..., 1])[:, :, :depth], n_used=used)

    # -- energy mesh (tfqmrgpu_ext.h section 19) ----------------------------------------------------------
    def shift_diagonal(self, sigma):
        """A := A_base + sigma * 1 on the device: the diagonal elements of A's diagonal blocks, from the diagonal that the last
        set_matrix('A') / set_blocks('A') / carry_from(.., 'A') left; shifts do not accumulate.  Bit for bit set_blocks('A') of all
        diagonal blocks with the sum formed on the host in the storage precision.  Returns the raw status"""
        sigma = complex(sigma)
        return _check(lib.tfqmrgpuExt_shiftDiagonal(self.handle, self.plan, sigma.real, sigma.imag), "tfqmrgpuExt_shiftDiagonal")

    def keep_sum(self, on=True):
        """keep a weighted sum of X on B's pattern in the plan (off by default); call after buffer_size.  Every call zeroes the sum"""
        return _check(lib.tfqmrgpuExt_keepSum(self.plan, int(bool(on))), "tfqmrgpuExt_keepSum")

    def add_to_sum(self, weight):
        """S += weight * X on the blocks of X that carry a block of B, in double on the device; X is what get_matrix would return now"""
        w = complex(weight)
        return _check(lib.tfqmrgpuExt_addToSum(self.handle, self.plan, w.real, w.imag), "tfqmrgpuExt_addToSum")

    def get_sum(self):
        """(S as complex128 [nnzbB, lm, ln] in B's block order, the number of add_to_sum calls since the sum was last zero)"""
        out = np.zeros((self.problem.nnzbB, self.lm, self.ln, 2), np.float64)
        n = C.c_int32(0)
        _check(lib.tfqmrgpuExt_getSum(self.handle, self.plan, C.c_void_p(out.ctypes.data), C.byref(n)), "tfqmrgpuExt_getSum")
        return out.view(np.complex128)[..., 0], int(n.value)      # (Re, Im) pairs are complex128 as they lie: no arithmetic touches the bits

    def clear_sum(self):
        return _check(lib.tfqmrgpuExt_clearSum(self.handle, self.plan), "tfqmrgpuExt_clearSum")

    def solve_mesh(self, sigma, weight, threshold, max_iterations, from_x=False):
        """the energy loop in one call: per energy shift_diagonal(sigma[e]); solve (the first energy unless from_x) or project_start
        where starts are held and refine_from; push_start where keep_starts is on; add_to_sum(weight[e]) where weights are given
        and keep_sum is on.  sigma, weight: complex sequences (weight may be None).  Returns a dict: status (of the call: 0, 9, or what
        ended the loop early), n_done, and per energy that ran iterations, residual, statuses"""
        sg = np.ascontiguousarray(np.asarray(sigma, dtype=np.complex128).reshape(-1)).view(np.float64)
        n = len(sg) // 2
        wt = None if weight is None else np.ascontiguousarray(np.asarray(weight, dtype=np.complex128).reshape(-1)).view(np.float64)
        if wt is not None and len(wt) != len(sg):
            raise ValueError("solve_mesh: one weight per energy")
        its, res, sts = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.int32)
        done = C.c_int32(0)
        st = lib.tfqmrgpuExt_solveMesh(self.handle, self.plan, n, _ptr(sg), None if wt is None else _ptr(wt), threshold, max_iterations,
                                       int(bool(from_x)), _ptr(its), _ptr(res), _ptr(sts), C.byref(done))
        _check(st, "tfqmrgpuExt_solveMesh", allowed=(0, 6, 9))
        k = int(done.value)
        return dict(status=st, n_done=k, iterations=its[:k].copy(), residual=res[:k].copy(), statuses=sts[:k].copy())

    # -- operands from another plan (tfqmrgpu_ext.h section 15) ---------------------------------------------
    def carry_from(self, src, var, old_block=None):
        """operand `var` ('A', 'B' or 'X') of this plan := that of the Solver `src`, device to device: block n becomes block
        old_block[n] of src (both in the caller's block orders, 0-based), -1 a zero block -- the oldBlock of grow_pattern and
        shrink_pattern; None: the identity, which needs as many blocks on either side.  Acts on this plan as set_matrix(var) does; the
        two plans may differ in precision.  Asynchronous on this Solver's stream; returns the raw status"""
        n = {"a": self.problem.nnzbA, "b": self.problem.nnzbB, "x": self.problem.nnzbX}.get(var.lower(), 0)
        idx = None
        if old_block is not None:
            idx = _i32(old_block).reshape(-1)
            n = len(idx)
        st = lib.tfqmrgpuExt_carry(self.handle, self.plan, src.plan, var.encode(), n, None if idx is None else C.c_void_p(idx.ctypes.data))
        return _check(st, "tfqmrgpuExt_carry('%s')" % var)

    def adopt(self, src, old_block_x=None):
        """A, B and X of the Solver `src` into this plan without a host transfer of values: A and B block for block (their patterns
        are those of src), X through old_block_x (carry_from).  What follows a grown or shrunk pattern and precedes solve_from"""
        self.carry_from(src, "A")
        self.carry_from(src, "B")
        return self.carry_from(src, "X", old_block_x)

    def set_operator(self, multiply):
        """user-defined operator (tfqmrgpu_ext.h section 5): multiply(Y_ptr, X_ptr, colindx_ptr, nnzbX, nCols, lm, ln,
        precision, stream) enqueues Y = A*X on device data in the caller's block order and returns the flop count;
        None restores the built-in block-sparse operator"""
        if multiply is None:
            self._operator = OPERATOR_CB(0)
        else:
            def thunk(ctx, y, x, colindx, nnzbX, nCols, lm, ln, precision, stream, flops):
                try:
                    flops[0] = float(multiply(y, x, colindx, nnzbX, nCols, lm, ln, precision.decode(), stream) or 0.)
                    return 0
                except Exception:                   # an exception must not unwind through the C frames
                    import traceback; traceback.print_exc()
                    return 14
            self._operator = OPERATOR_CB(thunk)     # keep the thunk alive as long as the plan may call it
        _check(lib.tfqmrgpuExt_setOperator(self.plan, self._operator, None), "tfqmrgpuExt_setOperator")

    def set_reduce_callback(self, fn):
        """several ranks (tfqmrgpu_ext.h section 4): fn(values, n) max-reduces the n doubles behind the ctypes pointer `values` over the
        ranks, in place; None makes the handle one rank again.  A call on the handle: it needs neither plan nor buffer"""
        self._reduce = REDUCE_CB(0) if fn is None else REDUCE_CB(lambda ctx, values, n: fn(values, n))
        # (kept alive as long as the handle may call it, also where the call below raises: the library has taken the pointer by then)
        _check(lib.tfqmrgpuExt_setReduceCallback(self.handle, self._reduce, None), "tfqmrgpuExt_setReduceCallback")

    def get_info(self):
        r, f, fa, it = C.c_double(0), C.c_double(0), C.c_double(0), C.c_int32(0)
        _check(lib.tfqmrgpu_bsrsv_getInfo(self.handle, self.plan, C.byref(r), C.byref(it), C.byref(f), C.byref(fa)),
               "tfqmrgpu_bsrsv_getInfo")
        return dict(residual=r.value, iterations=it.value, flops=f.value, flops_all=fa.value)

    def refinement_history(self, with_iterations=False):
        """mixed precision: relative residual (double arithmetic) in front of every float solve and at the end
        [, the float iterations of every solve]"""
        n = lib.tfqmrgpuExt_getRefinementHistory(self.plan, None, None, 0)
        h, it = np.zeros(max(n, 0), dtype=np.float64), np.zeros(max(n, 0), dtype=np.int32)
        if n > 0:
            lib.tfqmrgpuExt_getRefinementHistory(self.plan, _ptr(h), _ptr(it), n)
        return (h, it) if with_iterations else h

    def set_three_product_multiply(self, on=True):
        _check(lib.tfqmrgpuExt_setThreeProductMultiply(self.plan, int(on)), "tfqmrgpuExt_setThreeProductMultiply")

    def set_preconditioner(self, kind=PRECOND_BLOCK_JACOBI):
        """tfqmrgpu_ext.h section 7: PRECOND_NONE or PRECOND_BLOCK_JACOBI (applied from the right); call after buffer_size"""
        _check(lib.tfqmrgpuExt_setPreconditioner(self.plan, int(kind)), "tfqmrgpuExt_setPreconditioner")

    def keep_operator(self, on=True):
        """tfqmrgpu_ext.h section 9: keep the caller's A next to the scaled one, so that set_blocks('A') and a change of the
        preconditioner kind work on a preconditioned plan; call after buffer_size.  Raises TfqmrError (status 14, key 'A') when the A in
        the buffer is scaled already and the plan has no copy of the caller's"""
        return _check(lib.tfqmrgpuExt_keepOperator(self.plan, int(bool(on))), "tfqmrgpuExt_keepOperator")

    def get_preconditioner(self, values=True):
        """(M^-1 as complex [mb, LM, LM] -- None with values=False --, number of block rows whose M_ii is the unit matrix); between
        set_matrix('A') and the first solve this call performs the set-up (inversion and scaling of A) itself"""
        n = C.c_int32(0)
        m = np.zeros((self.problem.mb, 2, self.LM, self.LM), dtype=np.float32 if self.precision == "c" else np.float64) if values else None
        _check(lib.tfqmrgpuExt_getPreconditioner(self.handle, self.plan, _ptr(m) if values else None, C.byref(n)), "tfqmrgpuExt_getPreconditioner")
        return (m[:, 0].astype(np.float64) + 1j * m[:, 1]) if values else None, int(n.value)

    def residual(self):
        """tfqmrgpu_ext.h section 10: |B - A X|^2 and |B|^2 per (block column, right-hand side) of the caller's A, the plan's B and the
        X that get_matrix would return, summed in double on the device.  Returns a dict: residual2, bnorm2 [nCols, LN], columns [nCols]
        (the caller's block column indices), relative = sqrt(residual2 / bnorm2) (IEEE: NaN where both are 0, inf where only b is) and
        worst, the largest relative residual that is not NaN"""
        n = int(self.plan_view()["nCols"])
        r2, b2 = np.zeros((n, self.LN), np.float64), np.zeros((n, self.LN), np.float64)
        cols, worst = np.zeros(n, np.int32), C.c_double(0)
        _check(lib.tfqmrgpuExt_residual(self.handle, self.plan, _ptr(r2), _ptr(b2), _ptr(cols), C.byref(worst)), "tfqmrgpuExt_residual")
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.sqrt(r2 / b2)
        return dict(residual2=r2, bnorm2=b2, columns=cols, relative=rel, worst=worst.value)

    def truncation_leak(self):
        """tfqmrgpu_ext.h section 11: what A X puts on the block rows OUTSIDE each block column's pattern, |.|^2 per (block column,
        right-hand side) of the caller's A and the X that get_matrix would return, summed in double on the device; residual2 + leak2 is
        the residual of the untruncated system.  Returns a dict: leak2 [nCols, LN] float64, columns [nCols] (the caller's block column
        indices), n_leak_blocks, n_leak_pairs, and units [nCols], the work units that each column's leak positions are cut into"""
        n = int(self.plan_view()["nCols"])
        leak2, cols = np.zeros((n, self.LN), np.float64), np.zeros(n, np.int32)
        nb, npairs = C.c_uint64(0), C.c_uint64(0)
        _check(lib.tfqmrgpuExt_truncationLeak(self.handle, self.plan, _ptr(leak2), _ptr(cols), C.byref(nb), C.byref(npairs)), "tfqmrgpuExt_truncationLeak")
        units = np.zeros(n, np.uint32)
        lib.tfqmrgpuExt_leakUnits(self.plan, _ptr(units))
        return dict(leak2=leak2, columns=cols, n_leak_blocks=int(nb.value), n_leak_pairs=int(npairs.value), units=units)

    def leak_counts(self):
        """the pattern-only form of truncation_leak: (n_leak_blocks, n_leak_pairs).  Host analysis, no launch: needs create_plan and
        buffer_size only"""
        nb, npairs = C.c_uint64(0), C.c_uint64(0)
        _check(lib.tfqmrgpuExt_truncationLeak(self.handle, self.plan, None, None, C.byref(nb), C.byref(npairs)), "tfqmrgpuExt_truncationLeak")
        return int(nb.value), int(npairs.value)

    def leak_map(self, values=True):
        """tfqmrgpu_ext.h section 12: the truncation leak per leak position, ordered by (compressed block column, block row).  Returns a
        dict: rows, cols [n_leak_blocks] int32 (block row, 0-based; COMPRESSED block column), pos2 [n_leak_blocks, LN] float64 -- None with
        values=False, the pattern-only form: host analysis, no launch, needs create_plan and buffer_size only -- and n_leak_blocks"""
        n = self.leak_counts()[0]
        rows, cols = np.zeros(n, np.int32), np.zeros(n, np.int32)
        pos2 = np.zeros((n, self.LN), np.float64) if values else None
        nb = C.c_uint64(0)
        _check(lib.tfqmrgpuExt_leakMap(self.handle, self.plan, n, _addr(rows), _addr(cols), _addr(pos2), C.byref(nb)), "tfqmrgpuExt_leakMap")
        return dict(rows=rows, cols=cols, pos2=pos2, n_leak_blocks=int(nb.value))

    def grow_pattern(self, take=None):
        """tfqmrgpu_ext.h section 12: the BSR pattern of X with the leak positions `take` added (indices into the order of leak_map;
        None: all of them, an empty list: none).  Returns (rowPtrX, colIndX, oldBlock) as int32 arrays: the form create_plan reads, and
        for every new block the old block whose values it takes over, -1 for an added one.  Host only"""
        g = GrownPattern()
        if take is None:
            st = lib.tfqmrgpuExt_growPattern(self.plan, 0, None, C.byref(g))
        else:
            idx = np.ascontiguousarray(take, dtype=np.uint64).reshape(-1)
            st = lib.tfqmrgpuExt_growPattern(self.plan, len(idx), C.c_void_p(idx.ctypes.data), C.byref(g))
        _check(st, "tfqmrgpuExt_growPattern")
        return self._read_pattern(g)

    @staticmethod
    def _read_pattern(g):
        """(rowPtrX, colIndX, oldBlock) as host copies of a GrownPattern that the library filled, which is freed here"""
        try:
            return _copied(g.rowPtrX, g.mb + 1), _copied(g.colIndX, g.nnzbX), _copied(g.oldBlock, g.nnzbX)
        finally:
            lib.tfqmrgpuExt_freeGrownPattern(C.byref(g))

    def grow_problem(self, pr, take=None):
        """the Problem with the grown pattern of X (grow_pattern) and the same A and B as `pr`, the problem of this plan; where `pr`
        carries values of X they move to their new places, the added blocks are zero"""
        rowPtrX, colIndX, old = self.grow_pattern(take)
        X = None
        if pr.X is not None:
            X = np.zeros((len(colIndX), pr.LM, pr.LN), dtype=np.complex128)
            X[old >= 0] = pr.X[old[old >= 0]]
        return Problem(pr.rowPtrA, pr.colIndA, pr.A, rowPtrX, colIndX, pr.rowPtrB, pr.colIndB, pr.B, X, pr.tolerance, pr.index_offset)

    def drop_cost(self, cost=True, weight=True):
        """tfqmrgpu_ext.h section 13: what every block of X carries.  Returns a dict: cost2 [nnzbX, LN] float64, per block of X in the
        caller's order and right-hand side the sum of |A_ik X_kc (:, j)|^2 over the plan's products with that block -- dropping the
        block adds at most sqrt(cost2) to the residual norm of its column --, weight2 [nnzbX, LN] = |X_kc (:, j)|^2, and n_products
        (plan_view()["nPairs"]).  cost=False / weight=False: that array is None and is not computed; both False: the count alone,
        which needs create_plan and buffer_size only"""
        n = int(self.plan_view()["nnzbX"])
        cost2 = np.zeros((n, self.LN), np.float64) if cost else None
        weight2 = np.zeros((n, self.LN), np.float64) if weight else None
        count = C.c_uint64(0)
        _check(lib.tfqmrgpuExt_dropCost(self.handle, self.plan, _addr(cost2), _addr(weight2), C.byref(count)), "tfqmrgpuExt_dropCost")
        return dict(cost2=cost2, weight2=weight2, n_products=int(count.value))

    def shrink_pattern(self, drop):
        """tfqmrgpu_ext.h section 13: the BSR pattern of X without the blocks `drop` (block positions of X in the caller's order,
        0-based).  Returns (rowPtrX, colIndX, oldBlock) as int32 arrays: the form create_plan reads, and for every new block the old
        block whose values it takes over.  Host only, needs create_plan alone"""
        g = GrownPattern()
        idx = np.ascontiguousarray(drop, dtype=np.int32).reshape(-1)
        _check(lib.tfqmrgpuExt_shrinkPattern(self.plan, len(idx), C.c_void_p(idx.ctypes.data), C.byref(g)), "tfqmrgpuExt_shrinkPattern")
        return self._read_pattern(g)

    def shrink_problem(self, pr, drop):
        """the Problem with the shrunk pattern of X (shrink_pattern) and the same A and B as `pr`, the problem of this plan; where `pr`
        carries values of X the kept blocks keep theirs"""
        rowPtrX, colIndX, old = self.shrink_pattern(drop)
        X = None if pr.X is None else pr.X[old]
        return Problem(pr.rowPtrA, pr.colIndA, pr.A, rowPtrX, colIndX, pr.rowPtrB, pr.colIndB, pr.B, X, pr.tolerance, pr.index_offset)

    # -- selection on the device (tfqmrgpu_ext.h section 20) --------------------------------------------------
    def _select(self, fn, where, eta, index_dtype, sums):
        """the two calls of a selection: one for the count, one with exactly that room"""
        count = C.c_uint64(0)
        _check(fn(self.handle, self.plan, float(eta), 0, None, C.byref(count), None), where)
        idx = np.zeros(int(count.value), index_dtype)
        out = np.zeros((int(self.plan_view()["nCols"]), self.LN), np.float64) if sums else None
        _check(fn(self.handle, self.plan, float(eta), len(idx), _addr(idx), C.byref(count), _addr(out)), where)
        return idx, out

    def select_drop(self, eta, spent=True):
        """tfqmrgpu_ext.h section 20: the blocks of X (the caller's order, ascending, int32) that carry no block of B and whose
        cost2 <= eta^2 bnorm2 for every right-hand side, decided on the device from the records of drop_cost() and residual() -- what
        shrink_pattern and shrink_problem take as `drop`.  Returns a dict: blocks, and spent [nCols, LN] float64, the sum of sqrt(cost2)
        over the selected blocks of each block column (None with spent=False)"""
        blocks, out = self._select(lib.tfqmrgpuExt_selectDrop, "tfqmrgpuExt_selectDrop", eta, np.int32, spent)
        return dict(blocks=blocks, spent=out)

    def select_leak(self, eta, left=True):
        """tfqmrgpu_ext.h section 20: the leak positions (the order of leak_map(), ascending, uint64) with pos2 > eta^2 bnorm2 for some
        right-hand side with bnorm2 > 0, decided on the device from the records of leak_map() and residual() -- what grow_pattern and
        grow_problem take as `take`.  Returns a dict: take, and left [nCols, LN] float64, the sum of pos2 over the positions of each
        block column that were NOT selected (None with left=False)"""
        take, out = self._select(lib.tfqmrgpuExt_selectLeak, "tfqmrgpuExt_selectLeak", eta, np.uint64, left)
        return dict(take=take, left=out)

    def bound_history(self):
        n = lib.tfqmrgpuExt_getBoundHistory(self.plan, None, 0)
        h = np.zeros(max(n, 0), dtype=np.float64)
        if n > 0:
            lib.tfqmrgpuExt_getBoundHistory(self.plan, _ptr(h), n)
        return h

    PROFILE_CLASSES = ["dec35", "xpay_v6", "spmm_v4_dot", "dec34", "v5_nrm", "decT_c67", "x_v6_v7",
                       "spmm_v5_nrm_dot", "decT_final", "decide", "probe"]

    def set_profiling(self, on=True):
        _check(lib.tfqmrgpuExt_setProfiling(self.plan, int(on)), "tfqmrgpuExt_setProfiling")

    def profile(self, gated=False, first=False):
        """{kernel class: (launches, total ms)} of the last solve; gated=True: the launches that returned at once;
        first=True: of the launches that did work, those of the first iteration (which skip the operands that are zero there)"""
        n = len(self.PROFILE_CLASSES)
        cnt, ms = np.zeros(n, np.int64), np.zeros(n, np.float64)
        fn = lib.tfqmrgpuExt_getProfileGated if gated else lib.tfqmrgpuExt_getProfileFirst if first else lib.tfqmrgpuExt_getProfile
        _check(fn(self.plan, _ptr(cnt), _ptr(ms)), "tfqmrgpuExt_getProfile")
        return {k: (int(cnt[i]), float(ms[i])) for i, k in enumerate(self.PROFILE_CLASSES)}

    def multiply_kernel(self):
        """the kernel family of this plan's fused multiplies, e.g. 'k_spmm_ilv16' (needs the buffer)"""
        buf = C.create_string_buffer(64)
        _check(lib.tfqmrgpuExt_getMultiplyKernel(self.plan, buf, 64), "tfqmrgpuExt_getMultiplyKernel")
        return buf.value.decode()

    def late_v5(self):
        """whether a one-rank solve of this plan runs the 'late v5' slot: v5_nrm stores nothing, spmm_v5_nrm_dot applies its half step (needs the buffer)"""
        on = C.c_int32(-1)
        _check(lib.tfqmrgpuExt_getLateV5(self.plan, C.byref(on)), "tfqmrgpuExt_getLateV5")
        return bool(on.value)

    def close(self):
        if self.plan:
            lib.tfqmrgpu_bsrsv_destroyPlan(self.handle, self.plan)
            self.plan = C.c_void_p(None)
        if self._own_buffer and self.buffer:
            lib.tfqmrgpuDestroyWorkspace(self.buffer)
            self.buffer = C.c_void_p(None)
        if self.handle:
            lib.tfqmrgpuDestroyHandle(self.handle)
            self.handle = C.c_void_p(None)
            self._reduce = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def hash_shadow_vector(pr):
    """numpy restatement of the library's default shadow vector (tfq_device.hpp: shadow_key / shadow_quad / shadow_pick), float
    [nnzbX, 2, LM, LN] in the caller's block order -- what tests feed to the CPU oracle"""
    from .problems import _splitmix64
    rows = np.repeat(np.arange(pr.mb, dtype=np.uint64), np.diff(pr.rowPtrX))
    cols = (pr.colIndX.astype(np.int64) - pr.index_offset).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = _splitmix64((cols << np.uint64(32)) | rows) ^ np.uint64(1234)
        q = np.arange((pr.LM // 2) * pr.LN, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95)   # one hash per (pair of rows m, column c)
        h = _splitmix64(key[:, None] + q[None, :]).reshape(pr.nnzbX, pr.LM // 2, pr.LN)
    v = np.empty((pr.nnzbX, 2, pr.LM // 2, 2, pr.LN), dtype=np.float32)
    for odd in range(2):
        for plane in range(2):       # 16 bits each: (row 2m | 2m + 1) x (Re | Im)
            bits = (h >> np.uint64(16 * (2 * odd + plane))) & np.uint64(0xFFFF)
            v[:, plane, :, odd, :] = (bits + np.uint64(1)).astype(np.float32) * np.float32(1.0 / 65536.0)
    return v.reshape(pr.nnzbX, 2, pr.LM, pr.LN)


def solve_problem(pr, precision="z", threshold=None, max_iterations=2000, transA="n", shadow_mode=SHADOW_HASH, stream=None,
                  data_precision=None, three_products=False, preconditioner=PRECOND_NONE, allow_padding=False):
    """createPlan .. getMatrix in one go; returns (status, X[nnzbX, LM, LN] complex, info dict).
    preconditioner=PRECOND_BLOCK_JACOBI: info["n_identity"] = block rows whose M_ii is the unit matrix.
    allow_padding=True (tfqmrgpu_ext.h section 18): any block shape up to 64 x 64; info["padded_shape"] = (lm, ln, LM, LN)."""
    with Solver.open(pr, precision, preconditioner=None if preconditioner == PRECOND_NONE else preconditioner, allow_padding=allow_padding,
                     three_products=three_products, shadow_mode=shadow_mode, data_precision=data_precision, stream=stream) as s:
        s.set_matrix("A", pr.A, transA)
        s.set_matrix("B", pr.B, "n")
        status = s.solve(pr.tolerance if threshold is None else threshold, max_iterations)
        info = s.get_info()
        if preconditioner != PRECOND_NONE:
            info["n_identity"] = s.get_preconditioner(values=False)[1]
        info["bound_history"] = s.bound_history()
        info["refinement_history"] = s.refinement_history()
        info["buffer_bytes"] = s.buffer_bytes
        if allow_padding:
            info["padded_shape"] = s.padded_shape()
        X = s.get_matrix()
    return status, X, info


def shard_columns(pr, nranks, rank):
    """Sub-problem of `pr` owned by `rank`: contiguous range of compressed block columns of X/B
    (tfqmrgpuExt_shardColumns).  Returns (Problem, xBlocks, bBlocks)."""
    sh = Shard()
    st = lib.tfqmrgpuExt_shardColumns(pr.mb, _ptr(pr.rowPtrX), pr.nnzbX, _ptr(pr.colIndX), _ptr(pr.rowPtrB), pr.nnzbB,
                                      _ptr(pr.colIndB), pr.index_offset, nranks, rank, C.byref(sh))
    _check(st, "tfqmrgpuExt_shardColumns")
    try:
        xb, bb = _copied(sh.xBlocks, sh.nnzbX), _copied(sh.bBlocks, sh.nnzbB)
        off = pr.index_offset
        sub = Problem(pr.rowPtrA - off, pr.colIndA - off, pr.A,
                      _copied(sh.rowPtrX, sh.mb + 1), _copied(sh.colIndX, sh.nnzbX),
                      _copied(sh.rowPtrB, sh.mb + 1), _copied(sh.colIndB, sh.nnzbB), pr.B[bb],
                      None if pr.X is None else pr.X[xb], pr.tolerance, 0)
        sub.first_col, sub.n_cols = sh.firstCol, sh.nCols
    finally:
        lib.tfqmrgpuExt_freeShard(C.byref(sh))
    return sub, xb, bb
