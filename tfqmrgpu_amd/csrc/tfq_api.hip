// C-ABI of libtfQMRgpu.so (include/tfqmrgpu.h, include/tfqmrgpu_ext.h) for MI355X.
// Mirrors the entry points of real-space/tfQMRgpu tfQMRgpu/source/tfqmrgpu.cu (same names,
// argument meaning and status codes); the implementation behind them is this library's own.
// The solve itself -- the tfQMR driver, the refinement, the reset of Plan::last -- is tfq_solve.cpp; the preconditioner's set-up, the state of
// the A in the buffer and the ends of Plan::layout (bufferSize) and Plan::held (bufferSize, setBuffer) are tfq_precond_host.cpp; the calls that
// grade the caller's system (tfqmrgpu_ext.h sections 10 to 13) are tfq_grade_host.cpp; the start projection (section 17) is tfq_project_host.cpp;
// the energy mesh (section 19), its six entry points included, is tfq_mesh_host.cpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include "tfq_solve.hpp"
#include "tfq_precond.hpp"
#include "tfq_order.hpp"
#include "tfq_vec.hpp"
#include "tfq_switch.hpp"
#include "tfq_carry.hpp"
#include "tfq_project.hpp"

using namespace tfq;

namespace tfq {

static inline char lower(char c) { return char(c | 32); }

DevPlan resolve(Plan const& p) {
    DevPlan d{};
    char* b = p.buffer;
    auto at = [&](Window const& w) { return (void*)(b + w.offset); };
    d.LM = p.LM; d.LN = p.LN; d.dbl = ('z' == p.precision);
    d.nCols = p.nCols; d.nnzbX = p.nnzbX; d.nnzbB = p.nnzbB; d.nnzbA = p.nnzbA;
    d.nChunks = uint32_t(p.chunks.col.size());
    static int const hashEnv = lab_switch("TFQMRGPU_HASHV3", 1);
    d.hashV3 = (p.v3IsHash && hashEnv) ? 1 : 0;   // (lab builds, TFQMRGPU_HASHV3=0: the multiply kernels read v3 also in hash mode)
    d.ilv = p.ilv;
    static int const antEnv = lab_switch("TFQMRGPU_A_STREAM", 1);
    d.aOnce = (p.aOnce && antEnv) ? 1 : 0;   // (lab builds, TFQMRGPU_A_STREAM=0: A operands always through the caches)
    d.m3 = p.threeProducts ? 1 : 0;
    d.fold = 0; d.foldCount = (uint32_t*)at(p.wFold); d.self = (DevPlan const*)at(p.wSelf);
    d.R = ('m' == p.precision) ? at(p.wR) : p.warmR;          // (warmR: the R of a warm solve while it runs, tfq_solve.cpp: run_solve_from; null otherwise)
    d.x = at(p.wX); d.v4 = at(p.wV4); d.v5 = at(p.wV5); d.v6 = at(p.wV6); d.v7 = at(p.wV7);
    d.v8 = at(p.wV8); d.v9 = at(p.wV9); d.B = at(p.wB); d.A = at(p.wA); d.v3 = (float*)at(p.wV3);
    d.rho = at(p.wRho); d.alfa = at(p.wAlfa); d.beta = at(p.wBeta); d.c67 = at(p.wC67); d.eta = at(p.wEta);
    d.c67a = at(p.wC67a); d.eta2 = at(p.wEta2);
    d.z = (double*)at(p.wZ); d.d = (double*)at(p.wD); d.tau = (double*)at(p.wTau); d.var = (double*)at(p.wVar);
    d.invBn2 = (double*)at(p.wInvBn2); d.status = (int8_t*)at(p.wStatus); d.ctl = (Ctl*)at(p.wCtl);
    d.pz = (double*)at(p.wPz); d.pd = (double*)at(p.wPd); d.colrec = (double*)at(p.wColRec);
    d.colPart = (double*)at(p.wColPart); d.colSegMax = p.colSegMax;
    d.chunkFirst = (uint32_t*)at(p.wChunkFirst); d.chunkCol = (uint32_t*)at(p.wChunkCol);
    d.colChunkPtr = (uint32_t*)at(p.wColChunkPtr); d.colStart = (uint32_t*)at(p.wColStart);
    d.order = (uint32_t*)at(p.wOrder); d.bOfX = (uint32_t*)at(p.wBofX); d.starts = (uint32_t*)at(p.wStarts); d.pairs = (uint32_t*)at(p.wPairs);
    d.subset = (uint32_t*)at(p.wSubset); d.bColPtr = (uint32_t*)at(p.wBColPtr); d.bList = (uint32_t*)at(p.wBList);
    d.u2i = (uint32_t*)at(p.wU2I); d.rowI = (uint32_t*)at(p.wRowI); d.origCol = (int32_t*)at(p.wOrigCol);
    d.colBatch = p.colBatch.empty() ? nullptr : (uint8_t const*)at(p.wColBatch);
    d.orderB = p.colBatch.empty() ? nullptr : (uint32_t const*)at(p.wOrderB); d.nChunksB = uint32_t(p.chunks.orderB.size());
    return d;
}

// mixed precision: the double-precision side of the plan as a plan of its own (x, B, A in double, element order ilvZ, the chunk
// tables of the float plan) -- what the layout conversions and the refinement's multiply work on
DevPlan resolveZ(Plan const& p) {
    DevPlan d = resolve(p);
    char* b = p.buffer;
    d.dbl = true; d.ilv = p.ilvZ; d.hashV3 = 0; d.R = nullptr;
    d.x = b + p.wXz.offset; d.B = b + p.wBz.offset; d.A = b + p.wAz.offset;
    return d;
}

DevPlan resolve_callers(Plan const& p) { return ('m' == p.precision) ? resolveZ(p) : resolve(p); }

// glibc rand() (TYPE_3 additive feedback generator, seed 1) restated so that the shadow vector of
// the reference CPU path (tfqmrgpu_linalg.hxx:799-802) can be reproduced in any process state
struct GlibcRand {
    uint32_t ring[31];
    int f = 3, b = 0;      // r[i] = r[i-3] + r[i-31]
    explicit GlibcRand(uint32_t seed = 1) {
        int32_t word = int32_t(seed);
        ring[0] = uint32_t(word);
        for (int i = 1; i < 31; ++i) {          // srandom_r: Park-Miller steps fill the state
            int32_t const hi = word / 127773, lo = word % 127773;
            word = 16807 * lo - 2836 * hi;
            if (word < 0) word += 2147483647;
            ring[i] = uint32_t(word);
        }
        for (int i = 0; i < 310; ++i) (void)next();   // srandom_r discards 10*31 outputs
    }
    int32_t next() {
        ring[f] += ring[b];
        uint32_t const out = ring[f] >> 1;
        f = (f + 1) % 31; b = (b + 1) % 31;
        return int32_t(out);
    }
};

// staging area for raw user blocks: the work vectors v4..v9 (free outside of solve)
struct Stage { char* ptr; size_t bytes; };
static Stage stage_of(Plan const& p) {
    return { p.buffer + p.wV4.offset, (p.wV9.offset + p.wV9.bytes) - p.wV4.offset };
}

// move blocks between a host array in the caller's layout and a native device array.  userDbl: precision of the caller's array,
// nativeDbl / ilv: precision and element order of the library's; `also`: a second library-side copy of the same blocks (the float A of a
// mixed-precision plan next to its double A); `list` (device memory): the nBlocks blocks it names, in the caller's block order, instead of all
// blocks 0 ... nBlocks - 1 -- the caller's array is compact, its block k is block list[k] of the operand (setBlocks / getBlocks)
struct Target { void* native; bool dbl; int ilv; };

// is `ptr` memory the GPU can read and write directly (hipMalloc, hipMallocManaged)?  Then setMatrix / getMatrix convert in place
// of the caller's array, no staging and no PCIe: the "same A, new B, solve again" loop of a caller whose B and X live on the
// device (README.md:97-104 of the reference asks for plan reuse; with host arrays X alone is 0.1 s of copies per 35 ms solve on P2).
static bool on_device(void const* ptr) {
    hipPointerAttribute_t a{};
    if (hipSuccess != hipPointerGetAttributes(&a, ptr)) { (void)hipGetLastError(); return false; }   // plain host memory: not an error of the caller
    return hipMemoryTypeDevice == a.type || hipMemoryTypeManaged == a.type || a.isManaged;
}

static tfqmrgpuStatus_t transfer_blocks(Plan& p, hipStream_t s, int direction, bool userDbl, Target const& to,
    void* host, uint32_t const* u2n, uint32_t nBlocks, int nR, int nC, int uR, int uC, int layout, bool trans, bool conj, Stage const* own = nullptr,
    Target const* also = nullptr, uint32_t const* list = nullptr, uint8_t const* unit = nullptr)
{
    // uR x uC: the caller's block shape.  It is the library's nR x nC unless the plan is padded (tfqmrgpu_ext.h section 18): then the
    // two-shape kernels convert (tfq_pad.hip), and `unit` flags the diagonal blocks of A
    bool const oneShape = (uR == nR && uC == nC);
    auto convert = [&](int dir, Target const& t, void* stage, uint32_t first, uint32_t n, uint32_t const* l) {
        if (oneShape) launch_convert(dir, userDbl, t.dbl, t.native, stage, u2n, first, n, nR, nC, layout, trans, conj, t.ilv, s, l);
        else launch_convert_pad(dir, userDbl, t.dbl, t.native, stage, u2n, unit, first, n, nR, nC, uR, uC, layout, trans, conj, t.ilv, s, l);
    };
    if (on_device(host)) {   // the caller's array is device memory: one conversion kernel straight from / into it, asynchronous on the stream
        convert(direction, to, host, 0, nBlocks, list);
        if (also && 0 == direction) convert(0, *also, host, 0, nBlocks, list);
        TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
        return TFQMRGPU_STATUS_SUCCESS;
    }
    Stage const st = own ? *own : stage_of(p);
    size_t const blockBytes = size_t(2) * uR * uC * (userDbl ? 8 : 4);   // the stage is cut by the caller's blocks
    size_t const cap = st.bytes / blockBytes;
    if (cap < 1) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    for (uint32_t first = 0; first < nBlocks; ) {
        uint32_t const n = uint32_t(std::min<size_t>(cap, nBlocks - first));
        char* h = (char*)host + size_t(first) * blockBytes;
        uint32_t const* const l = list ? list + first : nullptr;
        if (0 == direction) {
            TFQ_HIP(hipMemcpyAsync(st.ptr, h, n * blockBytes, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
            convert(0, to, st.ptr, first, n, l);
            if (also) convert(0, *also, st.ptr, first, n, l);
        } else {
            convert(1, to, st.ptr, first, n, l);
            TFQ_HIP(hipMemcpyAsync(h, st.ptr, n * blockBytes, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        }
        // the stage is reused by the next batch and the host array belongs to the caller
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        first += n;
    }
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    return TFQMRGPU_STATUS_SUCCESS;
}

// an X-shaped native vector of the plan (float or double, as the caller's) <-> the caller's array [nnzbX][2][LM][LN] in its own block order
static tfqmrgpuStatus_t transfer_x_vector(Plan& p, DevPlan const& d, hipStream_t s, int direction, bool dbl, void* native, void* user, Stage const* own = nullptr) {
    return transfer_blocks(p, s, direction, dbl, Target{native, dbl, p.ilv}, user, d.u2i, p.nnzbX, p.LM, p.LN, p.LM, p.LN, TFQMRGPU_LAYOUT_RRRRIIII, false, false, own);
}

tfqmrgpuStatus_t upload(void* dst, void const* src, size_t bytes, hipStream_t s) {
    if (0 == bytes || !src) return TFQMRGPU_STATUS_SUCCESS;
    TFQ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    return TFQMRGPU_STATUS_SUCCESS;
}

} // namespace tfq

// ====================================================================================================
extern "C" {

tfqmrgpuStatus_t tfqmrgpu_bsrsv_allowedBlockSizes(int32_t* number, int32_t* blockSizes, int const arrayLength) {
    // reference tfqmrgpu.cu:75-93, including its quirks: the output array is only cleared when
    // *number != 0 on entry, and a pair is stored only while 2*n < arrayLength
    if (nullptr == number) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (nullptr == blockSizes) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (0 != *number) for (int i = 0; i < arrayLength; ++i) blockSizes[i] = 0;
    int n = 0, i = 0;
    for (auto const& sz : kAllowedBlockSizes) {
        ++n;
        if (2 * n < arrayLength) { blockSizes[2 * i] = sz[0]; blockSizes[2 * i + 1] = sz[1]; ++i; }
    }
    *number = n;
    return (n == i) ? TFQMRGPU_STATUS_SUCCESS : TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_blockSizeMissing(int const ldA, int const ldB) {
    // reference tfqmrgpu.cu:95-106: 12 + char=ldA + line=ldB
    return blockSizeAllowed(ldA, ldB) ? 0 : err(TFQMRGPU_BLOCKSIZE_MISSING, ldB, ldA);
}

tfqmrgpuStatus_t tfqmrgpuCreateHandle(tfqmrgpuHandle_t* handle) {       // reference tfqmrgpu.cu:110-115
    if (nullptr == handle)  return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (nullptr != *handle) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    auto h = new (std::nothrow) Handle();
    if (!h) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    *handle = (tfqmrgpuHandle_t)h;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuDestroyHandle(tfqmrgpuHandle_t handle) {       // reference tfqmrgpu.cu:117-121
    if (nullptr == handle) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    auto h = (Handle*)handle;
    if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    delete h;                               // (its device memory goes with it: DevMem)
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuSetStream(tfqmrgpuHandle_t handle, tfqmrgpuStream_t const streamId) { // tfqmrgpu.cu:124-128
    if (nullptr == handle) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    ((Handle*)handle)->stream = (void*)streamId;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuGetStream(tfqmrgpuHandle_t handle, tfqmrgpuStream_t* streamId) {     // tfqmrgpu.cu:130-134
    if (nullptr == handle || nullptr == streamId) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    *streamId = (tfqmrgpuStream_t)((Handle*)handle)->stream;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuCreateWorkspace(void** pBuffer, size_t const bytes, char const memType) { // tfqmrgpu.cu:682-694
    if (nullptr == pBuffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    hipError_t const e = ('m' == lower(memType)) ? hipMallocManaged(pBuffer, bytes) : hipMalloc(pBuffer, bytes);
    return (hipSuccess == e) ? TFQMRGPU_STATUS_SUCCESS : TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
}

tfqmrgpuStatus_t tfqmrgpuDestroyWorkspace(void* pBuffer) {              // tfqmrgpu.cu:696-698 (raw runtime code)
    return (tfqmrgpuStatus_t)hipFree(pBuffer);
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_createPlan(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t* plan, int const mb,
    int32_t const* bsrRowPtrA, int const nnzbA, int32_t const* bsrColIndA,
    int32_t const* bsrRowPtrX, int const nnzbX, int32_t const* bsrColIndX,
    int32_t const* bsrRowPtrB, int const nnzbB, int32_t const* bsrColIndB,
    int const indexOffset, int const echo)
{
    (void)handle;
    if (nullptr == plan)  return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (nullptr != *plan) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);     // tfqmrgpu.cu:161
    auto p = new (std::nothrow) Plan();
    if (!p) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    p->indexOffset = indexOffset;
    tfqmrgpuStatus_t st;
    try {   // no exception may cross the C boundary: a C or Fortran caller would be terminated instead of getting a status
        st = analyse(*p, mb, bsrRowPtrA, nnzbA, bsrColIndA, bsrRowPtrX, nnzbX, bsrColIndX,
                     bsrRowPtrB, nnzbB, bsrColIndB, indexOffset, echo);
    } catch (std::bad_alloc const&) { st = TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    if (st) { delete p; return st; }   // (the reference leaks the plan on its error paths)
    try {   // for the block-Jacobi preconditioner (tfqmrgpu_ext.h section 7): where the diagonal blocks of A are, and the block column of every block
        p->diagOfRow.assign(size_t(mb), ~0u);
        p->colOfA.resize(size_t(nnzbA));
        p->rowOfA.resize(size_t(nnzbA));   // (for the truncation leak, section 11)
        for (int r = 0; r < mb; ++r) {
            for (int32_t q = bsrRowPtrA[r] - indexOffset; q < bsrRowPtrA[r + 1] - indexOffset; ++q) {
                auto const col = uint32_t(bsrColIndA[q] - indexOffset);
                p->colOfA[q] = col;
                p->rowOfA[q] = uint32_t(r);
                if (col == uint32_t(r) && ~0u == p->diagOfRow[r]) p->diagOfRow[r] = uint32_t(q);
            }
        }
    } catch (std::bad_alloc const&) { delete p; return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    *plan = (tfqmrgpuBsrsvPlan_t)p;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_destroyPlan(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan) { // tfqmrgpu.cu:353-361
    (void)handle;
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    p->magic = 0;
    delete p;                               // (every piece of library-owned memory has its owner in the plan: DevMem, PinnedRing)
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_bufferSize(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    int const ldA, int const blockDim, int const ldB, int const RhsBlockDim, char const precision, size_t* pBufferSizeInBytes)
{
    // reference tfqmrgpu.cu:364-412
    // a plan with padding on (tfqmrgpu_ext.h section 18): ldA, ldB are the CALLER's shape, which may have fewer right-hand sides than rows;
    // the plan's shape is picked below, behind the checks, and everything behind the pick sees that shape only
    auto p = asPlan(plan);
    bool const padding = p && p->allowPad;
    int LM = ldA, LN = ldB;
    if (LM != blockDim)    return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (!padding && LM > LN) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (LN != RhsBlockDim) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (!p || !handle) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    char prec;
    switch (lower(precision)) {            // f,c -> c ; m -> m ; everything else -> z  (tfqmrgpu.cu:383-390)
        case 'f': case 'c': prec = 'c'; break;
        case 'm': prec = 'm'; break;
        default:  prec = 'z';
    }
    if (nullptr == pBufferSizeInBytes) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (padding) {
        if (ldA < 1 || ldB < 1) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
        if (!paddedBlockSize(ldA, ldB, LM, LN)) return err(TFQMRGPU_BLOCKSIZE_MISSING, ldB, ldA);   // above 64: with the caller's lm and ln, as without padding
    }
    if (!blockSizeAllowed(LM, LN)) return err(TFQMRGPU_BLOCKSIZE_MISSING, LN, LM); // tfqmrgpu.cu:70
    // 'm': accepted here AND solved (the reference accepts it here and refuses it in solve, tfqmrgpu.cu:42-44, 386): float vectors for
    // the iteration plus x, B and A in double (tfq_plan.cpp: layoutBuffer)
    tfqmrgpuStatus_t st;
    p->lm = ldA; p->ln = ldB;              // the caller's shape, for the operand calls; layoutBuffer and all behind it see (LM, LN)
    try { st = layoutBuffer(*p, LM, LN, prec); }
    catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    a_new_layout(*p);                      // whatever was sized or cut for the previous layout, or held values of its buffer, ends here
    p->precision = prec;
    p->buffer = nullptr;
    *pBufferSizeInBytes = p->bufferBytes;
    return st;
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_setBuffer(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, void* const pBuffer) {
    // reference tfqmrgpu.cu:415-450: register the buffer, create v3, upload the index lists
    if (nullptr == pBuffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);        // bufferSize has not been called
    hipStream_t const s = (hipStream_t)h->stream;
    p->buffer = (char*)pBuffer;
    a_new_buffer(*p);                      // whatever held values of the old buffer, or said what it holds, ends here
    auto at = [&](Window const& w) { return (void*)(p->buffer + w.offset); };
    for (auto const& l : indexLists(*p))   // (tfq_plan.cpp: the windows were sized from the same list)
        if (auto const st = upload(at(*l.window), l.data, l.bytes, s)) return st;
    TFQ_HIP(hipMemsetAsync(at(p->wCtl), 0, p->wCtl.bytes, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipMemsetAsync(at(p->wFold), 0, p->wFold.bytes, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)     // the plan's lists may change (bufferSize) once this call returns
    DevPlan const d = resolve(*p);
    {   // the device-resident copy that the folded column operations read (pointers and sizes only: nothing in it changes with a solve)
        static_assert(sizeof(DevPlan) <= 1024, "window wSelf");
        DevPlan self = d; self.fold = 1;
        TFQ_HIP(hipMemcpyAsync(at(p->wSelf), &self, sizeof self, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    }
    if (TFQMRGPU_SHADOW_GLIBC_RAND == p->shadowMode) {
        size_t const n = size_t(p->nnzbX) * 2 * p->LM * p->LN;
        std::vector<float> v3(n);
        GlibcRand rng(1);
        float const denom = 1. / 2147483647;                            // tfqmrgpu_linalg.hxx:799-801
        for (size_t i = 0; i < n; ++i) v3[i] = rng.next() * denom;
        if (auto const st = transfer_x_vector(*p, d, s, 0, false, d.v3, v3.data())) return st;
        p->v3IsHash = false; p->selfStale = true;
    } else {
        p->v3IsHash = true; p->selfStale = true;
        launch_shadow_hash(d, s);
        if (hipSuccess != hipGetLastError()) return TFQ_ERR(TFQMRGPU_STATUS_RANDOM_GEN_FAILED);
    }
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_getBuffer(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, void** pBuffer) { // tfqmrgpu.cu:453-462
    (void)handle;
    auto p = asPlan(plan);
    if (!p || !pBuffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    *pBuffer = (void*)p->buffer;
    return (nullptr == *pBuffer) ? TFQ_ERR(TFQMRGPU_POINTER_INVALID) : TFQMRGPU_STATUS_SUCCESS;
}

// the layout and transposition arguments of setMatrix / getMatrix (and of setBlocks / getBlocks), checked in the reference's order
static tfqmrgpuStatus_t layout_and_trans(tfqmrgpuDataLayout_t const layout, char const transposition, bool& conj, bool& trans) {
    switch (layout) {
        case TFQMRGPU_LAYOUT_RRRRIIII: case TFQMRGPU_LAYOUT_RIRIRIRI: case TFQMRGPU_LAYOUT_RRIIRRII: break;
        default: return err(TFQMRGPU_DATALAYOUT_UNKNOWN, layout % 10000);          // line field = layout
    }
    conj = false; trans = false;
    char const tr = lower(transposition);   // '*' | 32 == '*'
    switch (tr) {
        case 'h': case 'c': conj = true; trans = true; break;
        case '*': conj = true; break;
        case 't': trans = true; break;
        case 'n': break;
        default: return err(TFQMRGPU_TANSPOSITION_UNKNOWN, __LINE__ % 10000, tr);
    }
    return TFQMRGPU_STATUS_SUCCESS;
}

// an operand of the plan by its name, as far as the argument checks need it (no buffer yet)
struct Operand { int which; uint32_t nnzb; int nC, uC; };   // which: 0 A, 1 B, 2 X; blocks of LM x nC, the caller's (section 18) of lm x uC
static bool operand_of(Plan const& p, char const var, Operand& o) {
    switch (lower(var)) {
        case 'a': o = Operand{0, p.nnzbA, p.LM, p.lm}; return true;
        case 'b': o = Operand{1, p.nnzbB, p.LN, p.ln}; return true;
        case 'x': o = Operand{2, p.nnzbX, p.LN, p.ln}; return true;
        default: return false;
    }
}

// padded plans (tfqmrgpu_ext.h section 18): which blocks of A are diagonal blocks, by the caller's block index, in device memory.  Built
// from the pattern at the first padded transfer of A and uploaded once
static tfqmrgpuStatus_t pad_unit_flags(Plan& p, hipStream_t s) {
    if (p.padUnit) return TFQMRGPU_STATUS_SUCCESS;
    try {
        std::vector<uint8_t> unit(size_t(p.nnzbA), 0);
        for (size_t q = 0; q < unit.size(); ++q) unit[q] = (p.rowOfA[q] == p.colOfA[q]) ? 1 : 0;
        if (auto const st = p.padUnit.reserve(unit.size())) return st;
        // `unit` is a local: wait for the copy.  A copy that failed leaves no flags behind
        if (hipSuccess != hipMemcpyAsync(p.padUnit.ptr, unit.data(), unit.size(), hipMemcpyHostToDevice, s) || hipSuccess != hipStreamSynchronize(s)) {
            p.padUnit.release();
            return TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
        }
    } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    return TFQMRGPU_STATUS_SUCCESS;
}

// setMatrix / getMatrix (reference tfqmrgpu::set_or_getMatrix, tfqmrgpu.cu:467-603) and setBlocks / getBlocks (tfqmrgpu_ext.h section 8)
// are one path.  The whole operand is the case "no list" (listed == false): its blocks 0 ... nnzb - 1.  A listed call names nBlocks blocks
// in `blocks`; getBlocks(blocks == NULL) is a third case: the X blocks on B's pattern, by the plan's own list.  Every check is host code and
// comes before the first device call; the ORDER of the checks is each entry point's own and is pinned by tests
static tfqmrgpuStatus_t operand_transfer(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char const var, bool const listed, int32_t const nListed,
    int32_t const* blocks, void* values, char const precision, char const transposition, tfqmrgpuDataLayout_t const layout, bool const is_get)
{
    bool conj = false, trans = false;
    if (auto const st = layout_and_trans(layout, transposition, conj, trans)) return st;
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (listed && is_get && 'x' != lower(var))   // only X: the status of getMatrix itself (it looks at `var` first)
        return tfqmrgpu_bsrsv_getMatrix(handle, plan, var, values, precision, 0, 0, transposition, layout);
    Operand o{};
    if (!operand_of(*p, var, o)) return err(TFQMRGPU_VARIABLENAME_UNKNOWN, __LINE__ % 10000, var);
    bool const isA = (0 == o.which);
    if (isA) trans = !trans;                     // A is stored transposed (tfqmrgpu.cu:514-517)
    bool const onB = (listed && is_get && nullptr == blocks);   // the X blocks on B's pattern, in B's block order
    uint32_t nBlocks = o.nnzb;
    if (!listed) {
        if (isA && !is_get) a_named(*p);
        if (o.nnzb < 1) return TFQMRGPU_STATUS_SUCCESS;
    } else {
        // the list: every index inside the operand, and no block set twice (the later of two values would win by chance)
        if (onB) { if (nListed < 0 || uint32_t(nListed) != p->nnzbB) return TFQ_ERR(TFQMRGPU_POINTER_INVALID); }
        else if (nListed < 0) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, var);
        if (0 == nListed) return TFQMRGPU_STATUS_SUCCESS;
        nBlocks = uint32_t(nListed);
        if (!onB) {
            if (nullptr == blocks) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
            try {
                std::vector<bool> seen(is_get ? 0 : o.nnzb, false);
                for (int32_t k = 0; k < nListed; ++k) {
                    if (blocks[k] < 0 || uint32_t(blocks[k]) >= o.nnzb) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, var);
                    if (is_get) continue;   // reading a block twice is harmless
                    if (seen[blocks[k]]) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, var);
                    seen[blocks[k]] = true;
                }
            } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
        }
    }
    if (nullptr == p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    bool const mixed = ('m' == p->precision);
    bool const is_double = ('z' == p->precision);
    bool const user_double = ('z' == lower(precision));
    // 'z' plans take double data, every other plan float data (tfqmrgpu.cu:538-542); a mixed-precision plan takes either: its copies of
    // A, B and X are double (A also float), the values are converted on the way
    if (!mixed && user_double != is_double) return err(TFQMRGPU_PRECISION_MISSMATCH, __LINE__ % 10000, precision);
    if (nullptr == values) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    bool intoKept = false;                       // listed blocks of a scaled A: refused, or into the kept copy of the caller's A (section 9)
    if (listed && isA && !is_get) if (auto const st = a_patched(*p, blocks, nListed, intoKept)) return st;

    // where the operand lives: the buffer ('m': its double side, and for A the float copy of the inner solves beside it), or the kept copy
    hipStream_t const s = (hipStream_t)h->stream;
    DevPlan const d = resolve_callers(*p);
    Target to{ isA ? d.A : (1 == o.which) ? d.B : d.x, d.dbl, d.ilv };
    Target floatA{ p->buffer + p->wA.offset, false, p->ilv };
    if (intoKept) { auto const kept = kept_a(*p); to.native = kept.a; floatA.native = kept.aFloat; }
    uint32_t const* u2n = (2 == o.which && !onB) ? d.u2i : nullptr;
    uint32_t const* list = nullptr;
    if (onB) list = d.subset;                    // the plan's own list, which holds NATIVE block indices of X (Plan::subset_i)
    else if (listed) {
        if (auto const st = p->blockList.reserve(size_t(nBlocks) * 4)) return st;
        // stream order keeps this copy behind the launches of an earlier call; the caller's list is free again once the call returns
        TFQ_HIP(hipMemcpyAsync(p->blockList.ptr, blocks, size_t(nBlocks) * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        list = p->blockList.as<uint32_t>();      // (checked: 0 <= blocks[k] < nnzb, so int32 and uint32 read the same)
    }
    uint8_t const* unit = nullptr;               // a padded plan (section 18) puts 1 on the padded diagonal of A's diagonal blocks
    tfqmrgpuStatus_t st = TFQMRGPU_STATUS_SUCCESS;
    if (p->padded() && isA && !is_get) {
        st = pad_unit_flags(*p, s);
        unit = p->padUnit.as<uint8_t>();
    }
    if (!st) st = transfer_blocks(*p, s, is_get ? 1 : 0, user_double, to, values, u2n, nBlocks, p->LM, o.nC, p->lm, o.uC, layout, trans, conj, nullptr,
                                    (mixed && isA && !is_get) ? &floatA : nullptr, list, unit);
    if (!listed && isA && !is_get) a_set_whole(*p, !st);
    if (listed && isA && !is_get && !st) a_patch_written(*p, blocks, nListed);
    return st;
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_setMatrix(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char const var,
    void const* val, char const precision, int const ld, int const d2, char const trans, tfqmrgpuDataLayout_t const layout)
{
    (void)ld; (void)d2;   // ignored by the reference as well (tfqmrgpu.cu:615-616)
    return operand_transfer(handle, plan, var, false, 0, nullptr, (void*)val, precision, trans, layout, false);
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_getMatrix(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char const var,
    void* val, char const precision, int const ld, int const d2, char const trans, tfqmrgpuDataLayout_t const layout)
{
    (void)ld; (void)d2;
    if ('x' != lower(var)) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, var);  // only X (tfqmrgpu.cu:635-643)
    return operand_transfer(handle, plan, var, false, 0, nullptr, val, precision, trans, layout, true);
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_solve(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double const threshold, int const maxIterations) {
    auto p = asPlan(plan); auto h = (Handle*)handle;                    // tfqmrgpu.cu:648-661
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return run_solve(*h, *p, threshold, maxIterations);
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_getInfo(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double* residuum_reached, int32_t* iterations_needed, double* flops_performed, double* flops_performed_all)
{
    (void)handle;                                                        // tfqmrgpu.cu:663-679
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    int any = 0;
    if (residuum_reached)    { ++any; *residuum_reached = p->residuum_reached; }
    if (iterations_needed)   { ++any; *iterations_needed = p->last.iterations_needed; }
    if (flops_performed)     { ++any; *flops_performed = p->last.flops_performed; }
    if (flops_performed_all) { ++any; *flops_performed_all = p->flops_performed_all; }
    return any ? TFQMRGPU_STATUS_SUCCESS : TFQMRGPU_STATUS_NO_INFO_PASSED;
}

} // extern "C"

// one-call drivers, reference tfqmrgpu.cu:702-821
template <typename real_t>
static tfqmrgpuStatus_t bsrsv_onecall(int mb, int ldA, int ldB,
    int32_t const* rowPtrA, int nnzbA, int32_t const* colIndA, real_t const* Amat, char transA,
    int32_t const* rowPtrX, int nnzbX, int32_t const* colIndX, real_t* Xmat, char transX,
    int32_t const* rowPtrB, int nnzbB, int32_t const* colIndB, real_t const* Bmat, char transB,
    int32_t* iterations, float* residual, int indexOffset, int echo)
{
    char const zoc = (sizeof(real_t) == 8) ? 'z' : 'c';
    char const* const me = (zoc == 'z') ? "tfqmrgpu_bsrsv_z" : "tfqmrgpu_bsrsv_c";
    tfqmrgpuStatus_t stat;
    tfqmrgpuHandle_t handle = nullptr;
    tfqmrgpuBsrsvPlan_t plan = nullptr;
    void* buffer = nullptr;
    size_t bytes = 0;
    auto cleanup = [&]() {      // (the reference returns early and leaks on errors)
        if (buffer) tfqmrgpuDestroyWorkspace(buffer);
        if (plan) tfqmrgpu_bsrsv_destroyPlan(handle, plan);
        if (handle) tfqmrgpuDestroyHandle(handle);
    };
#define TFQ_STEP(call, name) stat = (call); if (stat) { if (echo > 0) std::printf("# %s: %s returned %d\n", me, name, stat); cleanup(); return stat; }
    if (echo > 0) std::printf("# %s: mb= %d, ldA= %d, ldB= %d, iterations= %d, residual= %.1e\n", me, mb, ldA, ldB,
                              iterations ? *iterations : 200, residual ? *residual : 1e-9);
    TFQ_STEP(tfqmrgpuCreateHandle(&handle), "tfqmrgpuCreateHandle")
    TFQ_STEP(tfqmrgpuSetStream(handle, 0), "tfqmrgpuSetStream")
    TFQ_STEP(tfqmrgpu_bsrsv_createPlan(handle, &plan, mb, rowPtrA, nnzbA, colIndA, rowPtrX, nnzbX, colIndX,
                                       rowPtrB, nnzbB, colIndB, indexOffset, echo), "tfqmrgpu_bsrsv_createPlan")
    TFQ_STEP(tfqmrgpu_bsrsv_bufferSize(handle, plan, ldA, ldA, ldB, ldB, zoc, &bytes), "tfqmrgpu_bsrsv_bufferSize")
    TFQ_STEP(tfqmrgpuCreateWorkspace(&buffer, bytes, 'd'), "tfqmrgpuCreateWorkspace")
    TFQ_STEP(tfqmrgpu_bsrsv_setBuffer(handle, plan, buffer), "tfqmrgpu_bsrsv_setBuffer")
    TFQ_STEP(tfqmrgpu_bsrsv_setMatrix(handle, plan, 'A', Amat, zoc, ldA, ldA, transA, TFQMRGPU_LAYOUT_RIRIRIRI), "tfqmrgpu_bsrsv_setMatrix('A')")
    TFQ_STEP(tfqmrgpu_bsrsv_setMatrix(handle, plan, 'B', Bmat, zoc, ldB, ldA, transB, TFQMRGPU_LAYOUT_RIRIRIRI), "tfqmrgpu_bsrsv_setMatrix('B')")
    double const threshold = residual ? *residual : 1e-9;
    int const maxiter = iterations ? *iterations : 200;
    TFQ_STEP(tfqmrgpu_bsrsv_solve(handle, plan, threshold, maxiter), "tfqmrgpu_bsrsv_solve")
    double residuum = 0, flops = 0, flops_all = 0; int32_t needed = 0;
    TFQ_STEP(tfqmrgpu_bsrsv_getInfo(handle, plan, &residuum, &needed, &flops, &flops_all), "tfqmrgpu_bsrsv_getInfo")
    if (echo > 1) std::printf("# tfQMRgpu needed %d iterations to converge to %.1e using %g GFlop\n", needed, residuum, flops * 1e-9);
    if (residual) *residual = float(residuum);
    if (iterations) *iterations = needed;
    TFQ_STEP(tfqmrgpu_bsrsv_getMatrix(handle, plan, 'X', Xmat, zoc, ldB, ldA, transX, TFQMRGPU_LAYOUT_RIRIRIRI), "tfqmrgpu_bsrsv_getMatrix")
#undef TFQ_STEP
    cleanup();
    return TFQMRGPU_STATUS_SUCCESS;
}

extern "C" {

tfqmrgpuStatus_t tfqmrgpu_bsrsv_z(int mb, int ldA, int ldB,
    int32_t const* rowPtrA, int nnzbA, int32_t const* colIndA, double const* Amat, char transA,
    int32_t const* rowPtrX, int nnzbX, int32_t const* colIndX, double* Xmat, char transX,
    int32_t const* rowPtrB, int nnzbB, int32_t const* colIndB, double const* Bmat, char transB,
    int32_t* iterations, float* residual, int indexOffset, int echo)
{
    return bsrsv_onecall<double>(mb, ldA, ldB, rowPtrA, nnzbA, colIndA, Amat, transA, rowPtrX, nnzbX, colIndX, Xmat, transX,
                                 rowPtrB, nnzbB, colIndB, Bmat, transB, iterations, residual, indexOffset, echo);
}

tfqmrgpuStatus_t tfqmrgpu_bsrsv_c(int mb, int ldA, int ldB,
    int32_t const* rowPtrA, int nnzbA, int32_t const* colIndA, float const* Amat, char transA,
    int32_t const* rowPtrX, int nnzbX, int32_t const* colIndX, float* Xmat, char transX,
    int32_t const* rowPtrB, int nnzbB, int32_t const* colIndB, float const* Bmat, char transB,
    int32_t* iterations, float* residual, int indexOffset, int echo)
{
    return bsrsv_onecall<float>(mb, ldA, ldB, rowPtrA, nnzbA, colIndA, Amat, transA, rowPtrX, nnzbX, colIndX, Xmat, transX,
                                rowPtrB, nnzbB, colIndB, Bmat, transB, iterations, residual, indexOffset, echo);
}

// ---- extensions (include/tfqmrgpu_ext.h) --------------------------------------------------------------

// the three views of a solve's profile: all launches that did work, those that returned at once, those of the first iteration
static tfqmrgpuStatus_t get_profile(tfqmrgpuBsrsvPlan_t plan, Plan::Profile const Plan::Last::*view, int64_t* launches, double* milliseconds) {
    auto p = asPlan(plan);
    if (!p || !launches || !milliseconds) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    auto const& v = p->last.*view;
    for (int k = 0; k < TFQMRGPU_PROFILE_CLASSES; ++k) { launches[k] = v.launches[k]; milliseconds[k] = v.ms[k]; }
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_planView(tfqmrgpuBsrsvPlan_t plan, tfqmrgpuPlanView_t* v) {
    auto p = asPlan(plan);
    if (!p || !v) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    v->nRows = p->nRows; v->nCols = p->nCols; v->nnzbA = p->nnzbA; v->nnzbX = p->nnzbX; v->nnzbB = p->nnzbB;
    v->nPairs = p->nPairs();
    v->pairs = p->pairs.data(); v->starts = p->starts.data(); v->subset = p->subset.data();
    v->colindx = p->colindx.data(); v->original_bsrColIndX = p->original_bsrColIndX.data();
    v->LM = p->LM; v->LN = p->LN; v->precision = p->precision;
    return TFQMRGPU_STATUS_SUCCESS;
}

int32_t tfqmrgpuExt_getBoundHistory(tfqmrgpuBsrsvPlan_t plan, double* bound2, int32_t capacity) {
    auto p = asPlan(plan);
    if (!p) return -1;
    auto const n = int32_t(p->last.boundHistory.size());
    for (int32_t i = 0; i < std::min(n, capacity); ++i) if (bound2) bound2[i] = p->last.boundHistory[i];
    return n;
}

tfqmrgpuStatus_t tfqmrgpuExt_setProfiling(tfqmrgpuBsrsvPlan_t plan, int on) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    p->profiling = (on < 0 || on > 2) ? 1 : on;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_getProfile(tfqmrgpuBsrsvPlan_t plan, int64_t* launches, double* milliseconds) {
    return get_profile(plan, &Plan::Last::all, launches, milliseconds);
}

tfqmrgpuStatus_t tfqmrgpuExt_getProfileGated(tfqmrgpuBsrsvPlan_t plan, int64_t* launches, double* milliseconds) {
    return get_profile(plan, &Plan::Last::gated, launches, milliseconds);
}

tfqmrgpuStatus_t tfqmrgpuExt_getProfileFirst(tfqmrgpuBsrsvPlan_t plan, int64_t* launches, double* milliseconds) {
    return get_profile(plan, &Plan::Last::first, launches, milliseconds);
}

tfqmrgpuStatus_t tfqmrgpuExt_getMultiplyKernel(tfqmrgpuBsrsvPlan_t plan, char* name, int32_t capacity) {
    auto p = asPlan(plan);
    if (!p || !name || capacity < 1) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (!p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    DevPlan d = resolve(*p);
    d.fold = folds(*p, false) ? 1 : 0;            // what run_tfqmr decides on one rank (a plan has no handle, and no ranks, of its own)
    std::snprintf(name, size_t(capacity), "%s", spmm_kernel_family(d));
    return TFQMRGPU_STATUS_SUCCESS;
}
tfqmrgpuStatus_t tfqmrgpuExt_getLateV5(tfqmrgpuBsrsvPlan_t plan, int32_t* on) {
    auto p = asPlan(plan);
    if (!p || !on || !p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    DevPlan d = resolve(*p);
    d.fold = folds(*p, false) ? 1 : 0;            // one rank, as tfqmrgpuExt_getMultiplyKernel
    *on = late_v5(*p, d) ? 1 : 0;
    return TFQMRGPU_STATUS_SUCCESS;
}
tfqmrgpuStatus_t tfqmrgpuExt_setThreeProductMultiply(tfqmrgpuBsrsvPlan_t plan, int on) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    p->threeProducts = (0 != on); p->selfStale = true;
    return TFQMRGPU_STATUS_SUCCESS;
}

int32_t tfqmrgpuExt_getRefinementHistory(tfqmrgpuBsrsvPlan_t plan, double* residual, int32_t* iterations, int32_t capacity) {
    auto p = asPlan(plan);
    if (!p) return -1;
    auto const n = int32_t(p->last.cycleResidual.size());
    for (int32_t i = 0; i < std::min(n, capacity); ++i) {
        if (residual) residual[i] = p->last.cycleResidual[i];
        if (iterations) iterations[i] = (size_t(i) < p->last.cycleIterations.size()) ? p->last.cycleIterations[i] : 0;   // the last entry has no solve behind it
    }
    return n;
}

tfqmrgpuStatus_t tfqmrgpuExt_setShadowMode(tfqmrgpuBsrsvPlan_t plan, int mode) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (mode != TFQMRGPU_SHADOW_HASH && mode != TFQMRGPU_SHADOW_GLIBC_RAND) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    p->shadowMode = mode;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_setShadowVector(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, float const* v3) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h || !v3 || !p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    DevPlan const d = resolve(*p);
    p->v3IsHash = false; p->selfStale = true;
    return transfer_x_vector(*p, d, (hipStream_t)h->stream, 0, false, d.v3, (void*)v3);
}

tfqmrgpuStatus_t tfqmrgpuExt_getShadowVector(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, float* v3) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h || !v3 || !p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    DevPlan const d = resolve(*p);
    return transfer_x_vector(*p, d, (hipStream_t)h->stream, 1, false, d.v3, (void*)v3);
}

tfqmrgpuStatus_t tfqmrgpuExt_getWorkVector(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int which, void* values) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h || !values || !p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if ('z' != p->precision && 'c' != p->precision) return err(TFQMRGPU_PRECISION_MISSMATCH, __LINE__ % 10000, p->precision);
    DevPlan const d = resolve(*p);
    void* v = nullptr;
    switch (which) {
        case 1: v = d.x; break;  case 4: v = d.v4; break;  case 5: v = d.v5; break;  case 6: v = d.v6; break;
        case 7: v = d.v7; break; case 8: v = d.v8; break;  case 9: v = d.v9; break;
        default: return err(TFQMRGPU_VARIABLENAME_UNKNOWN, __LINE__ % 10000, char('0' + (which & 7)));
    }
    // the usual staging area IS the work vectors: this getter brings its own
    DevMem mem;
    size_t const bytes = std::max(std::min<size_t>(p->S, size_t(64) << 20), size_t(2) * p->LM * p->LN * ('z' == p->precision ? 8 : 4));
    if (auto const st = mem.reserve(bytes)) return st;
    Stage const stage{mem.as<char>(), bytes};
    return transfer_x_vector(*p, d, (hipStream_t)h->stream, 1, 'z' == p->precision, v, values, &stage);
}

// ---- prepared launch order of the stand-alone multiply (tfq_order.cpp) -----------------------------------------------------------
namespace { struct MultiplyOrder { uint32_t magic = 0x6f726472u; uint32_t nY = 0; DevMem perm; }; }

tfqmrgpuStatus_t tfqmrgpuExt_multiplyPrepare(tfqmrgpuHandle_t handle, char precision, int lm, int ln, uint32_t nnzbY,
    uint32_t const* starts_d, uint32_t const* pairs_d, int mode, void** order)
{
    auto h = (Handle*)handle;
    if (!h || !starts_d || !pairs_d || !order) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    *order = nullptr;
    if (!multiply_shape_allowed(precision, lm, ln)) return err(TFQMRGPU_BLOCKSIZE_MISSING, ln, lm);
    uint32_t const ch = multiply_blocks_per_work_group(precision, lm, ln);
    if (0 == ch || 0 == nnzbY || mode <= 0) return TFQMRGPU_STATUS_SUCCESS;      // nothing to prepare: a null order is the caller's order
    hipStream_t const s = (hipStream_t)h->stream;
    try {
        std::vector<uint32_t> starts(size_t(nnzbY) + 1);
        TFQ_HIP(hipMemcpyAsync(starts.data(), starts_d, starts.size() * 4, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        std::vector<uint32_t> pairs(size_t(starts[nnzbY]) * 2);
        TFQ_HIP(hipMemcpyAsync(pairs.data(), pairs_d, pairs.size() * 4, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        for (uint32_t y = 0; y < nnzbY; ++y) if (starts[y + 1] < starts[y]) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
        auto const perm = multiply_order(nnzbY, starts.data(), pairs.data(), ch, mode, uint32_t(lm * lm), uint32_t(lm * ln));
        std::unique_ptr<MultiplyOrder> o(new MultiplyOrder);
        o->nY = nnzbY;
        if (auto const st = o->perm.reserve(size_t(nnzbY) * 4)) return st;
        TFQ_HIP(hipMemcpyAsync(o->perm.ptr, perm.data(), size_t(nnzbY) * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        *order = o.release();
    } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_multiplyRelease(void* order) {
    auto o = (MultiplyOrder*)order;
    if (!o) return TFQMRGPU_STATUS_SUCCESS;
    if (o->magic != 0x6f726472u) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    o->magic = 0; delete o;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_multiplyOrdered(tfqmrgpuHandle_t handle, char precision, int lm, int ln,
    uint32_t nnzbY, uint32_t const* starts_d, uint32_t const* pairs_d, void const* A_d, void const* X_d, void* Y_d, void const* order)
{
    auto h = (Handle*)handle;
    if (!h || !starts_d || !pairs_d || !A_d || !X_d || !Y_d) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    auto o = (MultiplyOrder const*)order;
    if (o && (o->magic != 0x6f726472u || o->nY != nnzbY)) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);   // an order belongs to ONE listing
    return launch_multiply(precision, lm, ln, nnzbY, starts_d, pairs_d, A_d, X_d, Y_d, (hipStream_t)h->stream, o ? o->perm.as<uint32_t>() : nullptr);
}

tfqmrgpuStatus_t tfqmrgpuExt_multiply(tfqmrgpuHandle_t handle, char precision, int lm, int ln,
    uint32_t nnzbY, uint32_t const* starts_d, uint32_t const* pairs_d, void const* A_d, void const* X_d, void* Y_d)
{
    auto h = (Handle*)handle;
    if (!h || !starts_d || !pairs_d || !A_d || !X_d || !Y_d) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return launch_multiply(precision, lm, ln, nnzbY, starts_d, pairs_d, A_d, X_d, Y_d, (hipStream_t)h->stream);
}

tfqmrgpuStatus_t tfqmrgpuExt_applyOperator(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int repetitions) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h || !p->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (p->opFn) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);       // a user-defined operator is the caller's to apply
    hipStream_t const s = (hipStream_t)h->stream;
    bool const mixed = ('m' == p->precision);
    DevPlan const d = resolve_callers(*p);                          // mixed: the double side (x, A), the product in v4 ... v7
    void* const y = mixed ? d.v4 : d.v9;                            // the work vectors are free outside of a solve
    for (int r = 0; r < std::max(1, std::abs(repetitions)); ++r) spmm_apply(d, d.x, y, s);
    // repetitions < 0: |repetitions| launches and nothing else (timing: X stays as it is, the product is left in the work vector)
    if (repetitions >= 0) TFQ_HIP(hipMemcpyAsync(d.x, y, mixed ? p->wXz.bytes : p->S, hipMemcpyDeviceToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- warm start: solve from the X in the plan (tfqmrgpu_ext.h section 14) ------------------------------------------------------------
tfqmrgpuStatus_t tfqmrgpuExt_solveFrom(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double const threshold, int const maxIterations) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);    // bufferSize has not been called
    // the order of section 10, with the precision between the operator and A: no buffer | user-defined operator | 'm' | A never set | A scaled and not kept
    tfqmrgpuStatus_t early = operands_ready(*p, false);
    if (!early && 'm' == p->precision) early = TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);   // run_mixed has its own cycle 0 and |b|^2: tfqmrgpuExt_refineFrom
    if (!early) early = operands_ready(*p, true);
    void const* const a = early ? nullptr : callers_a(*p, resolve(*p));
    return run_solve_from(*h, *p, threshold, maxIterations, a, early);
}

// ---- mixed-precision warm start: refine from the X in the plan (tfqmrgpu_ext.h section 16) ---------------------------------------------
tfqmrgpuStatus_t tfqmrgpuExt_refineFrom(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double const threshold, int const maxIterations) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);    // bufferSize has not been called
    if ('m' != p->precision) return tfqmrgpuExt_solveFrom(handle, plan, threshold, maxIterations);   // 'z', 'c': section 14, call for call
    // the order of section 14 without its precision check: no buffer | user-defined operator | A never set | A scaled and not kept
    tfqmrgpuStatus_t const early = operands_ready(*p, true);
    void const* const a = early ? nullptr : callers_a(*p, resolveZ(*p));   // the double A: the buffer's, or the double part of the kept copy
    return run_refine_from(*h, *p, threshold, maxIterations, a, early);
}

// ---- start projection: blend the kept solutions per right-hand side (tfqmrgpu_ext.h section 17; tfq_project_host.cpp) ------------------------
tfqmrgpuStatus_t tfqmrgpuExt_keepStarts(tfqmrgpuBsrsvPlan_t plan, int const depth) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return starts_keep(*p, depth);
}

tfqmrgpuStatus_t tfqmrgpuExt_pushStart(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return starts_push(*h, *p);
}

int32_t tfqmrgpuExt_startCount(tfqmrgpuBsrsvPlan_t plan) {
    auto p = asPlan(plan);
    return p ? p->held.startCount : 0;
}

int32_t tfqmrgpuExt_startDepth(tfqmrgpuBsrsvPlan_t plan) {
    auto p = asPlan(plan);
    return p ? p->startDepth : 0;
}

tfqmrgpuStatus_t tfqmrgpuExt_projectStart(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double* coefficients, int32_t* nUsed) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return starts_project(*h, *p, coefficients, nUsed);
}

tfqmrgpuStatus_t tfqmrgpuExt_commUniqueId(char id[128]) {
    if (!id) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (!g_rccl.load()) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    return g_rccl.GetUniqueId(id) ? TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED) : TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_commInit(tfqmrgpuHandle_t handle, int nranks, int rank, char const id[128]) {
    auto h = (Handle*)handle;
    if (!h || !id) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (!g_rccl.load()) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    UidByValue u; std::memcpy(u.internal, id, 128);
    void* comm = nullptr;
    if (g_rccl.CommInitRank(&comm, nranks, u, rank)) return TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
    h->comm = comm; h->nranks = nranks; h->rank = rank;
    return ensure_vote_buffer(*h);   // for the vote in front of every solve
}

tfqmrgpuStatus_t tfqmrgpuExt_commDestroy(tfqmrgpuHandle_t handle) {
    auto h = (Handle*)handle;
    if (!h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    h->comm = nullptr; h->nranks = 1; h->rank = 0;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_setOperator(tfqmrgpuBsrsvPlan_t plan, tfqmrgpuOperator_t multiply, void* ctx) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    p->opFn = (void*)multiply; p->opCtx = ctx;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_setPreconditioner(tfqmrgpuBsrsvPlan_t plan, int kind) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (TFQMRGPU_PRECOND_NONE != kind && TFQMRGPU_PRECOND_BLOCK_JACOBI != kind) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    p->precondKind = kind;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_keepOperator(tfqmrgpuBsrsvPlan_t plan, int on) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return a_keep(*p, 0 != on);
}

tfqmrgpuStatus_t tfqmrgpuExt_getPreconditioner(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, void* Minv, int32_t* nIdentity) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (TFQMRGPU_PRECOND_BLOCK_JACOBI != p->precondKind) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);
    if (auto const st = precond_prepare(*h, *p)) return st;   // (the first solve after setMatrix('A') would do the same)
    if (Minv) {
        auto const m = precond_mem(*p);
        hipStream_t const s = (hipStream_t)h->stream;
        TFQ_HIP(hipMemcpyAsync(Minv, m.minv, m.minvBytes, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    }
    if (nIdentity) *nIdentity = p->precondIdentity;
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- listed blocks (tfqmrgpu_ext.h section 8): operand_transfer with a list ----------------------------------------------------------
tfqmrgpuStatus_t tfqmrgpuExt_setBlocks(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char const var,
    int32_t const nBlocks, int32_t const* blocks, void const* values, char const precision, char const trans, tfqmrgpuDataLayout_t const layout)
{
    return operand_transfer(handle, plan, var, true, nBlocks, blocks, (void*)values, precision, trans, layout, false);
}

tfqmrgpuStatus_t tfqmrgpuExt_getBlocks(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char const var,
    int32_t const nBlocks, int32_t const* blocks, void* values, char const precision, char const trans, tfqmrgpuDataLayout_t const layout)
{
    return operand_transfer(handle, plan, var, true, nBlocks, blocks, values, precision, trans, layout, true);
}

// ---- carry an operand from one plan to another, device to device (tfqmrgpu_ext.h section 15) ---------------------------------------------
// The checks and the composed list are host code (tfq_carry_host.cpp), the copy is one launch of k_carry (tfq_carry.hip) over the
// destination window -- two for the A of an 'm' destination, which keeps a double and a float copy.  What the call does to the
// destination plan is what a whole setMatrix(var) does
tfqmrgpuStatus_t tfqmrgpuExt_carry(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t dst, tfqmrgpuBsrsvPlan_t src, char const var,
    int32_t const nBlocks, int32_t const* oldBlock)
{
    auto d = asPlan(dst); auto sp = asPlan(src); auto h = (Handle*)handle;
    if (!h || !d || !sp || d == sp) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == d->LM || 0 == sp->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);   // bufferSize has not been called
    Operand od{}, os{};
    if (!operand_of(*d, var, od) || !operand_of(*sp, var, os)) return err(TFQMRGPU_VARIABLENAME_UNKNOWN, __LINE__ % 10000, var);
    // (padded plans, section 18: the callers' shapes as well)
    if (d->LM != sp->LM || d->LN != sp->LN || d->lm != sp->lm || d->ln != sp->ln) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'L');
    if (!carry_map_ok(nBlocks, oldBlock, od.nnzb, os.nnzb)) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, var);
    if (0 == od.nnzb) return TFQMRGPU_STATUS_SUCCESS;               // nothing to carry: nothing is touched
    if (nullptr == d->buffer || nullptr == sp->buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    bool const isA = (0 == od.which), isX = (2 == od.which);
    if (isA) if (auto const st = operands_ready(*sp, true)) return st;   // the source checks of section 10, in its order

    // the list in the stored block orders: X-shaped vectors lie in each plan's internal order, A and B in the caller's.  A and B without a
    // list are the identity there too and need no list on the device
    hipStream_t const s = (hipStream_t)h->stream;
    uint32_t const* list = nullptr;
    if (oldBlock || isX) {
        std::vector<uint32_t> composed;
        try { carry_compose(composed, od.nnzb, oldBlock, isX ? d->i2u.data() : nullptr, isX ? sp->u2i.data() : nullptr); }
        catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
        if (auto const st = d->carryList.reserve(composed.size() * 4)) return st;
        // stream order keeps this copy behind the launches of an earlier call; `composed` is a local: wait for the copy
        TFQ_HIP(hipMemcpyAsync(d->carryList.ptr, composed.data(), composed.size() * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        list = d->carryList.as<uint32_t>();
    }

    // where the operand lives on either side: the buffer ('m': its double side), for the source A the caller's A (callers_a)
    bool const dMixed = ('m' == d->precision);
    DevPlan const dd = resolve_callers(*d);
    DevPlan const ds = resolve_callers(*sp);
    CarrySide const from{ isA ? const_cast<void*>(callers_a(*sp, ds)) : isX ? ds.x : ds.B, ds.dbl, ds.ilv };
    CarrySide const to{ isA ? dd.A : isX ? dd.x : dd.B, dd.dbl, dd.ilv };
    if (isA) a_named(*d);
    bool ok = carry_launch(to, from, list, od.nnzb, d->LM, od.nC, s);
    if (ok && isA && dMixed) ok = carry_launch(CarrySide{d->buffer + d->wA.offset, false, d->ilv}, from, list, od.nnzb, d->LM, od.nC, s);   // the float A of the inner solves
    tfqmrgpuStatus_t st = ok ? TFQMRGPU_STATUS_SUCCESS : TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    if (ok && hipSuccess != hipGetLastError()) st = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
    if (isA) a_set_whole(*d, !st);
    return st;
}

// ---- padded plans: any block shape up to 64 x 64 on the listed kernels (tfqmrgpu_ext.h section 18) -------------------------------------------
// The switch is read by bufferSize, which picks the plan's shape (tfq_plan.cpp: paddedBlockSize); the operand calls then convert between the
// caller's shape and the plan's (operand_transfer, tfq_pad.hip).  Nothing else knows of it
tfqmrgpuStatus_t tfqmrgpuExt_allowPadding(tfqmrgpuBsrsvPlan_t plan, int on) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    p->allowPad = (0 != on);
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_paddedShape(tfqmrgpuBsrsvPlan_t plan, int32_t* lm, int32_t* ln, int32_t* LM, int32_t* LN) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);    // bufferSize has not been called
    if (lm) *lm = p->lm;
    if (ln) *ln = p->ln;
    if (LM) *LM = p->LM;
    if (LN) *LN = p->LN;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_setReduceCallback(tfqmrgpuHandle_t handle, tfqmrgpuReduceMax_t fn, void* ctx) {
    auto h = (Handle*)handle;
    if (!h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    h->reduceFn = fn; h->reduceCtx = ctx;
    return fn ? ensure_vote_buffer(*h) : TFQMRGPU_STATUS_SUCCESS;
}

} // extern "C"
