// Energy mesh (tfqmrgpu_ext.h section 19), host side: shiftDiagonal -- its checks in front of the first device call, the captured diagonal
// of the caller's A, the launches of tfq_mesh.hip on every copy of A that setBlocks('A') would write --, the weighted sum of X on B's pattern,
// and solveMesh, the energy loop written once with the library's own public calls.  The library-owned device memory of all of it stands in
// Plan::held: it holds values of one buffer and ends with it.
#include <algorithm>
#include <new>
#include <vector>

#include "tfq_solve.hpp"
#include "tfq_precond.hpp"
#include "tfq_mesh.hpp"

namespace tfq {

// ---- 19a: A := A_base + sigma 1 -----------------------------------------------------------------------------------------------------------
tfqmrgpuStatus_t mesh_shift(Handle& h, Plan& p, double const sigmaRe, double const sigmaIm) {
    if (0 == p.LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);     // bufferSize has not been called
    if (p.opFn) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);         // a user-defined operator has no blocks to shift
    if (nullptr == p.buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (!p.held.haveA) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'A');
    uint32_t const mb = uint32_t(p.diagOfRow.size());
    for (uint32_t r = 0; r < mb; ++r)                               // A + sigma 1 has a diagonal block in every block row
        if (~0u == p.diagOfRow[r]) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'D');
    if (uint64_t(mb) * uint32_t(p.lm) > 0xffffffffull) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    if (0 == mb) return TFQMRGPU_STATUS_SUCCESS;

    // the last check, that of setBlocks('A') (a_patched makes it again): A M^-1 cannot be patched unless the plan keeps the caller's A
    bool intoKept = kept_is_callers_a(p);
    if (TFQMRGPU_PRECOND_NONE != p.held.precondInA && !intoKept) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);

    // everything that can fail for want of memory, or on its way to the device, comes before the first change of the plan's state or of A
    hipStream_t const s = (hipStream_t)h.stream;
    bool const mixed = ('m' == p.precision);
    DevPlan const d = resolve_callers(p);                           // 'm': the double side
    uint32_t const* diagDev = nullptr;                              // diagOfRow on the device: the preconditioner's copy where there is one
    if (p.layout.precond) diagDev = precond_mem(p).diag;
    else {
        if (!p.held.shiftDiag) {
            if (auto const st = p.held.shiftDiag.reserve(size_t(mb) * 4)) return st;
            if (hipSuccess != hipMemcpyAsync(p.held.shiftDiag.ptr, p.diagOfRow.data(), size_t(mb) * 4, hipMemcpyHostToDevice, s)) {
                p.held.shiftDiag.release();
                return TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
            }
        }
        diagDev = p.held.shiftDiag.as<uint32_t>();
    }
    if (!p.held.shiftBase) p.held.shiftBaseFresh = false;           // (no base, nothing fresh)
    if (auto const st = p.held.shiftBase.reserve(size_t(mb) * p.LM * 2 * (d.dbl ? 8 : 4))) return st;
    uint32_t nStale = 0;                                            // rows whose diagonal block setBlocks('A') has written since the capture
    std::vector<int32_t> diag;
    try {
        diag.assign(p.diagOfRow.begin(), p.diagOfRow.end());
        p.held.shiftStaleRow.resize(mb, uint8_t(0));                // (the flags exist from the first capture on: a_patch_written)
        if (p.held.shiftBaseFresh && p.held.shiftAnyStale) {
            std::vector<uint32_t> rows;
            for (uint32_t r = 0; r < mb; ++r) if (p.held.shiftStaleRow[r]) rows.push_back(r);
            nStale = uint32_t(rows.size());
            if (auto const st = p.held.shiftRows.reserve(size_t(mb) * 4)) return st;
            // stream order keeps this copy behind the launches of an earlier call; `rows` is a local: wait for the copy
            TFQ_HIP(hipMemcpyAsync(p.held.shiftRows.ptr, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
            TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        }
    } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }

    // the state effects of setBlocks('A') naming every diagonal block, through its own transition: the float floor goes; on a kept plan
    // every block row and column with a diagonal block is marked for the next set-up; haveA stays.  (What it can still refuse is its own
    // host memory, in front of its first mark.)  The captured base is not its business: a shift leaves it as it is
    if (auto const st = a_patched(p, diag.data(), int32_t(mb), intoKept)) return st;

    // where the caller's A lives: the buffer, or the kept copy while the buffer holds A M^-1 ('m': the float A of the inner solves beside it)
    auto const kept = intoKept ? kept_a(p) : KeptA{};
    DiagSide const a{ intoKept ? (void*)kept.a : d.A, d.dbl, d.ilv };
    if (!p.held.shiftBaseFresh) {                                   // behind a whole new A, which carries no shift: every row
        diag_capture_launch(a, p.held.shiftBase.ptr, diagDev, nullptr, mb, p.LM, p.lm, s);
        p.held.shiftBaseFresh = true;
    } else if (nStale) {                                            // the rows that setBlocks('A') has written, from the blocks it wrote; the others
        diag_capture_launch(a, p.held.shiftBase.ptr, diagDev, p.held.shiftRows.as<uint32_t>(), nStale, p.LM, p.lm, s);   // carry the last shift
    }
    std::fill(p.held.shiftStaleRow.begin(), p.held.shiftStaleRow.end(), uint8_t(0)); p.held.shiftAnyStale = false;
    diag_shift_launch(a, p.held.shiftBase.ptr, d.dbl, diagDev, mb, p.LM, p.lm, sigmaRe, sigmaIm, s);
    if (mixed) {
        DiagSide const aFloat{ intoKept ? (void*)kept.aFloat : (void*)(p.buffer + p.wA.offset), false, p.ilv };
        diag_shift_launch(aFloat, p.held.shiftBase.ptr, true, diagDev, mb, p.LM, p.lm, sigmaRe, sigmaIm, s);
    }
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- 19b: S += w X on the blocks of X that carry a block of B ------------------------------------------------------------------------------
namespace {
size_t sum_doubles(Plan const& p) { return size_t(p.nnzbB) * p.LM * p.LN * 2; }
// what the three calls with a handle check first, in the order of pushStart
tfqmrgpuStatus_t sum_ready(Plan const& p) {
    if (0 == p.LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);     // bufferSize has not been called
    if (!p.keepSum) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');
    if (nullptr == p.buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return TFQMRGPU_STATUS_SUCCESS;
}
}

// on or off, the sum that is held ends: S is zero behind keepSum(plan, 1) (the call has no stream: releasing waits for the device)
tfqmrgpuStatus_t sum_keep(Plan& p, bool const on) {
    p.keepSum = on;
    p.held.sumMem.release();
    p.held.sumTerms = 0;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t sum_add(Handle& h, Plan& p, double const wRe, double const wIm) {
    if (auto const st = sum_ready(p)) return st;
    hipStream_t const s = (hipStream_t)h.stream;
    if (!p.held.sumMem) {
        size_t const bytes = std::max<size_t>(sum_doubles(p) * sizeof(double), 256);
        if (auto const st = p.held.sumMem.reserve(bytes)) return st;
        if (hipSuccess != hipMemsetAsync(p.held.sumMem.ptr, 0, bytes, s)) { p.held.sumMem.release(); return TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED); }
    }
    if (!sum_add_launch(resolve_callers(p), p.held.sumMem.as<double>(), wRe, wIm, s)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    ++p.held.sumTerms;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t sum_get(Handle& h, Plan& p, double* const values, int32_t* const nTerms) {
    if (auto const st = sum_ready(p)) return st;
    if (values) {
        size_t const P = size_t(p.LM) * p.LN;
        std::vector<double> host;                                   // through a host vector: a failed copy leaves the caller's array untouched
        try { host.assign(sum_doubles(p), 0.); } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
        if (p.held.sumMem && !host.empty()) {                       // (no addToSum yet: zeros)
            hipStream_t const s = (hipStream_t)h.stream;
            TFQ_HIP(hipMemcpyAsync(host.data(), p.held.sumMem.ptr, host.size() * sizeof(double), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
            TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        }
        // the caller's compact shape (section 18): rows 0 ... lm - 1 and columns 0 ... ln - 1 of every block
        double* out = values;
        for (size_t b = 0; b < p.nnzbB; ++b)
            for (int r = 0; r < p.lm; ++r, out += size_t(2) * p.ln)
                std::copy_n(host.data() + (b * P + size_t(r) * p.LN) * 2, size_t(2) * p.ln, out);
    }
    if (nTerms) *nTerms = p.held.sumTerms;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t sum_clear(Handle& h, Plan& p) {
    if (auto const st = sum_ready(p)) return st;
    if (p.held.sumMem) TFQ_HIP(hipMemsetAsync(p.held.sumMem.ptr, 0, p.held.sumMem.bytes, (hipStream_t)h.stream), TFQMRGPU_STATUS_LAUNCH_FAILED)
    p.held.sumTerms = 0;
    return TFQMRGPU_STATUS_SUCCESS;
}

} // namespace tfq

using namespace tfq;

extern "C" {

tfqmrgpuStatus_t tfqmrgpuExt_shiftDiagonal(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double const sigmaRe, double const sigmaIm) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return mesh_shift(*h, *p, sigmaRe, sigmaIm);
}

tfqmrgpuStatus_t tfqmrgpuExt_keepSum(tfqmrgpuBsrsvPlan_t plan, int const on) {
    auto p = asPlan(plan);
    if (!p) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return sum_keep(*p, 0 != on);
}

tfqmrgpuStatus_t tfqmrgpuExt_addToSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double const wRe, double const wIm) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return sum_add(*h, *p, wRe, wIm);
}

tfqmrgpuStatus_t tfqmrgpuExt_getSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double* values, int32_t* nTerms) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return sum_get(*h, *p, values, nTerms);
}

tfqmrgpuStatus_t tfqmrgpuExt_clearSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    return sum_clear(*h, *p);
}

// ---- 19c: the energy loop ------------------------------------------------------------------------------------------------------------------
// Nothing but the public calls, in the order a caller would write them: what the mesh computes is what that loop computes, bit for bit
tfqmrgpuStatus_t tfqmrgpuExt_solveMesh(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int32_t const nE,
    double const* sigma, double const* weight, double const threshold, int const maxIterations, int const fromX,
    int32_t* iterations, double* residual, tfqmrgpuStatus_t* status, int32_t* nDone)
{
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (nDone) *nDone = 0;
    if (nullptr == sigma) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (nE <= 0) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'E');
    if (several_ranks(*h)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);   // from the handle alone: the same on every rank, no collective
    if (p->opFn) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    bool anyMaxIterations = false;
    for (int32_t e = 0; e < nE; ++e) {
        if (auto const st = tfqmrgpuExt_shiftDiagonal(handle, plan, sigma[2 * e], sigma[2 * e + 1])) return st;
        tfqmrgpuStatus_t solved;
        if (0 == e && 0 == fromX) solved = tfqmrgpu_bsrsv_solve(handle, plan, threshold, maxIterations);
        else {
            if (tfqmrgpuExt_startCount(plan) > 0) if (auto const st = tfqmrgpuExt_projectStart(handle, plan, nullptr, nullptr)) return st;
            solved = tfqmrgpuExt_refineFrom(handle, plan, threshold, maxIterations);
        }
        if (nDone) *nDone = e + 1;
        if (status) status[e] = solved;
        (void)tfqmrgpu_bsrsv_getInfo(handle, plan, residual ? residual + e : nullptr, iterations ? iterations + e : nullptr, nullptr, nullptr);
        if (TFQMRGPU_STATUS_MAX_ITERATIONS == solved) anyMaxIterations = true;
        else if (TFQMRGPU_STATUS_SUCCESS != solved) return solved;
        if (tfqmrgpuExt_startDepth(plan) > 0) if (auto const st = tfqmrgpuExt_pushStart(handle, plan)) return st;
        if (weight && p->keepSum) if (auto const st = tfqmrgpuExt_addToSum(handle, plan, weight[2 * e], weight[2 * e + 1])) return st;
    }
    return anyMaxIterations ? TFQMRGPU_STATUS_MAX_ITERATIONS : TFQMRGPU_STATUS_SUCCESS;
}

} // extern "C"
