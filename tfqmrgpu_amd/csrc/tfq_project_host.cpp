// Start projection (tfqmrgpu_ext.h section 17), host side: the ring of kept starts, and projectStart -- its checks in front of the first
// device call, the images W_i = A S_i by the plan's own multiply on the caller's A, the three launches of tfq_project.hip, the copy-out.
// Everything lives in two library-owned pieces of device memory: Plan::held.startMem, `depth` X-shaped vectors in the plan's storage type and
// internal order, and Plan::held.projectMem [images W | records | gamma | nUsed], allocated at the first projectStart.
#include <algorithm>
#include <new>
#include <vector>

#include "tfq_solve.hpp"
#include "tfq_precond.hpp"
#include "tfq_vec.hpp"
#include "tfq_project.hpp"

namespace tfq {

namespace {
// one X-shaped vector as the caller's X is stored: the plan's storage type, an 'm' plan's double X
size_t start_bytes(Plan const& p) { return ('m' == p.precision) ? p.wXz.bytes : p.S; }
size_t start_stride(Plan const& p) { return align256(start_bytes(p)); }
// start i (0: the newest) lies in slot (head + i) % depth of the ring
char* start_at(Plan const& p, int i) { return p.held.startMem.as<char>() + size_t((p.held.startHead + i) % p.startDepth) * start_stride(p); }
// the ring ends on its own (keepStarts; a new buffer ends it with the rest of Plan::held): the starts go, the depth stays
void starts_release(Plan& p) {
    p.held.startMem.release(); p.held.projectMem.release();
    p.held.startCount = 0; p.held.startHead = 0;
}
}

tfqmrgpuStatus_t starts_keep(Plan& p, int const depth) {
    if (depth < 0 || depth > kProjectMax) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');
    if (depth == p.startDepth) return TFQMRGPU_STATUS_SUCCESS;
    if (0 == depth || 0 == p.held.startCount) {      // nothing to carry over: the ring is allocated by the next pushStart
        starts_release(p);
        p.startDepth = depth;
        return TFQMRGPU_STATUS_SUCCESS;
    }
    // a ring of another depth with the newest starts in slots 0, 1, ...  (the call has no stream: it waits for the device)
    int const keep = std::min(p.held.startCount, depth);
    size_t const stride = start_stride(p);
    DevMem ring;
    if (auto const st = ring.reserve(std::max<size_t>(size_t(depth) * stride, 256))) return st;
    TFQ_HIP(hipDeviceSynchronize(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    for (int i = 0; i < keep; ++i)
        TFQ_HIP(hipMemcpy(ring.as<char>() + size_t(i) * stride, start_at(p, i), start_bytes(p), hipMemcpyDeviceToDevice), TFQMRGPU_STATUS_LAUNCH_FAILED)
    p.held.startMem = std::move(ring);
    p.held.projectMem.release();                     // sized by the depth
    p.startDepth = depth; p.held.startCount = keep; p.held.startHead = 0;
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t starts_push(Handle& h, Plan& p) {
    if (0 == p.LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);     // bufferSize has not been called
    if (0 == p.startDepth) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');
    if (nullptr == p.buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (auto const st = p.held.startMem.reserve(std::max<size_t>(size_t(p.startDepth) * start_stride(p), 256))) return st;
    int const head = (p.held.startHead + p.startDepth - 1) % p.startDepth;   // the slot of the oldest start, or a free one
    hipStream_t const s = (hipStream_t)h.stream;
    char* const slot = p.held.startMem.as<char>() + size_t(head) * start_stride(p);
    TFQ_HIP(hipMemcpyAsync(slot, resolve_callers(p).x, start_bytes(p), hipMemcpyDeviceToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    p.held.startHead = head;
    p.held.startCount = std::min(p.held.startCount + 1, p.startDepth);
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t starts_project(Handle& h, Plan& p, double* const coefficients, int32_t* const nUsed) {
    if (0 == p.LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);     // bufferSize has not been called
    if (auto const st = operands_ready(p, true)) return st;         // no buffer | user-defined operator | A never set | A scaled and not kept
    int const k = p.held.startCount, depth = p.startDepth;
    if (k < 1 || !p.held.startMem) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');

    hipStream_t const s = (hipStream_t)h.stream;
    DevPlan const d = resolve_callers(p);                           // 'm': the double copies of X, B and A
    size_t const LN = size_t(p.LN), nRhs = size_t(p.nCols) * LN;
    std::vector<double> gammaHost; std::vector<int32_t> usedHost;   // sized in front of the first device call
    try { if (coefficients) gammaHost.resize(nRhs * 2 * kProjectMax); if (nUsed) usedHost.resize(nRhs); }
    catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }

    size_t const stride = start_stride(p);
    size_t const atRec = size_t(depth) * stride;
    size_t const atGamma = atRec + align256(size_t(project_planes(depth)) * d.nChunks * LN * sizeof(double));
    size_t const atUsed = atGamma + align256(nRhs * 2 * kProjectMax * sizeof(double));
    if (auto const st = p.held.projectMem.reserve(std::max<size_t>(atUsed + align256(nRhs * sizeof(int32_t)), 256))) return st;
    char* const mem = p.held.projectMem.as<char>();
    double* const gamma = (double*)(mem + atGamma);
    int32_t* const used = (int32_t*)(mem + atUsed);

    // W_i = A S_i with the caller's A, truncated to the pattern of X as every product is
    DevPlan dA = d; dA.A = const_cast<void*>(callers_a(p, d));
    ProjectVecs pv{};
    for (int i = 0; i < k; ++i) {
        pv.s[i] = start_at(p, i); pv.w[i] = mem + size_t(i) * stride;
        spmm_apply(dA, pv.s[i], const_cast<void*>(pv.w[i]), s);
    }
    double const pivotMin = d.dbl ? TFQMRGPU_PROJECT_PIVOT_DOUBLE : TFQMRGPU_PROJECT_PIVOT_FLOAT;
    if (!project_launch(d, k, pv, (double*)(mem + atRec), pivotMin, gamma, used, s)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (!coefficients && !nUsed) return TFQMRGPU_STATUS_SUCCESS;    // nothing to fetch: the call stays asynchronous

    if (coefficients) TFQ_HIP(hipMemcpyAsync(gammaHost.data(), gamma, gammaHost.size() * sizeof(double), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (nUsed) TFQ_HIP(hipMemcpyAsync(usedHost.data(), used, usedHost.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (coefficients)   // [nCols][LN][depth][2] from the device's [nCols][LN][kProjectMax][2]
        for (size_t r = 0; r < nRhs; ++r)
            std::copy_n(gammaHost.data() + r * 2 * kProjectMax, size_t(2 * depth), coefficients + r * 2 * size_t(depth));
    if (nUsed) std::copy(usedHost.begin(), usedHost.end(), nUsed);
    return TFQMRGPU_STATUS_SUCCESS;
}

} // namespace tfq
