// The calls that grade the caller's system on the device (tfqmrgpu_ext.h sections 10 to 13): the per-right-hand-side residual, the
// truncation leak, the leak map with the grown pattern, the drop cost with the shrunk pattern.  Host code only: the kernels are reached
// through the launchers of tfq_vec.hpp (tfq_residual.hip, tfq_leak.hip, tfq_leak_map.hip, tfq_drop_cost.hip), the listings are built by
// tfq_leak_host.cpp.  Every call has the same three steps, each written once here: its checks in front of the first device call, in the
// documented order; its lists and records in ONE library-owned piece of device memory (dev_listing); its results through a host vector
// (Result, fetch), so that a failed copy leaves the caller's arrays untouched.
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <new>
#include <vector>

#include "tfq_solve.hpp"
#include "tfq_precond.hpp"
#include "tfq_vec.hpp"

using namespace tfq;

namespace tfq {

// the checks of every call that reads the operands.  needA: the call reads A (the patterns-only forms and the weights of section 13 do not)
tfqmrgpuStatus_t operands_ready(Plan const& p, bool const needA) {
    if (nullptr == p.buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (p.opFn) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);         // a user-defined operator is the caller's to apply
    if (!needA) return TFQMRGPU_STATUS_SUCCESS;
    if (!p.held.haveA) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'A');
    if (TFQMRGPU_PRECOND_NONE != p.held.precondInA && !kept_is_callers_a(p)) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);   // the caller's A is gone; keepOperator keeps it
    return TFQMRGPU_STATUS_SUCCESS;
}

void const* callers_a(Plan const& p, DevPlan const& d) {
    return (TFQMRGPU_PRECOND_NONE != p.held.precondInA) ? (void const*)kept_a(p).a : d.A;
}

namespace {

// what every call checks first: plan and handle | bufferSize has been called | the caller asks for something
tfqmrgpuStatus_t prologue(Plan const* p, Handle const* h, bool const anyOutput) {
    if (!p || !h) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);    // bufferSize has not been called
    return anyOutput ? TFQMRGPU_STATUS_SUCCESS : TFQMRGPU_STATUS_NO_INFO_PASSED;
}

// One library-owned piece of device memory `mem` made of N pieces, every piece on a 256-byte boundary: at[i] is where piece i begins.
// A piece is a host list, uploaded, or (host == nullptr) an area of records.  The first call reserves the memory and uploads the lists with
// one synchronise -- all of it or nothing; later calls find it there
struct Piece { void const* host; size_t bytes; };
template <int N>
tfqmrgpuStatus_t dev_listing(DevMem& mem, Piece const (&piece)[N], size_t (&at)[N], hipStream_t s) {
    size_t total = 0;
    for (int i = 0; i < N; ++i) { at[i] = total; total += align256(piece[i].bytes); }
    if (mem) return TFQMRGPU_STATUS_SUCCESS;
    if (auto const st = mem.reserve(std::max<size_t>(total, 256))) return st;
    tfqmrgpuStatus_t st = TFQMRGPU_STATUS_SUCCESS;
    for (int i = 0; i < N && !st; ++i) st = upload(mem.as<char>() + at[i], piece[i].host, piece[i].bytes, s);
    if (!st && hipSuccess != hipStreamSynchronize(s)) st = TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
    if (st) mem.release();
    return st;
}

// One array of results on its way from the device (`dev`) to the caller (`to`, or nullptr: the call reads `host` itself).  The host vector
// is sized in front of the first device call
struct Result {
    std::vector<double> host; void const* dev = nullptr; double* to = nullptr;
    bool size(size_t n) { try { host.resize(n); } catch (std::bad_alloc const&) { return false; } return true; }
};
// behind the launch: its error | the copies | one synchronise | the caller's arrays
tfqmrgpuStatus_t fetch(hipStream_t s, Result& a, Result* b = nullptr) {
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    for (Result* r : {&a, b})
        if (r && !r->host.empty()) TFQ_HIP(hipMemcpyAsync(r->host.data(), r->dev, r->host.size() * sizeof(double), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    for (Result* r : {&a, b}) if (r && r->to) std::copy(r->host.begin(), r->host.end(), r->to);
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- the leak listing (sections 11 and 12): the host analysis, once per plan and block shape
tfqmrgpuStatus_t leak_host(Plan& p) {
    auto& l = p.layout.leak;
    if (l.built) return TFQMRGPU_STATUS_SUCCESS;
    try {
        if (p.cscPtr.empty()) a_by_column(p.nRows, p.colOfA, p.cscPtr, p.cscBlock);
        if (!leak_listing(l, p.nRows, p.nCols, p.nnzbA, p.rowOfA.data(), p.colOfA.data(), p.cscPtr.data(), p.cscBlock.data(),
                          p.nnzbX, p.rowOfX.data(), p.col32.data(), p.u2i.data(), leak_unit_products(p.LM, p.LN))) {
            l = LeakListing{};
            return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
        }
    } catch (std::bad_alloc const&) { l = LeakListing{}; return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    return TFQMRGPU_STATUS_SUCCESS;
}

// the listing on the device, Plan::layout.leakDev.  ONE copy for truncationLeak and leakMap: whichever comes first uploads it
enum { kLeakPairs, kLeakPos, kLeakUnit, kLeakCol, kLeakRec, kLeakSum, kLeakPieces };
tfqmrgpuStatus_t leak_device(Plan& p, size_t (&at)[kLeakPieces], hipStream_t s) {
    auto const& l = p.layout.leak;
    Piece const piece[kLeakPieces] = {
        {l.pairs.data(), l.pairs.size() * 4}, {l.posStart.data(), l.posStart.size() * 4}, {l.unitFirst.data(), l.unitFirst.size() * 4},
        {l.colUnitPtr.data(), l.colUnitPtr.size() * 4},
        {nullptr, l.nUnits() * size_t(p.LN) * sizeof(double)}, {nullptr, size_t(p.nCols) * size_t(p.LN) * sizeof(double)}};
    return dev_listing(p.layout.leakDev, piece, at, s);
}

// a pattern of sections 12 and 13 into malloc'ed arrays for the caller (tfqmrgpuExt_freeGrownPattern releases them)
tfqmrgpuStatus_t export_pattern(Plan const& p, GrownPattern const& g, tfqmrgpuGrownPattern_t* to) {
    auto dup = [](std::vector<int32_t> const& v) {
        auto q = (int32_t*)std::malloc(std::max<size_t>(1, v.size()) * sizeof(int32_t));
        if (q) std::copy(v.begin(), v.end(), q);
        return q;
    };
    to->mb = int32_t(p.nRows); to->nnzbX = int32_t(g.colInd.size());
    to->rowPtrX = dup(g.rowPtr); to->colIndX = dup(g.colInd); to->oldBlock = dup(g.oldBlock);
    if (!to->rowPtrX || !to->colIndX || !to->oldBlock) {
        tfqmrgpuExt_freeGrownPattern(to);
        return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    }
    return TFQMRGPU_STATUS_SUCCESS;
}

} // namespace
} // namespace tfq

extern "C" {

// ---- per-right-hand-side residual of the caller's system (tfqmrgpu_ext.h section 10) --------------------------------------------------
tfqmrgpuStatus_t tfqmrgpuExt_residual(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double* residual2, double* bnorm2, int32_t* columns, double* worst)
{
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (auto const st = prologue(p, h, residual2 || bnorm2 || columns || worst)) return st;
    if (auto const st = operands_ready(*p, true)) return st;

    hipStream_t const s = (hipStream_t)h->stream;
    DevPlan const d = resolve_callers(*p);                          // 'm': the double copies of X, B and A
    size_t const nRec = size_t(d.nChunks) * 2 * p->LN, nCol = size_t(p->nCols) * 2 * p->LN;
    Result col;
    if (!col.size(nCol)) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    if (auto const st = p->layout.residualScratch.reserve(std::max<size_t>((nRec + nCol) * sizeof(double), 256))) return st;
    double* const rec = p->layout.residualScratch.as<double>();
    col.dev = rec + nRec;
    residual_launch(d, callers_a(*p, d), rec, rec + nRec, s);
    if (auto const st = fetch(s, col)) return st;

    size_t const LN = size_t(p->LN);
    double wmax = 0; bool any = false;                             // NaN entries (r = b = 0) are left out of the maximum
    for (size_t c = 0; c < p->nCols; ++c) {
        for (size_t j = 0; j < LN; ++j) {
            double const r2 = col.host[(2 * c) * LN + j], b2 = col.host[(2 * c + 1) * LN + j];
            if (residual2) residual2[c * LN + j] = r2;
            if (bnorm2) bnorm2[c * LN + j] = b2;
            double const quot = r2 / b2;
            if (quot == quot) { wmax = any ? std::max(wmax, quot) : quot; any = true; }
        }
        if (columns) columns[c] = p->original_bsrColIndX[c];
    }
    if (worst) *worst = any ? std::sqrt(wmax) : std::nan("");
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- truncation leak: what A X puts outside the pattern of X (tfqmrgpu_ext.h section 11) -----------------------------------------------
tfqmrgpuStatus_t tfqmrgpuExt_truncationLeak(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double* leak2, int32_t* columns, uint64_t* nLeakBlocks, uint64_t* nLeakPairs)
{
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (auto const st = prologue(p, h, leak2 || columns || nLeakBlocks || nLeakPairs)) return st;
    // everything but leak2 depends on the patterns alone: plan and bufferSize suffice
    if (leak2) if (auto const st = operands_ready(*p, true)) return st;
    if (auto const st = leak_host(*p)) return st;
    auto& l = p->layout.leak;
    if (leak2) {
        hipStream_t const s = (hipStream_t)h->stream;
        Result col; col.to = leak2;
        if (!col.size(size_t(p->nCols) * size_t(p->LN))) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
        size_t at[kLeakPieces];
        if (auto const st = leak_device(*p, at, s)) return st;
        char* const dev = p->layout.leakDev.as<char>();
        col.dev = dev + at[kLeakSum];
        DevPlan const d = resolve_callers(*p);                      // 'm': the double copies of X and A
        leak_launch(d, callers_a(*p, d), uint32_t(l.nUnits()), (uint32_t const*)(dev + at[kLeakPairs]), (uint32_t const*)(dev + at[kLeakPos]),
                    (uint32_t const*)(dev + at[kLeakUnit]), (uint32_t const*)(dev + at[kLeakCol]), (double*)(dev + at[kLeakRec]), (double*)(dev + at[kLeakSum]), s);
        if (auto const st = fetch(s, col)) return st;
    }
    if (columns) std::copy(p->original_bsrColIndX.begin(), p->original_bsrColIndX.end(), columns);
    if (nLeakBlocks) *nLeakBlocks = uint64_t(l.nPositions());
    if (nLeakPairs) *nLeakPairs = uint64_t(l.nProducts());
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- leak map: the leak per position, and the pattern of X grown by chosen positions (tfqmrgpu_ext.h section 12) ------------------------
tfqmrgpuStatus_t tfqmrgpuExt_leakMap(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    uint64_t capacity, int32_t* rows, int32_t* cols, double* pos2, uint64_t* nLeakBlocks)
{
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (auto const st = prologue(p, h, rows || cols || pos2 || nLeakBlocks)) return st;
    // everything but pos2 depends on the patterns alone, as in section 11
    if (pos2) if (auto const st = operands_ready(*p, true)) return st;
    if (auto const st = leak_host(*p)) return st;
    auto const& l = p->layout.leak;
    size_t const LN = size_t(p->LN), nPos = l.nPositions();
    if ((rows || cols || pos2) && capacity < uint64_t(nPos)) {      // the caller learns how much room the arrays need, and nothing else
        if (nLeakBlocks) *nLeakBlocks = uint64_t(nPos);
        return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');
    }
    if (pos2 && nPos) {
        hipStream_t const s = (hipStream_t)h->stream;
        Result rec; rec.to = pos2;
        if (!rec.size(nPos * LN)) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
        size_t at[kLeakPieces];
        if (auto const st = leak_device(*p, at, s)) return st;      // the listing of section 11, uploaded once for both calls
        if (auto const st = p->layout.leakMapRec.reserve(std::max<size_t>(nPos * LN * sizeof(double), 256))) return st;
        char* const dev = p->layout.leakDev.as<char>();
        rec.dev = p->layout.leakMapRec.ptr;
        DevPlan const d = resolve_callers(*p);                      // 'm': the double copies of X and A
        leak_map_launch(d, callers_a(*p, d), uint32_t(nPos), (uint32_t const*)(dev + at[kLeakPairs]), (uint32_t const*)(dev + at[kLeakPos]), p->layout.leakMapRec.as<double>(), s);
        if (auto const st = fetch(s, rec)) return st;
    }
    if (rows) for (size_t n = 0; n < nPos; ++n) rows[n] = int32_t(l.posRow[n]);
    if (cols) for (size_t n = 0; n < nPos; ++n) cols[n] = int32_t(l.posCol[n]);
    if (nLeakBlocks) *nLeakBlocks = uint64_t(nPos);
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_growPattern(tfqmrgpuBsrsvPlan_t plan, uint64_t nTake, uint64_t const* take, tfqmrgpuGrownPattern_t* grown) {
    auto p = asPlan(plan);
    if (!p || !grown) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    *grown = tfqmrgpuGrownPattern_t{};
    if (0 == p->LM) return TFQ_ERR(TFQMRGPU_UNDOCUMENTED_ERROR);    // bufferSize has not been called
    if (auto const st = leak_host(*p)) return st;
    auto const& l = p->layout.leak;
    GrownPattern g;
    try {
        int const bad = grow_pattern(g, p->nRows, p->nCols, p->nnzbX, p->rowOfX.data(), p->col32.data(), p->original_bsrColIndX.data(),
                                     p->indexOffset, l.nPositions(), l.posRow.data(), l.posCol.data(), nTake, take);
        if (1 == bad) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');   // an index >= nLeakBlocks, or one named twice
        if (bad) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);        // the index arrays are 32 bit
    } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    return export_pattern(*p, g, grown);
}

void tfqmrgpuExt_freeGrownPattern(tfqmrgpuGrownPattern_t* grown) {
    if (!grown) return;
    std::free(grown->rowPtrX); std::free(grown->colIndX); std::free(grown->oldBlock);
    *grown = tfqmrgpuGrownPattern_t{};
}

// ---- drop cost: what each block of X carries, and the pattern of X without chosen blocks (tfqmrgpu_ext.h section 13) ------------------
tfqmrgpuStatus_t tfqmrgpuExt_dropCost(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double* cost2, double* weight2, uint64_t* nProducts) {
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (auto const st = prologue(p, h, cost2 || weight2 || nProducts)) return st;
    if (!cost2 && !weight2) { *nProducts = uint64_t(p->nPairs()); return TFQMRGPU_STATUS_SUCCESS; }   // the plan alone: no buffer, no A
    if (auto const st = operands_ready(*p, nullptr != cost2)) return st;    // the weights do not read A

    size_t const n = size_t(p->nnzbX) * size_t(p->LN);
    Result cost, weight; cost.to = cost2; weight.to = weight2;
    try {
        if (!cost.size(cost2 ? n : 0) || !weight.size(weight2 ? n : 0)) throw std::bad_alloc();
        if (!p->drop.built) drop_listing(p->drop, p->nnzbX, p->nPairs(), p->pairs.data(), p->u2i.data());
    } catch (std::bad_alloc const&) { p->drop = DropListing{}; return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    hipStream_t const s = (hipStream_t)h->stream;
    auto const& l = p->drop;
    // the listing on the device, Plan::layout.dropDev
    enum { kStart, kAOf, kXOf, kCost, kWeight, kPieces };
    Piece const piece[kPieces] = {{l.start.data(), l.start.size() * 4}, {l.aOf.data(), l.aOf.size() * 4}, {l.xOf.data(), l.xOf.size() * 4},
                                  {nullptr, n * sizeof(double)}, {nullptr, n * sizeof(double)}};
    size_t at[kPieces];
    if (auto const st = dev_listing(p->layout.dropDev, piece, at, s)) return st;
    char* const dev = p->layout.dropDev.as<char>();
    cost.dev = dev + at[kCost]; weight.dev = dev + at[kWeight];
    DevPlan const d = resolve_callers(*p);                          // 'm': the double copies of X and A
    // the kernel writes the record of a block at the caller's index of that block: the copy-out is a plain copy
    drop_cost_launch(d, cost2 ? callers_a(*p, d) : nullptr, p->nnzbX, (uint32_t const*)(dev + at[kStart]), (uint32_t const*)(dev + at[kAOf]),
                     (uint32_t const*)(dev + at[kXOf]), cost2 ? (double*)(dev + at[kCost]) : nullptr, weight2 ? (double*)(dev + at[kWeight]) : nullptr, s);
    if (auto const st = fetch(s, cost, &weight)) return st;
    if (nProducts) *nProducts = uint64_t(p->nPairs());
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t tfqmrgpuExt_shrinkPattern(tfqmrgpuBsrsvPlan_t plan, uint64_t nDrop, int32_t const* drop, tfqmrgpuGrownPattern_t* shrunk) {
    auto p = asPlan(plan);
    if (!p || !shrunk) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    *shrunk = tfqmrgpuGrownPattern_t{};
    if (nDrop > 0 && !drop) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    GrownPattern g;
    try {
        std::vector<uint8_t> hasB(p->nnzbX, uint8_t(0));
        for (auto const x : p->subset) hasB[x] = 1;
        int const bad = shrink_pattern(g, p->nRows, p->nnzbX, p->rowOfX.data(), p->col32.data(), p->original_bsrColIndX.data(),
                                       p->indexOffset, hasB.data(), nDrop, drop);
        if (1 == bad) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');   // an index outside [0, nnzbX), or one named twice
        if (bad) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'B');        // the block carries a block of B
    } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    return export_pattern(*p, g, shrunk);
}

// how the listing is cut: work units per compressed block column
int64_t tfqmrgpuExt_leakUnits(tfqmrgpuBsrsvPlan_t plan, uint32_t* unitsPerColumn) {
    auto p = asPlan(plan);
    if (!p || !p->layout.leak.built) return 0;
    if (unitsPerColumn) for (uint32_t c = 0; c < p->nCols; ++c) unitsPerColumn[c] = p->layout.leak.colUnitPtr[c + 1] - p->layout.leak.colUnitPtr[c];
    return int64_t(p->layout.leak.nUnits());
}

} // extern "C"
