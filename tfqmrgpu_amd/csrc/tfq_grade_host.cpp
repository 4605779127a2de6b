// The calls that grade the caller's system on the device (tfqmrgpu_ext.h sections 10 to 13): the per-right-hand-side residual, the
// truncation leak, the leak map with the grown pattern, the drop cost with the shrunk pattern; and the two that decide on those grades
// there (section 20): selectDrop and selectLeak.  Host code only: the kernels are reached through the launchers of tfq_vec.hpp
// (tfq_residual.hip, tfq_leak.hip, tfq_leak_map.hip, tfq_drop_cost.hip) and tfq_select.hpp (tfq_select.hip), the listings are built by
// tfq_leak_host.cpp.  Every call has the same three steps, each written once here: its checks in front of the first device call, in the
// documented order; its lists and records in ONE library-owned piece of device memory (dev_listing); its results through a host vector
// (Result, fetch), so that a failed copy leaves the caller's arrays untouched.  The step in the middle of sections 10, 12 and 13 -- the
// records on the device -- is a function of its own (residual_records, leak_map_records, drop_records): the public call is that step and
// its copy-out, a call of section 20 is that step and its own kernels.
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <new>
#include <vector>

#include "tfq_solve.hpp"
#include "tfq_precond.hpp"
#include "tfq_vec.hpp"
#include "tfq_select.hpp"

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

// ---- the records on the device: what sections 10, 12 and 13 do between their checks and their copy-out
// section 10: col = [nCols][2][LN], |B - A X|^2 and |B|^2 of every block column
tfqmrgpuStatus_t residual_records(Plan& p, hipStream_t s, double const*& col) {
    DevPlan const d = resolve_callers(p);                           // 'm': the double copies of X, B and A
    size_t const nRec = size_t(d.nChunks) * 2 * p.LN, nCol = size_t(p.nCols) * 2 * p.LN;
    if (auto const st = p.layout.residualScratch.reserve(std::max<size_t>((nRec + nCol) * sizeof(double), 256))) return st;
    double* const rec = p.layout.residualScratch.as<double>();
    residual_launch(d, callers_a(p, d), rec, rec + nRec, s);
    col = rec + nRec;
    return TFQMRGPU_STATUS_SUCCESS;
}

// section 12: rec = [nPos][LN]; behind leak_host, for nPos > 0
tfqmrgpuStatus_t leak_map_records(Plan& p, hipStream_t s, double const*& rec) {
    size_t const nPos = p.layout.leak.nPositions();
    size_t at[kLeakPieces];
    if (auto const st = leak_device(p, at, s)) return st;           // the listing of section 11, uploaded once for both calls
    if (auto const st = p.layout.leakMapRec.reserve(std::max<size_t>(nPos * size_t(p.LN) * sizeof(double), 256))) return st;
    char* const dev = p.layout.leakDev.as<char>();
    DevPlan const d = resolve_callers(p);                           // 'm': the double copies of X and A
    leak_map_launch(d, callers_a(p, d), uint32_t(nPos), (uint32_t const*)(dev + at[kLeakPairs]), (uint32_t const*)(dev + at[kLeakPos]), p.layout.leakMapRec.as<double>(), s);
    rec = p.layout.leakMapRec.as<double>();
    return TFQMRGPU_STATUS_SUCCESS;
}

// section 13: cost, weight = [nnzbX][LN] each, in the caller's block order; only what is asked for is computed
tfqmrgpuStatus_t drop_records(Plan& p, bool const wantCost, bool const wantWeight, hipStream_t s, double const*& cost, double const*& weight) {
    try {
        if (!p.drop.built) drop_listing(p.drop, p.nnzbX, p.nPairs(), p.pairs.data(), p.u2i.data());
    } catch (std::bad_alloc const&) { p.drop = DropListing{}; return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    auto const& l = p.drop;
    size_t const n = size_t(p.nnzbX) * size_t(p.LN);
    // the listing on the device, Plan::layout.dropDev
    enum { kStart, kAOf, kXOf, kCost, kWeight, kPieces };
    Piece const piece[kPieces] = {{l.start.data(), l.start.size() * 4}, {l.aOf.data(), l.aOf.size() * 4}, {l.xOf.data(), l.xOf.size() * 4},
                                  {nullptr, n * sizeof(double)}, {nullptr, n * sizeof(double)}};
    size_t at[kPieces];
    if (auto const st = dev_listing(p.layout.dropDev, piece, at, s)) return st;
    char* const dev = p.layout.dropDev.as<char>();
    cost = (double const*)(dev + at[kCost]); weight = (double const*)(dev + at[kWeight]);
    DevPlan const d = resolve_callers(p);                           // 'm': the double copies of X and A
    // the kernel writes the record of a block at the caller's index of that block: the copy-out is a plain copy
    drop_cost_launch(d, wantCost ? callers_a(p, d) : nullptr, p.nnzbX, (uint32_t const*)(dev + at[kStart]), (uint32_t const*)(dev + at[kAOf]),
                     (uint32_t const*)(dev + at[kXOf]), wantCost ? (double*)(dev + at[kCost]) : nullptr, wantWeight ? (double*)(dev + at[kWeight]) : nullptr, s);
    return TFQMRGPU_STATUS_SUCCESS;
}

// ---- section 20: flags, ordered list and per-column sums from records that are on the device -------------------------------------------
// what a call copies out, through host memory of its own (sized in front of the first device call)
struct Selection {
    std::vector<uint32_t> list; uint32_t total = 0; Result sums;
};
// `mem`: the call's device memory, its pieces in this order (the host lists in front, `nLists` of them; then flags | tile counts |
// list | sums).  rec [nItems][LN], bnorm2 as select_flag_launch reads it; start [nCols + 1] and order (or nullptr) as select_sum_launch does
struct SelectPieces { uint32_t const *colOf, *start, *order; uint8_t* flag; uint32_t *tiles, *list; double* sums; };
tfqmrgpuStatus_t select_run(Plan const& p, SelectPieces const& m, uint32_t nItems, double const* rec, double const* col, double eta,
    bool leak, Selection& out, hipStream_t s)
{
    uint32_t const nTiles = select_tiles(nItems);
    // bnorm2 of column c: the second [LN] of its pair of records
    select_flag_launch(nItems, p.LN, rec, col + p.LN, uint32_t(2 * p.LN), m.colOf, eta * eta, leak, m.flag, m.tiles, s);
    select_compact_launch(nItems, m.flag, m.tiles, m.list, s);
    if (!out.sums.host.empty()) select_sum_launch(p.nCols, p.LN, rec, m.flag, m.start, m.order, !leak, !leak, m.sums, s);
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (nItems) TFQ_HIP(hipMemcpyAsync(&out.total, m.tiles + nTiles, sizeof(uint32_t), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    // as many entries as the caller has room for: whether that is all of them is known behind the synchronise
    if (!out.list.empty()) TFQ_HIP(hipMemcpyAsync(out.list.data(), m.list, out.list.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (!out.sums.host.empty()) TFQ_HIP(hipMemcpyAsync(out.sums.host.data(), m.sums, out.sums.host.size() * sizeof(double), hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    return TFQMRGPU_STATUS_SUCCESS;
}

// the checks of both calls, in the documented order
tfqmrgpuStatus_t select_checks(Plan const* p, Handle const* h, double eta, bool const anyOutput) {
    if (auto const st = prologue(p, h, anyOutput)) return st;
    if (!(eta >= 0)) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'E');    // negative, or a NaN
    return operands_ready(*p, true);
}
// the host memory of the copy-out: room for as many indices as the caller has, at most all items
bool select_host(Plan const& p, Selection& out, bool wantList, uint64_t capacity, size_t nItems, bool wantSums) {
    try {
        if (wantList) out.list.resize(size_t(std::min<uint64_t>(capacity, nItems)));
    } catch (std::bad_alloc const&) { return false; }
    return out.sums.size(wantSums ? size_t(p.nCols) * size_t(p.LN) : 0);
}

// behind the synchronise: the count first -- with too little room it is all the caller gets --, then the arrays
template <typename Index>
tfqmrgpuStatus_t select_deliver(Selection const& out, uint64_t capacity, Index* index, uint64_t* nSelected, double* sums) {
    if (index && capacity < uint64_t(out.total)) {
        if (nSelected) *nSelected = uint64_t(out.total);
        return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'X');
    }
    if (index) for (uint32_t n = 0; n < out.total; ++n) index[n] = Index(out.list[n]);
    if (sums) std::copy(out.sums.host.begin(), out.sums.host.end(), sums);
    if (nSelected) *nSelected = uint64_t(out.total);
    return TFQMRGPU_STATUS_SUCCESS;
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
    Result col;
    if (!col.size(size_t(p->nCols) * 2 * p->LN)) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    double const* dev = nullptr;
    if (auto const st = residual_records(*p, s, dev)) return st;
    col.dev = dev;
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
        double const* dev = nullptr;
        if (auto const st = leak_map_records(*p, s, dev)) return st;
        rec.dev = dev;
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
    if (!cost.size(cost2 ? n : 0) || !weight.size(weight2 ? n : 0)) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    hipStream_t const s = (hipStream_t)h->stream;
    double const *costDev = nullptr, *weightDev = nullptr;
    if (auto const st = drop_records(*p, nullptr != cost2, nullptr != weight2, s, costDev, weightDev)) return st;
    cost.dev = costDev; weight.dev = weightDev;
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

// ---- selection on the device: the blocks to drop, the leak positions to take (tfqmrgpu_ext.h section 20) ---------------------------------
tfqmrgpuStatus_t tfqmrgpuExt_selectDrop(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double eta, uint64_t capacity,
    int32_t* blocks, uint64_t* nSelected, double* spent)
{
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (auto const st = select_checks(p, h, eta, blocks || nSelected || spent)) return st;
    hipStream_t const s = (hipStream_t)h->stream;
    uint32_t const nX = p->nnzbX, nTiles = select_tiles(nX);
    Selection out;
    if (!select_host(*p, out, nullptr != blocks, capacity, nX, nullptr != spent)) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    // the lists: the column of every block in the caller's order, none for a block that carries B | the blocks of every column in the
    // internal order, which is sorted by (column, row), and the caller's index of each
    enum { kColOf, kStart, kOrder, kFlag, kTiles, kList, kSums, kPieces };
    std::vector<uint32_t> colOf;
    if (!p->layout.selectDrop) {
        try {
            colOf = p->col32;
            for (auto const x : p->subset) colOf[x] = kSelExcluded;
        } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    }
    Piece const piece[kPieces] = {{colOf.data(), size_t(nX) * 4}, {p->colStart.data(), p->colStart.size() * 4}, {p->i2u.data(), size_t(nX) * 4},
        {nullptr, nX}, {nullptr, (size_t(nTiles) + 1) * 4}, {nullptr, size_t(nX) * 4}, {nullptr, size_t(p->nCols) * size_t(p->LN) * sizeof(double)}};
    size_t at[kPieces];
    if (auto const st = dev_listing(p->layout.selectDrop, piece, at, s)) return st;
    char* const dev = p->layout.selectDrop.as<char>();
    SelectPieces const m{(uint32_t const*)(dev + at[kColOf]), (uint32_t const*)(dev + at[kStart]), (uint32_t const*)(dev + at[kOrder]),
                         (uint8_t*)(dev + at[kFlag]), (uint32_t*)(dev + at[kTiles]), (uint32_t*)(dev + at[kList]), (double*)(dev + at[kSums])};
    double const *cost = nullptr, *weight = nullptr, *col = nullptr;
    if (auto const st = drop_records(*p, true, false, s, cost, weight)) return st;      // cost2 as dropCost returns it
    if (auto const st = residual_records(*p, s, col)) return st;                        // bnorm2 as residual returns it
    if (auto const st = select_run(*p, m, nX, cost, col, eta, false, out, s)) return st;
    return select_deliver(out, capacity, blocks, nSelected, spent);
}

tfqmrgpuStatus_t tfqmrgpuExt_selectLeak(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double eta, uint64_t capacity,
    uint64_t* take, uint64_t* nSelected, double* left)
{
    auto p = asPlan(plan); auto h = (Handle*)handle;
    if (auto const st = select_checks(p, h, eta, take || nSelected || left)) return st;
    if (auto const st = leak_host(*p)) return st;
    auto const& l = p->layout.leak;
    uint32_t const nPos = uint32_t(l.nPositions()), nTiles = select_tiles(nPos);
    hipStream_t const s = (hipStream_t)h->stream;
    Selection out;
    if (!select_host(*p, out, nullptr != take, capacity, nPos, nullptr != left)) return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED);
    enum { kColOf, kStart, kFlag, kTiles, kList, kSums, kPieces };
    std::vector<uint32_t> start;                                    // the first position of every column: they are sorted by column
    try {
        if (!p->layout.selectLeak) {
            start.assign(size_t(p->nCols) + 1, 0u);
            for (auto const c : l.posCol) ++start[c + 1];
            for (uint32_t c = 0; c < p->nCols; ++c) start[c + 1] += start[c];
        }
    } catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    Piece const piece[kPieces] = {{l.posCol.data(), size_t(nPos) * 4}, {start.data(), (size_t(p->nCols) + 1) * 4},
        {nullptr, nPos}, {nullptr, (size_t(nTiles) + 1) * 4}, {nullptr, size_t(nPos) * 4}, {nullptr, size_t(p->nCols) * size_t(p->LN) * sizeof(double)}};
    size_t at[kPieces];
    if (auto const st = dev_listing(p->layout.selectLeak, piece, at, s)) return st;
    char* const dev = p->layout.selectLeak.as<char>();
    SelectPieces const m{(uint32_t const*)(dev + at[kColOf]), (uint32_t const*)(dev + at[kStart]), nullptr,
                         (uint8_t*)(dev + at[kFlag]), (uint32_t*)(dev + at[kTiles]), (uint32_t*)(dev + at[kList]), (double*)(dev + at[kSums])};
    double const *pos = nullptr, *col = nullptr;
    if (nPos) if (auto const st = leak_map_records(*p, s, pos)) return st;              // pos2 as leakMap returns it
    if (auto const st = residual_records(*p, s, col)) return st;
    if (auto const st = select_run(*p, m, nPos, pos, col, eta, true, out, s)) return st;
    return select_deliver(out, capacity, take, nSelected, left);
}

// how the listing is cut: work units per compressed block column
int64_t tfqmrgpuExt_leakUnits(tfqmrgpuBsrsvPlan_t plan, uint32_t* unitsPerColumn) {
    auto p = asPlan(plan);
    if (!p || !p->layout.leak.built) return 0;
    if (unitsPerColumn) for (uint32_t c = 0; c < p->nCols; ++c) unitsPerColumn[c] = p->layout.leak.colUnitPtr[c + 1] - p->layout.leak.colUnitPtr[c];
    return int64_t(p->layout.leak.nUnits());
}

} // extern "C"
