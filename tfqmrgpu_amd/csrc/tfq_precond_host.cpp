// Host side of the block-Jacobi right preconditioner (tfqmrgpu_ext.h sections 7 and 9; kernels: tfq_precond.hip): the plan's memory for it,
// the state of the A in the buffer with every transition of it, and the set-up in front of a solve.  No kernel lives here.
// With M = blockdiag(A) the iteration runs on (A M^-1) Y = B: A M^-1 has the pattern of A and takes its place in the buffer, once per
// setMatrix('A'); X = M^-1 Y has the pattern of Y and is formed in place at the end of a solve.  No iteration kernel knows about it.
#include <algorithm>
#include <new>
#include <vector>

#include "tfq_solve.hpp"
#include "tfq_precond.hpp"

namespace tfq {

// ---- the memory -------------------------------------------------------------------------------------------------------------------------
namespace {
// Plan::layout.precond: [M^-1 | diagOfRow | colOfA | counter | a flag per block row: M_ii is the unit matrix (plans that keep A)]
struct PrecondOffsets { size_t minvBytes, diag, colA, counter, identity, end; };
PrecondOffsets precond_offsets(Plan const& p) {
    size_t const real = ('c' == p.precision) ? 4 : 8;       // M^-1 in the plan's precision, double for 'm'
    PrecondOffsets o{};
    o.minvBytes = size_t(p.nRows) * 2 * p.LM * p.LM * real;
    size_t q = align256(o.minvBytes);
    o.diag = q;      q += align256(size_t(p.nRows) * 4);
    o.colA = q;      q += align256(size_t(p.nnzbA) * 4);
    o.counter = q;   q += 256;
    o.identity = q;  q += align256(size_t(p.nRows) * 4);
    o.end = q;
    return o;
}
// Plan::held.aKept: [A of the buffer's A window | 'm': the float A]
struct KeptSizes { size_t a, aFloat; };
KeptSizes kept_sizes(Plan const& p) {
    bool const mixed = ('m' == p.precision);
    return { mixed ? p.wAz.bytes : p.wA.bytes, mixed ? p.wA.bytes : 0 };
}
} // namespace

size_t precond_bytes(Plan const& p) { return precond_offsets(p).end; }
PrecondMem precond_mem(Plan const& p) {
    auto const o = precond_offsets(p);
    char* const b = p.layout.precond.as<char>();
    return { b, (uint32_t*)(b + o.diag), (uint32_t*)(b + o.colA), (uint32_t*)(b + o.counter), (uint32_t*)(b + o.identity), o.minvBytes };
}

size_t kept_a_bytes(Plan const& p) { auto const k = kept_sizes(p); return std::max<size_t>(align256(k.a) + align256(k.aFloat), 256); }
KeptA kept_a(Plan const& p) {
    auto const k = kept_sizes(p);
    char* const b = p.held.aKept.as<char>();
    return { b, ('m' == p.precision) ? b + align256(k.a) : nullptr, k.a, k.aFloat };
}

// ---- the state of the A in the buffer ----------------------------------------------------------------------------------------------------
// Plan::held has it -- haveA: a whole A has been set on this buffer; precondInA: what it has been scaled with; aKept: the caller's A while
// precondInA != NONE; dirtyRow, dirtyCol, anyDirty: what setBlocks('A') has written into aKept since the last set-up -- and beside it stand
// precondIdentity: the unit matrices of that scaling; mixedFloor: what the last 'm' solve learnt about this operator in float; cscPtr,
// cscBlock: A's pattern by block column.  What the caller has ASKED for -- precondKind, keepA -- is no part of it and survives every transition.

// nothing that setBlocks('A') wrote is waiting for a set-up: a whole new A, no copy any more, or the set-up has caught up
static void forget_dirty(Plan& p) {
    if (!p.held.anyDirty) return;
    std::fill(p.held.dirtyRow.begin(), p.held.dirtyRow.end(), uint8_t(0));
    std::fill(p.held.dirtyCol.begin(), p.held.dirtyCol.end(), uint8_t(0));
    p.held.anyDirty = false;
}
// the copy goes, and the marks with it: they say what differs between the copy and the buffer
static void release_kept(Plan& p) {
    p.held.aKept.release();
    forget_dirty(p);
}

// setBuffer: this buffer holds no A yet, scaled or not, and whatever held values of the old buffer goes: the kept copy with its marks, X0
// and R of a warm solve, the kept starts.  What is cut by the shape alone (Plan::layout: M^-1 and the index lists beside it, ...) stays: the
// shape is the same, and the next set-up writes M^-1 again
void a_new_buffer(Plan& p) { p.held = Plan::Held{}; }

// bufferSize: another block shape, and no buffer.  As a_new_buffer (the A of the new layout has not been set), and everything that was sized or
// cut for the previous shape goes as well.  Stays: cscPtr / cscBlock (the pattern has not changed), precondIdentity (read only behind a set-up,
// which writes it) -- and mixedFloor: a floor learnt on the old shape is not forgotten before setMatrix('A') names the new operator
// (a_named), which every solve of the new layout needs anyway
void a_new_layout(Plan& p) {
    p.layout = Plan::Layout{};
    a_new_buffer(p);
}

// setMatrix('A') has named its operand, and may still be refused (no buffer, the wrong precision, no values): a new operator is on its way,
// the remembered float floor goes.  BEFORE the argument checks, where setBlocks('A') forgets it behind its own (a_patched): a setMatrix('A')
// that is refused has forgotten the floor, a refused setBlocks('A') has not.  Both are as they have always been; the floor is a hint that
// costs the first cycle of the next 'm' solve two or three float iterations when it is missing, never a result
void a_named(Plan& p) { p.mixedFloor = 0; }

// setMatrix('A') behind its transfer (ok: it succeeded): the A in the buffer is a new one and not scaled -- M^-1 of the last one is stale, and
// so is a kept copy with its marks (the copy itself stays allocated: the next set-up fills it again).  The diagonal that shiftDiagonal has
// captured (section 19a) was that of the last A: the next shift captures all of it again.  Here and not in a_named: a setMatrix('A') that
// is refused has written nothing, and the A in the buffer may carry a shift that a capture would take for the base.  (A transfer that
// failed leaves no whole A -- !ok -- and shiftDiagonal refuses until one has succeeded, which comes through here again)
void a_set_whole(Plan& p, bool ok) {
    p.held.haveA = ok; p.held.precondInA = TFQMRGPU_PRECOND_NONE;
    forget_dirty(p);
    p.held.shiftBaseFresh = false;
    std::fill(p.held.shiftStaleRow.begin(), p.held.shiftStaleRow.end(), uint8_t(0)); p.held.shiftAnyStale = false;
}

// setBlocks('A') behind its transfer, which succeeded: the rows of the captured diagonal (section 19a) whose diagonal block it has written
// are captured again by the next shift, from the blocks it wrote; the other rows keep their base -- the A around them may carry a shift.
// One flag per block row (sized by the shift that captured the base; no base, no flags): patching one block any number of times is one flag
void a_patch_written(Plan& p, int32_t const* blocks, int32_t nBlocks) {
    if (!p.held.shiftBaseFresh || p.held.shiftStaleRow.size() != size_t(p.nRows)) return;
    for (int32_t k = 0; k < nBlocks; ++k) {
        uint32_t const q = uint32_t(blocks[k]), c = p.colOfA[q];
        if (p.diagOfRow[c] == q) { p.held.shiftStaleRow[c] = 1; p.held.shiftAnyStale = true; }
    }
}

// setBlocks('A') has passed its argument checks (0 <= blocks[k] < nnzbA, no block twice) and is about to write: where do the blocks go?
// A M^-1 cannot be patched, M changes with the diagonal blocks, and a whole setMatrix('A') brings the caller's A back -- unless the plan
// keeps it (section 9): then the patch goes into the copy (intoKept), and the next set-up redoes the block rows and columns that are marked
// here: the columns that hold a listed block, the rows whose diagonal block is listed.  Host code only: it comes before the first device
// call of setBlocks, so a transfer that fails afterwards leaves marks behind -- harmless, the set-up then redoes those rows and columns from
// the copy.  haveA stays: a patch makes no whole A.  mixedFloor goes: see a_named
tfqmrgpuStatus_t a_patched(Plan& p, int32_t const* blocks, int32_t nBlocks, bool& intoKept) {
    intoKept = kept_is_callers_a(p);
    if (TFQMRGPU_PRECOND_NONE != p.held.precondInA && !intoKept) return TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION);
    p.mixedFloor = 0;
    if (!intoKept) return TFQMRGPU_STATUS_SUCCESS;
    try {
        if (p.cscPtr.empty()) a_by_column(p.nRows, p.colOfA, p.cscPtr, p.cscBlock);   // once per plan: the blocks of A grouped by block column
        p.held.dirtyRow.resize(p.nRows, uint8_t(0)); p.held.dirtyCol.resize(p.nRows, uint8_t(0));
    } catch (std::bad_alloc const&) { p.cscPtr.clear(); return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
    for (int32_t k = 0; k < nBlocks; ++k) {
        uint32_t const q = uint32_t(blocks[k]), c = p.colOfA[q];
        p.held.dirtyCol[c] = 1;
        if (p.diagOfRow[c] == q) p.held.dirtyRow[c] = 1;
    }
    p.held.anyDirty = true;
    return TFQMRGPU_STATUS_SUCCESS;
}

// keepOperator.  On: refused when the A in the buffer is A M^-1 already and nobody has the caller's -- there is nothing to keep (a plan that
// is on has its copy).  Off: the copy and its marks go; from here on the plan is one that never kept anything.  precondInA stays either way
tfqmrgpuStatus_t a_keep(Plan& p, bool on) {
    if (on && !p.keepA && TFQMRGPU_PRECOND_NONE != p.held.precondInA) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'A');
    p.keepA = on;
    if (!on) release_kept(p);
    return TFQMRGPU_STATUS_SUCCESS;
}

// the set-up has scaled the A in the buffer with M^-1 of `kind`, which has nIdentity unit matrices (a partial set-up: has brought it up
// to date).  Whatever setBlocks('A') had marked has been redone, or the copy has just been taken
static void a_scaled(Plan& p, int kind, int32_t nIdentity) {
    p.held.precondInA = kind; p.precondIdentity = nIdentity;
    forget_dirty(p);
}
// the caller's A has gone back into the buffer from the kept copy, which had every patch: not scaled, nothing marked.  The floor that was
// remembered is that of the scaled operator.  haveA stays true
static void a_restored(Plan& p) {
    p.held.precondInA = TFQMRGPU_PRECOND_NONE; p.mixedFloor = 0;
    forget_dirty(p);
}

// ---- the set-up ------------------------------------------------------------------------------------------------------------------------
// the unit matrices of M: from the flags that the listed inversion keeps per block row (plans that keep A) ...
static tfqmrgpuStatus_t count_identity_flags(Plan const& p, PrecondMem const& m, hipStream_t s, int32_t& n) {
    std::vector<uint32_t> flags(p.nRows);
    TFQ_HIP(hipMemcpyAsync(flags.data(), m.identity, flags.size() * 4, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    n = 0;
    for (auto const f : flags) n += (0 != f);
    return TFQMRGPU_STATUS_SUCCESS;
}
// ... or from the device counter of the whole inversion
static tfqmrgpuStatus_t read_identity_counter(PrecondMem const& m, hipStream_t s, int32_t& n) {
    uint32_t c = 0;
    TFQ_HIP(hipMemcpyAsync(&c, m.counter, 4, hipMemcpyDeviceToHost, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    n = int32_t(c);
    return TFQMRGPU_STATUS_SUCCESS;
}

// setBlocks('A') has patched the kept copy since the last set-up: M^-1 again for the block rows whose diagonal block was written, and
// A_ij M_jj^-1 again, from the copy into the buffer, for every block of the block columns that hold a written block.  The listed kernels
// share their element loops with the whole set-up, so each block has the bits that a whole setMatrix('A') and a whole set-up would give it
static tfqmrgpuStatus_t precond_update(Handle& h, Plan& p) {
    hipStream_t const s = (hipStream_t)h.stream;
    std::vector<uint32_t> list;                             // [dirty rows | blocks of the dirty columns]
    for (uint32_t r = 0; r < p.nRows; ++r) if (p.held.dirtyRow[r]) list.push_back(r);
    uint32_t const nRowsListed = uint32_t(list.size());
    for (uint32_t c = 0; c < p.nRows; ++c) if (p.held.dirtyCol[c]) list.insert(list.end(), p.cscBlock.begin() + p.cscPtr[c], p.cscBlock.begin() + p.cscPtr[c + 1]);
    uint32_t const nBlocksListed = uint32_t(list.size()) - nRowsListed;
    if (auto const st = p.keepList.reserve(list.size() * 4)) return st;
    uint32_t const* const rows = p.keepList.as<uint32_t>();
    TFQ_HIP(hipMemcpyAsync(p.keepList.ptr, list.data(), list.size() * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    TFQ_HIP(hipStreamSynchronize(s), TFQMRGPU_STATUS_LAUNCH_FAILED)   // (`list` is a local)
    auto const m = precond_mem(p);
    auto const k = kept_a(p);
    bool const mixed = ('m' == p.precision), wDbl = ('c' != p.precision);
    DevPlan const d = resolve_callers(p);
    uint32_t const* const blocks = rows + nRowsListed;
    launch_precond_invert_listed(d.dbl, wDbl, k.a, m.diag, m.minv, m.identity, rows, nRowsListed, p.LM, d.ilv, s);
    launch_precond_apply_listed(d.dbl, wDbl, true, k.a, d.A, nBlocksListed, blocks, m.colA, m.minv, p.LM, p.LM, d.ilv, s);
    if (mixed) launch_precond_apply_listed(false, true, true, k.aFloat, p.buffer + p.wA.offset, nBlocksListed, blocks, m.colA, m.minv, p.LM, p.LM, p.ilv, s);
    int32_t nIdentity = 0;
    if (auto const st = count_identity_flags(p, m, s, nIdentity)) return st;   // a row can have become singular, or regular
    a_scaled(p, p.held.precondInA, nIdentity);
    return TFQMRGPU_STATUS_SUCCESS;
}

// the kind has changed on a plan that keeps A: the caller's A goes back into the buffer
static tfqmrgpuStatus_t precond_restore(Handle& h, Plan& p) {
    hipStream_t const s = (hipStream_t)h.stream;
    auto const k = kept_a(p);
    bool const mixed = ('m' == p.precision);
    TFQ_HIP(hipMemcpyAsync(p.buffer + (mixed ? p.wAz.offset : p.wA.offset), k.a, k.aBytes, hipMemcpyDeviceToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    if (mixed) TFQ_HIP(hipMemcpyAsync(p.buffer + p.wA.offset, k.aFloat, k.aFloatBytes, hipMemcpyDeviceToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    a_restored(p);
    return TFQMRGPU_STATUS_SUCCESS;
}

// what a solve needs before its first iteration: nothing when the preconditioner is off; otherwise M^-1 and the scaled A, made here
// when the A in the buffer is still the caller's (the first solve after setMatrix('A')) and reused by every later solve of that A.
// A plan that keeps A (section 9) copies the A window first; later it redoes what setBlocks('A') has touched, and follows a change of kind
static tfqmrgpuStatus_t precond_prepare_(Handle& h, Plan& p) {
    if (TFQMRGPU_PRECOND_NONE == p.precondKind && TFQMRGPU_PRECOND_NONE == p.held.precondInA) return TFQMRGPU_STATUS_SUCCESS;
    if (p.opFn) {   // a user-defined operator has no blocks to scale -- and never reads the A in the buffer, scaled or not
        return (TFQMRGPU_PRECOND_NONE != p.precondKind) ? TFQ_ERR(TFQMRGPU_NO_IMPLEMENTATION) : TFQMRGPU_STATUS_SUCCESS;
    }
    bool const kept = kept_is_callers_a(p);
    if (p.held.precondInA == p.precondKind) return (kept && p.held.anyDirty) ? precond_update(h, p) : TFQMRGPU_STATUS_SUCCESS;
    if (TFQMRGPU_PRECOND_NONE != p.held.precondInA) {
        // the kind has changed since A was scaled: only a fresh setMatrix('A') brings the caller's A back -- or the kept copy
        if (!kept) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'A');
        if (auto const st = precond_restore(h, p)) return st;
        if (TFQMRGPU_PRECOND_NONE == p.precondKind) return TFQMRGPU_STATUS_SUCCESS;
    }
    if (!p.buffer) return TFQ_ERR(TFQMRGPU_POINTER_INVALID);
    if (!p.held.haveA) return err(TFQMRGPU_UNDOCUMENTED_ERROR, __LINE__ % 10000, 'A');
    hipStream_t const s = (hipStream_t)h.stream;
    if (!p.layout.precond) {
        if (auto const st = p.layout.precond.reserve(precond_bytes(p))) return st;
        auto const m = precond_mem(p);
        TFQ_HIP(hipMemcpyAsync(m.diag, p.diagOfRow.data(), p.diagOfRow.size() * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        if (p.nnzbA) TFQ_HIP(hipMemcpyAsync(m.colA, p.colOfA.data(), p.colOfA.size() * 4, hipMemcpyHostToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
    }
    auto const m = precond_mem(p);
    bool const mixed = ('m' == p.precision), wDbl = ('c' != p.precision);
    DevPlan const d = resolve_callers(p);      // mixed: M^-1 comes from the double copy of A
    if (p.keepA) {   // the caller's A, device to device, before it is scaled in place: block order, transposition and element order are the buffer's
        if (!p.held.aKept) if (auto const st = p.held.aKept.reserve(kept_a_bytes(p))) return st;
        auto const k = kept_a(p);
        TFQ_HIP(hipMemcpyAsync(k.a, d.A, k.aBytes, hipMemcpyDeviceToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        if (mixed) TFQ_HIP(hipMemcpyAsync(k.aFloat, p.buffer + p.wA.offset, k.aFloatBytes, hipMemcpyDeviceToDevice, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        // every row through the listed form: it leaves the flag per row that a later partial set-up recounts from
        launch_precond_invert_listed(d.dbl, wDbl, d.A, m.diag, m.minv, m.identity, nullptr, p.nRows, p.LM, d.ilv, s);
    } else {
        TFQ_HIP(hipMemsetAsync(m.counter, 0, 4, s), TFQMRGPU_STATUS_LAUNCH_FAILED)
        launch_precond_invert(d.dbl, wDbl, d.A, m.diag, m.minv, m.counter, p.nRows, p.LM, d.ilv, s);
    }
    // A_ij := A_ij M_jj^-1; the blocks are stored transposed, so this is block := (M_jj^-1)^T block
    launch_precond_apply(d.dbl, wDbl, true, d.A, p.nnzbA, m.colA, m.minv, p.LM, p.LM, d.ilv, s);
    if (mixed) launch_precond_apply(false, true, true, p.buffer + p.wA.offset, p.nnzbA, m.colA, m.minv, p.LM, p.LM, p.ilv, s);   // the float copy of the inner solves
    int32_t nIdentity = 0;
    if (auto const st = p.keepA ? count_identity_flags(p, m, s, nIdentity) : read_identity_counter(m, s, nIdentity)) return st;
    a_scaled(p, p.precondKind, nIdentity);
    return TFQMRGPU_STATUS_SUCCESS;
}

tfqmrgpuStatus_t precond_prepare(Handle& h, Plan& p) {
    try { return precond_prepare_(h, p); }   // (the lists of a partial set-up are host vectors; no exception may cross the C boundary)
    catch (std::bad_alloc const&) { return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
}

// X := M^-1 Y at the end of a solve, on the solver's stream ('m': once, in double, on the refined solution)
tfqmrgpuStatus_t precond_back(Handle& h, Plan& p) {
    if (TFQMRGPU_PRECOND_BLOCK_JACOBI != p.held.precondInA) return TFQMRGPU_STATUS_SUCCESS;
    auto const m = precond_mem(p);
    DevPlan const d = resolve_callers(p);
    launch_precond_apply(d.dbl, 'c' != p.precision, false, d.x, p.nnzbX, d.rowI, m.minv, p.LM, p.LN, d.ilv, (hipStream_t)h.stream);
    TFQ_HIP(hipGetLastError(), TFQMRGPU_STATUS_LAUNCH_FAILED)
    p.last.flops_performed += 8. * p.LM * p.LM * p.LN * p.nnzbX;
    return TFQMRGPU_STATUS_SUCCESS;
}

} // namespace tfq
