// Host-side plan of one bsrsv problem: the reference-visible analysis results
// (bit-exact with real-space/tfQMRgpu createPlan, tfqmrgpu.cu:136-351) plus the
// MI355X-specific device layout derived from them; and the shape list and shape rules that the plan and the kernels share.
#pragma once
#include <cstdint>
#include <cstddef>
#include <utility>
#include <vector>
#include <hip/hip_runtime_api.h>

#include "tfqmrgpu.h"
#include "tfqmrgpu_ext.h"

namespace tfq {

// error code packing (tfqmrgpu.h:179-181 of the reference)
inline tfqmrgpuStatus_t err(int code, int line = 0, int key = 0) {
    return code + TFQMRGPU_CODE_LINE * line + TFQMRGPU_CODE_CHAR * key;
}
#define TFQ_ERR(code) ::tfq::err((code), __LINE__ % 10000)

inline size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

// ---- library-owned memory: every allocation the library makes for itself has ONE owner, whose destructor releases it.  destroyPlan,
// DestroyHandle and multiplyRelease are `delete`.  What in a plan must not outlive a layout or a buffer stands in the group that bufferSize
// or setBuffer ends with one assignment (Plan::Layout, Plan::Held): a new member of this kind needs a line in its group and nowhere else
struct DevMem {     // device memory (hipMalloc), move-only
    void* ptr = nullptr;
    size_t bytes = 0;
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { release(); std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); } return *this; }
    DevMem(DevMem const&) = delete;
    DevMem& operator=(DevMem const&) = delete;
    ~DevMem() { release(); }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
    // at least n bytes.  Grows only, and never copies: what is there is FREED before the larger piece is allocated -- a launch of an earlier
    // call may still read the old piece, and hipFree waits for the device
    tfqmrgpuStatus_t reserve(size_t n) {
        if (ptr && n <= bytes) return TFQMRGPU_STATUS_SUCCESS;
        release();
        if (hipSuccess != hipMalloc(&ptr, n)) { ptr = nullptr; return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
        bytes = n;
        return TFQMRGPU_STATUS_SUCCESS;
    }
    template <typename T> T* as() const { return static_cast<T*>(ptr); }
    explicit operator bool() const { return nullptr != ptr; }
};

// pinned host memory in kDepth slots with an event (no timing) behind each: the copies of the control block that a solve reads back
// (tfq_solve.cpp: Slots).  It lives with the plan: hipHostMalloc and event creation cost more than a small solve
struct PinnedRing {
    static constexpr int kDepth = 4;
    void* ptr = nullptr;
    hipEvent_t event[kDepth] = {};
    PinnedRing() = default;
    PinnedRing(PinnedRing const&) = delete;
    PinnedRing& operator=(PinnedRing const&) = delete;
    ~PinnedRing() { release(); }
    void release() {
        for (auto& e : event) { if (e) (void)hipEventDestroy(e); e = nullptr; }
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
    }
    tfqmrgpuStatus_t ensure(size_t slotBytes) {     // all of it or nothing
        if (ptr) return TFQMRGPU_STATUS_SUCCESS;
        if (hipSuccess != hipHostMalloc(&ptr, kDepth * slotBytes, hipHostMallocDefault)) { ptr = nullptr; return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
        for (auto& e : event)
            if (hipSuccess != hipEventCreateWithFlags(&e, hipEventDisableTiming)) { e = nullptr; release(); return TFQ_ERR(TFQMRGPU_STATUS_ALLOCATION_FAILED); }
        return TFQMRGPU_STATUS_SUCCESS;
    }
};

// Long block columns are summed by several work groups (tfq_colops.hpp: column_total).  A segment is what one work group sums in ONE
// round of loads (256 / LN lane groups x 16 records in flight); columns of at most four segments stay with one work group.  The plan sizes
// DevPlan::colPart by the same rule: a column with more segments than the plan counted would never see its last arrival.
constexpr uint32_t col_seg_len(int LN) { return uint32_t(256 / LN) * 16u; }
constexpr uint32_t col_segments(uint32_t n, int LN) { return (n <= 4 * col_seg_len(LN)) ? 1u : (n + col_seg_len(LN) - 1) / col_seg_len(LN); }
constexpr uint32_t kColSlot = 64;      // granule of the slot numbering of colPart (tfq_colops.hpp: col_part_slot; <= the shortest segment: LN = 64)

// The 15 (LM, LN) pairs of the solver, in the order of the reference's table (allowed_block_sizes.h:4-18): kAllowedBlockSizes is generated
// from it, and so are the instances of tfq_vec.hip and of the multiply's family launchers (tfq_spmm.hpp)
#define TFQ_SIZES(X, R) \
    X(R, 4, 4) X(R, 4, 5) X(R, 4, 8) X(R, 4, 32) X(R, 8, 8) X(R, 8, 9) X(R, 8, 10) X(R, 8, 32) X(R, 8, 64) \
    X(R, 16, 16) X(R, 16, 32) X(R, 16, 64) X(R, 32, 32) X(R, 32, 64) X(R, 64, 64)

// f(Shape<R, LM, LN>{}) for the instance of that list that a plan of this storage type and block shape needs.  false: there is none, and
// f has not been called -- a missing instance is the caller's error to report, never a fall-back
template <typename R, int LM_, int LN_> struct Shape { using real = R; static constexpr int LM = LM_, LN = LN_; };
template <typename F>
inline bool for_shape(bool dbl, int lm, int ln, F const& f) {
    int const key = lm * 1000 + ln;
#define TFQ_CASE(R, LM, LN) case LM * 1000 + LN: f(Shape<R, LM, LN>{}); return true;
    if (dbl) { switch (key) { TFQ_SIZES(TFQ_CASE, double) default: break; } }
    else     { switch (key) { TFQ_SIZES(TFQ_CASE, float)  default: break; } }
#undef TFQ_CASE
    return false;
}

// Waves per 16-row strip of a Y block in k_spmm_mfma | k_spmm_mfma_m (rb: bytes per accumulator element): two, each with LN / 2 columns,
// where the double accumulators of a whole strip and two operand slices would not fit the 256 VGPRs of two waves per SIMD
// (128 columns: 128 VGPRs of accumulators)
constexpr int mfma_col_split(int rb, int ln) { return (8 == rb && ln >= 128) ? 2 : 1; }
// Row tiles (16 rows each) per wave of these kernels, for mt row tiles per block and nt column tiles per wave: two where the block has them
// and the accumulators (2 * nt complex tiles) stay within 64 VGPRs
constexpr int mfma_row_tiles(int mt, int nt, int rb) { return (mt % 2 == 0 && 2 * nt * rb <= 32) ? 2 : 1; }
// Units of work (strips of a Y block, one per wave and pass) per Y block: the plan cuts its chunks by it, the stand-alone multiply its work groups
constexpr int mfma_units(int lm, int ln, int rb) {
    int const cs = mfma_col_split(rb, ln), mt = lm / 16;
    return (mt / mfma_row_tiles(mt, ln / (16 * cs), rb)) * cs;
}

struct Window { size_t offset = 0, bytes = 0; };

// one unit of work of the vector kernels: a run of blocks inside ONE block column
struct ChunkTable {
    std::vector<uint32_t> first;   // [nChunks+1] first internal block of each chunk
    std::vector<uint32_t> col;     // [nChunks]   compressed block column
    std::vector<uint32_t> colPtr;  // [nCols+1]   first chunk of each column
    std::vector<uint32_t> order;   // [nChunks]   launch order of the multiply (XCD aware)
    std::vector<uint32_t> orderB;  // column batches (Plan::colBatch): the chunks of the batches' first columns, in the same kind of order
};

// tfqmrgpuExt_truncationLeak (tfqmrgpu_ext.h section 11): the block products A_ik X_kc that land on a block row i outside block column c
// of X.  A leak position is one such (c, i); positions are sorted by (c, i), the products of a position by ascending k; a work unit is a
// run of positions of ONE column (tfq_leak_host.cpp)
struct LeakListing {
    std::vector<uint32_t> pairs;          // [2*nProducts] (A block in the caller's order, X block in the internal order), as Plan::pairs_i
    std::vector<uint32_t> posStart;       // [nPos+1] first product of each position
    std::vector<uint32_t> posCol, posRow; // [nPos] compressed block column and block row of each position
    std::vector<uint32_t> unitFirst;      // [nUnits+1] first position of each work unit
    std::vector<uint32_t> colUnitPtr;     // [nCols+1] first work unit of each column
    bool built = false;
    size_t nPositions() const { return posCol.size(); }
    size_t nProducts() const { return pairs.size() / 2; }
    size_t nUnits() const { return unitFirst.empty() ? 0 : unitFirst.size() - 1; }
};
// the blocks of A grouped by block column (ascending block index inside a column), from the block column of every block
void a_by_column(uint32_t nRows, std::vector<uint32_t> const& colOfA, std::vector<uint32_t>& cscPtr, std::vector<uint32_t>& cscBlock);
// products per work unit at most (a position with more is a unit of its own), by the block shape
uint32_t leak_unit_products(int LM, int LN);
// the listing from plain index arrays (all zero based): row and column of every A block, A by block column (a_by_column), row and
// compressed column of every X block in the caller's order, and its internal index.  false: more than 2^31 products
bool leak_listing(LeakListing& out, uint32_t nRows, uint32_t nCols,
    uint32_t nnzbA, uint32_t const* rowOfA, uint32_t const* colOfA, uint32_t const* cscPtr, uint32_t const* cscBlock,
    uint32_t nnzbX, uint32_t const* rowOfX, uint32_t const* colOfX, uint32_t const* u2i, uint32_t maxProducts);

// tfqmrgpuExt_growPattern (tfqmrgpu_ext.h section 12): the BSR pattern of X with chosen leak positions added, as the caller writes it
struct GrownPattern {
    std::vector<int32_t> rowPtr;          // [nRows+1] with the index offset
    std::vector<int32_t> colInd;          // [nnzb] the caller's block column indices
    std::vector<int32_t> oldBlock;        // [nnzb] the block of the old pattern (caller's order), -1: added
};
// The old pattern from plain index arrays -- row and compressed column of every X block in the caller's order, the caller's index of
// every compressed column (ascending) -- plus the positions take[0 .. nTake) of posRow / posCol (take == nullptr: all nPos, nTake ignored).
// Every block row keeps its old blocks in their order; the added ones follow, ascending by column.  0: done; 1: an index >= nPos or an
// index named twice; 2: more than 2^31 blocks.  `out` is empty unless 0 is returned
int grow_pattern(GrownPattern& out, uint32_t nRows, uint32_t nCols, uint32_t nnzbX, uint32_t const* rowOfX, uint32_t const* colOfX,
    int32_t const* callersCol, int indexOffset, size_t nPos, uint32_t const* posRow, uint32_t const* posCol, uint64_t nTake, uint64_t const* take);

// tfqmrgpuExt_dropCost (tfqmrgpu_ext.h section 13): the plan's own block products (Plan::pairs) grouped by their X operand.  Everything
// is indexed by the caller's block order of X, so that the kernel writes its record where the caller reads it; xOf says where the values
// of a block lie in the buffer.  The products of a block keep the order of the pair list (tfq_leak_host.cpp: drop_listing)
struct DropListing {
    std::vector<uint32_t> start;          // [nnzbX+1] first product of each X block
    std::vector<uint32_t> aOf;            // [nPairs] the A block of each product, in the caller's order of A
    std::vector<uint32_t> xOf;            // [nnzbX] internal index of each X block
    bool built = false;
};
// from the pair list (A block, X block in the caller's order) and the internal index of every X block: one stable counting sort by
// X block, O(nPairs + nnzbX)
void drop_listing(DropListing& out, uint32_t nnzbX, size_t nPairs, uint32_t const* pairs, uint32_t const* u2i);

// tfqmrgpuExt_shrinkPattern (section 13): the old pattern, as for grow_pattern, without the blocks drop[0 .. nDrop) (the caller's block
// order); hasB[x] != 0: block x carries a block of B.  Every block row keeps its other blocks in their order; oldBlock is never -1.
// 0: done; 1: an index < 0 or >= nnzbX or an index named twice; 2: a listed block carries B.  `out` is empty unless 0 is returned
int shrink_pattern(GrownPattern& out, uint32_t nRows, uint32_t nnzbX, uint32_t const* rowOfX, uint32_t const* colOfX,
    int32_t const* callersCol, int indexOffset, uint8_t const* hasB, uint64_t nDrop, int32_t const* drop);

// tfqmrgpuExt_carry (tfqmrgpu_ext.h section 15): the caller's block map between two plans (tfq_carry_host.cpp)
constexpr uint32_t kCarryZero = 0xffffffffu;   // an entry of the composed list: this block of the destination becomes zero
// nBlocks is the destination's block count; without a list (the identity) both operands have as many blocks; every entry is -1 (a zero
// block) or a block of the source
bool carry_map_ok(int64_t nBlocks, int32_t const* oldBlock, uint32_t nnzbDst, uint32_t nnzbSrc);
// out[n] = the STORED block of the source that stored block n of the destination takes, or kCarryZero.  dstI2U: the caller's index of
// every stored block of the destination, srcU2I: the stored index of every block of the source in the caller's order (nullptr: stored
// in the caller's order, as A and B are); oldBlock == nullptr: the identity.  The map has passed carry_map_ok
void carry_compose(std::vector<uint32_t>& out, uint32_t nnzbDst, int32_t const* oldBlock, uint32_t const* dstI2U, uint32_t const* srcU2I);

struct Handle {
    void* stream = nullptr;               // hipStream_t
    // multi-GPU stopping test (tfqmrgpu_ext.h section 4)
    void* comm = nullptr;                 // ncclComm_t, RCCL loaded lazily
    int nranks = 1, rank = 0;
    tfqmrgpuReduceMax_t reduceFn = nullptr;
    void* reduceCtx = nullptr;
    DevMem voteBuf;                       // 4 doubles of device memory for the collective in front of a solve (RCCL path)
};

struct Plan {
    uint32_t magic = 0x7f51a9d3u;

    // ---- analysis results, identical to the reference's bsrsv_plan_t members ----------
    uint32_t nRows = 0, nCols = 0, nnzbA = 0, nnzbX = 0, nnzbB = 0;
    int indexOffset = 0;
    std::vector<uint32_t> pairs;               // [2*nPairs] (inzA, inzX), user order
    std::vector<uint32_t> starts;              // [nnzbX+1]
    std::vector<uint32_t> subset;              // [nnzbB]
    std::vector<uint16_t> colindx;             // [nnzbX]
    std::vector<int32_t>  original_bsrColIndX; // [nCols]

    // ---- internal (device) order of the X-shaped vectors: sorted by (column, row) --------
    std::vector<uint32_t> col32;       // [nnzbX] compressed column of each user block (32 bit)
    std::vector<uint32_t> rowOfX;      // [nnzbX] block row of each user block
    std::vector<uint32_t> u2i, i2u;    // user index <-> internal index
    std::vector<uint32_t> colStart;    // [nCols+1] internal block range of each column
    std::vector<uint32_t> starts_i;    // [nnzbX+1] pair list regrouped by internal Y index
    std::vector<uint32_t> pairs_i;     // [2*nPairs] (inzA user, inzX internal)
    std::vector<uint32_t> subset_i;    // [nnzbB] internal X index of each B block
    std::vector<uint32_t> bcol;        // [nnzbB] compressed column of each B block
    std::vector<uint32_t> bColPtr, bList; // B blocks grouped by compressed column
    std::vector<uint32_t> bOfX;        // [nnzbX] internal order: B block sitting on this X block, or ~0
    std::vector<uint32_t> rowI;        // [nnzbX] block row, internal order
    std::vector<int32_t>  origCol;     // [nCols] original_bsrColIndX without the index offset (what the device keeps, DevPlan::origCol)
    ChunkTable chunks;

    // ---- fixed by bufferSize -----------------------------------------------------------------
    int LM = 0, LN = 0;
    int lm = 0, ln = 0;                // the caller's block shape, as given to bufferSize: (LM, LN) unless the plan is padded (tfqmrgpu_ext.h section 18)
    char precision = 0;               // 'c', 'z' or 'm' (mixed: float inner iterations, double refinement; tfq_solve.cpp: run_mixed)
    size_t realBytes = 0;              // 4 or 8 (the storage precision of the iteration vectors: 4 for 'm')
    size_t S = 0;                      // bytes of one X-shaped vector
    size_t bufferBytes = 0;
    bool aOnce = false;                // nPairs <= 1.5 x the A blocks that occur in the pair list: A is streamed once per multiply
    int ilv = 0;                       // element order inside the blocks of this plan's buffer (tfq_device.hpp: ilv_offset)
    int ilvZ = 0;                      // 'm': element order of the double-precision arrays (x, B, A, A x), the one a 'z' plan of this shape has

    // windows into the user's device buffer
    Window wX, wV4, wV5, wV6, wV7, wV8, wV9, wV3, wB, wA;
    Window wRho, wAlfa, wBeta, wC67, wEta, wC67a, wEta2; // [nCols][2][LN] real
    Window wZ, wD, wTau, wVar, wInvBn2;        // double scalars per right-hand side
    Window wStatus;                            // int8 [nCols][LN]
    Window wCtl;                               // device control block (tfq_device.hpp: Ctl)
    Window wPz, wPd;                           // per-chunk partial sums (double)
    Window wColRec;                            // per-column stopping-test record [nCols][2] double
    Window wColPart; uint32_t colSegMax = 1;   // shares of the segment work groups of long columns (tfq_colops.hpp: column_total), segments of the longest column
    Window wChunkFirst, wChunkCol, wColChunkPtr, wColStart, wOrigCol, wBofX, wOrder;
    Window wColBatch, wOrderB; std::vector<uint8_t> colBatch;   // batches of block columns with identical row patterns (empty: none); layoutBuffer
    Window wStarts, wPairs, wSubset, wBColPtr, wBList, wU2I, wRowI;
    // 'm' only: the solution, B and A in double; the residual of the refinement as the right-hand side of the inner (float) solve,
    // |b|^2 per right-hand side, the record of the refinement's stopping test
    Window wXz, wBz, wAz, wR, wBn2z, wRefine;
    Window wFold, wSelf;               // arrival counters [nCols + 1] and a device copy of the DevPlan for the folded column operations
    bool selfStale = true;             // the device copy of the DevPlan (wSelf) predates a change of a plan flag (shadow vector, product form): refresh before a folded solve
    bool foldOk = false;               // few enough chunks that an iteration slot is launch latency: fold (tfq_colops.hpp)

    char* buffer = nullptr;            // device buffer registered by setBuffer
    static constexpr int kDepth = PinnedRing::kDepth;   // iterations the host keeps enqueued ahead of the stopping decision
    PinnedRing ring;                   // pinned copies of the control block, one per in-flight iteration, and the event behind each copy
    int shadowMode = TFQMRGPU_SHADOW_HASH;
    bool v3IsHash = false;             // the buffer's v3 holds the counter-based hash (set by setBuffer, cleared by a user-supplied vector)
    bool threeProducts = false;        // tfqmrgpuExt_setThreeProductMultiply: Gauss' three real products per complex one in the double multiplies
    void* opFn = nullptr; void* opCtx = nullptr;   // user-defined operator (tfqmrgpu_ext.h section 5): the callback
    // block-Jacobi right preconditioner (tfqmrgpu_ext.h section 7)
    std::vector<uint32_t> diagOfRow;   // [nRows] the diagonal block of each block row of A, ~0u: the pattern has none
    std::vector<uint32_t> colOfA;      // [nnzbA] block column of each block of A
    std::vector<uint32_t> rowOfA;      // [nnzbA] block row of each block of A (for the truncation leak, section 11)
    std::vector<uint32_t> cscPtr, cscBlock;    // the blocks of A grouped by block column, built at the first setBlocks('A') into a kept copy or the first leak listing
    int precondKind = TFQMRGPU_PRECOND_NONE;     // what the caller asked for
    bool keepA = false;                // tfqmrgpuExt_keepOperator: keep the caller's own A next to the scaled one (tfqmrgpu_ext.h section 9)
    int32_t precondIdentity = 0;       // block rows whose M_ii is the unit matrix (no diagonal block, or a singular one), as of the last set-up; outlives bufferSize and setBuffer
    double mixedFloor = 0;             // 'm': the gain at which the first float solve of this plan's last solve ran into its floor (0: not known; forgotten with a new A, NOT with a new layout: a_new_layout)
    DropListing drop;                  // tfqmrgpuExt_dropCost (section 13): the pairs grouped by X block, built at the first call that needs it; patterns only, it outlives bufferSize
    void* warmR = nullptr;             // not null only while a warm solve runs: resolve() hands it to the driver as DevPlan::R
    int startDepth = 0;                // tfqmrgpuExt_keepStarts (section 17): the depth of the ring of kept starts; it stays, as the preconditioner kind does
    bool keepSum = false;              // tfqmrgpuExt_keepSum (section 19b): the plan keeps a weighted sum of X on B's pattern; it stays, as the depth of the starts does
    bool allowPad = false;             // tfqmrgpuExt_allowPadding (section 18): bufferSize may pick a listed shape above the caller's; it stays, as the preconditioner kind does
    DevMem padUnit;                    // padded plans: [nnzbA] bytes, 1 for the diagonal blocks of A (the caller's block order), built from diagOfRow and uploaded at the
                                       // first padded transfer of A; the pattern's, so it outlives layouts and buffers
    bool padded() const { return lm != LM || ln != LN; }

    // ---- device lists that only grow (reserve), each filled again by every call that reads it: they outlive layouts and buffers
    DevMem keepList;                   // [dirty rows | blocks of the dirty columns] of a partial set-up (tfq_precond_host.cpp: precond_update)
    DevMem blockList;                  // setBlocks / getBlocks (tfqmrgpu_ext.h section 8): the caller's block list
    DevMem carryList;                  // tfqmrgpuExt_carry (section 15), on the DESTINATION plan: the composed block list (tfq_carry_host.cpp: carry_compose)

    // ---- of the layout: sized or cut by (LM, LN, precision) and the chunk tables, built by the first call that needs it and found there by
    // every later one.  bufferSize ends it (tfq_precond_host.cpp: a_new_layout), with `layout = Layout{}`
    struct Layout {
        DevMem opScratch;              // user-defined operator: [xu | yu | i2u | colindx in the caller's block order] (tfq_solve.cpp: op_scratch)
        DevMem residualScratch;        // tfqmrgpuExt_residual (section 10): [nChunks][2][LN] + [nCols][2][LN] doubles
        // tfqmrgpuExt_truncationLeak (section 11): the listing (its work units are cut by the block shape, its X indices are the internal
        // ones) and its device copy [pairs | posStart | unitFirst | colUnitPtr | records [nUnits][LN] | column sums [nCols][LN]], uploaded
        // at the first call that asks for leak2
        LeakListing leak;
        DevMem leakDev;
        DevMem leakMapRec;             // tfqmrgpuExt_leakMap (section 12): one [LN] record of doubles per leak position; the listing on the device is leakDev's
        DevMem dropDev;                // tfqmrgpuExt_dropCost (section 13): Plan::drop on the device [start | aOf | xOf | cost records [nnzbX][LN] | weight records [nnzbX][LN]]
        // tfqmrgpuExt_selectDrop / selectLeak (section 20), each allocated and its lists uploaded by the first call of its kind:
        // [colOf (kSelExcluded: carries B) | colStart | i2u | flags [nnzbX] | tile counts | selected blocks | spent [nCols][LN]] and
        // [posCol | first position of each column | flags [nPos] | tile counts | selected positions | left [nCols][LN]]
        DevMem selectDrop, selectLeak;
        DevMem precond;                // block-Jacobi: [M^-1 | diagOfRow | colOfA | counter | flags], allocated at the first preconditioned solve
    } layout;

    // ---- of the buffer: values that belong to ONE registered buffer, and what that buffer holds.  bufferSize and setBuffer end it
    // (tfq_precond_host.cpp: a_new_buffer), with `held = Held{}`
    struct Held {
        // tfqmrgpuExt_solveFrom (section 14): [X0 | R], two X-shaped vectors of the plan's storage type, allocated by the first call.
        // tfqmrgpuExt_refineFrom (section 16) on an 'm' plan: the same two vectors, of doubles
        DevMem warm;
        // start projection (section 17; tfq_project_host.cpp): the ring of kept starts -- Plan::startDepth X-shaped vectors in the plan's storage
        // type and internal order, start i (0: the newest) in slot (startHead + i) % startDepth, allocated by the first pushStart -- and the
        // scratch of projectStart [images W | records | gamma | nUsed], allocated by its first call
        DevMem startMem, projectMem;
        int startCount = 0, startHead = 0;
        // the state of the A in the buffer: what it holds, and what is stale.  Written by the transitions of tfq_precond_host.cpp
        // (a_new_layout ... a_restored) and by nobody else
        bool haveA = false;            // a whole setMatrix('A') has succeeded on this buffer
        int precondInA = TFQMRGPU_PRECOND_NONE;  // what the A in the buffer has been scaled with (NONE: it is the caller's A)
        DevMem aKept;                  // device copy of the A window as it was before it was scaled ('m': the double A, then the float A);
                                       // it is the caller's A while precondInA != NONE, stale otherwise
        std::vector<uint8_t> dirtyRow, dirtyCol;   // [nRows] since the last set-up setBlocks('A') has written: the diagonal block of this row | a block of this column
        bool anyDirty = false;
        // energy mesh (section 19; tfq_mesh_host.cpp).  shiftBase: [nRows][LM][2] the diagonal of the caller's A in the storage type ('m':
        // double), captured by the first shiftDiagonal behind a WHOLE write of A (shiftBaseFresh: none since; a_set_whole clears it).
        // shiftStaleRow [nRows], shiftAnyStale: setBlocks('A') has written the diagonal block of this row since (a_patch_written): the next
        // shift captures these rows again, through the device list shiftRows.  shiftDiag: diagOfRow on the device where layout.precond has no
        // copy of it.  All allocated by the shiftDiagonal that first needs them.
        // sumMem: S [nnzbB][LM][LN][2] of double, allocated and cleared by the first addToSum; sumTerms: the addToSum calls since the last clear
        DevMem shiftBase, shiftDiag, shiftRows;
        bool shiftBaseFresh = false, shiftAnyStale = false;
        std::vector<uint8_t> shiftStaleRow;
        DevMem sumMem;
        int32_t sumTerms = 0;
    } held;

    // ---- of the last solve: what it leaves for getInfo, the histories and the profile.  The start of the next solve ends it
    // (tfq_solve.cpp: reset_results), with `last = Last{}`
    struct Profile { int64_t launches[16] = {}; double ms[16] = {}; };
    struct Last {
        double flops_performed = -1;   // (-1: no solve yet)
        int iterations_needed = -1;
        std::vector<double> boundHistory;
        std::vector<double> cycleResidual;     // 'm': relative residual (double arithmetic) in front of every inner solve and at the end
        std::vector<int32_t> cycleIterations;  // 'm': float iterations of every inner solve
        int refinementCycles = 0;
        Profile all;                   // the launches that did work
        Profile gated;                 // launches that found the solve stopped / no probe requested
        Profile first;                 // of `all`: the launches of the first iteration (they skip the operands that are zero there)
    } last;
    double residuum_reached = 0;       // of the last solve that came to its end: a solve that is refused behind its reset leaves it
    double flops_performed_all = 0;    // over all solves
    int profiling = 0;                 // 0 off, 1 every kernel class, 2 the two fused multiplies only

    size_t nPairs() const { return pairs.size() / 2; }
};

inline Plan* asPlan(tfqmrgpuBsrsvPlan_t p) {
    auto q = reinterpret_cast<Plan*>(p);
    return (q && q->magic == 0x7f51a9d3u) ? q : nullptr;
}

// index analysis, tfq_plan.cpp
tfqmrgpuStatus_t analyse(Plan& p, int mb,
    int32_t const* rowPtrA, int nnzbA, int32_t const* colIndA,
    int32_t const* rowPtrX, int nnzbX, int32_t const* colIndX,
    int32_t const* rowPtrB, int nnzbB, int32_t const* colIndB,
    int indexOffset, int echo);

// derive chunk tables + buffer windows for (LM, LN, precision); tfq_plan.cpp
tfqmrgpuStatus_t layoutBuffer(Plan& p, int LM, int LN, char precision);

// The index lists of a laid-out plan that setBuffer uploads, in the order of their windows in the buffer: layoutBuffer sizes the windows from
// this list and setBuffer walks it, so that a window and its upload cannot disagree.  data == nullptr: nothing to upload
struct IndexList { Window* window; void const* data; size_t bytes; };
std::vector<IndexList> indexLists(Plan& p);

// the 15 compiled (ldA, ldB) pairs of the reference (TFQ_SIZES)
extern int const kAllowedBlockSizes[15][2];
bool blockSizeAllowed(int lm, int ln);
// padded plans (tfqmrgpu_ext.h section 18): the listed shape with LM >= lm and LN >= ln that has the smallest LM for which such an LN exists,
// then the smallest such LN (the products cost LM^2 LN).  A listed shape picks itself.  false: there is none (lm or ln above 64)
bool paddedBlockSize(int lm, int ln, int& LM, int& LN);

} // namespace tfq
