// Block-Jacobi right preconditioner (tfqmrgpu_ext.h section 7): with M = blockdiag(A) the solver iterates on (A M^-1) Y = B and
// returns X = M^-1 Y.  Three kernels, none of them part of an iteration:
//   k_precond_invert   M_ii^-1 for every block row, once per setMatrix('A')
//   k_precond_apply    A_ij := A_ij M_jj^-1 over the blocks of A (once per setMatrix('A')), X_ic := M_ii^-1 Y_ic at the end of a solve
// Both products have ONE block product per result block, so they are done in place and need no pair list.
// Each has a listed form for a plan that keeps the caller's A (section 9): chosen block rows inverted from the kept copy, chosen blocks
// scaled from the copy into the buffer.  The element loops are shared (tfq_precond_invert_body.hpp, tfq_precond_apply_body.hpp), so a block comes out with the same bits.
#include "tfq_device.hpp"
#include "tfq_precond.hpp"

namespace tfq {

// ---- inversion ------------------------------------------------------------------------------------------------------------------
// Gauss-Jordan in place with row exchanges (partial pivoting by max(|Re|, |Im|): no sum that could overflow), the column exchanges that undo them are
// folded into the store.  The block lives in REGISTERS: thread (r, g) holds row r, columns g CPT ... g CPT + CPT - 1, as doubles -- at
// 64 x 64 that is 16 complex numbers = 64 VGPRs per thread, 256 threads; the LDS only carries what a step hands from thread to thread:
// column k (the multipliers), the two rows that change places, the exchange list.  3 KiB at LM = 64 where the block itself would be 64 KiB.
// Lanes of one row group read the same LDS address (a broadcast), lanes of different groups addresses LM x 16 bytes apart: no lane
// group of a ds_read_b128 sees two addresses on one bank.
// One wave per block up to 16 x 16, one work group of four waves above.
constexpr int invert_cpt(int LM) { return (LM <= 8) ? 1 : (LM <= 32) ? 4 : 16; }
constexpr int invert_threads(int LM) { return (LM * (LM / invert_cpt(LM)) < 64) ? 64 : LM * (LM / invert_cpt(LM)); }

template <typename TW>
__device__ inline void store_identity(TW* out, int LM, int t, int nt) {
    int const P = LM * LM;
    for (int e = t; e < P; e += nt) { out[e] = (e / LM == e % LM) ? TW(1) : TW(0); out[P + e] = TW(0); }
}

template <int LM, typename TA, typename TW>
__global__ __launch_bounds__(invert_threads(LM)) void k_precond_invert(TA const* A, uint32_t const* diagOfRow, TW* Minv, uint32_t* nIdentity, int ilv) {
    uint32_t const row = blockIdx.x;
#define TFQ_INVERT_REPORT_IDENTITY atomicAdd(nIdentity, 1u)
#include "tfq_precond_invert_body.hpp"
#undef TFQ_INVERT_REPORT_IDENTITY
}

// the listed form (tfqmrgpu_ext.h section 9): work group k inverts block row rows[k] (rows == nullptr: row k), A may be the kept copy of
// the operator; isIdentity[row] := 1 where the row got the unit matrix, 0 where not
template <int LM, typename TA, typename TW>
__global__ __launch_bounds__(invert_threads(LM)) void k_precond_invert_listed(TA const* A, uint32_t const* diagOfRow, TW* Minv, uint32_t* isIdentity,
                                                                              uint32_t const* rows, int ilv) {
    uint32_t const row = rows ? rows[blockIdx.x] : blockIdx.x;
    if (0 == threadIdx.x) isIdentity[row] = 0u;            // (thread 0 is also the one that reports: its two stores keep their order)
#define TFQ_INVERT_REPORT_IDENTITY isIdentity[row] = 1u
#include "tfq_precond_invert_body.hpp"
#undef TFQ_INVERT_REPORT_IDENTITY
}

template <typename TA, typename TW>
static void invert_dispatch(TA const* A, uint32_t const* diagOfRow, TW* Minv, uint32_t* nIdentity, uint32_t nRows, int LM, int ilv, hipStream_t s) {
    dim3 const g(nRows);
    switch (LM) {
        case 4:  k_precond_invert<4,  TA, TW><<<g, dim3(invert_threads(4)),  0, s>>>(A, diagOfRow, Minv, nIdentity, ilv); break;
        case 8:  k_precond_invert<8,  TA, TW><<<g, dim3(invert_threads(8)),  0, s>>>(A, diagOfRow, Minv, nIdentity, ilv); break;
        case 16: k_precond_invert<16, TA, TW><<<g, dim3(invert_threads(16)), 0, s>>>(A, diagOfRow, Minv, nIdentity, ilv); break;
        case 32: k_precond_invert<32, TA, TW><<<g, dim3(invert_threads(32)), 0, s>>>(A, diagOfRow, Minv, nIdentity, ilv); break;
        case 64: k_precond_invert<64, TA, TW><<<g, dim3(invert_threads(64)), 0, s>>>(A, diagOfRow, Minv, nIdentity, ilv); break;
        default: break;                                     // (bufferSize admits no other block size)
    }
}

void launch_precond_invert(bool aDbl, bool wDbl, void const* A, uint32_t const* diagOfRow, void* Minv, uint32_t* nIdentity,
                           uint32_t nRows, int LM, int ilv, hipStream_t s)
{
    if (0 == nRows) return;
    if (aDbl && wDbl)        invert_dispatch((double const*)A, diagOfRow, (double*)Minv, nIdentity, nRows, LM, ilv, s);
    else if (!aDbl && !wDbl) invert_dispatch((float const*)A, diagOfRow, (float*)Minv, nIdentity, nRows, LM, ilv, s);
}

template <typename TA, typename TW>
static void invert_listed_dispatch(TA const* A, uint32_t const* diagOfRow, TW* Minv, uint32_t* isIdentity, uint32_t const* rows, uint32_t nListed, int LM, int ilv, hipStream_t s) {
    dim3 const g(nListed);
    switch (LM) {
        case 4:  k_precond_invert_listed<4,  TA, TW><<<g, dim3(invert_threads(4)),  0, s>>>(A, diagOfRow, Minv, isIdentity, rows, ilv); break;
        case 8:  k_precond_invert_listed<8,  TA, TW><<<g, dim3(invert_threads(8)),  0, s>>>(A, diagOfRow, Minv, isIdentity, rows, ilv); break;
        case 16: k_precond_invert_listed<16, TA, TW><<<g, dim3(invert_threads(16)), 0, s>>>(A, diagOfRow, Minv, isIdentity, rows, ilv); break;
        case 32: k_precond_invert_listed<32, TA, TW><<<g, dim3(invert_threads(32)), 0, s>>>(A, diagOfRow, Minv, isIdentity, rows, ilv); break;
        case 64: k_precond_invert_listed<64, TA, TW><<<g, dim3(invert_threads(64)), 0, s>>>(A, diagOfRow, Minv, isIdentity, rows, ilv); break;
        default: break;                                     // (bufferSize admits no other block size)
    }
}

void launch_precond_invert_listed(bool aDbl, bool wDbl, void const* A, uint32_t const* diagOfRow, void* Minv, uint32_t* isIdentity,
                                  uint32_t const* rows, uint32_t nListed, int LM, int ilv, hipStream_t s)
{
    if (0 == nListed) return;
    if (aDbl && wDbl)        invert_listed_dispatch((double const*)A, diagOfRow, (double*)Minv, isIdentity, rows, nListed, LM, ilv, s);
    else if (!aDbl && !wDbl) invert_listed_dispatch((float const*)A, diagOfRow, (float*)Minv, isIdentity, rows, nListed, LM, ilv, s);
}

// ---- block := W block, in place --------------------------------------------------------------------------------------------------
// A work group takes one block (several when a block has fewer than 256 elements); a thread keeps up to 16 elements of the result in
// registers, the barrier between the last load and the first store is what makes the product safe in place.  Column s of the result
// needs column s of the operand only, and the operand block (at most 64 KiB) stays in the caches over the LM passes.
template <typename T, typename TW, bool TRANSW>
__global__ __launch_bounds__(256) void k_precond_apply(T* data, uint32_t nBlocks, uint32_t const* wOfBlock, TW const* Minv, int LM, int nC, int ilv, int bpw) {
    constexpr int MAXE = 16;
    int const P = LM * nC;
    int const tpb = 256 / bpw;                             // threads per block of the operand
    int const lb = int(threadIdx.x) / tpb, lt = int(threadIdx.x) % tpb;
    uint32_t const b = blockIdx.x * uint32_t(bpw) + uint32_t(lb);
    bool const live = (lb < bpw) && (b < nBlocks);
    T* const dst = data + size_t(live ? b : 0) * 2 * P;
    TW const* const W = Minv + size_t(live ? wOfBlock[b] : 0) * 2 * LM * LM;
    T* const src = dst;                                    // in place
#include "tfq_precond_apply_body.hpp"
}

// the listed, out-of-place form (tfqmrgpu_ext.h section 9): entry k reads block list[k] of `from` and writes block list[k] of `to`
template <typename T, typename TW, bool TRANSW>
__global__ __launch_bounds__(256) void k_precond_apply_listed(T const* from, T* to, uint32_t nListed, uint32_t const* list, uint32_t const* wOfBlock,
                                                              TW const* Minv, int LM, int nC, int ilv, int bpw) {
    constexpr int MAXE = 16;
    int const P = LM * nC;
    int const tpb = 256 / bpw;
    int const lb = int(threadIdx.x) / tpb, lt = int(threadIdx.x) % tpb;
    uint32_t const k = blockIdx.x * uint32_t(bpw) + uint32_t(lb);
    bool const live = (lb < bpw) && (k < nListed);
    uint32_t const b = live ? list[k] : 0u;
    T const* const src = from + size_t(b) * 2 * P;
    T* const dst = to + size_t(b) * 2 * P;
    TW const* const W = Minv + size_t(live ? wOfBlock[b] : 0) * 2 * LM * LM;
#include "tfq_precond_apply_body.hpp"
}

template <typename T, typename TW>
static void apply_dispatch(bool transW, T* data, uint32_t nBlocks, uint32_t const* wOfBlock, TW const* Minv, int LM, int nC, int ilv, hipStream_t s) {
    int const P = LM * nC;
    if (P > 16 * 256) return;                              // (the largest block of the solver is 64 x 64)
    int const bpw = (P >= 256) ? 1 : 256 / P;
    dim3 const g((nBlocks + uint32_t(bpw) - 1) / uint32_t(bpw)), b(256);
    if (transW) k_precond_apply<T, TW, true ><<<g, b, 0, s>>>(data, nBlocks, wOfBlock, Minv, LM, nC, ilv, bpw);
    else        k_precond_apply<T, TW, false><<<g, b, 0, s>>>(data, nBlocks, wOfBlock, Minv, LM, nC, ilv, bpw);
}

void launch_precond_apply(bool dataDbl, bool wDbl, bool transW, void* data, uint32_t nBlocks, uint32_t const* wOfBlock,
                          void const* Minv, int LM, int nC, int ilv, hipStream_t s)
{
    if (0 == nBlocks) return;
    if (dataDbl && wDbl)        apply_dispatch(transW, (double*)data, nBlocks, wOfBlock, (double const*)Minv, LM, nC, ilv, s);
    else if (!dataDbl && wDbl)  apply_dispatch(transW, (float*)data,  nBlocks, wOfBlock, (double const*)Minv, LM, nC, ilv, s);
    else if (!dataDbl && !wDbl) apply_dispatch(transW, (float*)data,  nBlocks, wOfBlock, (float const*)Minv,  LM, nC, ilv, s);
}

template <typename T, typename TW>
static void apply_listed_dispatch(bool transW, T const* src, T* dst, uint32_t nListed, uint32_t const* list, uint32_t const* wOfBlock, TW const* Minv, int LM, int nC, int ilv, hipStream_t s) {
    int const P = LM * nC;
    if (P > 16 * 256) return;                              // (the largest block of the solver is 64 x 64)
    int const bpw = (P >= 256) ? 1 : 256 / P;
    dim3 const g((nListed + uint32_t(bpw) - 1) / uint32_t(bpw)), b(256);
    if (transW) k_precond_apply_listed<T, TW, true ><<<g, b, 0, s>>>(src, dst, nListed, list, wOfBlock, Minv, LM, nC, ilv, bpw);
    else        k_precond_apply_listed<T, TW, false><<<g, b, 0, s>>>(src, dst, nListed, list, wOfBlock, Minv, LM, nC, ilv, bpw);
}

void launch_precond_apply_listed(bool dataDbl, bool wDbl, bool transW, void const* src, void* dst, uint32_t nListed, uint32_t const* list,
                                 uint32_t const* wOfBlock, void const* Minv, int LM, int nC, int ilv, hipStream_t s)
{
    if (0 == nListed) return;
    if (dataDbl && wDbl)        apply_listed_dispatch(transW, (double const*)src, (double*)dst, nListed, list, wOfBlock, (double const*)Minv, LM, nC, ilv, s);
    else if (!dataDbl && wDbl)  apply_listed_dispatch(transW, (float const*)src,  (float*)dst,  nListed, list, wOfBlock, (double const*)Minv, LM, nC, ilv, s);
    else if (!dataDbl && !wDbl) apply_listed_dispatch(transW, (float const*)src,  (float*)dst,  nListed, list, wOfBlock, (float const*)Minv,  LM, nC, ilv, s);
}

} // namespace tfq
