// Block-Jacobi right preconditioner (tfqmrgpu_ext.h section 7): with M = blockdiag(A) the solver iterates on (A M^-1) Y = B and
// returns X = M^-1 Y.  Three kernels, none of them part of an iteration:
//   k_precond_invert   M_ii^-1 for every block row, once per setMatrix('A')
//   k_precond_apply    A_ij := A_ij M_jj^-1 over the blocks of A (once per setMatrix('A')), X_ic := M_ii^-1 Y_ic at the end of a solve
// Both products have ONE block product per result block, so they are done in place and need no pair list.
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
    constexpr int CPT = invert_cpt(LM), NG = LM / CPT, NT = LM * NG, P = LM * LM;
    __shared__ double2 colv[LM], rowK[LM], rowP[LM];
    __shared__ int piv[LM];
    __shared__ int notFinite;
    uint32_t const row = blockIdx.x;
    uint32_t const ia = diagOfRow[row];
    int const t = threadIdx.x;
    TW* const out = Minv + size_t(row) * 2 * P;
    if (~0u == ia) {                                       // no diagonal block in the pattern: M_ii = 1
        store_identity(out, LM, t, int(blockDim.x));
        if (0 == t) atomicAdd(nIdentity, 1u);
        return;
    }
    bool const active = (t < NT);
    int const r = t % LM, g = (t / LM) % NG;
    TA const* const blk = A + size_t(ia) * 2 * P;
    double ar[CPT], ai[CPT];
#pragma unroll
    for (int j = 0; j < CPT; ++j) {                        // M[r][c] sits at (k = c, i = r) of the transposed block
        int const off = plane_offset(ilv, g * CPT + j, r, LM);
        ar[j] = double(blk[off]); ai[j] = double(blk[P + off]);
    }
    bool singular = false;
    if (0 == t) notFinite = 0;                          // (visible behind the first barrier of the loop below)
    for (int k = 0; k < LM; ++k) {
        int const gk = k / CPT, jk = k % CPT;
        if (active && g == gk) {
            double vr = 0, vi = 0;
#pragma unroll
            for (int j = 0; j < CPT; ++j) if (j == jk) { vr = ar[j]; vi = ai[j]; }
            colv[r] = make_double2(vr, vi);
        }
        __syncthreads();
        // the pivot: the first row of the largest magnitude among k ... LM - 1 -- every thread finds the same one
        int p = k; double best = -1.; bool finite = true;
        for (int q = k; q < LM; ++q) {
            double2 const v = colv[q];
            double const m = fmax(fabs(v.x), fabs(v.y));
            if (!(m <= 1.7e308)) finite = false;           // inf or NaN
            if (m > best) { best = m; p = q; }
        }
        if (!finite || !(best > 0.)) { singular = true; break; }   // (uniform: no thread waits at a barrier below)
        if (active && r == k) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) rowK[g * CPT + j] = make_double2(ar[j], ai[j]);
        }
        if (active && r == p) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) rowP[g * CPT + j] = make_double2(ar[j], ai[j]);
        }
        if (0 == t) piv[k] = p;
        __syncthreads();
        double2 const pv = colv[p];
        double2 inv;                                        // 1 / pivot without squaring it (Smith)
        if (fabs(pv.x) >= fabs(pv.y)) { double const q = pv.y / pv.x, d = pv.x + pv.y * q; inv = make_double2(1. / d, -q / d); }
        else                          { double const q = pv.x / pv.y, d = pv.x * q + pv.y; inv = make_double2(q / d, -1. / d); }
        // after the exchange row k is the pivot row and row p is what row k was
        double2 const f = (r == p) ? colv[k] : colv[r];     // this row's multiplier (row k itself: not used)
        if (r == p && p != k) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) { double2 const v = rowK[g * CPT + j]; ar[j] = v.x; ai[j] = v.y; }
        }
#pragma unroll
        for (int j = 0; j < CPT; ++j) {
            int const c = g * CPT + j;
            double2 pr = rowP[c];
            if (c == k) pr = make_double2(1., 0.);          // in place: column k becomes column k of the inverse
            double const sr = pr.x * inv.x - pr.y * inv.y, si = pr.x * inv.y + pr.y * inv.x;
            if (r == k) { ar[j] = sr; ai[j] = si; }
            else {
                double const br = (c == k) ? 0. : ar[j], bi = (c == k) ? 0. : ai[j];
                ar[j] = br - (f.x * sr - f.y * si); ai[j] = bi - (f.x * si + f.y * sr);
            }
        }
        __syncthreads();                                    // the next step rewrites colv, rowK, rowP
    }
    if (!singular) {                                        // an overflow on the way, or a NaN that never reached a pivot column: nothing but finite numbers is stored
        constexpr double kMax = (sizeof(TW) == 4) ? 3.4e38 : 1.7e308;   // finite in the precision it is stored in
        bool bad = false;
#pragma unroll
        for (int j = 0; j < CPT; ++j) bad = bad || !(fabs(ar[j]) <= kMax) || !(fabs(ai[j]) <= kMax);
        if (active && bad) notFinite = 1;
        __syncthreads();
        singular = (0 != notFinite);
    }
    if (singular) {                                         // a pivot that is zero or not finite, or a result that is not finite: M_ii = 1
        store_identity(out, LM, t, int(blockDim.x));
        if (0 == t) atomicAdd(nIdentity, 1u);
        return;
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {                        // inverse of the row-exchanged block -> of the block: its columns exchanged back, last exchange first
        int c = g * CPT + j;
        for (int k = LM - 1; k >= 0; --k) { int const pk = piv[k]; if (c == k) c = pk; else if (c == pk) c = k; }
        out[r * LM + c] = TW(ar[j]); out[P + r * LM + c] = TW(ai[j]);
    }
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
    T* const blk = data + size_t(live ? b : 0) * 2 * P;
    TW const* const W = Minv + size_t(live ? wOfBlock[b] : 0) * 2 * LM * LM;
    double accr[MAXE], acci[MAXE];
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
        accr[m] = 0.; acci[m] = 0.;
        int const e = lt + m * tpb;
        if (live && e < P) {
            int const r = e / nC, s = e % nC;
            for (int l = 0; l < LM; ++l) {
                int const wo = TRANSW ? l * LM + r : r * LM + l;
                double const wr = double(W[wo]), wi = double(W[LM * LM + wo]);
                int const io = plane_offset(ilv, l, s, nC);
                double const xr = double(blk[io]), xi = double(blk[P + io]);
                accr[m] += wr * xr - wi * xi; acci[m] += wr * xi + wi * xr;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MAXE; ++m) {
        int const e = lt + m * tpb;
        if (live && e < P) {
            int const o = plane_offset(ilv, e / nC, e % nC, nC);
            blk[o] = T(accr[m]); blk[P + o] = T(acci[m]);
        }
    }
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

} // namespace tfq
