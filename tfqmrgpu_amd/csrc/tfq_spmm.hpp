// Block-sparse multiply Y = A*X for gfx950 (MI355X), with the vector updates that follow it in the tfQMR iteration fused into the epilogue.
//
// Contract (same as the reference kernel gemmNxNf, real-space/tfQMRgpu tfqmrgpu_blockmult.hxx:9-93 and its launcher tfqmrgpu_blocksparse.hxx:71-199):
//     Y[iY][c][i][j] = sum_{p in starts[iY]..starts[iY+1]} sum_k A[pairs[2p]][c'][k][i] * X[pairs[2p+1]][c''][k][j]
// complex arithmetic on split Re/Im planes, A blocks stored transposed ([k][i]), accumulation in the storage precision.  Flop count
// nPairs*8*LM*LM*LN (tfqmrgpu_blocksparse.hxx:198).  A work group processes one chunk (run of Y blocks of one block column, tfq_plan.cpp), so
// the per-RHS scalars of the epilogue are uniform and the dot / norm contributions leave the work group as one [LN] record (deterministic order).
//
// Kernel families, one translation unit per group (every kernel instance lives in exactly one); spmm_select (tfq_spmm.hip) picks one per launch.
// On the plans that keep groups of rows interleaved (tfq_device.hpp: ilv_offset; every operand, epilogue operand and result of a lane is one
// 16-byte access), the hot shapes of the BASELINE configurations:
//  * tfq_spmm_ilv16.hip: k_spmm_ilv16 (16 x 16 complex<double>, row pairs: configs 2 and 4), k_spmm_ilv16f (16 x 16 complex<float>, row quads),
//    k_spmm_ilvf (16 | 32 | 64 x 32 | 64 complex<float>, row quads; 32 x 32: config 3);
//  * tfq_spmm_ilv8.hip: k_spmm_ilv8 | k_spmm_ilv8b (8 x 8 complex<double>, a block = one access; b: column batches, config 5), k_spmm_ilv8w
//    (8 x 32 | 64 | 9 | 10 complex<double>, row pairs), k_spmm_ilv8f (8 x 8 | 32 | 64 complex<float>, row quads, two products per tile);
// on the reference's native order (every other shape, caller-owned arrays of tfqmrgpuExt_multiply, TFQMRGPU_ILV=0):
//  * tfq_spmm_mfma.hip: k_spmm_mfma (LM and LN multiples of 16: a wave keeps a strip of a Y block in MFMA accumulators; in the stand-alone
//    multiply also 48 | 96 | 128 square, TFQ_MULTIPLY_SIZES), k_spmm_mfma_m (tfqmrgpuExt_multiply in `m`: float data, double accumulators);
//  * tfq_spmm_pad.hip: k_spmm_pad (tfqmrgpuExt_multiply on 6 | 12 | 24 square, and `m` on the 4- and 8-row shapes: operands through a
//    zero-padded LDS image into 16 x 16 MFMA tiles);
//  * tfq_spmm_ilv8.hip: k_spmm_mfma8 (LM == 8, and 4 x 32 z: [Re A; Im A] x [Re X | Im X] fills one 16 x 16 tile per 8 block columns);
//  * tfq_spmm_rows4.hip: k_spmm_m4 (4 x 4 | 8 | 32 in double, v_mfma_f64_4x4x4_4b_f64), k_spmm_s4w (4 x 8 | 32 in float, 4 x 4 without
//    epilogue: two | four neighbouring columns per lane), k_spmm_small4 (the other 4-row shapes: one lane per element, operands through LDS);
//  * tfq_spmm.hip: k_spmm_n16 (tfqmrgpuExt_multiply, 16 x 16), k_spmm_direct (one thread per output element; only as the epilogue of a
//    user-defined operator).
// This header: what the kernels of every family share (launch arguments, epilogue arithmetic, operand and stream helpers), the shapes each
// family takes and the family launchers.  tfq_spmm_ilv.hpp: what only the kernels on the interleaved orders share (work-group prologue, the
// epilogue operands of a 16-byte piece, the plane exchange).
// Three pieces below follow the rule of tfq_spmm_ilv.hpp -- a kernel uses one only where every instance keeps its assembly with it
// (scripts/isa_compare.sh against the parent commit), elsewhere the block stays written out in the kernel:
//   epi_scalar             k_spmm_small4, k_spmm_m4, k_spmm_s4w, k_spmm_ilv16, k_spmm_ilv16f, k_spmm_ilv8, k_spmm_mfma, k_spmm_direct
//   rhs_block              k_spmm_small4, k_spmm_m4, k_spmm_s4w, k_spmm_ilv16, k_spmm_ilv16f, k_spmm_ilv8b, k_spmm_ilv8w, k_spmm_ilv8f, k_spmm_direct
//   IndexPatch             k_spmm_small4, k_spmm_m4, k_spmm_s4w (limits, row ranges, clamped pair read; the staging loops written out)
#pragma once
#include <cstdlib>
#include <type_traits>

#include "tfq_device.hpp"
#include "tfq_vec.hpp"
#include "tfq_switch.hpp"
#include "tfq_colops.hpp"

namespace tfq {

struct SpmmArgs {
    void* Y; void const* A; void const* X;
    uint32_t const* starts; uint32_t const* pairs;
    uint32_t nY;                       // number of Y blocks (plain mode)
    uint32_t const* chunkFirst;        // nullptr: plain mode, chunk b = blocks [b*CH, (b+1)*CH)
    uint32_t const* chunkCol;
    uint32_t const* order;             // launch order: work group b processes chunk order[b] (nullptr: b)
    uint32_t CH;
    Ctl const* ctl; int gate;          // 0: always run, 1: skip when the solve has stopped, 2: only when probing
    void* e0; void const* e1; void const* sc; float const* v3;
    void const* B; uint32_t const* bOfX;       // bOfX == nullptr: B is a whole X-shaped vector (block y of B belongs to Y block y: the
                                               // residual of the mixed-precision refinement as the right-hand side, DevPlan::R)
    double* pz; double* pd;
    void const* Yext; uint32_t const* yPerm;   // k_spmm_direct only: take block y of the product from Yext[yPerm[y]]
    int hashV3;                        // the shadow vector is the counter-based hash (tfq_device.hpp): recompute it, do not read it
    int32_t const* origCol; uint32_t const* rowI;   // original block column per compressed column, block row per Y block
    int ilv;                           // element order of the plan's blocks (tfq_device.hpp: ilv_offset); the plain mode is always native
    int aOnce;                         // every A block is used about once per multiply (few block columns): stream A past the caches
    int first;                         // EPI_XPAY_DOT in the first iteration of a solve: old v4 = v8 = 0 by definition, not read (DevPlan::first)
                                       // (EPI_AXPY_NRM_DOT with `late`: v5 is B under X, or R, there -- nothing has written it yet)
    void const* e2; int late;          // EPI_AXPY_NRM_DOT of the "late v5" slot (DevPlan::lateV5, k_spmm_ilv16 only): e0 holds the v5 in FRONT of k_v5_nrm's half
                                       // step, which that kernel has summed but not stored; the epilogue applies it first -- v5 := alfa v8 + (alfa v9 + v5), v9 = e2
    int m3;                            // double shapes above 16 x 16: three real products per complex one (tfqmrgpuExt_setThreeProductMultiply)
    DevPlan const* foldPlan;           // not null: the column operation that consumes this launch's records runs in its tail (tfq_colops.hpp)
    uint8_t const* colBatch; uint32_t const* colStart; uint32_t const* colChunkPtr;   // k_spmm_ilv8b: (batch size << 4) | position per block column; block / chunk ranges of the columns
    uint32_t const* yOrder;            // plain mode, not null: a prepared order (tfq_order.cpp) -- position i of the launch computes Y block yOrder[i]
    uint32_t plainPer;                 // plain mode of k_spmm_mfma, not 0: XCD x (work groups x, x + 8, ...) takes the chunks [x * plainPer, (x + 1) * plainPer)
};

// data that a kernel touches once (epilogue vectors) moves non-temporally, so that the stream does not push the A and
// X blocks, which neighbouring work groups re-use, out of the L2 (measured on P2: fused multiply 0.825 -> 0.777 ms)
// Only where a wave's access covers runs of at least 64 bytes: 32-byte runs (the 8-column tiles of k_spmm_mfma8 in
// float) as non-temporal partial writes cost 2x (8x32 `c`: 1.27 -> 2.79 ms), so STREAM is a template switch.
template <bool STREAM, typename T> __device__ inline T ld_stream(T const* p) { if constexpr (STREAM) return __builtin_nontemporal_load(p); else return *p; }
template <bool STREAM, typename T> __device__ inline void st_stream(T* p, T v) { if constexpr (STREAM) __builtin_nontemporal_store(v, p); else *p = v; }

template <int EPI> struct EpiPlanes { static constexpr int N = (EPI == EPI_XPAY_DOT) ? 2 : (EPI == EPI_AXPY_NRM_DOT) ? 3 : (EPI == EPI_RESIDUAL) ? 1 : 0; };

// Every epilogue writes its complex updates and reductions as explicit fused multiply-adds (tfq_device.hpp: fma_), the same pattern in every kernel.
// v4 := v9 + s (v8 + s v4)   (u = old v4, x = v8, y = v9 = A v6; tfqmrgpu_core.hxx:196-202)
template <typename R> __device__ inline void epi_xpay2(R& nr, R& ni, R yr, R yi, R ur, R ui, R xr, R xi, R sr, R si) {
    R const tr = fma_(-si, ui, fma_(sr, ur, xr)), ti = fma_(sr, ui, fma_(si, ur, xi));
    nr = fma_(-si, ti, fma_(sr, tr, yr)); ni = fma_(sr, ti, fma_(si, tr, yi));
}
// v5 := s v8 + v5   (u = old v5, y = v8 = A v6; tfqmrgpu_core.hxx:224-228)
// (the "late v5" slot, SpmmArgs::late: the same form twice with the same s, first with y = v9 -- k_v5_nrm's half step, tfqmrgpu_core.hxx:205 -- then with y = v8)
template <typename R> __device__ inline void epi_axpy(R& nr, R& ni, R yr, R yi, R ur, R ui, R sr, R si) {
    nr = fma_(-si, yi, fma_(sr, yr, ur)); ni = fma_(sr, yi, fma_(si, yr, ui));
}
// pz += v3 . d (unconjugated), pd += |d|^2, in double
__device__ inline void epi_dot(double& p0, double& p1, double dr, double di, double wr, double wi) {
    p0 = __builtin_fma(-di, wi, __builtin_fma(dr, wr, p0)); p1 = __builtin_fma(di, wr, __builtin_fma(dr, wi, p1));
}
__device__ inline void epi_nrm(double& p, double dr, double di) { p = __builtin_fma(di, di, __builtin_fma(dr, dr, p)); }

// per-element epilogue; off = offset of the element's real part in an X-shaped vector, P = plane size.
// In two steps so that a kernel can request the operands (old v4|v5, v8, v3) before its block products and use
// them behind: EpiElem::load, epilogue_apply; epilogue() is the two in a row.
template <typename R, int EPI, bool STREAM>
struct EpiElem {
    R ur, ui, xr, xi; float wr, wi;
    __device__ inline void load(SpmmArgs const& a, size_t off, int P) {
        if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
            wr = ld_stream<STREAM>(a.v3 + off); wi = ld_stream<STREAM>(a.v3 + off + P);
        }
        if constexpr (EPI == EPI_XPAY_DOT) if (a.first) { ur = 0; ui = 0; xr = 0; xi = 0; return; }
        if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
            R const* u = (R const*)a.e0;
            ur = ld_stream<STREAM>(u + off); ui = ld_stream<STREAM>(u + off + P);
        }
        if constexpr (EPI == EPI_XPAY_DOT) {
            R const* v8 = (R const*)a.e1;
            xr = ld_stream<STREAM>(v8 + off); xi = ld_stream<STREAM>(v8 + off + P);
        }
    }
};

template <typename R, int EPI, bool STREAM>
__device__ inline void epilogue_apply(SpmmArgs const& a, size_t off, int P, R yr, R yi, R sr, R si,
                                      EpiElem<R, EPI, STREAM> const& o, uint32_t bq, int eoff, double* acc /* [planes] */)
{
    if constexpr (EPI == EPI_NONE) {
        st_stream<STREAM>((R*)a.Y + off, yr); st_stream<STREAM>((R*)a.Y + off + P, yi);
    } else if constexpr (EPI == EPI_XPAY_DOT) {
        // v9 := A v6 (kept for the v5 update); v4 := v8 + beta v4; v4 := v9 + beta v4; pz += v3 . v4
        // (tfqmrgpu_core.hxx:196-202)
        st_stream<STREAM>((R*)a.Y + off, yr); st_stream<STREAM>((R*)a.Y + off + P, yi);
        R* v4 = (R*)a.e0;
        R ur, ui;
        epi_xpay2(ur, ui, yr, yi, o.ur, o.ui, o.xr, o.xi, sr, si);
        st_stream<STREAM>(v4 + off, ur); st_stream<STREAM>(v4 + off + P, ui);
        epi_dot(acc[0], acc[1], ur, ui, o.wr, o.wi);
    } else if constexpr (EPI == EPI_AXPY_NRM_DOT) {
        // v8 := A v6; v5 := alfa v8 + v5; pd += |v5|^2; pz += v3 . v5  (tfqmrgpu_core.hxx:224-228,189)
        st_stream<STREAM>((R*)a.Y + off, yr); st_stream<STREAM>((R*)a.Y + off + P, yi);
        R* v5 = (R*)a.e0;
        R nr, ni;
        epi_axpy(nr, ni, yr, yi, o.ur, o.ui, sr, si);
        st_stream<STREAM>(v5 + off, nr); st_stream<STREAM>(v5 + off + P, ni);
        epi_dot(acc[0], acc[1], nr, ni, o.wr, o.wi);
        epi_nrm(acc[2], nr, ni);
    } else { // EPI_RESIDUAL: |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
        R rr = yr, ri = yi;
        if (bq != 0xffffffffu) {
            R const* b = (R const*)a.B + size_t(bq) * 2 * P;
            rr += R(-1) * b[eoff]; ri += R(-1) * b[eoff + P];
        }
        epi_nrm(acc[0], rr, ri);
    }
}

template <typename R, int EPI, bool STREAM = true>
__device__ inline void epilogue(SpmmArgs const& a, size_t off, int P, R yr, R yi, R sr, R si,
                                uint32_t bq, int eoff, double* acc /* [planes] */)
{
    EpiElem<R, EPI, STREAM> o;
    o.load(a, off, P);
    epilogue_apply<R, EPI, STREAM>(a, off, P, yr, yi, sr, si, o, bq, eoff, acc);
}

template <int EPI>
__device__ inline void write_record(SpmmArgs const& a, uint32_t chunk, int LN, int p, int j, double v) {
    // (folded: the record is read by ANOTHER work group of this launch, the last one of the column -- coherent store, tfq_colops.hpp: co_store)
    bool const co = (a.foldPlan != nullptr);
    if constexpr (EPI == EPI_XPAY_DOT) st_record(a.pz + (size_t(chunk) * 2 + p) * LN + j, v, co);
    else if constexpr (EPI == EPI_AXPY_NRM_DOT) { if (p < 2) st_record(a.pz + (size_t(chunk) * 2 + p) * LN + j, v, co); else st_record(a.pd + size_t(chunk) * LN + j, v, co); }
    else if constexpr (EPI == EPI_RESIDUAL) st_record(a.pd + size_t(chunk) * LN + j, v, co);
}

// the column operation behind a fused multiply, run by the last work group of the column (small systems, tfq_colops.hpp)
template <typename R, int LN, int EPI>
__device__ inline void spmm_fold(SpmmArgs const& a, uint32_t col) {
    __shared__ ColScratch sc;
    constexpr int WHAT = (EPI == EPI_XPAY_DOT) ? FOLD_DEC34 : (EPI == EPI_AXPY_NRM_DOT) ? FOLD_DECT_FINAL : FOLD_PROBE;
    fold_tail<R, LN, WHAT>(*a.foldPlan, col, sc);
}

__device__ inline bool gate_closed(SpmmArgs const& a) {
    if (a.gate == 0) return false;
    if (a.ctl->state != 0) return true;
    return (a.gate == 2 && a.ctl->probe == 0);
}

// The scalar of an updating epilogue for right-hand side j of block column col: its real (im = 0) or imaginary (im = 1) part
template <typename R> __device__ __forceinline__ R epi_scalar(SpmmArgs const& a, uint32_t col, int LN, int im, int j) {
    return ((R const*)a.sc)[(size_t(col) * 2 + im) * LN + j];
}

// EPI_RESIDUAL: the block of B that belongs to Y block y (every other epilogue: none)
template <int EPI> __device__ __forceinline__ uint32_t rhs_block(SpmmArgs const& a, uint32_t y) {
    if constexpr (EPI == EPI_RESIDUAL) return a.bOfX ? a.bOfX[y] : y;
    return 0xffffffffu;
}

// The index patch of the 4-row kernels: the row ranges and index pairs of a whole chunk, fetched into LDS once, so that a batch of products waits
// for one memory latency.  This struct holds the limits and the reads; the kernel declares the two arrays (Starts, Pairs), hands them to the reads
// and, where inLds, fills them -- starts[i] = a.starts[first + i] for i <= nRows, pairs[i] = a.pairs[2 * qBase + i] for i < 2 * (qEnd - qBase) -- with a
// barrier behind.  (Those two loops stay written out in the three kernels: as a constructor or member here they change the assembly.)
// A chunk of more than kRows rows or kPairs pairs is not staged (!inLds): its kernel reads the lists from global memory
template <uint32_t kPairs> struct IndexPatch {
    static constexpr uint32_t kRows = 256;
    using Starts = uint32_t[kRows + 1]; using Pairs = uint32_t[2 * kPairs];
    uint32_t qBase, qEnd, nRows; bool inLds;   // the chunk's products are [qBase, qEnd) of the pair list
    __device__ __forceinline__ IndexPatch(SpmmArgs const& a, uint32_t first, uint32_t last)
        : qBase(a.starts[first]), qEnd(a.starts[last]), nRows(last - first) {      // (uniform: scalar loads)
        inLds = (nRows <= kRows) && (qEnd - qBase <= kPairs);
    }
    // row kr of the chunk has the products [start(kr), start(kr + 1)), as positions in the patch
    __device__ __forceinline__ uint32_t start(Starts const& starts, uint32_t kr) const { return starts[kr] - qBase; }
    // (A block, X block) of product q; a q past the patch reads its last slot (unconditional: all reads of a batch in flight at once)
    __device__ __forceinline__ static void pair(Pairs const& pairs, uint32_t q, uint32_t& ia, uint32_t& ix) {
        uint32_t const qc = min(q, kPairs - 1);
        ia = pairs[2 * qc]; ix = pairs[2 * qc + 1];
    }
};

using d4 = __attribute__((ext_vector_type(4))) double;
using f4 = __attribute__((ext_vector_type(4))) float;
template <typename R> struct Acc;
template <> struct Acc<double> {
    using T = d4;
    __device__ static inline T mma(double a, double b, T c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    // C/D layout of v_mfma_f64_16x16x4_f64: register r of lane l is row (l/16) + 4 r, column l%16
    __device__ static inline int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <> struct Acc<float> {
    using T = f4;
    __device__ static inline T mma(float a, float b, T c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    // C/D layout of v_mfma_f32_16x16x4_f32: register r of lane l is row 4 (l/16) + r, column l%16
    __device__ static inline int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

// NT consecutive elements as one access (NT * sizeof(R) bytes, naturally aligned by construction)
template <typename R, int N> struct VecOf { using T = R __attribute__((ext_vector_type(N))); };
template <typename R, int N>
__device__ inline void vload(R (&dst)[N], R const* p) {
    if constexpr (N == 1) dst[0] = *p;
    else {
        auto const v = *reinterpret_cast<typename VecOf<R, N>::T const*>(p);
#pragma unroll
        for (int i = 0; i < N; ++i) dst[i] = v[i];
    }
}
template <typename R, int N>
__device__ inline void vstore(R* p, R const (&src)[N]) {
    if constexpr (N == 1) *p = src[0];
    else {
        typename VecOf<R, N>::T v;
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = src[i];
        *reinterpret_cast<typename VecOf<R, N>::T*>(p) = v;
    }
}
// the same for data that is touched once (epilogue vectors): non-temporal where STREAM (see ld_stream above)
template <bool STREAM, typename R, int N>
__device__ inline void vload_stream(R (&dst)[N], R const* p) {
    if constexpr (!STREAM) vload<R, N>(dst, p);
    else if constexpr (N == 1) dst[0] = __builtin_nontemporal_load(p);
    else {
        auto const v = __builtin_nontemporal_load(reinterpret_cast<typename VecOf<R, N>::T const*>(p));
#pragma unroll
        for (int i = 0; i < N; ++i) dst[i] = v[i];
    }
}
template <bool STREAM, typename R, int N>
__device__ inline void vstore_stream(R* p, R const (&src)[N]) {
    if constexpr (!STREAM) vstore<R, N>(p, src);
    else if constexpr (N == 1) __builtin_nontemporal_store(src[0], p);
    else {
        typename VecOf<R, N>::T v;
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = src[i];
        __builtin_nontemporal_store(v, reinterpret_cast<typename VecOf<R, N>::T*>(p));
    }
}

// the vectors an epilogue reads, for the NT neighbouring elements of one lane in one row
template <typename R, int EPI, int NT, bool HASH = false, int STREAMSEL = -1>
struct EpiOps {
    static constexpr bool STREAM = (STREAMSEL < 0) ? (16 * NT * sizeof(R) >= 128) : (STREAMSEL != 0);   // a lane group covers whole 128-byte lines (STREAMSEL: the kernel knows better)
    R ur[NT], ui[NT], xr[NT], xi[NT];
    float wr[NT], wi[NT];
    __device__ inline void load(SpmmArgs const& a, size_t off, int P) {
        if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
            if constexpr (!HASH) { vload_stream<STREAM, float, NT>(wr, a.v3 + off); vload_stream<STREAM, float, NT>(wi, a.v3 + off + P); }   // HASH: recomputed in epilogue_row
        }
        if constexpr (EPI == EPI_XPAY_DOT) if (a.first) {          // first iteration of a solve: old v4 = v8 = 0, not read
#pragma unroll
            for (int n = 0; n < NT; ++n) { ur[n] = 0; ui[n] = 0; xr[n] = 0; xi[n] = 0; }
            return;
        }
        if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
            vload_stream<STREAM, R, NT>(ur, (R const*)a.e0 + off); vload_stream<STREAM, R, NT>(ui, (R const*)a.e0 + off + P);
        }
        if constexpr (EPI == EPI_XPAY_DOT) { vload_stream<STREAM, R, NT>(xr, (R const*)a.e1 + off); vload_stream<STREAM, R, NT>(xi, (R const*)a.e1 + off + P); }
    }
};

// epilogue for VW neighbouring elements at `off` (same arithmetic per element as epilogue<> above); the elements
// are columns n0 .. n0 + VW - 1 of the NT columns of the lane (per-RHS scalars sr/si and partial sums are per column)
template <typename R, int EPI, int VW, int NPL, int NT, bool HASH = false, int LN = 16, typename OPS>
__device__ inline void epilogue_row(SpmmArgs const& a, size_t off, int P, R const (&yr)[VW], R const (&yi)[VW],
                                    R const (&sr)[NT], R const (&si)[NT], int n0, OPS const& o,
                                    uint32_t bq, int eoff, double (&part)[NPL > 0 ? NPL : 1][NT], uint64_t key)
{
    if constexpr (EPI != EPI_RESIDUAL) { vstore_stream<OPS::STREAM, R, VW>((R*)a.Y + off, yr); vstore_stream<OPS::STREAM, R, VW>((R*)a.Y + off + P, yi); }
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
        R nr[VW], ni[VW];
#pragma unroll
        for (int n = 0; n < VW; ++n) {
            R const cr = sr[n0 + n], ci = si[n0 + n];
            if constexpr (EPI == EPI_XPAY_DOT) epi_xpay2(nr[n], ni[n], yr[n], yi[n], o.ur[n], o.ui[n], o.xr[n], o.xi[n], cr, ci);
            else epi_axpy(nr[n], ni[n], yr[n], yi[n], o.ur[n], o.ui[n], cr, ci);
            double wr, wi;   // the shadow vector: read, or recomputed from its hash (tfq_device.hpp)
            if constexpr (HASH) { uint64_t const hq = shadow_quad(key, uint32_t(eoff + n) / (2 * LN), uint32_t(eoff + n) % LN, LN); int const odd = (uint32_t(eoff + n) / LN) & 1; wr = shadow_pick(hq, odd, 0); wi = shadow_pick(hq, odd, 1); }
            else { wr = o.wr[n]; wi = o.wi[n]; }
            epi_dot(part[0][n0 + n], part[1][n0 + n], nr[n], ni[n], wr, wi);
            if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[2][n0 + n], nr[n], ni[n]);
        }
        vstore_stream<OPS::STREAM, R, VW>((R*)a.e0 + off, nr); vstore_stream<OPS::STREAM, R, VW>((R*)a.e0 + off + P, ni);
    } else if constexpr (EPI == EPI_RESIDUAL) {
        R br[VW] = {}, bi[VW] = {};
        if (bq != 0xffffffffu) {
            R const* b = (R const*)a.B + size_t(bq) * 2 * P;
            vload<R, VW>(br, b + eoff); vload<R, VW>(bi, b + eoff + P);
        }
#pragma unroll
        for (int n = 0; n < VW; ++n) {
            R const rr = yr[n] + R(-1) * br[n], ri = yi[n] + R(-1) * bi[n];
            epi_nrm(part[0][n0 + n], rr, ri);
        }
    }
}

using d2v = __attribute__((ext_vector_type(2))) double;
using f2v = __attribute__((ext_vector_type(2))) float;
using f4v = __attribute__((ext_vector_type(4))) float;

// ---------------------------------------------------------------------------------------------------
// The kernel families of the multiply, in the order spmm_select (tfq_spmm.hip) tries them
enum class SpmmKernel { s4w, m4, ilv16, ilv16f, ilvf, ilv8b, ilv8, ilv8f, ilv8w, mfma, mfma8, small4, direct };

// The block shapes of each family (dbl: complex<double>).  spmm_select tests them at run time; a family launcher instantiates its
// kernels under `if constexpr` of the same predicates, i.e. for exactly the shapes the selector can hand it.
// 4-row blocks: k_spmm_s4w in float, k_spmm_m4 in double, where the columns come in fours
constexpr bool takes_s4w(bool dbl, int lm, int ln) { return lm == 4 && !dbl && ln % 4 == 0; }
constexpr bool takes_m4(bool dbl, int lm, int ln) { return lm == 4 && dbl && ln % 4 == 0; }
// the interleaved element orders (plan-owned blocks only): row pairs in double, row quads in float
constexpr bool takes_ilv16(bool dbl, int lm, int ln) { return lm == 16 && ln == 16 && dbl; }
constexpr bool takes_ilv16f(bool dbl, int lm, int ln) { return lm == 16 && ln == 16 && !dbl; }
constexpr bool takes_ilvf(bool dbl, int lm, int ln) { return !dbl && lm % 16 == 0 && (ln == 32 || ln == 64); }
constexpr bool takes_ilv8(bool dbl, int lm, int ln) { return lm == 8 && ln == 8 && dbl; }   // k_spmm_ilv8 and, with column batches, k_spmm_ilv8b
constexpr bool takes_ilv8f(bool dbl, int lm, int ln) { return lm == 8 && (ln == 8 || ln == 32 || ln == 64) && !dbl; }
constexpr bool takes_ilv8w(bool dbl, int lm, int ln) { return lm == 8 && (ln == 32 || ln == 64 || ln == 9 || ln == 10) && dbl; }
// the native order
constexpr bool takes_mfma(bool, int lm, int ln) { return lm % 16 == 0 && ln % 16 == 0; }
// k_spmm_mfma8: all 8-row shapes; of the 4-row ones only 4 x 32 in double -- elsewhere the half-empty tile moves too few bytes per memory
// instruction and k_spmm_small4 wins (measured, 5-point stencils of 256 MB per vector, multiply / iteration in ms, direct | tile | small4:
// 4x4 z 0.74/2.44 | 0.79/2.62 | 0.33/1.73, 4x5 z 0.76/2.71 | 0.65/2.46 | 0.51/2.21, 4x8 z 0.71/2.35 | 0.42/1.84 | 0.34/1.65, 4x32 z
// 0.67/2.35 | 0.24/1.62 | 0.35/1.69, 4x4 c 0.53/2.55 | 1.39/4.25 | 0.45/2.41, 4x5 c 0.97/3.30 | 1.12/3.79 | 0.77/2.82, 4x8 c 0.51/1.96 |
// 0.72/2.53 | 0.48/2.04, 4x32 c 0.49/1.95 | 0.30/2.10 | 0.45/2.00)
constexpr bool takes_mfma8(bool dbl, int lm, int ln) { return lm == 8 || (lm == 4 && dbl && ln == 32); }
// the 4-row shapes that k_spmm_mfma8 does not take, where k_spmm_s4w (s4w_columns) or k_spmm_m4 (lab: TFQMRGPU_M4=0) does not either
constexpr bool takes_small4(bool dbl, int lm, int ln) { return lm == 4 && !takes_mfma8(dbl, lm, ln); }

// Columns per lane of k_spmm_s4w for a launch of a takes_s4w shape; 0: the launch takes k_spmm_small4 (one column per lane).
// The multiply without epilogue gains on all three shapes with four (4 x 4 | 8 | 32 c: 0.387 -> 0.276, 0.267 -> 0.218, 0.265 -> 0.178 ms); the fused
// forms hold the epilogue operands and double partial sums of four columns per lane (169 VGPRs: two waves per SIMD) and gain only where a block has
// many column quads: 4 x 32 (-21 %); 4 x 8 is level, 4 x 4 loses 13 % (profiles/r04_four_row_shapes.txt).  The fused launches of 4 x 8 take TWO
// columns per lane (129 VGPRs): 0.472 / 0.434 -> 0.419 / 0.392 ms, iteration 1.497 -> 1.398; 4 x 4 stays with k_spmm_small4 (two columns per
// lane: 1.652 -> 1.684).  Lab: TFQMRGPU_S4W=0 = k_spmm_small4 for all; 2 = four columns for every launch; 3 = two columns for the fused ones.
inline int s4w_columns(int ln, int epi) {
    static int const use_s4w = lab_switch("TFQMRGPU_S4W", 1);
    if (use_s4w && (epi == EPI_NONE || ln == 32 || use_s4w == 2)) return 4;
    if (ln < 32 && ((use_s4w == 1 && ln == 8) || use_s4w == 3)) return 2;
    return 0;
}

// A variant choice of a family launcher as a template argument: f(std::true_type) where the run-time flag v is set and the kernel has the
// variant (OK), else f(std::false_type); the argument converts to the bool constant
template <bool OK, typename F> inline void variant(bool v, F&& f) {
    if constexpr (OK) if (v) { f(std::true_type{}); return; }
    f(std::false_type{});
}

// The block shapes the library is compiled for: TFQ_SIZES (tfq_plan.hpp), the solver's.
// The further shapes of the stand-alone multiply (tfqmrgpuExt_multiply, the reference's `bench multi`): the plain product only, on
// k_spmm_mfma in `c` and `z` and on k_spmm_mfma_m in `m`; no solver family is instantiated for them and the solver's list does not change
#define TFQ_MULTIPLY_SIZES(X, R) X(R, 48, 48) X(R, 96, 96) X(R, 128, 128)
// ... and those that do not fill 16 x 16 tiles, on k_spmm_pad: in every precision, and the 4- and 8-row shapes of TFQ_SIZES in `m`
#define TFQ_PAD_SIZES(X, R) X(R, 6, 6) X(R, 12, 12) X(R, 24, 24)
#define TFQ_PAD_M_SIZES(X, R) X(R, 4, 4) X(R, 4, 5) X(R, 4, 8) X(R, 4, 32) X(R, 8, 8) X(R, 8, 9) X(R, 8, 10) X(R, 8, 32) X(R, 8, 64)
#define TFQ_SIZE_IS(R, LM, LN) || (lm == LM && ln == LN)
constexpr bool solver_shape(int lm, int ln) { return false TFQ_SIZES(TFQ_SIZE_IS, 0); }            // one of TFQ_SIZES
constexpr bool wide_shape(int lm, int ln) { return false TFQ_MULTIPLY_SIZES(TFQ_SIZE_IS, 0); }     // one of TFQ_MULTIPLY_SIZES
constexpr bool pad_shape(int lm, int ln) { return false TFQ_PAD_SIZES(TFQ_SIZE_IS, 0); }           // one of TFQ_PAD_SIZES
#undef TFQ_SIZE_IS
#define TFQ_SIZE_IN(R, LM, LN) && solver_shape(LM, LN)
static_assert(true TFQ_PAD_M_SIZES(TFQ_SIZE_IN, 0), "TFQ_PAD_M_SIZES: shapes of TFQ_SIZES");
#undef TFQ_SIZE_IN

// The precisions of the stand-alone multiply (the reference's `bench multi`): `z` | `d` complex<double>, `m` float data summed in double,
// every other letter complex<float>
enum class MulPrec { c, z, m };

// Launches Family<R, LM, LN, EPI>::go(k, a, nWG, s) for the precision, shape and epilogue of a launch (nothing when nWG == 0);
// false: the shape is not one of TFQ_SIZES
template <template <typename, int, int, int> class Family, typename R, int LM, int LN>
void spmm_epi(SpmmKernel k, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    if (0 == nWG) return;
    switch (epi) {
    case EPI_NONE:         Family<R, LM, LN, EPI_NONE>::go(k, a, nWG, s); break;
    case EPI_XPAY_DOT:     Family<R, LM, LN, EPI_XPAY_DOT>::go(k, a, nWG, s); break;
    case EPI_AXPY_NRM_DOT: Family<R, LM, LN, EPI_AXPY_NRM_DOT>::go(k, a, nWG, s); break;
    case EPI_RESIDUAL:     Family<R, LM, LN, EPI_RESIDUAL>::go(k, a, nWG, s); break;
    }
}
template <template <typename, int, int, int> class Family>
bool spmm_switch(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    int const key = lm * 1000 + ln;
#define TFQ_CASE(R, LM, LN) case LM * 1000 + LN: spmm_epi<Family, R, LM, LN>(k, epi, a, nWG, s); return true;
    if (dbl) { switch (key) { TFQ_SIZES(TFQ_CASE, double) default: return false; } }
    else     { switch (key) { TFQ_SIZES(TFQ_CASE, float)  default: return false; } }
#undef TFQ_CASE
}

// The launchers of the family files: launch kernel family k (spmm_select's choice for this launch) on nWG work groups; false: the
// shape is not one of TFQ_SIZES
bool spmm_mfma(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s);    // mfma
// the stand-alone multiply (plain mode, no epilogue): k_spmm_mfma on TFQ_MULTIPLY_SIZES, and k_spmm_mfma_m (precision `m`) on every shape of
// TFQ_SIZES and TFQ_MULTIPLY_SIZES with LM and LN multiples of 16; false: not such a shape
bool spmm_mfma_wide(bool dbl, int lm, int ln, SpmmArgs const& a, uint32_t nWG, hipStream_t s);
bool spmm_mfma_m(int lm, int ln, SpmmArgs const& a, uint32_t nWG, hipStream_t s);
// k_spmm_pad on TFQ_PAD_SIZES (and TFQ_PAD_M_SIZES in `m`), a.nY Y blocks; false: not such a shape
bool spmm_pad(MulPrec p, int lm, int ln, SpmmArgs const& a, hipStream_t s);
bool spmm_ilv16(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s);   // ilv16, ilv16f, ilvf
bool spmm_ilv8(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s);    // ilv8b, ilv8, ilv8f, ilv8w, mfma8
bool spmm_rows4(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s);   // s4w, m4, small4

} // namespace tfq
