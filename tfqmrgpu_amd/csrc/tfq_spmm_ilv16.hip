// The 16-row kernels on the plans' interleaved element orders: k_spmm_ilv16, k_spmm_ilv16f, k_spmm_ilvf (tfq_spmm.hpp)
#include "tfq_spmm_ilv.hpp"

namespace tfq {

// ---------------------------------------------------------------------------------------------------
// 16 x 16 complex<double> on the ROW-PAIR-INTERLEAVED element order (tfq_device.hpp: plane[r/2][s][r%2] for every block of
// the plan, A blocks with r = k): the structure of k_spmm_mfma (one wave owns the 16 x 16 strip of a Y block in MFMA
// accumulators, two operand register sets, epilogue operands requested behind the first two block products), but every
// access is 16 bytes per lane -- one wave instruction moves 1 KiB instead of 512 bytes:
//   k-steps: lane group lr = lane / 16 loads the k pairs lr and lr + 4, i.e. k = 2 lr, 2 lr + 1, 2 lr + 8, 2 lr + 9 feed the
//            four MFMA steps of a block product (which k a step contracts is free as long as A and X agree);
//   rows:    lane column a supplies A row rowp(a) = 2 (a % 4 + 4 (a / 8)) + (a / 4) % 2, so that the accumulator registers
//            (0, 1) and (2, 3) of lane group lr are the row pairs (2 lr, 2 lr + 1), (2 lr + 8, 2 lr + 9) of column lane % 16:
//            the epilogue reads and writes them as two 16-byte accesses per vector and plane.
// Measured on P2 against k_spmm_mfma on the native order (same box, scripts/lab, profiles/r02_lab.txt): fused multiplies
// 0.684 / 0.660 -> 0.628 / 0.595 ms.  The sums of a block product run over k in another order than in the native kernel
// (results differ in the last bits, within the tolerances of the parity tests).
__device__ inline int ilv_rowp(int a) { return 2 * ((a & 3) + 4 * (a >> 3)) + ((a >> 2) & 1); }

// ANT: the A operands are loaded non-temporally.  For an operator applied to one or two block columns every A block is used
// once per multiply -- the kernel is a stream of A through HBM, and 16-byte non-temporal loads take it from 5.5 to 6.6 TB/s
// (one block column, 1.3 GB of A: plain multiply 0.69 -> 0.82 of 8 TB/s, fused 0.76 -> 0.85, profiles/r02_lab.txt); with
// many columns A is re-used out of the caches and must stay there (the plan decides: SpmmArgs::aOnce).
// LATE (EPI_AXPY_NRM_DOT, SpmmArgs::late): the v5 this launch finds is the one in FRONT of k_v5_nrm's half step, which that kernel has summed but not
// stored.  The epilogue requests the v9 piece of its Y block with its other operands and forms v5 + alfa v9 first -- the two fused multiply-adds of
// k_v5_nrm on the same operands, the same bits -- then its own step, and stores v5 once: a store of S leaves a kernel that is bound by HBM and enters one
// that is not.  With FIRST the old v5 is the right-hand side (the B block under the Y block, or zeros; DevPlan::R: block y of R), as ld_rhs reads it
template <int EPI, bool HASH, bool ANT = false, bool FIRST = false, bool LATE = false>   // FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256, 2) void k_spmm_ilv16(SpmmArgs a) {
    static_assert(!LATE || EPI == EPI_AXPY_NRM_DOT, "the pending half step belongs to the v5 update");
    if (gate_closed(a)) return;
    using R = double;
    constexpr int LN = 16, P = 256, NPL = EpiPlanes<EPI>::N;
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    using T4 = d4;
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    // the index lists through the constant address space: uniform reads become scalar loads whatever the stores around them
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts;
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;   // XCD-aware launch order (tfq_plan.cpp)
    uint32_t const first = a.chunkFirst[chunk], last = a.chunkFirst[chunk + 1], col = a.chunkCol[chunk];
    R sr = 0, si = 0;
    if constexpr (UPD) { sr = epi_scalar<R>(a, col, LN, 0, lc); si = epi_scalar<R>(a, col, LN, 1, lc); }
    double part[NPL > 0 ? NPL : 1] = {};
    __shared__ double s[4][NPL > 0 ? NPL : 1][LN];

    struct Ops { d2v ar[2], ai[2], xr[2], xi[2]; };   // [k pair lr | lr + 4]
    R const* const A0 = (R const*)a.A + (lr * 16 + ilv_rowp(lc)) * 2;
    R const* const X0 = (R const*)a.X + (lr * 16 + lc) * 2;
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        R const* Ab = A0 + size_t(pairs[2 * size_t(q)]) * 2 * P;
        R const* Xb = X0 + size_t(pairs[2 * size_t(q) + 1]) * 2 * P;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if constexpr (ANT) { o.ar[h] = __builtin_nontemporal_load((d2v const*)(Ab + h * 128)); o.ai[h] = __builtin_nontemporal_load((d2v const*)(Ab + P + h * 128)); }
            else { o.ar[h] = *(d2v const*)(Ab + h * 128); o.ai[h] = *(d2v const*)(Ab + P + h * 128); }
            o.xr[h] = *(d2v const*)(Xb + h * 128); o.xi[h] = *(d2v const*)(Xb + P + h * 128);
        }
    };
    for (uint32_t u = wave; u < last - first; u += 4) {
        uint32_t const y = first + u;
        uint64_t const key = HASH ? shadow_key(uint32_t(a.origCol[col]), a.rowI[y]) : 0;
        T4 cre = T4{0, 0, 0, 0}, cim = T4{0, 0, 0, 0};
        auto mma = [&](Ops const& o) __attribute__((always_inline)) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    R const nai = -o.ai[h][e];
                    cre = Acc<R>::mma(o.ar[h][e], o.xr[h][e], cre);
                    cim = Acc<R>::mma(o.ar[h][e], o.xi[h][e], cim);
                    cre = Acc<R>::mma(nai, o.xi[h][e], cre);
                    cim = Acc<R>::mma(o.ai[h][e], o.xr[h][e], cim);
                }
        };
        uint32_t const q0 = starts[y], q1 = starts[y + 1];
        Ops o0, o1;
        // the epilogue operands of EPI_AXPY_NRM_DOT (4 loads) are requested in FRONT of the first two block products' operands, those of
        // EPI_XPAY_DOT (8 loads) behind them: measured both ways, profiles/r02_ab_traversal.txt (vmcnt retires in order)
        constexpr bool EPI_FIRST = (EPI == EPI_AXPY_NRM_DOT);
        if constexpr (!EPI_FIRST) {
            if (q0 < q1) fetch(o0, q0);
            if (q0 + 1 < q1) fetch(o1, q0 + 1);
        }
        // this lane's elements of the Y block: rows (2 lr, 2 lr + 1) and (2 lr + 8, 2 lr + 9) of column lc
        int const eb[2] = { (lr * 16 + lc) * 2, ((lr + 4) * 16 + lc) * 2 };
        size_t const yoff = size_t(y) * 2 * P;
        d2v ur[2], ui[2], vr[2], vi[2]; f2v wr[2], wi[2];
        d2v pr[2], pi[2];                   // LATE: the v9 piece
        uint32_t bu = 0xffffffffu;          // LATE && FIRST: the block of the right-hand side that is the old v5 of this Y block (none: zeros)
        if constexpr (LATE && FIRST) bu = a.bOfX ? a.bOfX[y] : y;
        if constexpr (UPD) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {   // old v4 | v5, v8, v3 [, v9]: touched once, non-temporal
                if constexpr (LATE) { pr[h] = ld_stream<true>((d2v const*)((R const*)a.e2 + yoff + eb[h])); pi[h] = ld_stream<true>((d2v const*)((R const*)a.e2 + yoff + eb[h] + P)); }
                if constexpr (EPI == EPI_XPAY_DOT && FIRST) { ur[h] = d2v{0, 0}; ui[h] = d2v{0, 0}; vr[h] = d2v{0, 0}; vi[h] = d2v{0, 0}; }   // first iteration: old v4 = v8 = 0, not read
                else if constexpr (LATE && FIRST) {   // first iteration: v5 = B scattered onto zeros, not yet in memory
                    ur[h] = d2v{0, 0}; ui[h] = d2v{0, 0};
                    if (bu != 0xffffffffu) {
                        R const* b = (R const*)a.B + size_t(bu) * 2 * P;
                        ur[h] = ld_stream<true>((d2v const*)(b + eb[h])); ui[h] = ld_stream<true>((d2v const*)(b + eb[h] + P));
                    }
                } else {
                ur[h] = ld_stream<true>((d2v const*)((R const*)a.e0 + yoff + eb[h])); ui[h] = ld_stream<true>((d2v const*)((R const*)a.e0 + yoff + eb[h] + P));
                if constexpr (EPI == EPI_XPAY_DOT) { vr[h] = ld_stream<true>((d2v const*)((R const*)a.e1 + yoff + eb[h])); vi[h] = ld_stream<true>((d2v const*)((R const*)a.e1 + yoff + eb[h] + P)); }
                }
                if constexpr (!HASH) { wr[h] = __builtin_nontemporal_load((f2v const*)(a.v3 + yoff + eb[h])); wi[h] = __builtin_nontemporal_load((f2v const*)(a.v3 + yoff + eb[h] + P)); }
            }
        }
        if constexpr (EPI_FIRST) {
            if (q0 < q1) fetch(o0, q0);
            if (q0 + 1 < q1) fetch(o1, q0 + 1);
        }
        // (r03, profiles/r03_ab_exact_waits.txt: the conditional prefetches make the compiler wait with vmcnt(0) in front of every pair of
        //  products; both forms with exact waits -- prefetch index clamped to the last product, or straight-line tails behind a loop that
        //  always prefetches -- measured 4-8 % SLOWER on P2: redundant cache-hot fetches, or 192 VGPRs = two waves per SIMD)
        uint32_t q = q0;
        for (; q + 2 <= q1; q += 2) {
            mma(o0);
            if (q + 2 < q1) fetch(o0, q + 2);
            mma(o1);
            if (q + 3 < q1) fetch(o1, q + 3);
        }
        if (q < q1) mma(o0);

        uint32_t const bq = rhs_block<EPI>(a, y);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // the shadow vector recomputed: one hash for this pair of rows (tfq_device.hpp: shadow_quad).  Drawn here, inside the loop:
            // both hashes in front of it cost spmm_v4_dot 2 % (0.626 against 0.614 ms on P2, profiles/r02_ab_hash.txt)
            uint64_t const hqh = HASH ? shadow_quad(key, uint32_t(lr + 4 * h), uint32_t(lc), LN) : 0;
            d2v yr, yi, nr, ni;
            d2v br = d2v{0, 0}, bi = d2v{0, 0};
            if constexpr (EPI == EPI_RESIDUAL) if (bq != 0xffffffffu) {
                R const* b = (R const*)a.B + size_t(bq) * 2 * P;
                br = *(d2v const*)(b + eb[h]); bi = *(d2v const*)(b + eb[h] + P);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                yr[e] = cre[2 * h + e]; yi[e] = cim[2 * h + e];
                // explicit fused multiply-adds: the HASH and the v3-reading instance of this kernel must round alike
                // (tests/test_gpu_hash_mode.py compares them bit by bit), whatever the compiler would contract on its own
                if constexpr (EPI == EPI_XPAY_DOT) {         // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                    R const tr = __builtin_fma(-si, ui[h][e], __builtin_fma(sr, ur[h][e], vr[h][e]));
                    R const ti = __builtin_fma(sr, ui[h][e], __builtin_fma(si, ur[h][e], vi[h][e]));
                    nr[e] = __builtin_fma(-si, ti, __builtin_fma(sr, tr, yr[e]));
                    ni[e] = __builtin_fma(sr, ti, __builtin_fma(si, tr, yi[e]));
                } else if constexpr (EPI == EPI_AXPY_NRM_DOT) { // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
                    R tr = ur[h][e], ti = ui[h][e];
                    if constexpr (LATE) {                       // v5 := alfa v9 + v5 first, as k_v5_nrm has summed it (tfqmrgpu_core.hxx:205; tfq_vec.hip: axpy)
                        tr = __builtin_fma(-si, pi[h][e], __builtin_fma(sr, pr[h][e], ur[h][e]));
                        ti = __builtin_fma(sr, pi[h][e], __builtin_fma(si, pr[h][e], ui[h][e]));
                    }
                    nr[e] = __builtin_fma(-si, yi[e], __builtin_fma(sr, yr[e], tr));
                    ni[e] = __builtin_fma(sr, yi[e], __builtin_fma(si, yr[e], ti));
                }
                if constexpr (UPD) {
                    double w0, w1;      // the logical elements (rows 2 (lr + 4 h) + e, column lc) are one quad of the shadow vector's hash
                    if constexpr (HASH) { w0 = shadow_pick(hqh, e, 0); w1 = shadow_pick(hqh, e, 1); }
                    else { w0 = wr[h][e]; w1 = wi[h][e]; }
                    epi_dot(part[0], part[1], nr[e], ni[e], w0, w1);
                    if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[2], nr[e], ni[e]);
                } else if constexpr (EPI == EPI_RESIDUAL) {     // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
                    R const rr = yr[e] + R(-1) * br[e], ri = yi[e] + R(-1) * bi[e];
                    double const dr = rr, di = ri;
                    part[0] += dr * dr + di * di;   // (not epi_nrm: this kernel's sum leaves the contraction to the compiler)
                }
            }
            if constexpr (EPI != EPI_RESIDUAL) {
                st_stream<true>((d2v*)((R*)a.Y + yoff + eb[h]), yr); st_stream<true>((d2v*)((R*)a.Y + yoff + eb[h] + P), yi);
            }
            if constexpr (UPD) {
                st_stream<true>((d2v*)((R*)a.e0 + yoff + eb[h]), nr); st_stream<true>((d2v*)((R*)a.e0 + yoff + eb[h] + P), ni);
            }
        }
    }
    if constexpr (NPL > 0) {
        // rows live on lane / 16 (and registers): add the four lane groups, then the four waves in order
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
            double v = part[p];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane < 16) s[wave][p][lane] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < NPL * LN; e += 256) {
            int const p = e / LN, j = e % LN;
            double const sum = ((s[0][p][j] + s[1][p][j]) + s[2][p][j]) + s[3][p][j];
            write_record<EPI>(a, chunk, LN, p, j, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// 16 x 16 complex<float> with groups of FOUR rows interleaved (plane[r/4][s][r%4]): the float counterpart of k_spmm_ilv16.
// A lane of v_mfma_f32_16x16x4_f32 loads the k quad lr = lane / 16 (k = 4 lr .. 4 lr + 3) of its column as ONE 16-byte access --
// MFMA step e contracts k = 4 lr + e -- and its four accumulator registers are the rows 4 lr .. 4 lr + 3 of column lane % 16
// (the C layout of the f32 instruction), i.e. again one 16-byte piece of every epilogue vector: a block product takes 4 wave-wide
// loads of 1 KiB (16 of 256 bytes in k_spmm_mfma<float, 16, 16>), an epilogue 2 accesses per vector.  16 x 16 in float is the
// default shape of the reference's own benchmark (`bench_tfqmrgpu multi`, bench_tfqmrgpu.cu:445-450).

template <int EPI, bool HASH, bool ANT = false, bool FIRST = false>   // FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256, 2) void k_spmm_ilv16f(SpmmArgs a) {
    if (gate_closed(a)) return;
    using R = float;
    constexpr int LN = 16, P = 256, NPL = EpiPlanes<EPI>::N;
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts;
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;
    uint32_t const first = a.chunkFirst[chunk], last = a.chunkFirst[chunk + 1], col = a.chunkCol[chunk];
    R sr = 0, si = 0;
    if constexpr (UPD) { sr = epi_scalar<R>(a, col, LN, 0, lc); si = epi_scalar<R>(a, col, LN, 1, lc); }
    double part[NPL > 0 ? NPL : 1] = {};
    __shared__ double s[4][NPL > 0 ? NPL : 1][LN];

    int const mine = (lr * 16 + lc) * 4;                       // this lane's 16 bytes of a plane: quad lr, column (or A row) lc
    struct Ops { f4v ar, ai, xr, xi; };
    R const* const A0 = (R const*)a.A + mine;
    R const* const X0 = (R const*)a.X + mine;
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        R const* Ab = A0 + size_t(pairs[2 * size_t(q)]) * 2 * P;
        R const* Xb = X0 + size_t(pairs[2 * size_t(q) + 1]) * 2 * P;
        if constexpr (ANT) { o.ar = __builtin_nontemporal_load((f4v const*)Ab); o.ai = __builtin_nontemporal_load((f4v const*)(Ab + P)); }
        else { o.ar = *(f4v const*)Ab; o.ai = *(f4v const*)(Ab + P); }
        o.xr = *(f4v const*)Xb; o.xi = *(f4v const*)(Xb + P);
    };
    for (uint32_t u = wave; u < last - first; u += 4) {
        uint32_t const y = first + u;
        uint64_t const key = HASH ? shadow_key(uint32_t(a.origCol[col]), a.rowI[y]) : 0;
        f4 cre = f4{0, 0, 0, 0}, cim = f4{0, 0, 0, 0};
        auto mma = [&](Ops const& o) __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                R const nai = -o.ai[e];
                cre = Acc<R>::mma(o.ar[e], o.xr[e], cre);
                cim = Acc<R>::mma(o.ar[e], o.xi[e], cim);
                cre = Acc<R>::mma(nai, o.xi[e], cre);
                cim = Acc<R>::mma(o.ai[e], o.xr[e], cim);
            }
        };
        uint32_t const q0 = starts[y], q1 = starts[y + 1];
        Ops o0, o1;
        size_t const yoff = size_t(y) * 2 * P + mine;          // rows 4 lr .. 4 lr + 3 of column lc
        // the epilogue operands are requested in front of the first products' operands: -1 % (profiles/r02_ab_traversal.txt)
        f4v ur, ui, vr, vi, wr, wi;
        if constexpr (UPD) {
            if constexpr (EPI == EPI_XPAY_DOT && FIRST) { ur = f4v{0, 0, 0, 0}; ui = ur; vr = ur; vi = ur; }   // first iteration: old v4 = v8 = 0, not read
            else {
            ur = __builtin_nontemporal_load((f4v const*)((R const*)a.e0 + yoff)); ui = __builtin_nontemporal_load((f4v const*)((R const*)a.e0 + yoff + P));
            if constexpr (EPI == EPI_XPAY_DOT) { vr = __builtin_nontemporal_load((f4v const*)((R const*)a.e1 + yoff)); vi = __builtin_nontemporal_load((f4v const*)((R const*)a.e1 + yoff + P)); }
            }
            if constexpr (!HASH) { wr = __builtin_nontemporal_load((f4v const*)(a.v3 + yoff)); wi = __builtin_nontemporal_load((f4v const*)(a.v3 + yoff + P)); }
        }
        if (q0 < q1) fetch(o0, q0);
        if (q0 + 1 < q1) fetch(o1, q0 + 1);
        uint32_t q = q0;
        for (; q + 2 <= q1; q += 2) {
            mma(o0);
            if (q + 2 < q1) fetch(o0, q + 2);
            mma(o1);
            if (q + 3 < q1) fetch(o1, q + 3);
        }
        if (q < q1) mma(o0);

        uint64_t hq[2] = {0, 0};   // the shadow vector recomputed: one hash per pair of rows (tfq_device.hpp: shadow_quad)
        if constexpr (HASH) { hq[0] = shadow_quad(key, uint32_t(2 * lr), uint32_t(lc), LN); hq[1] = shadow_quad(key, uint32_t(2 * lr + 1), uint32_t(lc), LN); }
        f4v yr, yi, nr, ni;
        f4v br = f4v{0, 0, 0, 0}, bi = f4v{0, 0, 0, 0};
        if constexpr (EPI == EPI_RESIDUAL) {
            uint32_t const bq = rhs_block<EPI>(a, y);
            if (bq != 0xffffffffu) { R const* b = (R const*)a.B + size_t(bq) * 2 * P + mine; br = *(f4v const*)b; bi = *(f4v const*)(b + P); }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            yr[e] = cre[e]; yi[e] = cim[e];
            // explicit fused multiply-adds: the HASH and the v3-reading instance must round alike (tests compare them bit by bit)
            if constexpr (EPI == EPI_XPAY_DOT) {         // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                R const tr = __builtin_fmaf(-si, ui[e], __builtin_fmaf(sr, ur[e], vr[e]));
                R const ti = __builtin_fmaf(sr, ui[e], __builtin_fmaf(si, ur[e], vi[e]));
                nr[e] = __builtin_fmaf(-si, ti, __builtin_fmaf(sr, tr, yr[e]));
                ni[e] = __builtin_fmaf(sr, ti, __builtin_fmaf(si, tr, yi[e]));
            } else if constexpr (EPI == EPI_AXPY_NRM_DOT) { // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
                nr[e] = __builtin_fmaf(-si, yi[e], __builtin_fmaf(sr, yr[e], ur[e]));
                ni[e] = __builtin_fmaf(sr, yi[e], __builtin_fmaf(si, yr[e], ui[e]));
            }
            if constexpr (UPD) {
                double w0, w1;          // rows 4 lr + e of column lc: two quads of the shadow vector's hash
                if constexpr (HASH) { w0 = shadow_pick(hq[e >> 1], e & 1, 0); w1 = shadow_pick(hq[e >> 1], e & 1, 1); }
                else { w0 = wr[e]; w1 = wi[e]; }
                epi_dot(part[0], part[1], nr[e], ni[e], w0, w1);
                if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[2], nr[e], ni[e]);
            } else if constexpr (EPI == EPI_RESIDUAL) {     // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
                R const rr = yr[e] + R(-1) * br[e], ri = yi[e] + R(-1) * bi[e];
                epi_nrm(part[0], rr, ri);
            }
        }
        if constexpr (EPI != EPI_RESIDUAL) { __builtin_nontemporal_store(yr, (f4v*)((R*)a.Y + yoff)); __builtin_nontemporal_store(yi, (f4v*)((R*)a.Y + yoff + P)); }
        if constexpr (UPD) { __builtin_nontemporal_store(nr, (f4v*)((R*)a.e0 + yoff)); __builtin_nontemporal_store(ni, (f4v*)((R*)a.e0 + yoff + P)); }
    }
    if constexpr (NPL > 0) {
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
            double v = part[p];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane < 16) s[wave][p][lane] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < NPL * LN; e += 256) {
            int const p = e / LN, j = e % LN;
            double const sum = ((s[0][p][j] + s[1][p][j]) + s[2][p][j]) + s[3][p][j];
            write_record<EPI>(a, chunk, LN, p, j, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// complex<float> blocks of 16 | 32 rows and 32 columns on the quad-interleaved element order (32 x 32 = BASELINE config 3; written for
// LM, LN multiples of 16; with 64 columns and all four column tiles in one wave it was level with (16 x 64, 32 x 64) or 10 % behind (64 x 64)
// k_spmm_mfma in round 2 -- four tiles of accumulators and operands cost a wave per SIMD; since round 3 a wave takes half of the columns, NH below):
// k_spmm_ilv16f's access pattern with MS x NT MFMA tiles per wave.  A wave owns a strip of MS * 16 rows of a Y block (MS = 2 where the
// block has two row tiles and 32 columns, else 1: the accumulators stay within 32 VGPRs).  A slice is one group of four k quads (quads
// lr + 4 m, 16 k values): MS + NT pairs of wave-wide 1-KiB loads feed 16 MS NT MFMAs (32 x 32: 8 loads for 64 MFMAs, against 16 loads of 512
// bytes in k_spmm_mfma<float, 32, 32>), and every accumulator tile is one 16-byte piece of each epilogue vector (8-byte pieces there).
// The ablations of profiles/r02_ab_config3.txt are why: that kernel gains time with every operand load instruction that is removed.
// No epilogue-operand prefetch (the registers of the tiles: three waves per SIMD matter more), v3 is read.
template <int LM, int LN, int EPI, bool FIRST = false>   // FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256, 3) void k_spmm_ilvf(SpmmArgs a) {   // two column tiles per wave: three waves per SIMD (168 VGPRs at most)
    if (gate_closed(a)) return;
    using R = float;
    constexpr int P = LM * LN, Q = LM * LM, MT = LM / 16, NPL = EpiPlanes<EPI>::N;
    // 64 columns (r03): a wave works on ONE half of the columns (NH = 2 halves of two tiles; the units of a Y block are dealt (strip, half) with the
    // half running fastest, so wave w of a work group keeps half w % 2 and its per-column scalars and sums) -- all four tiles in one wave need the
    // registers of two waves per SIMD, and the epilogue stream then does not overlap with the matrix work (32 x 64: 0.526 ms = multiply 0.354 + stream)
    constexpr int NH = (LN / 16 > 2) ? LN / 32 : 1, NT = LN / 16 / NH;
    constexpr int MS = (MT % 2 == 0 && NT <= 2) ? 2 : 1;          // row tiles per wave
    constexpr int MU = MT / MS;                                   // strips per Y block
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    int const c0 = (NH > 1) ? (wave % NH) * 16 * NT : 0;      // first column of this wave's half
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts;
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;
    uint32_t const first = a.chunkFirst[chunk], last = a.chunkFirst[chunk + 1], col = a.chunkCol[chunk];
    R sr[NT], si[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { sr[nt] = 0; si[nt] = 0; }
    if constexpr (UPD) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            sr[nt] = ((R const*)a.sc)[(size_t(col) * 2 + 0) * LN + c0 + lc + 16 * nt];   // (written out: epi_scalar changes the assembly)
            si[nt] = ((R const*)a.sc)[(size_t(col) * 2 + 1) * LN + c0 + lc + 16 * nt];
        }
    }
    double part[NPL > 0 ? NPL : 1][NT] = {};
    __shared__ double s[4][NPL > 0 ? NPL : 1][LN];

    // 16 bytes of a plane: quad g (rows | k values 4 g .. 4 g + 3) of column c of an X-shaped block, of row c of a (transposed) A block
    auto pieceX = [](int g, int c) { return (g * LN + c) * 4; };
    auto pieceA = [](int g, int c) { return (g * LM + c) * 4; };
    struct Ops { f4v ar[MS], ai[MS], xr[NT], xi[NT]; };
    uint32_t const nUnits = (last - first) * MU * NH;             // unit = strip of MS * 16 rows of one Y block [x half of its columns]
    for (uint32_t u = wave; u < nUnits; u += 4) {                 // (u % NH == wave % NH: 4 is a multiple of NH)
        uint32_t const y = first + (u / NH) / MU;
        int const t0 = int((u / NH) % MU) * MS;                   // first row tile of the strip
        auto fetch = [&](Ops& o, uint32_t q, int m) __attribute__((always_inline)) {
            R const* Ab = (R const*)a.A + size_t(pairs[2 * size_t(q)]) * 2 * Q;
            R const* Xb = (R const*)a.X + size_t(pairs[2 * size_t(q) + 1]) * 2 * P;
            // tile by tile, A and X in turn: vmcnt retires in order and the first MFMAs need the first tiles of both (3 % on 32 x 32)
#pragma unroll
            for (int t = 0; t < (MS > NT ? MS : NT); ++t) {
                if (t < MS) {
                    int const at = pieceA(lr + 4 * m, lc + 16 * (t0 + t));
                    o.ar[t] = *(f4v const*)(Ab + at); o.ai[t] = *(f4v const*)(Ab + Q + at);
                }
                if (t < NT) {
                    int const at = pieceX(lr + 4 * m, c0 + lc + 16 * t);
                    o.xr[t] = *(f4v const*)(Xb + at); o.xi[t] = *(f4v const*)(Xb + P + at);
                }
            }
        };
        f4 cre[MS][NT], cim[MS][NT];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { cre[ms][nt] = f4{0, 0, 0, 0}; cim[ms][nt] = f4{0, 0, 0, 0}; }
        auto mma = [&](Ops const& o) __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 4; ++e)                           // MFMA step e contracts k = 4 (lr + 4 m) + e
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) {
                    R const nai = -o.ai[ms][e];
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        cre[ms][nt] = Acc<R>::mma(o.ar[ms][e], o.xr[nt][e], cre[ms][nt]);
                        cim[ms][nt] = Acc<R>::mma(o.ar[ms][e], o.xi[nt][e], cim[ms][nt]);
                        cre[ms][nt] = Acc<R>::mma(nai, o.xi[nt][e], cre[ms][nt]);
                        cim[ms][nt] = Acc<R>::mma(o.ai[ms][e], o.xr[nt][e], cim[ms][nt]);
                    }
                }
        };
        // the slices of the strip in one sequence: slice t = k group (t % MT) of block product q0 + t / MT; two register sets
        uint32_t const q0 = starts[y], q1 = starts[y + 1];
        Ops o0, o1;
        if constexpr (2 == MT) {          // the two register sets are the two slices of a block product (2-5 % faster than the general form below)
            if (q0 < q1) { fetch(o0, q0, 0); fetch(o1, q0, 1); }
            for (uint32_t q = q0; q < q1; ++q) {
                mma(o0);
                if (q + 1 < q1) fetch(o0, q + 1, 0);
                mma(o1);
                if (q + 1 < q1) fetch(o1, q + 1, 1);
            }
        } else {
            uint32_t const nT = (q1 - q0) * MT;
            if (nT > 0) fetch(o0, q0, 0);
            if (nT > 1) fetch(o1, q0 + 1 / MT, 1 % MT);          // (MT == 1: slice 1 is the next block product)
            for (uint32_t t = 0; t < nT; t += 2) {
                mma(o0);
                if (t + 2 < nT) fetch(o0, q0 + (t + 2) / MT, int((t + 2) % MT));
                if (t + 1 < nT) mma(o1);
                if (t + 3 < nT) fetch(o1, q0 + (t + 3) / MT, int((t + 3) % MT));
            }
        }

        uint32_t bq = 0xffffffffu;   // (written out: rhs_block changes the assembly)
        if constexpr (EPI == EPI_RESIDUAL) bq = a.bOfX ? a.bOfX[y] : y;
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                // accumulator registers 0 .. 3 of tile (ms, nt): rows 16 (t0 + ms) + 4 lr .. + 3 of column 16 nt + lc = one 16-byte piece
                int const at = pieceX(4 * (t0 + ms) + lr, c0 + 16 * nt + lc);
                size_t const yoff = size_t(y) * 2 * P + at;
                f4v ur, ui, vr, vi, wr, wi;
                if constexpr (UPD) {
                    if constexpr (EPI == EPI_XPAY_DOT && FIRST) { ur = f4v{0, 0, 0, 0}; ui = ur; vr = ur; vi = ur; }   // first iteration: old v4 = v8 = 0, not read
                    else {
                    ur = __builtin_nontemporal_load((f4v const*)((R const*)a.e0 + yoff)); ui = __builtin_nontemporal_load((f4v const*)((R const*)a.e0 + yoff + P));
                    if constexpr (EPI == EPI_XPAY_DOT) { vr = __builtin_nontemporal_load((f4v const*)((R const*)a.e1 + yoff)); vi = __builtin_nontemporal_load((f4v const*)((R const*)a.e1 + yoff + P)); }
                    }
                    wr = __builtin_nontemporal_load((f4v const*)(a.v3 + yoff)); wi = __builtin_nontemporal_load((f4v const*)(a.v3 + yoff + P));
                }
                f4v br = f4v{0, 0, 0, 0}, bi = f4v{0, 0, 0, 0};
                if constexpr (EPI == EPI_RESIDUAL) if (bq != 0xffffffffu) {
                    R const* b = (R const*)a.B + size_t(bq) * 2 * P + at;
                    br = *(f4v const*)b; bi = *(f4v const*)(b + P);
                }
                f4v yr, yi, nr, ni;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    yr[e] = cre[ms][nt][e]; yi[e] = cim[ms][nt][e];
                    if constexpr (EPI == EPI_XPAY_DOT) {         // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                        R const tr = __builtin_fmaf(-si[nt], ui[e], __builtin_fmaf(sr[nt], ur[e], vr[e]));
                        R const ti = __builtin_fmaf(sr[nt], ui[e], __builtin_fmaf(si[nt], ur[e], vi[e]));
                        nr[e] = __builtin_fmaf(-si[nt], ti, __builtin_fmaf(sr[nt], tr, yr[e]));
                        ni[e] = __builtin_fmaf(sr[nt], ti, __builtin_fmaf(si[nt], tr, yi[e]));
                    } else if constexpr (EPI == EPI_AXPY_NRM_DOT) { // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
                        nr[e] = __builtin_fmaf(-si[nt], yi[e], __builtin_fmaf(sr[nt], yr[e], ur[e]));
                        ni[e] = __builtin_fmaf(sr[nt], yi[e], __builtin_fmaf(si[nt], yr[e], ui[e]));
                    }
                    if constexpr (UPD) {
                        double const w0 = wr[e], w1 = wi[e], dr = nr[e], di = ni[e];
                        part[0][nt] = __builtin_fma(-di, w1, __builtin_fma(dr, w0, part[0][nt]));
                        part[1][nt] = __builtin_fma(di, w0, __builtin_fma(dr, w1, part[1][nt]));
                        if constexpr (EPI == EPI_AXPY_NRM_DOT) part[2][nt] = __builtin_fma(di, di, __builtin_fma(dr, dr, part[2][nt]));
                    } else if constexpr (EPI == EPI_RESIDUAL) {     // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
                        R const rr = yr[e] + R(-1) * br[e], ri = yi[e] + R(-1) * bi[e];
                        double const dr = rr, di = ri;
                        part[0][nt] = __builtin_fma(di, di, __builtin_fma(dr, dr, part[0][nt]));
                    }
                }
                if constexpr (EPI != EPI_RESIDUAL) { __builtin_nontemporal_store(yr, (f4v*)((R*)a.Y + yoff)); __builtin_nontemporal_store(yi, (f4v*)((R*)a.Y + yoff + P)); }
                if constexpr (UPD) { __builtin_nontemporal_store(nr, (f4v*)((R*)a.e0 + yoff)); __builtin_nontemporal_store(ni, (f4v*)((R*)a.e0 + yoff + P)); }
            }
    }
    if constexpr (NPL > 0) {
        // rows live on lane / 16 (and registers): add the four lane groups, then the four waves in order
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                double v = part[p][nt];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (lane < 16) s[wave][p][c0 + lane + 16 * nt] = v;
            }
        __syncthreads();
        for (int e = threadIdx.x; e < NPL * LN; e += 256) {
            int const p = e / LN, j = e % LN;
            double sum;
            if constexpr (NH > 1) sum = s[(j / (16 * NT)) % NH][p][j] + s[(j / (16 * NT)) % NH + 2][p][j];   // the two waves of this column's half
            else sum = ((s[0][p][j] + s[1][p][j]) + s[2][p][j]) + s[3][p][j];
            write_record<EPI>(a, chunk, LN, p, j, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// (r03: k_spmm_ilvz, the wide complex<double> shapes on the row-pair-interleaved order with one column tile per wave and three waves per SIMD, was
//  4-22 % slower than k_spmm_mfma below -- twice the operand loads per MFMA; two tiles per wave spill at 168 VGPRs -- and is in the git history only:
//  commit 167d902, profiles/r03_ab_ilvz.txt)

template <typename R, int LM, int LN, int EPI> struct Ilv16Family {
    static void go(SpmmKernel k, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
        constexpr bool dbl = sizeof(R) == 8;
        // (the first-iteration launch of EPI_XPAY_DOT is its own instance: a test of the flag per Y block costs the steady launches 0.5 %)
        constexpr bool canFirst = (EPI == EPI_XPAY_DOT);
        constexpr bool canHash = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
        // (late v5: only this kernel has the form, spmm_late_v5 in tfq_spmm.hip grants the flag to no other; its first iteration is an instance too)
        constexpr bool canLate = (EPI == EPI_AXPY_NRM_DOT);
        if constexpr (takes_ilv16(dbl, LM, LN)) if (SpmmKernel::ilv16 == k) {
            variant<canHash>(a.hashV3, [&](auto H) { variant<true>(a.aOnce, [&](auto ANT) { variant<canLate>(a.late, [&](auto L) {
                variant<canFirst || decltype(L)::value>(a.first, [&](auto F) {
                    k_spmm_ilv16<EPI, decltype(H)::value, decltype(ANT)::value, decltype(F)::value, decltype(L)::value><<<dim3(nWG), dim3(256), 0, s>>>(a); }); }); }); });
            return;
        }
        if constexpr (takes_ilv16f(dbl, LM, LN)) if (SpmmKernel::ilv16f == k) {
            variant<canHash>(a.hashV3, [&](auto H) { variant<true>(a.aOnce, [&](auto ANT) { variant<canFirst>(a.first, [&](auto F) {
                k_spmm_ilv16f<EPI, H, ANT, F><<<dim3(nWG), dim3(256), 0, s>>>(a); }); }); });
            return;
        }
        if constexpr (takes_ilvf(dbl, LM, LN)) if (SpmmKernel::ilvf == k) {
            variant<canFirst>(a.first, [&](auto F) { k_spmm_ilvf<LM, LN, EPI, F><<<dim3(nWG), dim3(256), 0, s>>>(a); });
        }
    }
};

bool spmm_ilv16(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    return spmm_switch<Ilv16Family>(k, dbl, lm, ln, epi, a, nWG, s);
}

} // namespace tfq
