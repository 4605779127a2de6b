// k_spmm_mfma: LM and LN multiples of 16, on the reference's native element order (tfq_spmm.hpp).  One wavefront owns a 16 x LN strip of one
// Y block and keeps it in MFMA accumulators (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32).  The native layouts ARE the MFMA operand
// layouts: lane l feeds A[k0 + l/16][i0 + l%16] and X[k0 + l/16][columns of lane l%16], i.e. four consecutive rows per load instruction,
// so operands go global -> VGPR fully coalesced with no LDS transpose.  With several 16-column tiles per strip a lane owns NEIGHBOURING
// columns (ColMap) and moves them as one 16-byte access.  4 real MFMA chains per complex product (-Im(A) is formed once per operand), 3 in
// double above 16 x 16 (Slice::mma3); the 16 x 16 instances recompute the shadow vector from its hash instead of reading it (HASH).
#include "tfq_spmm.hpp"

namespace tfq {

// Column map of the MFMA kernel: a lane touches NT block columns (one per accumulator tile).  They are chosen as
// NT/VW groups of VW NEIGHBOURS, VW * sizeof(R) = 16 bytes where NT allows: tile nt of lane column lc holds block
// column (nt/VW) * 16 VW + lc * VW + nt % VW (not nt * 16 + lc).  X operands and every epilogue vector then move
// as 16-byte accesses, 256 contiguous bytes per row and lane group (the memory pipe retires one wave-wide access
// per 16 clocks whatever its width, scripts/ta_rate.hip).  Which 16 columns share a tile is free.
// VW: the largest power of two with VW * sizeof(R) <= 16 that divides NT (3 | 6 tiles: one | two columns per access).
constexpr int col_vw(int nt, int rb) { int v = 16 / rb; while (nt % v) v /= 2; return v; }
template <typename R, int NT> struct ColMap {
    static constexpr int VW = col_vw(NT, int(sizeof(R)));                            // columns per access
    static constexpr int NG = NT / VW;                                             // accesses per row
    __device__ static inline int col(int lc, int nt) { return (nt / VW) * 16 * VW + lc * VW + nt % VW; }
};

// row tiles per wave (tfq_plan.hpp: the rule by which the plan cuts its chunks as well)
template <typename R, int MT, int NT> struct RowTiles { static constexpr int MS = mfma_row_tiles(MT, NT, int(sizeof(R))); };

// operands of one "slice" = KSL consecutive MFMA k-steps (4 k each) of one block product, for a strip of
// MS * 16 block rows: the wave owns MS row tiles, tile ms of lane column lc holds block row i0 + lc * MS + ms, so
// that the A operand too moves as one MS-wide access and every X operand feeds MS tiles
template <typename R, int MS, int NT, int KSL>
struct Slice {
    R ar[KSL][MS], ai[KSL][MS], xr[KSL][NT], xi[KSL][NT];
    // Ab: A block + first row of this lane (i0 + lc * MS), Xb: X block + first column of this lane (lc * VW)
    template <int LM, int LN>
    __device__ inline void load(R const* __restrict__ Ab, R const* __restrict__ Xb, int k0, int lr) {
        constexpr int P = LM * LN, VW = ColMap<R, NT>::VW, NG = ColMap<R, NT>::NG;
#pragma unroll
        for (int s = 0; s < KSL; ++s) {
            int const k = k0 + 4 * s + lr;
            vload<R, MS>(ar[s], Ab + k * LM); vload<R, MS>(ai[s], Ab + LM * LM + k * LM);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                R vr[VW], vi[VW];
                vload<R, VW>(vr, Xb + k * LN + g * 16 * VW);
                vload<R, VW>(vi, Xb + P + k * LN + g * 16 * VW);
#pragma unroll
                for (int n = 0; n < VW; ++n) { xr[s][g * VW + n] = vr[n]; xi[s][g * VW + n] = vi[n]; }
            }
        }
    }
    // complex product from THREE real products (Gauss): P1 = Re A Re X, P2 = Im A Im X, P3 = (Re A + Im A)(Re X + Im X);
    // Re = P1 - P2, Im = P3 - P1 - P2.  A quarter fewer MFMAs (the f64 matrix pipe of this part sustains ~49 TFLOP/s,
    // scripts/clock_in_kernel.hip, and bounds the multiply) for two extra additions per operand element.
    template <typename T4>
    __device__ inline void mma3(T4 (&p1)[MS][NT], T4 (&p2)[MS][NT], T4 (&p3)[MS][NT]) const {
#pragma unroll
        for (int s = 0; s < KSL; ++s) {
            R sx[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) sx[nt] = xr[s][nt] + xi[s][nt];
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) {
                R const sa = ar[s][ms] + ai[s][ms];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    p1[ms][nt] = Acc<R>::mma(ar[s][ms], xr[s][nt], p1[ms][nt]);
                    p2[ms][nt] = Acc<R>::mma(ai[s][ms], xi[s][nt], p2[ms][nt]);
                    p3[ms][nt] = Acc<R>::mma(sa, sx[nt], p3[ms][nt]);
                }
            }
        }
    }
    // the precision `m`: float operands widened to double in registers (v_cvt_f64_f32; the product of two floats is exact in double),
    // double accumulators, the four real products in the order of mma below
    __device__ inline void mma_f64(d4 (&cre)[MS][NT], d4 (&cim)[MS][NT]) const {
        static_assert(std::is_same<R, float>::value, "float operands");
#pragma unroll
        for (int s = 0; s < KSL; ++s)
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) {
                double const a_r = ar[s][ms], a_i = ai[s][ms], na_i = -a_i;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    double const x_r = xr[s][nt], x_i = xi[s][nt];
                    cre[ms][nt] = Acc<double>::mma(a_r, x_r, cre[ms][nt]);
                    cim[ms][nt] = Acc<double>::mma(a_r, x_i, cim[ms][nt]);
                    cre[ms][nt] = Acc<double>::mma(na_i, x_i, cre[ms][nt]);
                    cim[ms][nt] = Acc<double>::mma(a_i, x_r, cim[ms][nt]);
                }
            }
    }
    template <typename T4>
    __device__ inline void mma(T4 (&cre)[MS][NT], T4 (&cim)[MS][NT]) const {
#pragma unroll
        for (int s = 0; s < KSL; ++s)
#pragma unroll
            for (int ms = 0; ms < MS; ++ms) {
                R const nai = -ai[s][ms];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    cre[ms][nt] = Acc<R>::mma(ar[s][ms], xr[s][nt], cre[ms][nt]);
                    cim[ms][nt] = Acc<R>::mma(ar[s][ms], xi[s][nt], cim[ms][nt]);
                    cre[ms][nt] = Acc<R>::mma(nai, xi[s][nt], cre[ms][nt]);
                    cim[ms][nt] = Acc<R>::mma(ai[s][ms], xr[s][nt], cim[ms][nt]);
                }
            }
    }
};

// CLAMP: the operand prefetch inside a strip carries no condition (the slice index is clamped to the last slice instead: two
// redundant, cache-resident slice loads per strip), so that the compiler can count the loads in flight and waits for exactly the
// slice it is about to multiply -- with the conditional form it drains the whole queue (s_waitcnt vmcnt(0)) in front of every
// slice.  Used where a strip has many slices (blocks of 32 rows and more: the matrix-pipe-bound shapes).
template <typename R, int LM, int LN, int EPI, bool PRE, bool M3, bool HASH, bool CLAMP = false>
__global__ __launch_bounds__(256, 2) void k_spmm_mfma(SpmmArgs a) {   // at least 2 waves per SIMD: 256 VGPRs at most
    if (gate_closed(a)) return;
    static_assert(LM % 16 == 0 && LN % 16 == 0, "MFMA tiles are 16 x 16");
    constexpr int CS = mfma_col_split(sizeof(R), LN);   // waves per strip, LN / CS columns each
    static_assert(CS == 1 || EPI == EPI_NONE, "the epilogues take whole rows");
    constexpr int P = LM * LN, MT = LM / 16, NT = LN / (16 * CS);
    constexpr int MS = RowTiles<R, MT, NT>::MS;      // row tiles per wave
    constexpr int MU = MT / MS;                      // strips per Y block
    constexpr int KSL = (MS * NT >= 4) ? 2 : 4;      // k-steps per slice: bounds the registers of the prefetch
    constexpr int SPP = LM / (4 * KSL);              // slices per block product
    constexpr int NPL = EpiPlanes<EPI>::N;
    constexpr int VW = ColMap<R, NT>::VW, NG = ColMap<R, NT>::NG;
    using T4 = typename Acc<R>::T;
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    int const c0 = lc * VW;                          // first block column of this lane, further groups 16 VW apart
    // work groups that are dispatched to the same XCD (blockIdx % 8, observed round-robin) get neighbouring
    // chunks (a.order, tfq_plan.cpp), so that the A blocks shared by neighbouring block columns are served
    // by that XCD's L2
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : a.plainPer ? (blockIdx.x & 7u) * a.plainPer + (blockIdx.x >> 3) : blockIdx.x;
    uint32_t first, last, col = 0;
    if (a.chunkFirst) { first = a.chunkFirst[chunk]; last = a.chunkFirst[chunk + 1]; col = a.chunkCol[chunk]; }
    else { first = min(chunk * a.CH, a.nY); last = min(first + a.CH, a.nY); }

    R sr[NT], si[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { sr[nt] = 0; si[nt] = 0; }
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            sr[nt] = epi_scalar<R>(a, col, LN, 0, ColMap<R, NT>::col(lc, nt));
            si[nt] = epi_scalar<R>(a, col, LN, 1, ColMap<R, NT>::col(lc, nt));
        }
    }
    double part[NPL > 0 ? NPL : 1][NT] = {};

    uint32_t const nUnits = (last - first) * MU * CS;   // unit = strip of MS * 16 rows (and LN / CS columns) of one Y block
    using CU32o = __attribute__((address_space(4))) uint32_t const*;
    CU32o const yOrder = (CU32o)(uintptr_t)a.yOrder;
    for (uint32_t u = wave; u < nUnits; u += 4) {
        uint32_t const y = a.yOrder ? yOrder[first + u / (MU * CS)] : first + u / (MU * CS);   // (plain mode with a prepared order: which Y block this position computes)
        int const i0 = int((u / CS) % MU) * 16 * MS;
        int const cb = int(u % CS) * (LN / CS);      // first block column of this unit
        uint64_t const key = HASH ? shadow_key(uint32_t(a.origCol[col]), a.rowI[y]) : 0;
        T4 cre[MS][NT], cim[MS][NT], cp3[M3 ? MS : 1][M3 ? NT : 1];   // M3: P1, P2, P3
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                cre[ms][nt] = T4{0, 0, 0, 0}; cim[ms][nt] = T4{0, 0, 0, 0};
                if constexpr (M3) cp3[ms][nt] = T4{0, 0, 0, 0};
            }
        auto mma = [&](Slice<R, MS, NT, KSL> const& o) __attribute__((always_inline)) {
            if constexpr (M3) o.mma3(cre, cim, cp3); else o.mma(cre, cim);
        };
        // index lists through the constant address space: uniform reads stay scalar loads whatever the stores around them
        using CU32 = __attribute__((address_space(4))) uint32_t const*;
        CU32 const cstarts = (CU32)(uintptr_t)a.starts; CU32 const cpairs = (CU32)(uintptr_t)a.pairs;
        uint32_t const q0 = cstarts[y];
        uint32_t const nT = (cstarts[y + 1] - q0) * SPP;   // slices of this strip
        R const* const A0 = (R const*)a.A + i0 + lc * MS;
        R const* const X0 = (R const*)a.X + cb + c0;
        auto fetch = [&](Slice<R, MS, NT, KSL>& o, uint32_t t) {
            uint32_t const q = q0 + t / SPP;
            int const k0 = int(t % SPP) * (4 * KSL);
            o.template load<LM, LN>(A0 + size_t(cpairs[2 * size_t(q)]) * 2 * LM * LM,
                                    X0 + size_t(cpairs[2 * size_t(q) + 1]) * 2 * P, k0, lr);
        };
        // block row of accumulator register r of row tile ms
        auto row_of = [&](int ms, int r) { return i0 + Acc<R>::row(lane, r) * MS + ms; };
        // software pipeline, two register sets: the loads of slices t+1, t+2 are in flight while the MFMAs
        // of slice t issue.  With PRE the operands of the epilogue (old v4|v5, v8, v3) are requested right
        // behind the first two slices: vmcnt retires in order, so they must be younger than the slices
        // whose MFMAs should start first and they have two slices of matrix work to arrive.
        constexpr int NSET = 2;
        Slice<R, MS, NT, KSL> o[NSET];
        if constexpr (CLAMP) {
            if (nT > 0) {
#pragma unroll
                for (int i = 0; i < NSET; ++i) fetch(o[i], (uint32_t(i) < nT) ? uint32_t(i) : nT - 1);
            }
        } else {
            if (nT > 0) fetch(o[0], 0);
            if (nT > 1) fetch(o[1], 1);
        }
        EpiOps<R, EPI, VW, HASH> ops[PRE ? MS * 4 * NG : 1];
        if constexpr (PRE) {
#pragma unroll
            for (int ms = 0; ms < MS; ++ms)
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int g = 0; g < NG; ++g)
                        ops[(ms * 4 + r) * NG + g].load(a, size_t(y) * 2 * P + row_of(ms, r) * LN + c0 + g * 16 * VW, P);
        }
        uint32_t t = 0;
        for (; t + NSET <= nT; t += NSET) {
#pragma unroll
            for (int i = 0; i < NSET; ++i) {
                mma(o[i]);
                uint32_t const tn = t + NSET + i;
                if constexpr (CLAMP) {
                    // (pinning the loads right behind the MFMAs of their set with sched_barrier was measured and is slower:
                    //  32 x 32 c with cache-hot operands 102.6 -> 95.0 TFLOP/s; hipcc's own interleaving is kept)
                    fetch(o[i], (tn < nT) ? tn : nT - 1);
                } else if (tn < nT) fetch(o[i], tn);
            }
        }
#pragma unroll
        for (int i = 0; i < NSET - 1; ++i) if (t + i < nT) mma(o[i]);

        uint32_t bq = 0xffffffffu;   // (written out: rhs_block changes the assembly)
        if constexpr (EPI == EPI_RESIDUAL) bq = a.bOfX ? a.bOfX[y] : y;
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < NG; ++g) {       // accesses of at most 16 bytes per lane
                    int const e = row_of(ms, r) * LN + cb + c0 + g * 16 * VW;
                    size_t const off = size_t(y) * 2 * P + e;
                    R yr[VW], yi[VW];
#pragma unroll
                    for (int n = 0; n < VW; ++n) {
                        if constexpr (M3) {
                            R const p1 = cre[ms][g * VW + n][r], p2 = cim[ms][g * VW + n][r];
                            yr[n] = p1 - p2; yi[n] = (cp3[ms][g * VW + n][r] - p1) - p2;
                        } else { yr[n] = cre[ms][g * VW + n][r]; yi[n] = cim[ms][g * VW + n][r]; }
                    }
                    if constexpr (!PRE) ops[0].load(a, off, P);
                    epilogue_row<R, EPI, VW, NPL, NT, HASH, LN>(a, off, P, yr, yi, sr, si, g * VW, ops[PRE ? (ms * 4 + r) * NG + g : 0], bq, e, part, key);
                }
    }

    if constexpr (NPL > 0) {
        // rows live on lane/16 (and registers): add the four lane groups, then the four waves in order
        __shared__ double s[4][NPL][LN];
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                double v = part[p][nt];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (lane < 16) s[wave][p][ColMap<R, NT>::col(lane, nt)] = v;
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

template <typename R, int LM, int LN, int EPI> struct MfmaFamily {
    static void go(SpmmKernel, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
        if constexpr (takes_mfma(sizeof(R) == 8, LM, LN)) {
            // epilogue operands prefetched under the MFMAs where the registers allow it (one 16-column tile in double, two in float)
            // (not for 32 x 32 float: the prefetched operands take the fused kernels from 168 / 132 to 224 / 198 VGPRs = two waves per SIMD
            //  instead of three; measured on config 3: 0.2998 / 0.2930 ms with, 0.2947 / 0.2887 ms without)
            constexpr bool pre = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) && ((LN / 16) * sizeof(R) <= 8) && !(sizeof(R) == 4 && LM == 32 && LN == 32);
            static int const use_pre = lab_switch("TFQMRGPU_EPI_PREFETCH", 1);
            // Three real products per complex one (Gauss) where the matrix pipe bounds the kernel: double, every shape but 16 x 16
            // (whose multiply is bound by the operand stream: 0.486 ms on P2 with either form).  Im = P3 - P1 - P2 carries the rounding
            // of the real parts: an imaginary part 10^-k times smaller than the real part loses k digits against the four-product form.
            // A drop-in caller did not ask for that, so it is OPT-IN per plan (tfqmrgpuExt_setThreeProductMultiply; until r02 it was the
            // default); never in float (the float floor of the FD fixture, 4.6e-5, moves above its threshold of 1e-4).
            // Lab builds: TFQMRGPU_3M=1 everywhere above 16 x 16, 2: 16 x 16 too.
            static int const use_m3 = lab_switch("TFQMRGPU_3M", 0);
            // the shadow vector recomputed in registers where it is the library's hash and a lane owns one column (16 x 16): the
            // fused kernels then read S/2 (`z`) or S (`c`) less (P2: 0.743 / 0.684 -> 0.719 / 0.673 ms); wider shapes and the
            // tile kernels lose and keep reading it (measured with the hash everywhere: 8 x 8 z +4 %, 32 x 32 c fused +19 %, 16 x 64 c
            // iteration +18 %, 32 x 64 c +41 %: more registers, and the hash competes with the epilogue for the vector ALU;
            // 16 x 32 z and 64 x 64 z would gain 1 %)
            constexpr bool canHash = (LN == 16) && (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
            bool const m3 = sizeof(R) == 8 && (((use_m3 || a.m3) && (LM / 16) * (LN / 16) >= 2) || use_m3 >= 2);
            // unconditional (clamped) operand prefetch where a strip has at least 8 slices per block product (LM >= 32)
            constexpr bool canClamp = (LM >= 32);
            static int const use_clamp = lab_switch("TFQMRGPU_CLAMP", 1);
            // (the shapes of the stand-alone multiply alone, TFQ_MULTIPLY_SIZES, have the four-product form only)
            constexpr bool canM3 = solver_shape(LM, LN);
            variant<canM3>(m3, [&](auto M3) { variant<canHash>(a.hashV3, [&](auto H) { variant<pre>(use_pre, [&](auto PRE) { variant<canClamp>(use_clamp, [&](auto CLAMP) {
                k_spmm_mfma<R, LM, LN, EPI, PRE, M3, H, CLAMP><<<dim3(nWG), dim3(256), 0, s>>>(a); }); }); }); });
        }
    }
};

bool spmm_mfma(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    return spmm_switch<MfmaFamily>(k, dbl, lm, ln, epi, a, nWG, s);
}

bool spmm_mfma_wide(bool dbl, int lm, int ln, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
#define TFQ_CASE(R, LM, LN) case LM * 1000 + LN: if (nWG) MfmaFamily<R, LM, LN, EPI_NONE>::go(SpmmKernel::mfma, a, nWG, s); return true;
    if (dbl) { switch (lm * 1000 + ln) { TFQ_MULTIPLY_SIZES(TFQ_CASE, double) default: return false; } }
    else     { switch (lm * 1000 + ln) { TFQ_MULTIPLY_SIZES(TFQ_CASE, float)  default: return false; } }
#undef TFQ_CASE
}

// ---------------------------------------------------------------------------------------------------
// k_spmm_mfma_m: the precision `m` of the stand-alone multiply, the reference's gemmNxNf<float, LM, LN, NA, double> (float data, sums in
// double, tfqmrgpu_blockmult.hxx:28,62-77,88).  k_spmm_mfma's plain mode with float operands and double accumulators: the operands move
// as in the `c` instance (ColMap<float>: 16-byte column accesses), are widened in registers (Slice::mma_f64) and summed by
// v_mfma_f64_16x16x4_f64 in the order of the `z` instance; each Y element is rounded to float once, when it is stored.  Row tiles per wave
// and column split as `z` (the accumulators are double), so that a prepared order (tfqmrgpuExt_multiplyPrepare) counts the same units.
template <int LM, int LN, bool CLAMP>
__global__ __launch_bounds__(256, 2) void k_spmm_mfma_m(SpmmArgs a) {   // at least 2 waves per SIMD: 256 VGPRs at most
    static_assert(LM % 16 == 0 && LN % 16 == 0, "MFMA tiles are 16 x 16");
    using R = float;
    constexpr int CS = mfma_col_split(8, LN);
    constexpr int P = LM * LN, MT = LM / 16, NT = LN / (16 * CS);
    constexpr int MS = RowTiles<double, MT, NT>::MS;
    constexpr int MU = MT / MS;
    constexpr int KSL = (MS * NT >= 4) ? 2 : 4;
    constexpr int SPP = LM / (4 * KSL);
    constexpr int VW = ColMap<R, NT>::VW, NG = ColMap<R, NT>::NG;
    constexpr bool STREAM = EpiOps<R, EPI_NONE, VW>::STREAM;
    using T4 = Acc<double>::T;
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    int const c0 = lc * VW;
    uint32_t const chunk = a.plainPer ? (blockIdx.x & 7u) * a.plainPer + (blockIdx.x >> 3) : blockIdx.x;
    uint32_t const first = min(chunk * a.CH, a.nY), last = min(first + a.CH, a.nY);
    uint32_t const nUnits = (last - first) * MU * CS;
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const yOrder = (CU32)(uintptr_t)a.yOrder;
    CU32 const cstarts = (CU32)(uintptr_t)a.starts; CU32 const cpairs = (CU32)(uintptr_t)a.pairs;
    for (uint32_t u = wave; u < nUnits; u += 4) {
        uint32_t const y = a.yOrder ? yOrder[first + u / (MU * CS)] : first + u / (MU * CS);
        int const i0 = int((u / CS) % MU) * 16 * MS;
        int const cb = int(u % CS) * (LN / CS);
        T4 cre[MS][NT], cim[MS][NT];
#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { cre[ms][nt] = T4{0, 0, 0, 0}; cim[ms][nt] = T4{0, 0, 0, 0}; }
        uint32_t const q0 = cstarts[y];
        uint32_t const nT = (cstarts[y + 1] - q0) * SPP;
        R const* const A0 = (R const*)a.A + i0 + lc * MS;
        R const* const X0 = (R const*)a.X + cb + c0;
        auto fetch = [&](Slice<R, MS, NT, KSL>& o, uint32_t t) {
            uint32_t const q = q0 + t / SPP;
            int const k0 = int(t % SPP) * (4 * KSL);
            o.template load<LM, LN>(A0 + size_t(cpairs[2 * size_t(q)]) * 2 * LM * LM,
                                    X0 + size_t(cpairs[2 * size_t(q) + 1]) * 2 * P, k0, lr);
        };
        constexpr int NSET = 2;                      // the software pipeline of k_spmm_mfma
        Slice<R, MS, NT, KSL> o[NSET];
        if constexpr (CLAMP) {
            if (nT > 0) {
#pragma unroll
                for (int i = 0; i < NSET; ++i) fetch(o[i], (uint32_t(i) < nT) ? uint32_t(i) : nT - 1);
            }
        } else {
            if (nT > 0) fetch(o[0], 0);
            if (nT > 1) fetch(o[1], 1);
        }
        uint32_t t = 0;
        for (; t + NSET <= nT; t += NSET) {
#pragma unroll
            for (int i = 0; i < NSET; ++i) {
                o[i].mma_f64(cre, cim);
                uint32_t const tn = t + NSET + i;
                if constexpr (CLAMP) fetch(o[i], (tn < nT) ? tn : nT - 1);
                else if (tn < nT) fetch(o[i], tn);
            }
        }
#pragma unroll
        for (int i = 0; i < NSET - 1; ++i) if (t + i < nT) o[i].mma_f64(cre, cim);

#pragma unroll
        for (int ms = 0; ms < MS; ++ms)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    size_t const off = size_t(y) * 2 * P + (i0 + Acc<double>::row(lane, r) * MS + ms) * LN + cb + c0 + g * 16 * VW;
                    R yr[VW], yi[VW];
#pragma unroll
                    for (int n = 0; n < VW; ++n) { yr[n] = R(cre[ms][g * VW + n][r]); yi[n] = R(cim[ms][g * VW + n][r]); }   // the one rounding
                    vstore_stream<STREAM, R, VW>((R*)a.Y + off, yr); vstore_stream<STREAM, R, VW>((R*)a.Y + off + P, yi);
                }
    }
}

template <int LM, int LN> bool mfma_m_go(SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    if constexpr (takes_mfma(true, LM, LN)) {
        // the clamped prefetch of k_spmm_mfma where a strip has many slices, except 96 x 96: six column tiles of double accumulators and the
        // widened operands of two slices need 256 VGPRs and 44 bytes of scratch there (218 VGPRs without the clamp)
        constexpr bool canClamp = (LM >= 32 && LN != 96);
        static int const use_clamp = lab_switch("TFQMRGPU_CLAMP", 1);
        if (nWG) variant<canClamp>(use_clamp, [&](auto CLAMP) { k_spmm_mfma_m<LM, LN, CLAMP><<<dim3(nWG), dim3(256), 0, s>>>(a); });
        return true;
    } else return false;
}

bool spmm_mfma_m(int lm, int ln, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
#define TFQ_CASE(R, LM, LN) case LM * 1000 + LN: return mfma_m_go<LM, LN>(a, nWG, s);
    switch (lm * 1000 + ln) { TFQ_SIZES(TFQ_CASE, float) TFQ_MULTIPLY_SIZES(TFQ_CASE, float) default: return false; }
#undef TFQ_CASE
}

} // namespace tfq
