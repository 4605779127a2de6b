// k_spmm_pad: the stand-alone multiply (tfqmrgpuExt_multiply, plain mode) on block shapes that do not fill 16 x 16 MFMA tiles: 6 x 6,
// 12 x 12 and 24 x 24 in `c`, `z` and `m`, and `m` (float data, double sums) on the 4- and 8-row shapes of the solver.
// Every Re and Im plane of these shapes is a whole number of 16-byte pieces, in float and in double, so every plane starts 16-byte
// aligned.  One wave computes one Y block: it fetches the four operand planes of a block product with 16-byte global loads into VGPRs
// (the next product's loads are in flight under the MFMAs of the current one) and writes them element by element (ds_write) into a
// ZERO-PADDED image in its own LDS patch: rows and columns padded to multiples of 16, k to a multiple of 4.  (Not global_load_lds: its
// destination is wave-uniform base + lane x size, a padded image is not.)  The pad is cleared once per wave; the products overwrite only
// their valid elements.  The MFMA operands come from the image as in k_spmm_n16 (tfq_spmm.hip): v_mfma_f64_16x16x4_f64 for `z` and `m`
// (float elements widened in registers), v_mfma_f32_16x16x4_f32 for `c`, four real products per complex one in the order of k_spmm_mfma;
// only the LM x LN valid elements of the Y block are stored, each rounded to the storage type once.
// Staging: whole tiles, no k-slices.  The largest image, 24 x 24 `z` padded to 32 x 32 with k = 24, is 24 KiB per wave; such shapes
// run two waves per work group (48 KiB), every other shape four (at most 48 KiB: 24 x 24 `c` | `m`).
#include "tfq_spmm.hpp"

namespace tfq {

constexpr int up_to(int v, int m) { return (v + m - 1) / m * m; }

template <typename S, int LM, int LN> struct PadShape {
    static constexpr int MP = up_to(LM, 16), NP = up_to(LN, 16), KP = up_to(LM, 4);   // padded rows, columns, k
    static constexpr int IA = KP * MP, IX = KP * NP;             // elements of the image of one A | X plane
    static constexpr int IMG = 2 * IA + 2 * IX;                   // A re | A im | X re | X im
    static constexpr int W = (4 * IMG * int(sizeof(S)) <= 64 * 1024) ? 4 : 2;   // waves (Y blocks) per work group
};

// S: storage type of A, X and Y; RA: accumulator type (double for `z` and `m`)
template <typename S, typename RA, int LM, int LN>
__global__ __launch_bounds__(256) void k_spmm_pad(SpmmArgs a) {
    using Sh = PadShape<S, LM, LN>;
    constexpr int MP = Sh::MP, NP = Sh::NP, KP = Sh::KP, IA = Sh::IA, IX = Sh::IX, W = Sh::W;
    constexpr int MT = MP / 16, NT = NP / 16, KS = KP / 4;
    constexpr int PA = LM * LM, PX = LM * LN;                     // elements per plane
    constexpr int VE = 16 / sizeof(S);                            // elements of a 16-byte piece
    static_assert(PA % VE == 0 && PX % VE == 0, "planes of whole 16-byte pieces");
    constexpr int NA = PA / VE, NX = PX / VE;                     // pieces per plane
    constexpr int CA = (NA + 63) / 64, CX = (NX + 63) / 64;       // pieces per lane and plane
    using V = S __attribute__((ext_vector_type(VE)));
    using T4 = typename Acc<RA>::T;
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts;
    __shared__ __attribute__((aligned(16))) S img[W][Sh::IMG];
    S* const my = img[wave];
    uint32_t const y = blockIdx.x * W + uint32_t(wave);           // (no barrier below: a wave without a Y block just leaves)
    if (y >= a.nY) return;
    for (int e = lane; e < Sh::IMG; e += 64) my[e] = S(0);         // the pad, once

    struct Ops { V a[2][CA], x[2][CX]; };
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        S const* Ab = (S const*)a.A + size_t(pairs[2 * size_t(q)]) * 2 * PA;
        S const* Xb = (S const*)a.X + size_t(pairs[2 * size_t(q) + 1]) * 2 * PX;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int t = 0; t < CA; ++t) { int const c = lane + 64 * t; if (NA % 64 == 0 || c < NA) o.a[p][t] = *(V const*)(Ab + p * PA + c * VE); }
#pragma unroll
            for (int t = 0; t < CX; ++t) { int const c = lane + 64 * t; if (NX % 64 == 0 || c < NX) o.x[p][t] = *(V const*)(Xb + p * PX + c * VE); }
        }
    };
    // piece c of a plane holds elements c VE ... of [k][i] (A, LM x LM) | [k][j] (X, LM x LN): into the padded image
    auto stage = [&](Ops const& o) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int t = 0; t < CA; ++t) {
                int const c = lane + 64 * t;
                if (NA % 64 == 0 || c < NA)
#pragma unroll
                    for (int n = 0; n < VE; ++n) { int const e = c * VE + n; my[p * IA + (e / LM) * MP + e % LM] = o.a[p][t][n]; }
            }
#pragma unroll
            for (int t = 0; t < CX; ++t) {
                int const c = lane + 64 * t;
                if (NX % 64 == 0 || c < NX)
#pragma unroll
                    for (int n = 0; n < VE; ++n) { int const e = c * VE + n; my[2 * IA + p * IX + (e / LN) * NP + e % LN] = o.x[p][t][n]; }
            }
        }
    };
    T4 cre[MT][NT], cim[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { cre[mt][nt] = T4{0, 0, 0, 0}; cim[mt][nt] = T4{0, 0, 0, 0}; }
    auto mma = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {                            // k = 4 s + lr: lane (lr, lc) feeds A[k][i = 16 mt + lc] and X[k][j = 16 nt + lc]
            int const k = 4 * s + lr;
            RA xr[NT], xi[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { xr[nt] = RA(my[2 * IA + k * NP + 16 * nt + lc]); xi[nt] = RA(my[2 * IA + IX + k * NP + 16 * nt + lc]); }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                RA const ar = RA(my[k * MP + 16 * mt + lc]), ai = RA(my[IA + k * MP + 16 * mt + lc]), nai = -ai;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    cre[mt][nt] = Acc<RA>::mma(ar, xr[nt], cre[mt][nt]);
                    cim[mt][nt] = Acc<RA>::mma(ar, xi[nt], cim[mt][nt]);
                    cre[mt][nt] = Acc<RA>::mma(nai, xi[nt], cre[mt][nt]);
                    cim[mt][nt] = Acc<RA>::mma(ai, xr[nt], cim[mt][nt]);
                }
            }
        }
    };
    uint32_t const q0 = starts[y], q1 = starts[y + 1];
    Ops o;
    if (q0 < q1) fetch(o, q0);
    for (uint32_t q = q0; q < q1; ++q) {
        __builtin_amdgcn_wave_barrier();          // LDS operations of one wave complete in order: the image is free when these writes execute
        stage(o);
        __builtin_amdgcn_wave_barrier();
        if (q + 1 < q1) fetch(o, q + 1);          // in flight under the MFMAs of this product
        mma();
    }
    S* const Yb = (S*)a.Y + size_t(y) * 2 * PX;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int const i = 16 * mt + Acc<RA>::row(lane, r), j = 16 * nt + lc;
                if ((MP == LM || i < LM) && (NP == LN || j < LN)) {
                    Yb[i * LN + j] = S(cre[mt][nt][r]); Yb[PX + i * LN + j] = S(cim[mt][nt][r]);   // the one rounding (`m`)
                }
            }
}

template <typename S, typename RA, int LM, int LN> void pad_go(SpmmArgs const& a, hipStream_t s) {
    constexpr int W = PadShape<S, LM, LN>::W;
    uint32_t const nWG = (a.nY + W - 1) / W;
    if (nWG) k_spmm_pad<S, RA, LM, LN><<<dim3(nWG), dim3(64 * W), 0, s>>>(a);
}

bool spmm_pad(MulPrec p, int lm, int ln, SpmmArgs const& a, hipStream_t s) {
    int const key = lm * 1000 + ln;
#define TFQ_CASE(R, LM, LN) case LM * 1000 + LN: pad_go<R, R, LM, LN>(a, s); return true;
#define TFQ_CASE_M(R, LM, LN) case LM * 1000 + LN: pad_go<float, double, LM, LN>(a, s); return true;
    switch (p) {
    case MulPrec::c: switch (key) { TFQ_PAD_SIZES(TFQ_CASE, float) default: return false; }
    case MulPrec::z: switch (key) { TFQ_PAD_SIZES(TFQ_CASE, double) default: return false; }
    case MulPrec::m: switch (key) { TFQ_PAD_SIZES(TFQ_CASE_M, 0) TFQ_PAD_M_SIZES(TFQ_CASE_M, 0) default: return false; }
    }
#undef TFQ_CASE
#undef TFQ_CASE_M
    return false;
}

} // namespace tfq
