// The one copy of every device piece of the four calls that grade the caller's system in double whatever the plan's precision:
// tfq_residual.hip, tfq_leak.hip, tfq_leak_map.hip and tfq_drop_cost.hip (tfqmrgpu_ext.h sections 10 to 13).  All of them add block
// products A_b X_b, square what they get and sum the squares per column of the block; a kernel says which list it walks, whether the
// products of a work item are added before they are squared, whether B is subtracted, and which tail it ends in.  Everything else is here,
// written once: the same statements in the same order in every kernel, which is what their bit-for-bit promises rest on.
//   multiples of 16 rows and columns: a wave keeps a 16-row strip of a product block, all its columns, on v_mfma_f64_16x16x4_f64
//                                     (TFQ_GRADE_STRIP_STEP, TFQ_GRADE_STRIP_PAIR); lane (lr, lc) = (lane / 16, lane % 16)
//   the 4- and 8-row shapes:          one lane per element of a product block (GradeLanes, TFQ_GRADE_LANE_PAIR)
//   the per-unit tail:                TFQ_GRADE_UNIT_TAIL (the lanes of a work group that share a column, through LDS in rank order)
// Still written in place: the shuffle tail and the per-round LDS tail of k_leak_map and k_drop_cost (one and two record planes, whose
// statements interleave differently), and the lane geometry of k_residual and k_leak, where GradeLanes changes the compiled code
#pragma once
#include "tfq_spmm.hpp"

namespace tfq {

// plane_offset with the group size as a constant in each branch (the order is uniform over the launch: a scalar branch, no division)
__device__ __forceinline__ int res_offset(int ilv, int r, int s, int nC) {
    switch (ilv) {
        case 2:  return plane_offset(2, r, s, nC);
        case 4:  return plane_offset(4, r, s, nC);
        default: return plane_offset(0, r, s, nC);
    }
}

// One fixed pattern of fused multiply-adds (the rule of tfq_device.hpp: fma_): y += a x (complex)
__device__ __forceinline__ void res_cmac(double& yr, double& yi, double ar, double ai, double xr, double xi) {
    yr = fma_(-ai, xi, fma_(ar, xr, yr)); yi = fma_(ai, xr, fma_(ar, xi, yi));
}

using GradeAcc = typename Acc<double>::T;   // the accumulators of one 16 x 16 tile: register r of the lane is row Acc<double>::row(lane, r), column lc

// The products are statement macros, not functions: a function, however forcibly inlined, reaches the kernel behind the compiler's early
// passes and leaves other code than the same statements written in place (LABBOOK.md, "Grading kernels").  They use the kernel's names:
// LM, LN, P = LM * LN, NT = LN / 16, NACC; ilv; Ab, Xb (RA const*, the blocks of the pair)

// ---- multiples of 16: the strip product of one (A block, X block) pair ------------------------------------------------------------
// one k-step of the rows i0 ... i0 + 15: lane (lr, lc) feeds A[k][i0 + lc] and X[k][16 n + lc]; the statements behind K declare xr, xi for column tile n
#define TFQ_GRADE_STRIP_STEP(K, ...) \
    int const k = (K), oa = res_offset(ilv, k, i0 + lc, LM); \
    double const ar = double(Ab[oa]), ai = double(Ab[LM * LM + oa]); \
    _Pragma("unroll") \
    for (int n = 0; n < NT; ++n) { \
        __VA_ARGS__ \
        cre[n] = Acc<double>::mma(ar, xr, cre[n]); \
        cim[n] = Acc<double>::mma(ar, xi, cim[n]); \
        cre[n] = Acc<double>::mma(-ai, xi, cre[n]); \
        cim[n] = Acc<double>::mma(ai, xr, cim[n]); \
    }
// the X operand read from the block where it is needed
#define TFQ_GRADE_X_FROM_BLOCK \
    int const ox = res_offset(ilv, k, 16 * n + lc, LN); \
    double const xr = double(Xb[ox]), xi = double(Xb[P + ox]);
// cre, cim [NT] += A_b X_b on that strip
#define TFQ_GRADE_STRIP_PAIR \
    _Pragma("unroll 4") \
    for (int k0 = 0; k0 < LM; k0 += 4) { TFQ_GRADE_STRIP_STEP(k0 + lr, TFQ_GRADE_X_FROM_BLOCK) }
// sq [NT] += |.|^2 of the lane's four rows of every column tile
#define TFQ_GRADE_STRIP_SQUARE(sq) \
    _Pragma("unroll") \
    for (int n = 0; n < NT; ++n) \
        _Pragma("unroll") \
        for (int r = 0; r < 4; ++r) epi_nrm(sq[n], cre[n][r], cim[n][r]);

// ---- the 4- and 8-row shapes: one lane per element of a product block ----------------------------------------------------------------
// Lane t of the 256 has the elements e0 + 256 n, n < NACC, of block g of the GRP blocks in flight (a lane with g >= GRP
// has none): rows (e0 + 256 n) / LN, all in column j (256 % LN == 0)
template <int LM, int LN>
struct GradeLanes {
    static constexpr int P = LM * LN;                           // elements per plane
    static constexpr int NACC = (P >= 256) ? P / 256 : 1;       // elements per lane
    static constexpr int GRP = (P >= 256) ? 1 : 256 / P;        // blocks in flight per work group
    static_assert(P < 256 || (P % 256 == 0 && 256 % LN == 0), "block does not tile the work group");
    // Lanes that share a column.  The per-item kernels (k_leak_map, k_drop_cost) keep the blocks in flight apart: the lanes of ONE block.
    // The per-unit kernels (k_residual, k_leak) add them up as well: the lanes of all GRP blocks
    static constexpr int RANKS_ITEM = (P >= 256) ? 256 / LN : LM;
    static constexpr int RANKS_UNIT = (P >= 256) ? 256 / LN : GRP * LM;
    int g, e0, j;
};

// the geometry of lane t, `GradeLanes<LM, LN> const l = TFQ_GRADE_LANES(t);` (an aggregate filled in place, not a constructor: see the products)
#define TFQ_GRADE_LANES(t) { (P >= 256) ? 0 : (t) / P, (P >= 256) ? (t) : (t) % P, ((P >= 256) ? (t) : (t) % P) % LN }

// yr, yi [NACC] += A_b X_b for the elements of lane (e0, j)
#define TFQ_GRADE_LANE_PAIR \
    _Pragma("unroll") \
    for (int k = 0; k < LM; ++k) { \
        int const ox = res_offset(ilv, k, j, LN); \
        double const xr = double(Xb[ox]), xi = double(Xb[P + ox]); \
        _Pragma("unroll") \
        for (int n = 0; n < NACC; ++n) { \
            int const oa = res_offset(ilv, k, (e0 + n * 256) / LN, LM); \
            res_cmac(yr[n], yi[n], double(Ab[oa]), double(Ab[LM * LM + oa]), xr, xi); \
        } \
    }

// ---- the tails: NP planes of records, [LN] doubles per plane -----------------------------------------------------------------------------
// Per work unit, the lanes of the work group that share a column added through LDS in rank order (a statement macro, as the products).
// Every lane has written its sum for plane p and column c as number `rank` of the RANKS lanes of that column to s[(p * LN + c) * RANKS + rank];
// REC: the entry e < N = NP * LN of the unit's record
#define TFQ_GRADE_UNIT_TAIL(N, RANKS, REC) \
    __syncthreads(); \
    for (int e = t; e < (N); e += 256) { \
        double sum = 0; \
        _Pragma("unroll 1") \
        for (int r = 0; r < (RANKS); ++r) sum += s[e * (RANKS) + r]; \
        REC = sum; \
    }

} // namespace tfq
