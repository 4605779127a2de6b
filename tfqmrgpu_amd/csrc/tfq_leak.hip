// Truncation leak: the part of A X that falls on block rows OUTSIDE a block column's pattern, |.|^2 per (block column, right-hand side),
// summed in double whatever the plan's precision (tfqmrgpu_ext.h section 11).  Not part of a solve: it reads A and X where the plan keeps
// them and writes only into memory that the library owns.  What is this kernel's own: it walks the leak listing (tfq_leak_host.cpp) by
// work units, adds the products of a position before it squares them, subtracts nothing, and ends in the per-unit tail with one record
// plane.  The products and that tail are tfq_grade.hpp's.
//   k_leak<RA, LM, LN>   one work group per work unit (a run of leak positions of ONE block column): the product sum of every position,
//                        squared and summed per column of the block; one [LN] record per unit
//   k_leak_col<LN>       one work group per block column: the records of its units added in unit order; a column without units gets 0
// No atomics, and every sum has one fixed order: two calls on the same data give the same bits.
#include "tfq_grade.hpp"

namespace tfq {

struct LeakArgs {
    void const *A, *X;                      // storage type RA; A blocks transposed ([k][i]) in the caller's block order, X in the internal order
    uint32_t const *posStart, *pairs;       // products per leak position; (A block, X block) per product
    uint32_t const *unitFirst, *colUnitPtr;
    int ilv;                                // element order of both operands (tfq_device.hpp: plane_offset)
    double* rec;                            // [nUnits][LN]
    double* col;                            // [nCols][LN]
};

template <typename RA, int LM, int LN>
__global__ __launch_bounds__(256) void k_leak(LeakArgs a) {
    constexpr int P = LM * LN;                            // elements per plane
    constexpr bool MFMA = (LM % 16 == 0 && LN % 16 == 0);
    int const t = threadIdx.x;
    uint32_t const unit = blockIdx.x;
    uint32_t const first = a.unitFirst[unit], last = a.unitFirst[unit + 1];
    RA const* const A = (RA const*)a.A; RA const* const X = (RA const*)a.X;
    int const ilv = a.ilv;

    if constexpr (MFMA) {
        // v_mfma_f64_16x16x4_f64 on operands converted to double in registers: a wave keeps a strip of 16 rows of a position, all its columns
        constexpr int MT = LM / 16, NT = LN / 16;
        int const lane = t & 63, wave = t >> 6, lr = lane >> 4, lc = lane & 15;
        double l2[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) l2[n] = 0;
        uint32_t const strips = (last - first) * MT;
        for (uint32_t u = uint32_t(wave); u < strips; u += 4) {
            uint32_t const y = first + u / MT;
            int const i0 = int(u % MT) * 16;
            GradeAcc cre[NT], cim[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) { cre[n] = GradeAcc{0, 0, 0, 0}; cim[n] = GradeAcc{0, 0, 0, 0}; }
            for (uint32_t q = a.posStart[y]; q < a.posStart[y + 1]; ++q) {
                RA const* Ab = A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
                RA const* Xb = X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
TFQ_GRADE_STRIP_PAIR      // lane (lr, lc) feeds A[k][i0 + lc] and X[k][16 n + lc], k = k0 + lr
            }
            TFQ_GRADE_STRIP_SQUARE(l2)        // register r of the lane: row lr + 4 r of the strip, column 16 n + lc
        }
        // lanes that share a column: rank = (wave, lr); summed in rank order
        __shared__ double s[LN * 16];
        int const rank = wave * 4 + lr;
#pragma unroll
        for (int n = 0; n < NT; ++n) s[(16 * n + lc) * 16 + rank] = l2[n];
        TFQ_GRADE_UNIT_TAIL(LN, 16, a.rec[size_t(unit) * LN + e])
    } else {
        // one lane per element of a position's block, the 4- and 8-row shapes
        constexpr int NACC = (P >= 256) ? P / 256 : 1;   // elements per lane
        constexpr int GRP = (P >= 256) ? 1 : 256 / P;    // positions in flight per work group
        static_assert(P < 256 || (P % 256 == 0 && 256 % LN == 0), "block does not tile the work group");
        int const g = (P >= 256) ? 0 : t / P;
        int const e0 = (P >= 256) ? t : t % P;
        bool const active = (g < GRP);
        int const j = e0 % LN;                           // the same for all NACC elements of a lane (256 % LN == 0)
        double l2 = 0;
        if (active) for (uint32_t y = first + uint32_t(g); y < last; y += GRP) {
            double yr[NACC], yi[NACC];
#pragma unroll
            for (int n = 0; n < NACC; ++n) { yr[n] = 0; yi[n] = 0; }
            for (uint32_t q = a.posStart[y]; q < a.posStart[y + 1]; ++q) {
                RA const* Ab = A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
                RA const* Xb = X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
                TFQ_GRADE_LANE_PAIR
            }
#pragma unroll
            for (int n = 0; n < NACC; ++n) epi_nrm(l2, yr[n], yi[n]);
        }
        // lanes that share a column: rank = position among them; summed in rank order
        constexpr int RANKS = (P >= 256) ? 256 / LN : GRP * LM;
        __shared__ double s[LN * RANKS];
        int const rank = (P >= 256) ? t / LN : g * LM + e0 / LN;
        if (active) s[j * RANKS + rank] = l2;
        TFQ_GRADE_UNIT_TAIL(LN, RANKS, a.rec[size_t(unit) * LN + e])
    }
}

template <int LN>
__global__ __launch_bounds__(64) void k_leak_col(LeakArgs a) {
    uint32_t const col = blockIdx.x;
    int const e = threadIdx.x;                            // right-hand side
    if (e >= LN) return;
    double sum = 0;                                       // a column without units: exactly 0
    for (uint32_t u = a.colUnitPtr[col]; u < a.colUnitPtr[col + 1]; ++u) sum += a.rec[size_t(u) * LN + e];
    a.col[size_t(col) * LN + e] = sum;
}

template <typename RA, int LM, int LN>
static void leak_run(uint32_t nUnits, uint32_t nCols, LeakArgs const& a, hipStream_t s) {
    static_assert(LN <= 64, "k_leak_col: one lane per right-hand side");
    if (0 == nCols) return;
    if (nUnits) k_leak<RA, LM, LN><<<dim3(nUnits), dim3(256), 0, s>>>(a);
    k_leak_col<LN><<<dim3(nCols), dim3(64), 0, s>>>(a);
}

void leak_launch(DevPlan const& d, void const* A, uint32_t nUnits, uint32_t const* pairs, uint32_t const* posStart,
    uint32_t const* unitFirst, uint32_t const* colUnitPtr, double* rec, double* col, hipStream_t s)
{
    LeakArgs a{};
    a.A = A; a.X = d.x;
    a.posStart = posStart; a.pairs = pairs; a.unitFirst = unitFirst; a.colUnitPtr = colUnitPtr;
    a.ilv = d.ilv; a.rec = rec; a.col = col;
    for_shape(d.dbl, d.LM, d.LN, [&](auto sh) { using S = decltype(sh); leak_run<typename S::real, S::LM, S::LN>(nUnits, d.nCols, a, s); });
}

} // namespace tfq
