// Per-right-hand-side residual of the caller's system, |B - A X|^2 and |B|^2 per (block column, right-hand side), summed in double whatever
// the plan's precision (tfqmrgpu_ext.h section 10).  Not part of a solve: it reads A, X and B where the plan keeps them and writes only
// into scratch that the library owns.
//   k_residual<RA, LM, LN>   one work group per chunk (a run of blocks of ONE block column, tfq_plan.cpp: cutChunks -- the unit of work of
//                            the fused multiplies): the truncated product A X of every block of the chunk, minus its B block, squared and
//                            summed per column of the block; two [LN] records per chunk
//   k_residual_col<LN>       one work group per block column: the records of its chunks added in chunk order
// What is this kernel's own: it walks the plan's pair list by chunks, adds the products of a Y block before it squares them, subtracts B,
// and ends in the per-unit tail with two record planes.  The products and that tail are tfq_grade.hpp's.
// No atomics, and every sum has one fixed order: two calls on the same data give the same bits.
#include "tfq_grade.hpp"

namespace tfq {

struct ResidualArgs {
    void const *A, *X, *B;                  // storage type RA; A blocks transposed ([k][i]) in the caller's block order, X in the internal order
    uint32_t const *starts, *pairs, *bOfX;  // products per internal X block; (A block, X block) per product; B block on an X block, or ~0
    uint32_t const *chunkFirst, *colChunkPtr;
    int ilv;                                // element order of all three operands (tfq_device.hpp: plane_offset)
    double* rec;                            // [nChunks][2][LN]: |A x - b|^2, |b|^2
    double* col;                            // [nCols][2][LN]
};

// r = y - b, sums of squares (res_offset, res_cmac: tfq_grade.hpp)
__device__ __forceinline__ void res_square(double& r2, double& b2, double yr, double yi, double br, double bi) {
    double const rr = fma_(-1., br, yr), ri = fma_(-1., bi, yi);
    epi_nrm(r2, rr, ri); epi_nrm(b2, br, bi);
}

template <typename RA, int LM, int LN>
__global__ __launch_bounds__(256) void k_residual(ResidualArgs a) {
    constexpr int P = LM * LN;                            // elements per plane
    constexpr bool MFMA = (LM % 16 == 0 && LN % 16 == 0);
    int const t = threadIdx.x;
    uint32_t const chunk = blockIdx.x;
    uint32_t const first = a.chunkFirst[chunk], last = a.chunkFirst[chunk + 1];
    RA const* const A = (RA const*)a.A; RA const* const X = (RA const*)a.X; RA const* const B = (RA const*)a.B;
    int const ilv = a.ilv;

    if constexpr (MFMA) {
        // v_mfma_f64_16x16x4_f64 on operands converted to double in registers: a wave keeps a strip of 16 rows of a Y block, all its columns
        constexpr int MT = LM / 16, NT = LN / 16;
        int const lane = t & 63, wave = t >> 6, lr = lane >> 4, lc = lane & 15;
        double r2[NT], b2[NT];
#pragma unroll
        for (int n = 0; n < NT; ++n) { r2[n] = 0; b2[n] = 0; }
        uint32_t const units = (last - first) * MT;
        for (uint32_t u = uint32_t(wave); u < units; u += 4) {
            uint32_t const y = first + u / MT;
            int const i0 = int(u % MT) * 16;
            GradeAcc cre[NT], cim[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) { cre[n] = GradeAcc{0, 0, 0, 0}; cim[n] = GradeAcc{0, 0, 0, 0}; }
            for (uint32_t q = a.starts[y]; q < a.starts[y + 1]; ++q) {
                RA const* Ab = A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
                RA const* Xb = X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
TFQ_GRADE_STRIP_PAIR      // lane (lr, lc) feeds A[k][i0 + lc] and X[k][16 n + lc], k = k0 + lr
            }
            uint32_t const bq = a.bOfX[y];
            RA const* Bb = B + size_t(bq != 0xffffffffu ? bq : 0) * 2 * P;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {             // register r of the lane: row Acc::row(lane, r) of the strip, column 16 n + lc
                    double br = 0, bi = 0;
                    if (bq != 0xffffffffu) {
                        int const ob = res_offset(ilv, i0 + Acc<double>::row(lane, r), 16 * n + lc, LN);
                        br = double(Bb[ob]); bi = double(Bb[P + ob]);
                    }
                    res_square(r2[n], b2[n], cre[n][r], cim[n][r], br, bi);
                }
        }
        // lanes that share a column: rank = (wave, lr); summed in rank order
        __shared__ double s[2 * LN * 16];
        int const rank = wave * 4 + lr;
#pragma unroll
        for (int n = 0; n < NT; ++n) { s[(16 * n + lc) * 16 + rank] = r2[n]; s[(LN + 16 * n + lc) * 16 + rank] = b2[n]; }
        TFQ_GRADE_UNIT_TAIL(2 * LN, 16, a.rec[size_t(chunk) * 2 * LN + e])
    } else {
        // one lane per element of a Y block, the 4- and 8-row shapes
        constexpr int NACC = (P >= 256) ? P / 256 : 1;   // elements per lane
        constexpr int GRP = (P >= 256) ? 1 : 256 / P;    // Y blocks in flight per work group
        static_assert(P < 256 || (P % 256 == 0 && 256 % LN == 0), "block does not tile the work group");
        int const g = (P >= 256) ? 0 : t / P;
        int const e0 = (P >= 256) ? t : t % P;
        bool const active = (g < GRP);
        int const j = e0 % LN;                           // the same for all NACC elements of a lane (256 % LN == 0)
        double r2 = 0, b2 = 0;
        if (active) for (uint32_t y = first + uint32_t(g); y < last; y += GRP) {
            double yr[NACC], yi[NACC];
#pragma unroll
            for (int n = 0; n < NACC; ++n) { yr[n] = 0; yi[n] = 0; }
            for (uint32_t q = a.starts[y]; q < a.starts[y + 1]; ++q) {
                RA const* Ab = A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
                RA const* Xb = X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
                TFQ_GRADE_LANE_PAIR
            }
            uint32_t const bq = a.bOfX[y];
            RA const* Bb = B + size_t(bq != 0xffffffffu ? bq : 0) * 2 * P;
#pragma unroll
            for (int n = 0; n < NACC; ++n) {
                double br = 0, bi = 0;
                if (bq != 0xffffffffu) {
                    int const ob = res_offset(ilv, (e0 + n * 256) / LN, j, LN);
                    br = double(Bb[ob]); bi = double(Bb[P + ob]);
                }
                res_square(r2, b2, yr[n], yi[n], br, bi);
            }
        }
        // lanes that share a column: rank = position among them; summed in rank order
        constexpr int RANKS = (P >= 256) ? 256 / LN : GRP * LM;
        __shared__ double s[2 * LN * RANKS];
        int const rank = (P >= 256) ? t / LN : g * LM + e0 / LN;
        if (active) { s[j * RANKS + rank] = r2; s[(LN + j) * RANKS + rank] = b2; }
        TFQ_GRADE_UNIT_TAIL(2 * LN, RANKS, a.rec[size_t(chunk) * 2 * LN + e])
    }
}

template <int LN>
__global__ __launch_bounds__(128) void k_residual_col(ResidualArgs a) {
    uint32_t const col = blockIdx.x;
    int const e = threadIdx.x;                            // (plane, right-hand side)
    if (e >= 2 * LN) return;
    double sum = 0;
    for (uint32_t ch = a.colChunkPtr[col]; ch < a.colChunkPtr[col + 1]; ++ch) sum += a.rec[size_t(ch) * 2 * LN + e];
    a.col[size_t(col) * 2 * LN + e] = sum;
}

template <typename RA, int LM, int LN>
static void residual_run(DevPlan const& d, ResidualArgs const& a, hipStream_t s) {
    static_assert(2 * LN <= 128, "k_residual_col: one lane per (plane, right-hand side)");
    if (0 == d.nChunks || 0 == d.nCols) return;
    k_residual<RA, LM, LN><<<dim3(d.nChunks), dim3(256), 0, s>>>(a);
    k_residual_col<LN><<<dim3(d.nCols), dim3(128), 0, s>>>(a);
}

void residual_launch(DevPlan const& d, void const* A, double* rec, double* col, hipStream_t s) {
    ResidualArgs a{};
    a.A = A; a.X = d.x; a.B = d.B;
    a.starts = d.starts; a.pairs = d.pairs; a.bOfX = d.bOfX; a.chunkFirst = d.chunkFirst; a.colChunkPtr = d.colChunkPtr;
    a.ilv = d.ilv; a.rec = rec; a.col = col;
    for_shape(d.dbl, d.LM, d.LN, [&](auto sh) { using S = decltype(sh); residual_run<typename S::real, S::LM, S::LN>(d, a, s); });
}

} // namespace tfq
