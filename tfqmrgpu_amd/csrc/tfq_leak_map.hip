// Leak map: the truncation leak of tfq_leak.hip per leak POSITION -- |(A X)(i, c)(:, j)|^2 for every block row i outside the pattern of
// block column c that receives a product, per right-hand side j, in double whatever the plan's precision (tfqmrgpu_ext.h section 12).
// Not part of a solve: it reads A and X where the plan keeps them and writes only into memory that the library owns.  What is
// this kernel's own: it walks the positions of the leak listing one by one, adds the products of a position before it squares them and
// keeps one record per position (the products and the lane geometry are tfq_grade.hpp's):
//   k_leak_map<RA, LM, LN>   one work group per run of kLeakMapRun consecutive positions of the listing (its work units are not used:
//                            a record belongs to ONE position, so there is nothing to add across positions and no second kernel)
//     LM, LN multiples of 16: a whole position per wave, wave w of the group takes the positions w, w + 4, ... of the run.  It walks the
//                            LM / 16 strips of the position on v_mfma_f64_16x16x4_f64, keeps l2[NT] across them, adds the four row groups
//                            of a column in ascending lr by shuffles and writes the [LN] record.  No LDS, no barrier, no cross-wave sum
//     the 4- and 8-row shapes: one lane per element (P / 256 elements per lane where the block has more than 256), 256 / P positions in
//                            flight per round; the lanes that share a column of a position are added through LDS in rank order.  The
//                            round count is a constant, so that every wave reaches every barrier; the work is predicated
// No atomics, and every sum has one fixed order: two calls on the same data give the same bits.
#include "tfq_grade.hpp"

namespace tfq {

constexpr uint32_t kLeakMapRun = 32;        // positions per work group

struct LeakMapArgs {
    void const *A, *X;                      // storage type RA; A blocks transposed ([k][i]) in the caller's block order, X in the internal order
    uint32_t const *posStart, *pairs;       // the listing's: products per leak position; (A block, X block) per product
    uint32_t nPos;
    int ilv;
    double* rec;                            // [nPos][LN]
};

template <typename RA, int LM, int LN>
__global__ __launch_bounds__(256) void k_leak_map(LeakMapArgs a) {
    constexpr int P = LM * LN;                            // elements per plane
    constexpr bool MFMA = (LM % 16 == 0 && LN % 16 == 0);
    int const t = threadIdx.x;
    uint32_t const first = blockIdx.x * kLeakMapRun;
    uint32_t const last = (a.nPos - first < kLeakMapRun) ? a.nPos : first + kLeakMapRun;   // (the grid: first < nPos)
    RA const* const A = (RA const*)a.A; RA const* const X = (RA const*)a.X;
    int const ilv = a.ilv;

    if constexpr (MFMA) {
        constexpr int NT = LN / 16;
        int const lane = t & 63, wave = t >> 6, lr = lane >> 4, lc = lane & 15;
        for (uint32_t y = first + uint32_t(wave); y < last; y += 4) {      // y is the same for the whole wave: the shuffles below see all 64 lanes
            uint32_t const q0 = a.posStart[y], q1 = a.posStart[y + 1];
            double l2[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) l2[n] = 0;
#pragma unroll 1
            for (int i0 = 0; i0 < LM; i0 += 16) {
                GradeAcc cre[NT], cim[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) { cre[n] = GradeAcc{0, 0, 0, 0}; cim[n] = GradeAcc{0, 0, 0, 0}; }
                for (uint32_t q = q0; q < q1; ++q) {
                    RA const* Ab = A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
                    RA const* Xb = X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
TFQ_GRADE_STRIP_PAIR      // lane (lr, lc) feeds A[k][i0 + lc] and X[k][16 n + lc], k = k0 + lr
                }
                TFQ_GRADE_STRIP_SQUARE(l2)        // register r of the lane: row lr + 4 r of the strip, column 16 n + lc
            }
            // the four lanes (lr, lc) of a column, added in ascending lr; every lane computes the sum, the lanes lr == 0 store it
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                double sum = __shfl(l2[n], lc, 64);
#pragma unroll
                for (int r = 1; r < 4; ++r) sum += __shfl(l2[n], 16 * r + lc, 64);
                if (0 == lr) a.rec[size_t(y) * LN + 16 * n + lc] = sum;
            }
        }
    } else {
        using L = GradeLanes<LM, LN>;
        constexpr int NACC = L::NACC, GRP = L::GRP;
        constexpr int ROUNDS = (int(kLeakMapRun) + GRP - 1) / GRP;
        constexpr int RANKS = L::RANKS_ITEM;     // lanes that share a column of a position
        static_assert(GRP * LN <= 256, "one lane per entry of the records of a round");
        __shared__ double s[GRP * LN * RANKS];
        L const l = TFQ_GRADE_LANES(t);
        int const g = l.g, e0 = l.e0, j = l.j;
        int const rank = (P >= 256) ? t / LN : e0 / LN;  // P < 256: the row of the element
#pragma unroll 1
        for (int round = 0; round < ROUNDS; ++round) {
            uint32_t const y0 = first + uint32_t(round * GRP);
            uint32_t const y = y0 + uint32_t(g);
            if (g < GRP && y < last) {
                double yr[NACC], yi[NACC];
#pragma unroll
                for (int n = 0; n < NACC; ++n) { yr[n] = 0; yi[n] = 0; }
                for (uint32_t q = a.posStart[y]; q < a.posStart[y + 1]; ++q) {
                    RA const* Ab = A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
                    RA const* Xb = X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
                    TFQ_GRADE_LANE_PAIR
                }
                double l2 = 0;
#pragma unroll
                for (int n = 0; n < NACC; ++n) epi_nrm(l2, yr[n], yi[n]);
                s[(g * LN + j) * RANKS + rank] = l2;
            }
            __syncthreads();
            if (t < GRP * LN && y0 + uint32_t(t / LN) < last) {      // lane t: position y0 + t / LN of the round, right-hand side t % LN
                double sum = 0;
#pragma unroll 1
                for (int r = 0; r < RANKS; ++r) sum += s[t * RANKS + r];
                a.rec[size_t(y0 + uint32_t(t / LN)) * LN + t % LN] = sum;
            }
            __syncthreads();                                         // the patch is written again in the next round
        }
    }
}

template <typename RA, int LM, int LN>
static void leak_map_run(LeakMapArgs const& a, hipStream_t s) {
    if (0 == a.nPos) return;
    k_leak_map<RA, LM, LN><<<dim3((a.nPos + kLeakMapRun - 1) / kLeakMapRun), dim3(256), 0, s>>>(a);
}

void leak_map_launch(DevPlan const& d, void const* A, uint32_t nPos, uint32_t const* pairs, uint32_t const* posStart, double* rec, hipStream_t s) {
    LeakMapArgs a{};
    a.A = A; a.X = d.x;
    a.posStart = posStart; a.pairs = pairs; a.nPos = nPos;
    a.ilv = d.ilv; a.rec = rec;
    for_shape(d.dbl, d.LM, d.LN, [&](auto sh) { using S = decltype(sh); leak_map_run<typename S::real, S::LM, S::LN>(a, s); });
}

} // namespace tfq
