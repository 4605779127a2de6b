// Drop cost: per block n of X and right-hand side j, cost2 = the sum over the plan's own block products A_ik X_kc whose X operand is block n
// of |A_ik X_kc (:, j)|^2 -- every product squared ON ITS OWN -- and weight2 = |X_kc (:, j)|^2, in double whatever the plan's precision
// (tfqmrgpu_ext.h section 13).  Not part of a solve: it reads A and X where the plan keeps them and writes only into memory that the
// library owns.  What is this kernel's own: the X block of a work item is fixed and each of its products is squared on its own; two record
// planes (cost, weight).  The products and the lane geometry are tfq_grade.hpp's.
//   k_drop_cost<RA, LM, LN>   one work group per run of kDropRun consecutive X blocks of the caller's order (DropListing, tfq_plan.hpp)
//     LM, LN multiples of 16: one X block per wave, the four waves of the group take four consecutive blocks at a time (wave w: the
//                            blocks w, w + 4, ... of the run).  The wave converts its X operands to double ONCE and keeps them in
//                            registers across all products of the block (64 x 64: they would take all 256 VGPRs, X is loaded again in
//                            every strip there); per product and 16-row strip it zeroes the v_mfma_f64_16x16x4_f64 accumulators, runs
//                            the LM / 4 k-steps and folds |re|^2 + |im|^2 into l2[NT].  weight2 comes from the same registers.  The four
//                            row groups of a column are added in ascending lr by shuffles.  No LDS, no barrier
//     the 4- and 8-row shapes: one lane per element of the product block (P / 256 elements per lane where the block has more than 256),
//                            256 / P blocks in flight per round; the lanes that share a column of a block are added through LDS in rank
//                            order.  The round count is a constant, so that every wave reaches every barrier; the work is predicated
// A work item reads start[n], start[n + 1] and xOf[n] and writes the records of block n, for n < nX only.
// No atomics, and every sum has one fixed order: two calls on the same data give the same bits.
#include "tfq_grade.hpp"

namespace tfq {

constexpr uint32_t kDropRun = 32;           // X blocks per work group

struct DropArgs {
    void const *A, *X;                      // storage type RA; A blocks transposed ([k][i]) in the caller's block order, X in the internal order; A is not read where cost == nullptr
    uint32_t const *start, *aOf, *xOf;      // the listing's: products per X block; the A block of every product; where the X block lies
    uint32_t nX;
    int ilv;
    double *cost, *weight;                  // [nX][LN] each, either may be nullptr
};

template <typename RA, int LM, int LN>
__global__ __launch_bounds__(256) void k_drop_cost(DropArgs a) {
    constexpr int P = LM * LN;                            // elements per plane
    constexpr bool MFMA = (LM % 16 == 0 && LN % 16 == 0);
    int const t = threadIdx.x;
    uint32_t const first = blockIdx.x * kDropRun;
    uint32_t const last = (a.nX - first < kDropRun) ? a.nX : first + kDropRun;   // (the grid: first < nX)
    RA const* const A = (RA const*)a.A; RA const* const X = (RA const*)a.X;
    int const ilv = a.ilv;
    bool const withCost = (nullptr != a.cost);

    if constexpr (MFMA) {
        constexpr int NT = LN / 16, KT = LM / 4;
        constexpr bool KEEP = (KT * NT * 4 <= 128);        // X of the lane in at most 128 VGPRs (all shapes but 64 x 64)
        constexpr int KR = KEEP ? KT : 1;
        int const lane = t & 63, wave = t >> 6, lr = lane >> 4, lc = lane & 15;
        for (uint32_t y = first + uint32_t(wave); y < last; y += 4) {      // y is the same for the whole wave: the shuffles below see all 64 lanes
            uint32_t const q0 = a.start[y], q1 = withCost ? a.start[y + 1] : q0;
            RA const* const Xb = X + size_t(a.xOf[y]) * 2 * P;
            // lane (lr, lc) feeds X[k][16 n + lc], k = 4 kt + lr
            double xrk[KR][NT], xik[KR][NT], l2[NT], w2[NT];
#pragma unroll
            for (int n = 0; n < NT; ++n) { l2[n] = 0; w2[n] = 0; }
            auto load_x = [&](int const kt) {
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    int const ox = res_offset(ilv, 4 * kt + lr, 16 * n + lc, LN);
                    double const r = double(Xb[ox]), i = double(Xb[P + ox]);
                    if constexpr (KEEP) { xrk[kt][n] = r; xik[kt][n] = i; }
                    epi_nrm(w2[n], r, i);
                }
            };
            if constexpr (KEEP) {
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) load_x(kt);
            } else {
#pragma unroll 4
                for (int kt = 0; kt < KT; ++kt) load_x(kt);
            }
            for (uint32_t q = q0; q < q1; ++q) {
                RA const* Ab = A + size_t(a.aOf[q]) * 2 * LM * LM;
#pragma unroll 1
                for (int i0 = 0; i0 < LM; i0 += 16) {
                    GradeAcc cre[NT], cim[NT];
#pragma unroll
                    for (int n = 0; n < NT; ++n) { cre[n] = GradeAcc{0, 0, 0, 0}; cim[n] = GradeAcc{0, 0, 0, 0}; }
                    auto k_step = [&](int const kt) {      // the X operand from the lane's registers where it keeps them
                        TFQ_GRADE_STRIP_STEP(4 * kt + lr,
                            double xr, xi;
                            if constexpr (KEEP) { xr = xrk[kt][n]; xi = xik[kt][n]; }
                            else { int const ox = res_offset(ilv, k, 16 * n + lc, LN); xr = double(Xb[ox]); xi = double(Xb[P + ox]); })
                    };
                    if constexpr (KEEP) {                  // (the registers of X are indexed by kt: unrolled in full)
#pragma unroll
                        for (int kt = 0; kt < KT; ++kt) k_step(kt);
                    } else {
#pragma unroll 4
                        for (int kt = 0; kt < KT; ++kt) k_step(kt);
                    }
                    TFQ_GRADE_STRIP_SQUARE(l2)        // register r of the lane: row lr + 4 r of the strip, column 16 n + lc
                }
            }
            // the four lanes (lr, lc) of a column, added in ascending lr; every lane computes the sums, the lanes lr == 0 store them
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                double sum = __shfl(l2[n], lc, 64), wsum = __shfl(w2[n], lc, 64);
#pragma unroll
                for (int r = 1; r < 4; ++r) { sum += __shfl(l2[n], 16 * r + lc, 64); wsum += __shfl(w2[n], 16 * r + lc, 64); }
                if (0 == lr) {
                    if (withCost) a.cost[size_t(y) * LN + 16 * n + lc] = sum;
                    if (a.weight) a.weight[size_t(y) * LN + 16 * n + lc] = wsum;
                }
            }
        }
    } else {
        using L = GradeLanes<LM, LN>;
        constexpr int NACC = L::NACC, GRP = L::GRP;
        constexpr int ROUNDS = (int(kDropRun) + GRP - 1) / GRP;
        constexpr int RANKS = L::RANKS_ITEM;     // lanes that share a column of a block
        static_assert(GRP * LN <= 256, "one lane per entry of the records of a round");
        __shared__ double s[2][GRP * LN * RANKS];
        L const l = TFQ_GRADE_LANES(t);
        int const g = l.g, e0 = l.e0, j = l.j;
        int const rank = (P >= 256) ? t / LN : e0 / LN;  // P < 256: the row of the element
#pragma unroll 1
        for (int round = 0; round < ROUNDS; ++round) {
            uint32_t const y0 = first + uint32_t(round * GRP);
            uint32_t const y = y0 + uint32_t(g);
            if (g < GRP && y < last) {
                RA const* const Xb = X + size_t(a.xOf[y]) * 2 * P;
                double l2 = 0, w2 = 0;
#pragma unroll
                for (int n = 0; n < NACC; ++n) {         // the product block has the shape of the X block: the lane's own elements of X
                    int const ox = res_offset(ilv, (e0 + n * 256) / LN, j, LN);
                    epi_nrm(w2, double(Xb[ox]), double(Xb[P + ox]));
                }
                uint32_t const q0 = a.start[y], q1 = withCost ? a.start[y + 1] : q0;
                for (uint32_t q = q0; q < q1; ++q) {
                    RA const* Ab = A + size_t(a.aOf[q]) * 2 * LM * LM;
                    double yr[NACC], yi[NACC];
#pragma unroll
                    for (int n = 0; n < NACC; ++n) { yr[n] = 0; yi[n] = 0; }
                    TFQ_GRADE_LANE_PAIR
#pragma unroll
                    for (int n = 0; n < NACC; ++n) epi_nrm(l2, yr[n], yi[n]);
                }
                s[0][(g * LN + j) * RANKS + rank] = l2;
                s[1][(g * LN + j) * RANKS + rank] = w2;
            }
            __syncthreads();
            if (t < GRP * LN && y0 + uint32_t(t / LN) < last) {      // lane t: block y0 + t / LN of the round, right-hand side t % LN
                double sum = 0, wsum = 0;
#pragma unroll 1
                for (int r = 0; r < RANKS; ++r) { sum += s[0][t * RANKS + r]; wsum += s[1][t * RANKS + r]; }
                size_t const at = size_t(y0 + uint32_t(t / LN)) * LN + t % LN;
                if (withCost) a.cost[at] = sum;
                if (a.weight) a.weight[at] = wsum;
            }
            __syncthreads();                                         // the patch is written again in the next round
        }
    }
}

template <typename RA, int LM, int LN>
static void drop_cost_run(DropArgs const& a, hipStream_t s) {
    if (0 == a.nX) return;
    k_drop_cost<RA, LM, LN><<<dim3((a.nX + kDropRun - 1) / kDropRun), dim3(256), 0, s>>>(a);
}

void drop_cost_launch(DevPlan const& d, void const* A, uint32_t nX, uint32_t const* start, uint32_t const* aOf, uint32_t const* xOf,
    double* cost, double* weight, hipStream_t s)
{
    DropArgs a{};
    a.A = A; a.X = d.x;
    a.start = start; a.aOf = aOf; a.xOf = xOf; a.nX = nX;
    a.ilv = d.ilv; a.cost = cost; a.weight = weight;
    for_shape(d.dbl, d.LM, d.LN, [&](auto sh) { using S = decltype(sh); drop_cost_run<typename S::real, S::LM, S::LN>(a, s); });
}

} // namespace tfq
