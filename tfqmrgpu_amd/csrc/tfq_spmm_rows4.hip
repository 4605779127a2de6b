// The 4-row kernels: k_spmm_small4, k_spmm_m4, k_spmm_s4w (tfq_spmm.hpp)
#include "tfq_spmm.hpp"

namespace tfq {

// ---------------------------------------------------------------------------------------------------
// 4-row blocks that are too small for the tile kernel (4 x 4, and the float 4-row shapes: a block is 128 ... 1024 bytes).
// A thread group of 16, 20, 32 or 64 lanes owns one sub-block of 4 x min(LN, 16) elements, one element per lane; the operands
// of a block product are read ONCE per group (4 memory instructions per wave and product instead of 16 per lane in
// k_spmm_direct), pass through a group-private LDS patch and are broadcast from there.  Groups never straddle a wave and
// LDS operations of one wave complete in order, so no barrier is needed inside the product loop.
template <typename R, int LN, int EPI>
__global__ __launch_bounds__(256) void k_spmm_small4(SpmmArgs a) {
    if (gate_closed(a)) return;
    constexpr int LM = 4, P = LM * LN;
    constexpr int LNS = (LN > 16) ? 16 : LN;             // columns of a sub-block
    constexpr int NSUB = LN / LNS;                       // sub-blocks per block (LN = 32: 2)
    constexpr int PE = LM * LNS;                         // elements of a sub-block: 16, 20, 32, 64
    constexpr int GPW = 64 / PE;                         // thread groups per wave, PE lanes each: 4, 3 (4 x 5: lanes 60..63 idle), 2, 1
    constexpr int NG = 4 * GPW;                          // thread groups per work group
    constexpr int NPL = EpiPlanes<EPI>::N;
    static_assert(LN % LNS == 0 && NG % NSUB == 0, "a thread group keeps its sub-block index");
    // (r04: the patches of a wave's groups are read by ONE LDS instruction; at their natural strides -- 128 | 256 bytes in float -- the groups' segments share
    //  banks: padded by 16 bytes, as in k_spmm_s4w: 4 x 4 c iteration -2.7 %, 4 x 5 c -1 %; in double (4 x 5 z) a pad measured 0.4 % slower: none)
    constexpr int PADR = (sizeof(R) == 4) ? 4 : 0;
    __shared__ R As[NG][2 * LM * LM + PADR];
    __shared__ R Xs[NG][2 * PE + PADR];
    int const t = threadIdx.x, wv = t >> 6, ln = t & 63;
    bool const valid = (ln < GPW * PE);
    int const g = wv * GPW + (valid ? ln / PE : GPW - 1), e = valid ? ln % PE : PE;   // idle lanes walk with the wave's last group and touch nothing
    int const i = valid ? e / LNS : 0, jj = valid ? e % LNS : 0;
    int const j = (g % NSUB) * LNS + jj;                 // block column of this lane
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;   // XCD-aware launch order (tfq_plan.cpp)
    uint32_t first, last, col = 0;
    if (a.chunkFirst) { first = a.chunkFirst[chunk]; last = a.chunkFirst[chunk + 1]; col = a.chunkCol[chunk]; }
    else { first = chunk * a.CH; last = min(first + a.CH, a.nY); }

    R sr = 0, si = 0;
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
        sr = epi_scalar<R>(a, col, LN, 0, j); si = epi_scalar<R>(a, col, LN, 1, j);
    }
    double part[NPL > 0 ? NPL : 1] = {};

    // Three dependent requests lead to a product (row range -> index pairs -> operands).  As in k_spmm_m4 the work group fetches
    // the row ranges and index pairs of its whole chunk into LDS first, and a thread group requests the operands of up to NB
    // products before it multiplies the first: one memory latency per NB products instead of two per product.
    using Patch = IndexPatch<2048>;                      // (a float chunk of 4 x 4 blocks has 128 rows)
    constexpr int NB = (sizeof(R) == 8) ? 6 : 8;
    __shared__ typename Patch::Starts sStarts;
    __shared__ typename Patch::Pairs sPairs;
    uint32_t const nItems = (last - first) * NSUB;       // item = sub-block of a Y block; item % NSUB == g % NSUB
    Patch const ip(a, first, last);
    if (ip.inLds) {   // (staging written out: IndexPatch, tfq_spmm.hpp)
        for (uint32_t x = t; x <= ip.nRows; x += 256) sStarts[x] = a.starts[first + x];
        for (uint32_t x = t; x < 2 * (ip.qEnd - ip.qBase); x += 256) sPairs[x] = a.pairs[2 * size_t(ip.qBase) + x];
    }
    __syncthreads();

    auto multiply = [&](R const (&pa)[2], R const (&px)[2], R& yr, R& yi) __attribute__((always_inline)) {
        __builtin_amdgcn_wave_barrier();
        if (e < LM * LM) { As[g][e] = pa[0]; As[g][LM * LM + e] = pa[1]; }
        if (valid) { Xs[g][e] = px[0]; Xs[g][PE + e] = px[1]; }
        __builtin_amdgcn_wave_barrier();
        R cr = 0, ci = 0;
#pragma unroll
        for (int k = 0; k < LM; ++k) {
            R const ar = As[g][k * LM + i], ai = As[g][LM * LM + k * LM + i];
            R const xr = Xs[g][k * LNS + jj], xi = Xs[g][PE + k * LNS + jj];
            cr = fma_(-ai, xi, fma_(ar, xr, cr));
            ci = fma_(ai, xr, fma_(ar, xi, ci));
        }
        yr += cr; yi += ci;
    };

    for (uint32_t it = g; it < nItems; it += NG) {
        uint32_t const kr = it / NSUB, y = first + kr;
        int const eb = i * LN + j;
        size_t const off = size_t(y) * 2 * P + eb;
        EpiElem<R, EPI, false> eo;
        if (valid) eo.load(a, off, P);
        R yr = 0, yi = 0;
        if (ip.inLds) {
            uint32_t const q0 = ip.start(sStarts, kr), q1 = ip.start(sStarts, kr + 1);
            for (uint32_t qb = q0; qb < q1; qb += NB) {
                R pa[NB][2], px[NB][2];
                uint32_t ia[NB], ix[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) Patch::pair(sPairs, qb + u, ia[u], ix[u]);
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    pa[u][0] = 0; pa[u][1] = 0; px[u][0] = 0; px[u][1] = 0;
                    if (qb + u < q1) {
                        R const* Ab = (R const*)a.A + size_t(ia[u]) * 2 * (LM * LM);
                        R const* Xb = (R const*)a.X + size_t(ix[u]) * 2 * P;
                        if (e < LM * LM) { pa[u][0] = Ab[e]; pa[u][1] = Ab[LM * LM + e]; }
                        if (valid) { px[u][0] = Xb[i * LN + j]; px[u][1] = Xb[P + i * LN + j]; }
                    }
                }
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    if (qb + u < q1) multiply(pa[u], px[u], yr, yi);
            }
        } else {   // a chunk whose index data exceed the LDS patch: one product in flight, indices from global memory
            uint32_t const q0 = a.starts[y], q1 = a.starts[y + 1];
            R pa[2] = {0, 0}, px[2] = {0, 0};                // operands of the next product, in flight
            auto fetch = [&](uint32_t q) __attribute__((always_inline)) {
                R const* Ab = (R const*)a.A + size_t(a.pairs[2 * size_t(q)]) * 2 * (LM * LM);
                R const* Xb = (R const*)a.X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
                if (e < LM * LM) { pa[0] = Ab[e]; pa[1] = Ab[LM * LM + e]; }
                if (valid) { px[0] = Xb[i * LN + j]; px[1] = Xb[P + i * LN + j]; }
            };
            if (q0 < q1) fetch(q0);
            for (uint32_t q = q0; q < q1; ++q) {
                R const ca[2] = {pa[0], pa[1]}, cx[2] = {px[0], px[1]};
                if (q + 1 < q1) fetch(q + 1);
                multiply(ca, cx, yr, yi);
            }
        }
        if (valid) {
            uint32_t const bq = rhs_block<EPI>(a, y);
            epilogue_apply<R, EPI, false>(a, off, P, yr, yi, sr, si, eo, bq, eb, part);
        }
    }

    if constexpr (NPL > 0) {
        // threads that share a block column: groups with the same sub-block index, 4 rows each; added in a fixed order
        __shared__ double red[NPL][256];
#pragma unroll
        for (int p = 0; p < NPL; ++p) red[p][t] = valid ? part[p] : 0.0;
        __syncthreads();
        for (int x = t; x < NPL * LN; x += 256) {
            int const p = x / LN, jx = x % LN;
            double sum = 0;
            // (not unrolled: with 4 columns and three records the compiler unrolled all 64 terms of a sum and held them in registers --
            //  134 VGPRs for k_spmm_small4<., 4, EPI_AXPY_NRM_DOT> against 76 for its siblings, half the waves per SIMD; r03)
#pragma unroll 1
            for (int gg = jx / LNS; gg < NG; gg += NSUB)
                for (int r = 0; r < LM; ++r) sum += red[p][(gg / GPW) * 64 + (gg % GPW) * PE + r * LNS + jx % LNS];
            write_record<EPI>(a, chunk, LN, p, jx, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// 4-row blocks in double whose columns come in fours: four 4 x 4 x 4 products per v_mfma_f64_4x4x4_4b_f64.  The instruction
// keeps its four blocks interleaved at 4 lanes (measured with one-hot operands, scripts/mfma4_probe.hip): with lo = lane % 4,
// b = lane / 4 % 4, hi = lane / 16 a lane holds  A_b[i = lo][k = hi],  B_b[k = hi][j = lo]  and receives  D_b[i = hi][j = lo].
// A blocks are stored as [k][i] and X, Y blocks as [i][j], so a lane loads and stores its elements straight from the planes,
// at hi * 4 + lo (A) and hi * LN + its column(s) (X, Y): no LDS patch, no broadcast -- k_spmm_small4 spends 25 LDS
// instructions per Y block on them.  Where LN is a multiple of 8 a lane keeps W = 2 NEIGHBOURING columns (the 4 x 4
// products of the even and of the odd columns of an octet: which four columns share a product is free), so that X and
// every epilogue vector move as 16-byte accesses -- the memory pipe retires one wave-wide access per 16 clocks whatever
// its width (scripts/ta_rate.hip), and these kernels are bound by that rate (profiles/r04_small_shapes.txt).
// A slot (b of a wave, 16 per work group) walks over Y sub-blocks of 4 x 4 W columns; the four slots of a wave step
// together, a slot that has run out of products feeds zeros.
template <int LN, int EPI>
__global__ __launch_bounds__(256) void k_spmm_m4(SpmmArgs a) {
    using R = double;
    if (gate_closed(a)) return;
    constexpr int W = (LN % 8 == 0) ? 2 : 1;             // neighbouring columns of a lane
    constexpr int LM = 4, P = LM * LN, CQ = 4 * W, NSUB = LN / CQ, NS = 16, NB = 8 / W;   // NB: products of a trip
    constexpr int NPL = EpiPlanes<EPI>::N;
    static_assert(LN % CQ == 0 && NS % NSUB == 0, "a slot keeps its column group");
    int const t = threadIdx.x, wv = t >> 6, lane = t & 63;
    int const lo = lane & 3, b = (lane >> 2) & 3, hi = lane >> 4;
    int const slot = wv * 4 + b;
    int const j0 = (slot % NSUB) * CQ + W * lo;          // first block column of this lane (X and Y)
    int const ea = hi * LM + lo, ex = hi * LN + j0;      // this lane's element of an A block, its first of an X or Y block
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;   // XCD-aware launch order (tfq_plan.cpp)
    uint32_t first, last, col = 0;
    if (a.chunkFirst) { first = a.chunkFirst[chunk]; last = a.chunkFirst[chunk + 1]; col = a.chunkCol[chunk]; }
    else { first = chunk * a.CH; last = min(first + a.CH, a.nY); }

    R sr[W], si[W];
#pragma unroll
    for (int w = 0; w < W; ++w) { sr[w] = 0; si[w] = 0; }
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
#pragma unroll
        for (int w = 0; w < W; ++w) { sr[w] = epi_scalar<R>(a, col, LN, 0, j0 + w); si[w] = epi_scalar<R>(a, col, LN, 1, j0 + w); }
    }
    double part[NPL > 0 ? NPL : 1][W] = {};

    // An item = a 4 x CQ sub-block of a Y block (item % NSUB == slot % NSUB); slot s takes items s, s + 16, ...  Three dependent
    // requests lead to a product (row range -> index pairs -> operands).  The work group fetches the row ranges and the index
    // pairs of its whole chunk into LDS first (two latencies, once), so that a trip -- up to NB products of four items per
    // wave -- waits for ONE memory latency; k_spmm_small4 waits for two per product.
    using Patch = IndexPatch<1024>;                      // chunks of at most 256 Y blocks (tfq_plan.cpp: 16 KiB of 256-byte blocks = 64)
    __shared__ typename Patch::Starts sStarts;
    __shared__ typename Patch::Pairs sPairs;
    uint32_t const nItems = (last - first) * NSUB;
    Patch const ip(a, first, last);
    if (ip.inLds) {   // (staging written out: IndexPatch, tfq_spmm.hpp)
        for (uint32_t x = t; x <= ip.nRows; x += 256) sStarts[x] = a.starts[first + x];
        for (uint32_t x = t; x < 2 * (ip.qEnd - ip.qBase); x += 256) sPairs[x] = a.pairs[2 * size_t(ip.qBase) + x];
    }
    __syncthreads();

    auto product = [&](R ar, R ai, R const (&xr)[W], R const (&xi)[W], R (&yr)[W], R (&yi)[W]) __attribute__((always_inline)) {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            yr[w] = __builtin_amdgcn_mfma_f64_4x4x4f64(ar, xr[w], yr[w], 0, 0, 0);
            yr[w] = __builtin_amdgcn_mfma_f64_4x4x4f64(-ai, xi[w], yr[w], 0, 0, 0);
            yi[w] = __builtin_amdgcn_mfma_f64_4x4x4f64(ar, xi[w], yi[w], 0, 0, 0);
            yi[w] = __builtin_amdgcn_mfma_f64_4x4x4f64(ai, xr[w], yi[w], 0, 0, 0);
        }
    };

    for (uint32_t it0 = 0; it0 < nItems; it0 += NS) {    // uniform over the work group
        uint32_t const it = it0 + slot;
        bool const live = (it < nItems);
        uint32_t const k = (live ? it : 0) / NSUB, y = first + k;
        size_t const off = size_t(y) * 2 * P + ex;
        EpiOps<R, EPI, W> eo;
        if (live) eo.load(a, off, P);
        R yr[W], yi[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { yr[w] = 0; yi[w] = 0; }
        if (ip.inLds) {
            uint32_t const q0 = live ? ip.start(sStarts, k) : 0, q1 = live ? ip.start(sStarts, k + 1) : 0;
            for (uint32_t qb = q0; __any(qb < q1); qb += NB) {
                R ar[NB], ai[NB], xr[NB][W], xi[NB][W];
                uint32_t ia[NB], ix[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) Patch::pair(sPairs, qb + u, ia[u], ix[u]);
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    ar[u] = 0; ai[u] = 0;
#pragma unroll
                    for (int w = 0; w < W; ++w) { xr[u][w] = 0; xi[u][w] = 0; }
                    if (qb + u < q1) {
                        R const* Ab = (R const*)a.A + size_t(ia[u]) * 2 * (LM * LM);
                        R const* Xb = (R const*)a.X + size_t(ix[u]) * 2 * P;
                        ar[u] = Ab[ea]; ai[u] = Ab[LM * LM + ea]; vload<R, W>(xr[u], Xb + ex); vload<R, W>(xi[u], Xb + P + ex);
                    }
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    if (u > 0 && !__any(qb + u < q1)) continue;
                    product(ar[u], ai[u], xr[u], xi[u], yr, yi);
                }
            }
        } else {   // a chunk whose index data exceed the LDS patch (rows of hundreds of products): one product at a time, from global memory
            uint32_t const q0 = live ? a.starts[y] : 0, q1 = live ? a.starts[y + 1] : 0;
            for (uint32_t q = q0; __any(q < q1); ++q) {
                R ar = 0, ai = 0, xr[W], xi[W];
#pragma unroll
                for (int w = 0; w < W; ++w) { xr[w] = 0; xi[w] = 0; }
                if (q < q1) {
                    R const* Ab = (R const*)a.A + size_t(a.pairs[2 * size_t(q)]) * 2 * (LM * LM);
                    R const* Xb = (R const*)a.X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
                    ar = Ab[ea]; ai = Ab[LM * LM + ea]; vload<R, W>(xr, Xb + ex); vload<R, W>(xi, Xb + P + ex);
                }
                product(ar, ai, xr, xi, yr, yi);
            }
        }
        if (live) {
            uint32_t const bq = rhs_block<EPI>(a, y);
            epilogue_row<R, EPI, W, NPL, W>(a, off, P, yr, yi, sr, si, 0, eo, bq, ex, part, 0);
        }
    }

    if constexpr (NPL > 0) {
        // lanes that share a block column: the slots with the same column group, 4 rows each; added in a fixed order
        __shared__ double red[NPL][W][256];
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w) red[p][w][t] = part[p][w];
        __syncthreads();
        for (int x = t; x < NPL * LN; x += 256) {
            int const p = x / LN, jx = x % LN, jl = (jx % CQ) / W, jw = jx % W;
            double sum = 0;
#pragma unroll 1
            for (int ss = jx / CQ; ss < NS; ss += NSUB)
                for (int r = 0; r < LM; ++r) sum += red[p][jw][(ss / 4) * 64 + r * 16 + (ss % 4) * 4 + jl];
            write_record<EPI>(a, chunk, LN, p, jx, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// 4 x 4 | 8 | 32 in float: k_spmm_small4's arithmetic (operands of a product once per thread group through a group-private LDS patch, a per-product
// sum added to the block, k = 0..3 in order: bit-identical block products) with FOUR neighbouring columns per lane instead of one.  A lane of
// k_spmm_small4 moves 4 bytes per memory instruction, 256 per wave, and these kernels are bound by the NUMBER of wave-wide memory instructions
// (profiles/r04_four_row_shapes.txt): here X and every epilogue vector move as 16-byte accesses, a thread group is 4 | 8 | 16 lanes (row i, column quad),
// a wave works on 16 | 8 | 4 block products at once.
template <int LN, int EPI, int W = 4>   // W: neighbouring columns of a lane, 4 (16-byte accesses) or 2
__global__ __launch_bounds__(256) void k_spmm_s4w(SpmmArgs a) {
    using R = float;
    if (gate_closed(a)) return;
    constexpr int LM = 4, P = LM * LN;
    constexpr int LNS = (LN > 16) ? 16 : LN;             // columns of a sub-block
    constexpr int NSUB = LN / LNS;                       // sub-blocks per block (LN = 32: 2)
    constexpr int QL = LNS / W;                          // column quads of a sub-block: 1, 2, 4
    constexpr int PE = LM * QL;                          // lanes of a thread group: 4, 8, 16
    constexpr int AV = (LM * LM) / PE;                   // elements of an A plane a lane fetches: 4, 2, 1
    constexpr int NG = 256 / PE;                         // thread groups per work group
    constexpr int NB = 4;                                // products whose operands are requested at once
    constexpr int NPL = EpiPlanes<EPI>::N;
    static_assert(LN % LNS == 0 && LNS % W == 0 && NG % NSUB == 0, "a thread group keeps its sub-block index");
    // (the patches of the 16 | 8 | 4 groups of a wave are read by one LDS instruction: strides of 128 | 256 | 512 bytes would put them all on the
    //  same banks -- one pad of 16 bytes per column quad keeps the 16 segments of an instruction on 16 different bank quads)
    constexpr int SA = 2 * LM * LM + 4, SX = 2 * LM * LNS + 4 * ((QL * W) / 4);
    __shared__ __attribute__((aligned(16))) R AsF[NG * SA];
    __shared__ __attribute__((aligned(16))) R XsF[NG * SX];
    int const t = threadIdx.x, g = t / PE, e = t % PE;
    int const i = e / QL, jq = e % QL;
    int const j0 = (g % NSUB) * LNS + W * jq;            // first block column of this lane
    R* const As = AsF + g * SA; R* const Xs = XsF + g * SX;   // this group's patches: [re | im] planes
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;   // XCD-aware launch order (tfq_plan.cpp)
    uint32_t first, last, col = 0;
    if (a.chunkFirst) { first = a.chunkFirst[chunk]; last = a.chunkFirst[chunk + 1]; col = a.chunkCol[chunk]; }
    else { first = chunk * a.CH; last = min(first + a.CH, a.nY); }

    R sr[W], si[W];
#pragma unroll
    for (int w = 0; w < W; ++w) { sr[w] = 0; si[w] = 0; }
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
#pragma unroll
        for (int w = 0; w < W; ++w) { sr[w] = epi_scalar<R>(a, col, LN, 0, j0 + w); si[w] = epi_scalar<R>(a, col, LN, 1, j0 + w); }
    }
    double part[NPL > 0 ? NPL : 1][W] = {};

    using Patch = IndexPatch<2048>;                      // the chunk's row ranges and index pairs in LDS, as k_spmm_small4
    __shared__ typename Patch::Starts sStarts;
    __shared__ typename Patch::Pairs sPairs;
    uint32_t const nItems = (last - first) * NSUB;       // item = sub-block of a Y block; item % NSUB == g % NSUB
    Patch const ip(a, first, last);
    if (ip.inLds) {   // (staging written out: IndexPatch, tfq_spmm.hpp)
        for (uint32_t x = t; x <= ip.nRows; x += 256) sStarts[x] = a.starts[first + x];
        for (uint32_t x = t; x < 2 * (ip.qEnd - ip.qBase); x += 256) sPairs[x] = a.pairs[2 * size_t(ip.qBase) + x];
    }
    __syncthreads();

    struct Ops { R a[2][AV]; R x[2][W]; };
    auto fetch = [&](Ops& o, uint32_t ia, uint32_t ix) __attribute__((always_inline)) {
        R const* Ab = (R const*)a.A + size_t(ia) * 2 * (LM * LM) + AV * e;
        R const* Xb = (R const*)a.X + size_t(ix) * 2 * P + i * LN + j0;
        vload<R, AV>(o.a[0], Ab); vload<R, AV>(o.a[1], Ab + LM * LM);
        vload<R, W>(o.x[0], Xb); vload<R, W>(o.x[1], Xb + P);
    };
    auto multiply = [&](Ops const& o, R (&yr)[W], R (&yi)[W]) __attribute__((always_inline)) {
        __builtin_amdgcn_wave_barrier();                 // groups never straddle a wave, LDS operations of a wave complete in order
        vstore<R, AV>(As + AV * e, o.a[0]); vstore<R, AV>(As + LM * LM + AV * e, o.a[1]);
        vstore<R, W>(Xs + i * LNS + W * jq, o.x[0]); vstore<R, W>(Xs + LM * LNS + i * LNS + W * jq, o.x[1]);
        __builtin_amdgcn_wave_barrier();
        R cr[W], ci[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { cr[w] = 0; ci[w] = 0; }
#pragma unroll
        for (int k = 0; k < LM; ++k) {
            R const ar = As[k * LM + i], ai = As[LM * LM + k * LM + i];
            R xr[W], xi[W];
            vload<R, W>(xr, Xs + k * LNS + W * jq); vload<R, W>(xi, Xs + LM * LNS + k * LNS + W * jq);
#pragma unroll
            for (int w = 0; w < W; ++w) {
                cr[w] = fma_(-ai, xi[w], fma_(ar, xr[w], cr[w]));
                ci[w] = fma_(ai, xr[w], fma_(ar, xi[w], ci[w]));
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) { yr[w] += cr[w]; yi[w] += ci[w]; }
    };

    for (uint32_t it = g; it < nItems; it += NG) {
        uint32_t const kr = it / NSUB, y = first + kr;
        int const eb = i * LN + j0;
        size_t const off = size_t(y) * 2 * P + eb;
        EpiOps<R, EPI, W, false, (P * sizeof(R) >= 128) ? 1 : 0> eo;   // (4 x 4: a plane is 64 bytes, half a line -- no non-temporal accesses)
        eo.load(a, off, P);
        R yr[W], yi[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { yr[w] = 0; yi[w] = 0; }
        if (ip.inLds) {
            uint32_t const q0 = ip.start(sStarts, kr), q1 = ip.start(sStarts, kr + 1);
            for (uint32_t qb = q0; qb < q1; qb += NB) {
                Ops o[NB];
                uint32_t ia[NB], ix[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) Patch::pair(sPairs, qb + u, ia[u], ix[u]);
#pragma unroll
                for (int u = 0; u < NB; ++u) if (qb + u < q1) fetch(o[u], ia[u], ix[u]);
#pragma unroll
                for (int u = 0; u < NB; ++u) if (qb + u < q1) multiply(o[u], yr, yi);
            }
        } else {   // a chunk whose index data exceed the LDS patch: one product at a time, indices from global memory
            for (uint32_t q = a.starts[y]; q < a.starts[y + 1]; ++q) {
                Ops o;
                fetch(o, a.pairs[2 * size_t(q)], a.pairs[2 * size_t(q) + 1]);
                multiply(o, yr, yi);
            }
        }
        uint32_t const bq = rhs_block<EPI>(a, y);
        epilogue_row<R, EPI, W, NPL, W>(a, off, P, yr, yi, sr, si, 0, eo, bq, eb, part, 0);
    }

    if constexpr (NPL > 0) {
        // lanes that share a block column: the groups with the same sub-block index, 4 rows each; added in a fixed order
        __shared__ double red[NPL][W][256];
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int w = 0; w < W; ++w) red[p][w][t] = part[p][w];
        __syncthreads();
        for (int x = t; x < NPL * LN; x += 256) {
            int const p = x / LN, jx = x % LN, jl = (jx % LNS) / W, jw = jx % W;
            double sum = 0;
#pragma unroll 1
            for (int gg = jx / LNS; gg < NG; gg += NSUB)
                for (int r = 0; r < LM; ++r) sum += red[p][jw][gg * PE + r * QL + jl];
            write_record<EPI>(a, chunk, LN, p, jx, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

template <typename R, int LM, int LN, int EPI> struct Rows4Family {
    static void go(SpmmKernel k, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
        constexpr bool dbl = sizeof(R) == 8;
        if constexpr (takes_s4w(dbl, LM, LN)) if (SpmmKernel::s4w == k) {   // two or four columns per lane: s4w_columns
            if constexpr (LN < 32) if (2 == s4w_columns(LN, EPI)) { k_spmm_s4w<LN, EPI, 2><<<dim3(nWG), dim3(256), 0, s>>>(a); return; }
            k_spmm_s4w<LN, EPI><<<dim3(nWG), dim3(256), 0, s>>>(a);
            return;
        }
        if constexpr (takes_m4(dbl, LM, LN)) if (SpmmKernel::m4 == k) { k_spmm_m4<LN, EPI><<<dim3(nWG), dim3(256), 0, s>>>(a); return; }
        if constexpr (takes_small4(dbl, LM, LN)) if (SpmmKernel::small4 == k) k_spmm_small4<R, LN, EPI><<<dim3(nWG), dim3(256), 0, s>>>(a);
    }
};

bool spmm_rows4(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    return spmm_switch<Rows4Family>(k, dbl, lm, ln, epi, a, nWG, s);
}

} // namespace tfq
