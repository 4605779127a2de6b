// The 8-row kernels: k_spmm_ilv8, k_spmm_ilv8b, k_spmm_ilv8w, k_spmm_ilv8f on the interleaved orders, k_spmm_mfma8 (tfq_spmm.hpp)
#include "tfq_spmm_ilv.hpp"

namespace tfq {

// ---------------------------------------------------------------------------------------------------
// 8 x 8 complex<double> on the row-pair-interleaved element order (BASELINE config 5: the bandwidth-bound shape).
// A block is 1 KiB = ONE wave-wide 16-byte access: lane (lr = lane / 16, c = (lane % 16) / 8, j = lane % 8) holds the k pair lr
// (k = 2 lr, 2 lr + 1) of plane c (Re | Im) and column j.  The matrix tile is filled like in k_spmm_mfma8:
//      [Re A; Im A] (16 x 8)  x  [Re X | Im X] (8 x 16)  =  [Q00 Q01; Q10 Q11],   Y = (Q00 - Q11) + i (Q01 + Q10)
// with the A rows supplied in the order pi(a) = 2 (a % 4) + a / 4, so that accumulator registers (0, 1) | (2, 3) of a lane are the
// rows (2 lr, 2 lr + 1) of Q0c | Q1c: one exchange with the lane 8 further (the other plane) gives every lane one 16-byte piece
// of Re Y (c = 0) or Im Y (c = 1) -- the Y block, each epilogue operand and each result are again ONE access per wave.
// Per Y block: 2 loads per block product + 2 (3) epilogue loads + 2 stores, against 4 per product + 8 + 4 eight-byte accesses and
// an LDS round trip in k_spmm_mfma8.

template <int EPI, bool HASH, bool FIRST = false>   // FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256) void k_spmm_ilv8(SpmmArgs a) {
    if (gate_closed(a)) return;
    using R = double;
    constexpr int LN = 8, P = 64, NPL = EpiPlanes<EPI>::N;
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    using T4 = d4;
    ChunkWG const g(a);
    int const lr = g.lane >> 4, lc = g.lane & 15, cp = lc >> 3, j = lc & 7;
    R sr = 0, si = 0;
    if constexpr (UPD) { sr = epi_scalar<R>(a, g.col, LN, 0, j); si = epi_scalar<R>(a, g.col, LN, 1, j); }
    double part[NPL > 0 ? NPL : 1] = {};
    __shared__ double s[4][NPL > 0 ? NPL : 1][LN];

    int const mine = cp * P + (lr * 8 + j) * 2;                                 // this lane's 16 bytes of an X-shaped block
    R const* const A0 = (R const*)a.A + cp * P + (lr * 8 + 2 * (j & 3) + (j >> 2)) * 2;   // A: row pi(j) of plane cp, k pair lr
    R const* const X0 = (R const*)a.X + mine;
    struct Ops { d2v av, xv; };
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        o.av = *(d2v const*)(A0 + size_t(g.pairs[2 * size_t(q)]) * 2 * P);
        o.xv = *(d2v const*)(X0 + size_t(g.pairs[2 * size_t(q) + 1]) * 2 * P);
    };
    for (uint32_t u = g.wave; u < g.last - g.first; u += 4) {
        uint32_t const y = g.first + u;
        uint64_t const key = HASH ? shadow_key(uint32_t(a.origCol[g.col]), a.rowI[y]) : 0;
        T4 acc = T4{0, 0, 0, 0};
        uint32_t const q0 = g.starts[y], nq = g.starts[y + 1] - q0;
        constexpr int DEPTH = 4;
        Ops o[DEPTH];
        size_t const yoff = size_t(y) * 2 * P + mine;
        // the epilogue operands travel while the products are computed, requested in front of the first products' operands: -1 % (profiles/r02_ab_traversal.txt)
        EpiPiece<d2v> eo;
        eo.template load<EPI, FIRST, HASH>(a, yoff);
#pragma unroll
        for (int dd = 0; dd < DEPTH; ++dd) if (uint32_t(dd) < nq) fetch(o[dd], q0 + dd);
        for (uint32_t base = 0; base < nq; base += DEPTH) {
#pragma unroll
            for (int dd = 0; dd < DEPTH; ++dd) {
                if (base + dd < nq) {
                    acc = Acc<R>::mma(o[dd].av[0], o[dd].xv[0], acc);
                    acc = Acc<R>::mma(o[dd].av[1], o[dd].xv[1], acc);
                    if (base + dd + DEPTH < nq) fetch(o[dd], q0 + base + dd + DEPTH);
                }
            }
        }
        // lanes of plane 0 hold (Q00, Q10), lanes of plane 1 (Q01, Q11), rows 2 lr and 2 lr + 1: Re Y = Q00 - Q11, Im Y = Q01 + Q10
        d2v const qa = d2v{acc[0], acc[1]}, qb = xor8(d2v{acc[2], acc[3]});
        d2v const yM = cp ? d2v{qa[0] + qb[0], qa[1] + qb[1]} : d2v{qa[0] - qb[0], qa[1] - qb[1]};   // this lane's plane of Y
        auto const [yr, yi] = planes(yM, xor8(yM), cp);
        if constexpr (UPD) {
            auto const [ur, ui] = planes(eo.u, xor8(eo.u), cp);
            d2v nr, ni;
            ReIm<d2v> w;    // the shadow vector: Re and Im of the two elements
            if constexpr (HASH) {
                uint64_t const hq = shadow_quad(key, uint32_t(lr), uint32_t(j), LN);   // rows 2 lr, 2 lr + 1 of column j
#pragma unroll
                for (int e = 0; e < 2; ++e) { w.r[e] = shadow_pick(hq, e, 0); w.i[e] = shadow_pick(hq, e, 1); }
            } else {
                f2v const wM = eo.w, wO = xor8(wM);
                d2v const wOd = d2v{wO[0], wO[1]}, wMd = d2v{wM[0], wM[1]};
                w = planes(wMd, wOd, cp);
            }
            if constexpr (EPI == EPI_XPAY_DOT) {          // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                auto const [vr, vi] = planes(eo.v, xor8(eo.v), cp);
#pragma unroll
                for (int e = 0; e < 2; ++e) { R a, b; epi_xpay2(a, b, yr[e], yi[e], ur[e], ui[e], vr[e], vi[e], sr, si); nr[e] = a; ni[e] = b; }
            } else {                                      // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
#pragma unroll
                for (int e = 0; e < 2; ++e) { R a, b; epi_axpy(a, b, yr[e], yi[e], ur[e], ui[e], sr, si); nr[e] = a; ni[e] = b; }
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {                 // every lane has both parts: the lanes of plane 0 are the ones that count
                epi_dot(part[0], part[1], nr[e], ni[e], w.r[e], w.i[e]);
                if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[2], nr[e], ni[e]);
            }
            __builtin_nontemporal_store(yM, (d2v*)((R*)a.Y + yoff));
            __builtin_nontemporal_store(cp ? ni : nr, (d2v*)((R*)a.e0 + yoff));
        } else if constexpr (EPI == EPI_RESIDUAL) {       // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
            uint32_t const bq = a.bOfX ? a.bOfX[y] : y;   // (written out: rhs_block changes the assembly)
            d2v bM = d2v{0, 0};
            if (bq != 0xffffffffu) bM = *(d2v const*)((R const*)a.B + size_t(bq) * 2 * P + mine);
            auto const [br, bi] = planes(bM, xor8(bM), cp);
#pragma unroll
            for (int e = 0; e < 2; ++e) epi_nrm(part[0], yr[e] + R(-1) * br[e], yi[e] + R(-1) * bi[e]);
        } else {
            __builtin_nontemporal_store(yM, (d2v*)((R*)a.Y + yoff));
        }
    }
    if constexpr (NPL > 0) {
        // the rows of a column sit 16 lanes apart (lr); lanes 0..7 (plane 0, lr 0) hold the column sums
#pragma unroll
        for (int p = 0; p < NPL; ++p) {
            double v = part[p];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (g.lane < 8) s[g.wave][p][g.lane] = v;
        }
        __syncthreads();
        for (int e = threadIdx.x; e < NPL * LN; e += 256) {
            int const p = e / LN, jj = e % LN;
            double const sum = ((s[0][p][jj] + s[1][p][jj]) + s[2][p][jj]) + s[3][p][jj];
            write_record<EPI>(a, g.chunk, LN, p, jj, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, g.col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// 8 x 8 complex<double>, COLUMN-BATCHED (r03).  Block columns whose row patterns are identical (Plan::colBatch: dense right-hand-side columns, BASELINE
// config 5) are multiplied nb <= kColBatchMax = 2 at a time: the work group of chunk c of the FIRST column of a batch also does chunk c of the other columns -- same
// block rows, same A blocks, the X / Y blocks a column's block count further on -- so that an A block is fetched once for nb block products; the launch
// runs over the chunks of the batches' first columns only (DevPlan::orderB).  With blocks of 1 KiB the operand path bounds this shape (timing-only probe, profiles/r03_probes.txt:
// 3 of 4 A fetches skipped = -16 % / -22 % on the fused multiplies).  Chunks, records and every sum are those of k_spmm_ilv8: bit-identical results.
template <int EPI, bool HASH, int NB, bool FIRST = false>   // NB: columns of a batch at most; FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256, 3) void k_spmm_ilv8b(SpmmArgs a) {
    if (gate_closed(a)) return;
    using R = double;
    constexpr int LN = 8, P = 64, NPL = EpiPlanes<EPI>::N;
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    using T4 = d4;
    ChunkWG const g(a);
    int const lr = g.lane >> 4, lc = g.lane & 15, cp = lc >> 3, j = lc & 7;
    uint32_t const cb = a.colBatch[g.col];
    if (cb & 15u) return;                       // (a later column of a batch: not in this launch's order, SpmmArgs::order = DevPlan::orderB)
    int const nb = int(cb >> 4);                // 1 ... NB columns
    uint32_t dBlk[NB], dChk[NB];                // how far the blocks / chunks of column col + k lie behind those of column col
    R sr[NB], si[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        dBlk[k] = 0; dChk[k] = 0; sr[k] = 0; si[k] = 0;
        if (k < nb) {
            dBlk[k] = a.colStart[g.col + k] - a.colStart[g.col]; dChk[k] = a.colChunkPtr[g.col + k] - a.colChunkPtr[g.col];
            if constexpr (UPD) { sr[k] = ((R const*)a.sc)[(size_t(g.col + k) * 2 + 0) * LN + j]; si[k] = ((R const*)a.sc)[(size_t(g.col + k) * 2 + 1) * LN + j]; }   // (written out: epi_scalar changes the assembly)
        }
    }
    double part[NB][NPL > 0 ? NPL : 1] = {};
    __shared__ double s[NB][4][NPL > 0 ? NPL : 1][LN];

    int const mine = cp * P + (lr * 8 + j) * 2;                                 // this lane's 16 bytes of an X-shaped block
    R const* const A0 = (R const*)a.A + cp * P + (lr * 8 + 2 * (j & 3) + (j >> 2)) * 2;   // A: row pi(j) of plane cp, k pair lr
    R const* const X0 = (R const*)a.X + mine;
    struct Ops { d2v av; d2v xv[NB]; };
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        o.av = *(d2v const*)(A0 + size_t(g.pairs[2 * size_t(q)]) * 2 * P);
        uint32_t const xb = g.pairs[2 * size_t(q) + 1];
#pragma unroll
        for (int k = 0; k < NB; ++k) if (k < nb) o.xv[k] = *(d2v const*)(X0 + size_t(xb + dBlk[k]) * 2 * P);
    };
    for (uint32_t u = g.wave; u < g.last - g.first; u += 4) {
        uint32_t const y = g.first + u;
        T4 acc[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = T4{0, 0, 0, 0};
        uint32_t const q0 = g.starts[y], nq = g.starts[y + 1] - q0;
        constexpr int DEPTH = 2;   // block products in flight (3 | 4 measured level or slower, profiles/r03_column_batches.txt)
        Ops o[DEPTH];
#pragma unroll
        for (int dd = 0; dd < DEPTH; ++dd) if (uint32_t(dd) < nq) fetch(o[dd], q0 + dd);
        for (uint32_t base = 0; base < nq; base += DEPTH) {
#pragma unroll
            for (int dd = 0; dd < DEPTH; ++dd) {
                if (base + dd < nq) {
#pragma unroll
                    for (int k = 0; k < NB; ++k) if (k < nb) {
                        acc[k] = Acc<R>::mma(o[dd].av[0], o[dd].xv[k][0], acc[k]);
                        acc[k] = Acc<R>::mma(o[dd].av[1], o[dd].xv[k][1], acc[k]);
                    }
                    if (base + dd + DEPTH < nq) fetch(o[dd], q0 + base + dd + DEPTH);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) if (k < nb) {
            size_t const yoff = size_t(y + dBlk[k]) * 2 * P + mine;
            EpiPiece<d2v> eo;
            eo.template load<EPI, FIRST, HASH>(a, yoff);   // (requested here, not in front of the products: measured better with two columns per wave)
            // lanes of plane 0 hold (Q00, Q10), lanes of plane 1 (Q01, Q11), rows 2 lr and 2 lr + 1: Re Y = Q00 - Q11, Im Y = Q01 + Q10
            d2v const qa = d2v{acc[k][0], acc[k][1]}, qb = xor8(d2v{acc[k][2], acc[k][3]});
            d2v const yM = cp ? d2v{qa[0] + qb[0], qa[1] + qb[1]} : d2v{qa[0] - qb[0], qa[1] - qb[1]};   // this lane's plane of Y
            auto const [yr, yi] = planes(yM, xor8(yM), cp);
            if constexpr (UPD) {
                auto const [ur, ui] = planes(eo.u, xor8(eo.u), cp);
                d2v nr, ni;
                ReIm<d2v> w;    // the shadow vector: Re and Im of the two elements
                if constexpr (HASH) {
                    uint64_t const key = shadow_key(uint32_t(a.origCol[g.col + k]), a.rowI[y]);   // (the batch's columns have the same block rows)
                    uint64_t const hq = shadow_quad(key, uint32_t(lr), uint32_t(j), LN);       // rows 2 lr, 2 lr + 1 of column j
#pragma unroll
                    for (int e = 0; e < 2; ++e) { w.r[e] = shadow_pick(hq, e, 0); w.i[e] = shadow_pick(hq, e, 1); }
                } else {
                    f2v const wM = eo.w, wO = xor8(wM);
                    d2v const wOd = d2v{wO[0], wO[1]}, wMd = d2v{wM[0], wM[1]};
                    w = planes(wMd, wOd, cp);
                }
                if constexpr (EPI == EPI_XPAY_DOT) {          // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                    auto const [vr, vi] = planes(eo.v, xor8(eo.v), cp);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        R const tr = __builtin_fma(-si[k], ui[e], __builtin_fma(sr[k], ur[e], vr[e]));
                        R const ti = __builtin_fma(sr[k], ui[e], __builtin_fma(si[k], ur[e], vi[e]));
                        nr[e] = __builtin_fma(-si[k], ti, __builtin_fma(sr[k], tr, yr[e]));
                        ni[e] = __builtin_fma(sr[k], ti, __builtin_fma(si[k], tr, yi[e]));
                    }
                } else {                                      // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        nr[e] = __builtin_fma(-si[k], yi[e], __builtin_fma(sr[k], yr[e], ur[e]));
                        ni[e] = __builtin_fma(sr[k], yi[e], __builtin_fma(si[k], yr[e], ui[e]));
                    }
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {                 // every lane has both parts: the lanes of plane 0 are the ones that count
                    epi_dot(part[k][0], part[k][1], nr[e], ni[e], w.r[e], w.i[e]);
                    if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[k][2], nr[e], ni[e]);
                }
                __builtin_nontemporal_store(yM, (d2v*)((R*)a.Y + yoff));
                __builtin_nontemporal_store(cp ? ni : nr, (d2v*)((R*)a.e0 + yoff));
            } else if constexpr (EPI == EPI_RESIDUAL) {       // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
                uint32_t const bq = rhs_block<EPI>(a, y + dBlk[k]);
                d2v bM = d2v{0, 0};
                if (bq != 0xffffffffu) bM = *(d2v const*)((R const*)a.B + size_t(bq) * 2 * P + mine);
                auto const [br, bi] = planes(bM, xor8(bM), cp);
#pragma unroll
                for (int e = 0; e < 2; ++e) epi_nrm(part[k][0], yr[e] + R(-1) * br[e], yi[e] + R(-1) * bi[e]);
            } else {
                __builtin_nontemporal_store(yM, (d2v*)((R*)a.Y + yoff));
            }
        }
    }
    if constexpr (NPL > 0) {
        // the rows of a column sit 16 lanes apart (lr); lanes 0..7 (plane 0, lr 0) hold the column sums
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int p = 0; p < NPL; ++p) {
                double v = part[k][p];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (g.lane < 8) s[k][g.wave][p][g.lane] = v;
            }
        __syncthreads();
        for (int e = threadIdx.x; e < NB * NPL * LN; e += 256) {
            int const k = e / (NPL * LN), p = (e / LN) % NPL, jj = e % LN;
            if (k < nb) {
                double const sum = ((s[k][0][p][jj] + s[k][1][p][jj]) + s[k][2][p][jj]) + s[k][3][p][jj];
                uint32_t dc = dChk[0];
#pragma unroll
                for (int kk = 1; kk < NB; ++kk) if (kk == k) dc = dChk[kk];
                write_record<EPI>(a, g.chunk + dc, LN, p, jj, sum);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// 8 x 32 and 8 x 64 complex<double> on the row-pair-interleaved order: k_spmm_ilv8's tile ([Re A; Im A] x [Re X | Im X], one exchange
// with the lane 8 further) once per group of 8 block columns.  A wave-wide 16-byte access covers both planes and all 8 rows of ONE
// column group (8 segments of 128 bytes), so a block product is 1 + LN / 8 loads of 1 KiB (k_spmm_mfma8 on the native order: 2 + 2 LN / 8
// of 512 bytes) and every vector of the epilogue LN / 8 accesses per Y block.  No epilogue prefetch (the accumulators of 8 column groups
// are 64 registers), the shadow vector is read.
template <int LN, int EPI, bool FIRST = false>   // FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256) void k_spmm_ilv8w(SpmmArgs a) {
    if (gate_closed(a)) return;
    using R = double;
    static_assert(LN > 8 && (LN % 8 == 0 || LN < 16), "groups of 8 block columns, the last one of 8 x 9 | 8 x 10 ragged");
    constexpr int NTB = (LN + 7) / 8;                 // column groups of a block
    constexpr bool RAGGED = (LN % 8 != 0);            // (r04) 8 x 9, 8 x 10: the second group has 1 | 2 columns -- its other lanes load nothing, multiply zeros and store nothing
    constexpr int NT = (NTB > 4) ? 4 : NTB;           // column groups of one unit of work of a wave (8 x 64: a Y block is two units;
                                                      //  all 8 groups in one wave need 255-271 VGPRs = one wave per SIMD)
    constexpr int HALVES = NTB / NT;
    constexpr int P = 8 * LN, PA = 64, NPL = EpiPlanes<EPI>::N;
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    using T4 = d4;
    ChunkWG const g(a);
    int const lr = g.lane >> 4, lc = g.lane & 15, cp = lc >> 3, j = lc & 7;
    double part[NPL > 0 ? NPL : 1][NT] = {};
    __shared__ double s[4][NPL > 0 ? NPL : 1][LN];
    if constexpr (NPL > 0) {   // (8 x 64: a wave meets both halves of the columns only if it has at least two units: clear what it may not write)
        for (int e = threadIdx.x; e < 4 * NPL * LN; e += 256) (&s[0][0][0])[e] = 0;
        __syncthreads();
    }

    R const* const A0 = (R const*)a.A + cp * PA + (lr * 8 + 2 * (j & 3) + (j >> 2)) * 2;   // A: row pi(j) of plane cp, k pair lr (as k_spmm_ilv8)
    struct Ops { d2v av, xv[NT]; };
    // units u = wave, wave + 4, ...: unit u is (Y block u / HALVES, half u % HALVES of its column groups); 4 is a multiple of HALVES,
    // so a wave keeps its half
    static_assert(4 % HALVES == 0, "a wave keeps its half of the column groups");
    int const t0 = (g.wave % HALVES) * NT;                  // first column group of this wave's units
    // this lane's 16 bytes of column group t0 + t of an X-shaped block: plane cp, row pair lr, column 8 (t0 + t) + j
    auto mine = [&](int t) { return cp * P + (lr * LN + 8 * (t0 + t) + j) * 2; };
    auto live = [&](int t) { return !RAGGED || 8 * (t0 + t) + j < LN; };      // this lane's column of group t exists
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        o.av = *(d2v const*)(A0 + size_t(g.pairs[2 * size_t(q)]) * 2 * PA);
        R const* Xb = (R const*)a.X + size_t(g.pairs[2 * size_t(q) + 1]) * 2 * P;
#pragma unroll
        for (int t = 0; t < NT; ++t) o.xv[t] = live(t) ? *(d2v const*)(Xb + mine(t)) : d2v{0, 0};
    };
    for (uint32_t u = g.wave; u < (g.last - g.first) * HALVES; u += 4) {
        uint32_t const y = g.first + u / HALVES;
        T4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = T4{0, 0, 0, 0};
        uint32_t const q0 = g.starts[y], q1 = g.starts[y + 1];
        auto mma = [&](Ops const& o) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = Acc<R>::mma(o.av[0], o.xv[t][0], acc[t]);
                acc[t] = Acc<R>::mma(o.av[1], o.xv[t][1], acc[t]);
            }
        };
        // (r04) with at most two column groups per wave (8 x 9, 8 x 10) the epilogue operands are requested in FRONT of the block products, as k_spmm_ilv8 does:
        // 20 registers; with four groups they are not (the accumulators of four groups are 32, the operand sets 40 registers)
        constexpr bool PRE = UPD && (NT <= 2);
        size_t const yb = size_t(y) * 2 * P;
        d2v uP[PRE ? NT : 1], vP[PRE ? NT : 1]; f2v wP[PRE ? NT : 1];
        if constexpr (PRE) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                uP[t] = d2v{0, 0}; vP[t] = d2v{0, 0}; wP[t] = f2v{0, 0};
                if (live(t)) {
                    if constexpr (!(EPI == EPI_XPAY_DOT && FIRST)) {
                        uP[t] = ld_stream<!RAGGED>((d2v const*)((R const*)a.e0 + yb + mine(t)));
                        if constexpr (EPI == EPI_XPAY_DOT) vP[t] = ld_stream<!RAGGED>((d2v const*)((R const*)a.e1 + yb + mine(t)));
                    }
                    wP[t] = ld_stream<!RAGGED>((f2v const*)(a.v3 + yb + mine(t)));
                }
            }
        }
        Ops o0, o1;
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

        uint32_t const bq = rhs_block<EPI>(a, y);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            size_t const yoff = yb + mine(t);
            bool const on = live(t);
            // lanes of plane 0 hold (Q00, Q10), lanes of plane 1 (Q01, Q11), rows 2 lr and 2 lr + 1: Re Y = Q00 - Q11, Im Y = Q01 + Q10
            d2v const qa = d2v{acc[t][0], acc[t][1]}, qb = xor8(d2v{acc[t][2], acc[t][3]});
            d2v const yM = cp ? d2v{qa[0] + qb[0], qa[1] + qb[1]} : d2v{qa[0] - qb[0], qa[1] - qb[1]};   // this lane's plane of Y
            auto const [yr, yi] = planes(yM, xor8(yM), cp);
            if constexpr (UPD) {
                R const srt = on ? ((R const*)a.sc)[(size_t(g.col) * 2 + 0) * LN + 8 * (t0 + t) + j] : R(0);   // (written out: epi_scalar changes the assembly)
                R const sit = on ? ((R const*)a.sc)[(size_t(g.col) * 2 + 1) * LN + 8 * (t0 + t) + j] : R(0);
                d2v uM = d2v{0, 0}, vM = d2v{0, 0}; f2v wM = f2v{0, 0};
                if constexpr (PRE) { uM = uP[t]; vM = vP[t]; wM = wP[t]; }
                else {
                    if constexpr (!(EPI == EPI_XPAY_DOT && FIRST)) {   // (first iteration of a solve: old v4 = v8 = 0, not read)
                        if (on) uM = ld_stream<!RAGGED>((d2v const*)((R const*)a.e0 + yoff));
                        if constexpr (EPI == EPI_XPAY_DOT) if (on) vM = ld_stream<!RAGGED>((d2v const*)((R const*)a.e1 + yoff));
                    }
                    if (on) wM = ld_stream<!RAGGED>((f2v const*)(a.v3 + yoff));
                }
                auto const [ur, ui] = planes(uM, xor8(uM), cp);
                f2v const wO = xor8(wM);
                d2v const wOd = d2v{wO[0], wO[1]}, wMd = d2v{wM[0], wM[1]};
                auto const [w0, w1] = planes(wMd, wOd, cp);
                d2v nr, ni;
                if constexpr (EPI == EPI_XPAY_DOT) {          // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                    auto const [vr, vi] = planes(vM, xor8(vM), cp);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        R const tr = __builtin_fma(-sit, ui[e], __builtin_fma(srt, ur[e], vr[e]));
                        R const ti = __builtin_fma(srt, ui[e], __builtin_fma(sit, ur[e], vi[e]));
                        nr[e] = __builtin_fma(-sit, ti, __builtin_fma(srt, tr, yr[e]));
                        ni[e] = __builtin_fma(srt, ti, __builtin_fma(sit, tr, yi[e]));
                    }
                } else {                                      // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        nr[e] = __builtin_fma(-sit, yi[e], __builtin_fma(srt, yr[e], ur[e]));
                        ni[e] = __builtin_fma(srt, yi[e], __builtin_fma(sit, yr[e], ui[e]));
                    }
                }
#pragma unroll
                for (int e = 0; e < 2; ++e) {                 // every lane has both parts: the lanes of plane 0 are the ones that count
                    epi_dot(part[0][t], part[1][t], nr[e], ni[e], w0[e], w1[e]);
                    if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[2][t], nr[e], ni[e]);
                }
                if (on) {
                    st_stream<!RAGGED>((d2v*)((R*)a.Y + yoff), yM);
                    st_stream<!RAGGED>((d2v*)((R*)a.e0 + yoff), cp ? ni : nr);
                }
            } else if constexpr (EPI == EPI_RESIDUAL) {       // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
                d2v bM = d2v{0, 0};
                if (bq != 0xffffffffu && on) bM = *(d2v const*)((R const*)a.B + size_t(bq) * 2 * P + mine(t));
                auto const [br, bi] = planes(bM, xor8(bM), cp);
#pragma unroll
                for (int e = 0; e < 2; ++e) epi_nrm(part[0][t], yr[e] + R(-1) * br[e], yi[e] + R(-1) * bi[e]);
            } else {
                if (on) st_stream<!RAGGED>((d2v*)((R*)a.Y + yoff), yM);
            }
        }
    }
    if constexpr (NPL > 0) {
        // the rows of a column sit 16 lanes apart (lr); lanes 0..7 (plane 0, lr 0) hold the column sums of their column group
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                double v = part[p][t];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (g.lane < 8 && (!RAGGED || 8 * (t0 + t) + g.lane < LN)) s[g.wave][p][8 * (t0 + t) + g.lane] = v;
            }
        __syncthreads();
        for (int e = threadIdx.x; e < NPL * LN; e += 256) {
            int const p = e / LN, jj = e % LN;
            double const sum = ((s[0][p][jj] + s[1][p][jj]) + s[2][p][jj]) + s[3][p][jj];
            write_record<EPI>(a, g.chunk, LN, p, jj, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, g.col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// 8 x 8, 8 x 32 and 8 x 64 complex<float> with groups of FOUR rows interleaved (plane[r/4][s][r%4], the order of k_spmm_ilv16f): the float
// counterpart of k_spmm_ilv8 / k_spmm_ilv8w.  The tile is again [Re A; Im A] (16 x 8) x [Re X | Im X] (8 x 16) per group of 8 block columns, but
// a 16-byte access of a lane is a k QUAD, and a block of 8 rows has only two of them where v_mfma_f32_16x16x4_f32 has four k slots per
// step: the upper two slots take the NEXT block product of the same Y block (lane groups 0, 1: product q, lane groups 2, 3: product q + 1;
// both sums land in the same accumulators), so ONE wave-wide 1-KiB access fetches the A blocks of two products, one per column group their X
// blocks (k_spmm_mfma8<float> on the native order: 4 bytes per lane and access).  Accumulator registers 0..3 of a lane are the rows
// 4 (lane / 16) .. + 3 of [Re A; Im A] X: lane groups 0, 1 hold the Re A part, groups 2, 3 the Im A part; Re Y = Q00 - Q11 and Im Y = Q01 + Q10
// meet through one exchange with lane ^ 40 (other lane-group half, other plane), after which lanes 0 .. 31 hold one 16-byte piece of Y each
// (quad lane / 16 of column lane % 8, plane (lane % 16) / 8) -- the Y block, every epilogue operand and every result of a column group
// is one half-wave access.  The shadow vector is read.
template <int LN, int EPI, bool FIRST = false>   // FIRST: the launch of the first iteration of a solve (SpmmArgs::first)
__global__ __launch_bounds__(256) void k_spmm_ilv8f(SpmmArgs a) {
    if (gate_closed(a)) return;
    using R = float;
    static_assert(LN % 8 == 0, "groups of 8 block columns");
    constexpr int NTB = LN / 8;                       // column groups of a block
    constexpr int NT = (NTB > 4) ? 4 : NTB;           // column groups of one unit of work of a wave
    constexpr int HALVES = NTB / NT;
    constexpr int P = 8 * LN, PA = 64, NPL = EpiPlanes<EPI>::N;
    constexpr bool UPD = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15, cp = lc >> 3, j = lc & 7;
    int const g = lr & 1;                             // k quad (operands) | row quad (results, lanes 0 .. 31)
    bool const second = (lr >= 2);                    // operands: this lane feeds the second product of a pair
    bool const owner = (lr < 2);                      // results: lanes 0 .. 31 own the pieces of Y
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts;
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;
    uint32_t const first = a.chunkFirst[chunk], last = a.chunkFirst[chunk + 1], col = a.chunkCol[chunk];
    double part[NPL > 0 ? NPL : 1][NT] = {};
    __shared__ double s[4][NPL > 0 ? NPL : 1][LN];
    if constexpr (NPL > 0 && HALVES > 1) {   // a wave writes the sums of its half of the column groups only
        for (int e = threadIdx.x; e < 4 * NPL * LN; e += 256) (&s[0][0][0])[e] = 0;
        __syncthreads();
    }
    static_assert(4 % HALVES == 0, "a wave keeps its half of the column groups");
    int const t0 = (wave % HALVES) * NT;              // first column group of this wave's units
    // 16 bytes of an X-shaped block: plane cp, quad g, column 8 (t0 + t) + j;  of an A block (transposed): plane cp, k quad g, row j
    auto mine = [&](int t) { return cp * P + (g * LN + 8 * (t0 + t) + j) * 4; };
    int const mineA = cp * PA + (g * 8 + j) * 4;
    struct Ops { f4v av, xv[NT]; };
    auto fetch = [&](Ops& o, uint32_t q, uint32_t q1) __attribute__((always_inline)) {   // products q (lane groups 0, 1) and q + 1 (2, 3)
        bool const two = (q + 1 < q1);
        uint32_t const ia0 = pairs[2 * size_t(q)], ix0 = pairs[2 * size_t(q) + 1];
        uint32_t const ia1 = two ? pairs[2 * size_t(q) + 2] : ia0, ix1 = two ? pairs[2 * size_t(q) + 3] : ix0;
        uint32_t const ia = second ? ia1 : ia0, ix = second ? ix1 : ix0;
        o.av = f4v{0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < NT; ++t) o.xv[t] = f4v{0, 0, 0, 0};
        if (!second || two) {
            o.av = *(f4v const*)((R const*)a.A + size_t(ia) * 2 * PA + mineA);
            R const* Xb = (R const*)a.X + size_t(ix) * 2 * P;
#pragma unroll
            for (int t = 0; t < NT; ++t) o.xv[t] = *(f4v const*)(Xb + mine(t));
        }
    };
    for (uint32_t u = wave; u < (last - first) * HALVES; u += 4) {
        uint32_t const y = first + u / HALVES;
        f4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f4{0, 0, 0, 0};
        uint32_t const q0 = starts[y], q1 = starts[y + 1];
        auto mma = [&](Ops const& o) __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 4; ++e)                   // step e contracts k = 4 g + e of product q (slots 0, 1) and q + 1 (slots 2, 3)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = Acc<R>::mma(o.av[e], o.xv[t][e], acc[t]);
        };
        Ops o0, o1;
        if (q0 < q1) fetch(o0, q0, q1);
        if (q0 + 2 < q1) fetch(o1, q0 + 2, q1);
        uint32_t q = q0;
        for (; q + 4 <= q1 + 1 && q + 2 < q1; q += 4) {   // two pairs per trip while a second pair exists
            mma(o0);
            if (q + 4 < q1) fetch(o0, q + 4, q1);
            mma(o1);
            if (q + 6 < q1) fetch(o1, q + 6, q1);
        }
        if (q < q1) mma(o0);

        uint32_t const bq = rhs_block<EPI>(a, y);
        size_t const yb = size_t(y) * 2 * P;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            // lane (lr, cp): lr < 2: [Re A X] rows of quad lr, x (Re | Im) X; lr >= 2: [Im A X] rows of quad lr - 2.  Partner lane ^ 40.
            f4v const v = f4v{acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
            f4v const o = f4v{__shfl_xor(v[0], 40), __shfl_xor(v[1], 40), __shfl_xor(v[2], 40), __shfl_xor(v[3], 40)};
            // owners: plane 0: Re Y = Q00 - Q11, plane 1: Im Y = Q01 + Q10
            f4v const yM = cp ? f4v{v[0] + o[0], v[1] + o[1], v[2] + o[2], v[3] + o[3]} : f4v{v[0] - o[0], v[1] - o[1], v[2] - o[2], v[3] - o[3]};
            auto const [yr, yi] = planes(yM, xor8(yM), cp);
            size_t const yoff = yb + mine(t);
            if constexpr (UPD) {
                R const srt = ((R const*)a.sc)[(size_t(col) * 2 + 0) * LN + 8 * (t0 + t) + j];   // (written out: epi_scalar changes the assembly)
                R const sit = ((R const*)a.sc)[(size_t(col) * 2 + 1) * LN + 8 * (t0 + t) + j];
                f4v uM = f4v{0, 0, 0, 0}, vM = f4v{0, 0, 0, 0}, wM = f4v{0, 0, 0, 0};
                if (owner) {
                    if constexpr (!(EPI == EPI_XPAY_DOT && FIRST)) {   // (first iteration of a solve: old v4 = v8 = 0, not read)
                        uM = __builtin_nontemporal_load((f4v const*)((R const*)a.e0 + yoff));
                        if constexpr (EPI == EPI_XPAY_DOT) vM = __builtin_nontemporal_load((f4v const*)((R const*)a.e1 + yoff));
                    }
                    wM = __builtin_nontemporal_load((f4v const*)(a.v3 + yoff));
                }
                auto x8 = [](f4v z) { return f4v{__shfl_xor(z[0], 8), __shfl_xor(z[1], 8), __shfl_xor(z[2], 8), __shfl_xor(z[3], 8)}; };
                auto const [ur, ui] = planes(uM, x8(uM), cp);
                auto const [w0, w1] = planes(wM, x8(wM), cp);
                f4v nr, ni;
                if constexpr (EPI == EPI_XPAY_DOT) {          // v9 := A v6; v4 := v8 + beta v4; v4 := v9 + beta v4 (tfqmrgpu_core.hxx:196-202)
                    auto const [vr, vi] = planes(vM, x8(vM), cp);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        R const tr = __builtin_fmaf(-sit, ui[e], __builtin_fmaf(srt, ur[e], vr[e]));
                        R const ti = __builtin_fmaf(srt, ui[e], __builtin_fmaf(sit, ur[e], vi[e]));
                        nr[e] = __builtin_fmaf(-sit, ti, __builtin_fmaf(srt, tr, yr[e]));
                        ni[e] = __builtin_fmaf(srt, ti, __builtin_fmaf(sit, tr, yi[e]));
                    }
                } else {                                      // v8 := A v6; v5 := alfa v8 + v5 (tfqmrgpu_core.hxx:224-228)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        nr[e] = __builtin_fmaf(-sit, yi[e], __builtin_fmaf(srt, yr[e], ur[e]));
                        ni[e] = __builtin_fmaf(srt, yi[e], __builtin_fmaf(sit, yr[e], ui[e]));
                    }
                }
                if (owner) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {             // every owner lane has both parts: the lanes of plane 0 are the ones that count
                        epi_dot(part[0][t], part[1][t], nr[e], ni[e], w0[e], w1[e]);
                        if constexpr (EPI == EPI_AXPY_NRM_DOT) epi_nrm(part[2][t], nr[e], ni[e]);
                    }
                    __builtin_nontemporal_store(yM, (f4v*)((R*)a.Y + yoff));
                    __builtin_nontemporal_store(cp ? ni : nr, (f4v*)((R*)a.e0 + yoff));
                }
            } else if constexpr (EPI == EPI_RESIDUAL) {       // |A x - b|^2, nothing stored (tfqmrgpu_core.hxx:265-269)
                f4v bM = f4v{0, 0, 0, 0};
                if (owner && bq != 0xffffffffu) bM = *(f4v const*)((R const*)a.B + size_t(bq) * 2 * P + mine(t));
                f4v const bO = f4v{__shfl_xor(bM[0], 8), __shfl_xor(bM[1], 8), __shfl_xor(bM[2], 8), __shfl_xor(bM[3], 8)};
                f4v const br = cp ? bO : bM, bi = cp ? bM : bO;
                if (owner) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        R const rr = yr[e] + R(-1) * br[e], ri = yi[e] + R(-1) * bi[e];
                        epi_nrm(part[0][t], rr, ri);
                    }
                }
            } else {
                if (owner) __builtin_nontemporal_store(yM, (f4v*)((R*)a.Y + yoff));
            }
        }
    }
    if constexpr (NPL > 0) {
        // owner lanes of plane 0: lane j of lane group 0 | 1 holds the sums of quad 0 | 1 of column 8 (t0 + t) + j
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                double v = part[p][t];
                v += __shfl_xor(v, 16);
                if (lane < 8) s[wave][p][8 * (t0 + t) + lane] = v;
            }
        __syncthreads();
        for (int e = threadIdx.x; e < NPL * LN; e += 256) {
            int const p = e / LN, jj = e % LN;
            double const sum = ((s[0][p][jj] + s[1][p][jj]) + s[2][p][jj]) + s[3][p][jj];
            write_record<EPI>(a, chunk, LN, p, jj, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// ---------------------------------------------------------------------------------------------------
// MFMA kernel for 8-row blocks (LM == 8, LN % 8 == 0).  A 16x16 tile would be half empty, so the tile is
// filled with the complex structure instead:   [Re A]             [Re A Re X | Re A Im X]
//                                               [Im A] (16 x 8)  x  [Re X | Im X] (8 x 16)  =  [Im A Re X | Im A Im X]
// i.e. all four real products of one 8x8 complex block product come out of ONE accumulator tile with
// K = 8 -> 2 MFMAs (every flop useful).  The native layouts again are the operand layouts: lane l feeds
// A[c = (l%16)/8][k0 + l/16][(l%16)%8] and X[c = (l%16)/8][k0 + l/16][8 nt + (l%16)%8].
// After the pair loop the tile goes through a wave-private LDS patch and comes back as one complex
// element per lane:  Y = (Q00 - Q11) + i (Q01 + Q10),  lane l <-> element (row l/8, column l%8).
template <typename R, int LM, int LN, int EPI, bool PRE>
__global__ __launch_bounds__(256) void k_spmm_mfma8(SpmmArgs a) {
    if (gate_closed(a)) return;
    static_assert(LM == 4 || LM == 8, "[Re A; Im A] must fit the 16 rows of a tile");
    constexpr int P = LM * LN, NT = (LN + 7) / 8;   // LN = 5, 9, 10: the last tile has 5, 1 or 2 columns, the rest is masked
    constexpr int KS = LM / 4;                       // MFMA k-steps per block product
    constexpr int NPL = EpiPlanes<EPI>::N;
    constexpr bool RAGGED = (LN % 8 != 0);
    using T4 = typename Acc<R>::T;
    __shared__ R tile[4][16][17];                      // one patch per wave, padded rows
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    int const part8 = lc >> 3, j8 = lc & 7;            // X operand: plane and column inside the tile
    int const pa = lc / LM, ia = lc % LM;              // A operand: plane (LM == 4: lanes with pa >= 2 feed zeros) and row
    int const ei = lane >> 3, ej = lane & 7;           // epilogue side: element (ei, ej) of the LM x 8 tile (ei < LM)
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;   // XCD-aware launch order (tfq_plan.cpp)
    uint32_t first, last, col = 0;
    if (a.chunkFirst) { first = a.chunkFirst[chunk]; last = a.chunkFirst[chunk + 1]; col = a.chunkCol[chunk]; }
    else { first = chunk * a.CH; last = min(first + a.CH, a.nY); }

    R sr[NT], si[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { sr[nt] = 0; si[nt] = 0; }
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) if (!RAGGED || nt * 8 + ej < LN) {
            sr[nt] = ((R const*)a.sc)[(size_t(col) * 2 + 0) * LN + nt * 8 + ej];   // (written out: epi_scalar changes the assembly)
            si[nt] = ((R const*)a.sc)[(size_t(col) * 2 + 1) * LN + nt * 8 + ej];
        }
    }
    double part[NPL > 0 ? NPL : 1][NT] = {};

    // (row ranges and index pairs are the same for every lane of a wave: scalar loads from the constant address space -- as plain global
    //  loads the index pair of a product was waited for with s_waitcnt vmcnt(0) right in front of its operand requests, which drained the
    //  DEPTH products "in flight" every time; r04, profiles/r04_four_row_shapes.txt)
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts;
    struct Ops { R a[KS]; R x[KS][NT]; };
    R const* const A0 = (R const*)a.A + (pa & 1) * (LM * LM) + ia;   // + k*LM
    R const* const X0 = (R const*)a.X + part8 * P + j8;              // + k*LN + nt*8
    for (uint32_t y = first + wave; y < last; y += 4) {
        T4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = T4{0, 0, 0, 0};
        uint32_t const q0 = starts[y], q1 = starts[y + 1];
        // the operands of this block's epilogue travel while its products are computed (PRE; TFQMRGPU_EPI_PREFETCH=0: behind them)
        EpiElem<R, EPI, LN == 8> eo[PRE ? NT : 1];
        if constexpr (PRE) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if ((LM == 8 || ei < LM) && (!RAGGED || nt * 8 + ej < LN))
                    eo[nt].load(a, size_t(y) * 2 * P + ei * LN + nt * 8 + ej, P);
        }
        auto fetch = [&](Ops& o, uint32_t q) {
            R const* Ab = A0 + size_t(pairs[2 * size_t(q)]) * 2 * LM * LM;
            R const* Xb = X0 + size_t(pairs[2 * size_t(q) + 1]) * 2 * P;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                int const k = 4 * s + lr;
                o.a[s] = (LM == 8 || pa < 2) ? Ab[k * LM] : R(0);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) o.x[s][nt] = (!RAGGED || nt * 8 + j8 < LN) ? Xb[k * LN + nt * 8] : R(0);
            }
        };
        auto mma = [&](Ops const& o) {
#pragma unroll
            for (int s = 0; s < KS; ++s)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[nt] = Acc<R>::mma(o.a[s], o.x[s][nt], acc[nt]);
        };
        // the block products are tiny (2 MFMAs, 2 KiB of operands): keep DEPTH of them in flight
        constexpr int DEPTH = (NT <= 2) ? 4 : 2;
        Ops o[DEPTH];
        uint32_t const nq = q1 - q0;
#pragma unroll
        for (int dd = 0; dd < DEPTH; ++dd) if (uint32_t(dd) < nq) fetch(o[dd], q0 + dd);
        for (uint32_t base = 0; base < nq; base += DEPTH) {
#pragma unroll
            for (int dd = 0; dd < DEPTH; ++dd) {
                if (base + dd < nq) {
                    mma(o[dd]);
                    if (base + dd + DEPTH < nq) fetch(o[dd], q0 + base + dd + DEPTH);
                }
            }
        }

        uint32_t bq = 0xffffffffu;   // (written out: rhs_block changes the assembly)
        if constexpr (EPI == EPI_RESIDUAL) bq = a.bOfX ? a.bOfX[y] : y;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int r = 0; r < 4; ++r) tile[wave][Acc<R>::row(lane, r)][lc] = acc[nt][r];
            __builtin_amdgcn_wave_barrier();           // LDS operations of one wave complete in order
            int const er = ei % LM;                    // LM == 4: the upper half of the lanes has no element
            R const yr = tile[wave][er][ej] - tile[wave][er + LM][ej + 8];
            R const yi = tile[wave][er][ej + 8] + tile[wave][er + LM][ej];
            int const e = ei * LN + nt * 8 + ej;
            double accp[NPL > 0 ? NPL : 1] = {};
            if ((LM == 8 || ei < LM) && (!RAGGED || nt * 8 + ej < LN)) {   // STREAM for LN == 8: the tile is one contiguous plane
                if constexpr (PRE) epilogue_apply<R, EPI, LN == 8>(a, size_t(y) * 2 * P + e, P, yr, yi, sr[nt], si[nt], eo[nt], bq, e, accp);
                else epilogue<R, EPI, LN == 8>(a, size_t(y) * 2 * P + e, P, yr, yi, sr[nt], si[nt], bq, e, accp);
            }
#pragma unroll
            for (int p = 0; p < NPL; ++p) part[p][nt] += accp[p];
        }
    }

    if constexpr (NPL > 0) {
        // the rows of a column sit 8 lanes apart: add them, then the four waves in order
        __shared__ double s[4][NPL][LN];
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                double v = part[p][nt];
                v += __shfl_xor(v, 8);
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                if (lane < 8 && (!RAGGED || nt * 8 + lane < LN)) s[wave][p][nt * 8 + lane] = v;
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

template <typename R, int LM, int LN, int EPI> struct Ilv8Family {
    static void go(SpmmKernel k, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
        constexpr bool dbl = sizeof(R) == 8;
        constexpr bool canFirst = (EPI == EPI_XPAY_DOT);
        constexpr bool canHash8 = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
        // (column batches: block columns with identical row patterns, multiplied kColBatchMax at a time -- tfq_plan.cpp: colBatch; the launch runs over the first columns' chunks)
        if constexpr (takes_ilv8(dbl, LM, LN)) if (SpmmKernel::ilv8b == k) {
            variant<canHash8>(a.hashV3, [&](auto H) { variant<canFirst>(a.first, [&](auto F) {
                k_spmm_ilv8b<EPI, H, kColBatchMax, F><<<dim3(nWG), dim3(256), 0, s>>>(a); }); });
            return;
        }
        if constexpr (takes_ilv8(dbl, LM, LN)) if (SpmmKernel::ilv8 == k) {
            variant<canHash8>(a.hashV3, [&](auto H) { variant<canFirst>(a.first, [&](auto F) {
                k_spmm_ilv8<EPI, H, F><<<dim3(nWG), dim3(256), 0, s>>>(a); }); });
            return;
        }
        if constexpr (takes_ilv8f(dbl, LM, LN)) if (SpmmKernel::ilv8f == k) {
            variant<canFirst>(a.first, [&](auto F) { k_spmm_ilv8f<LN, EPI, F><<<dim3(nWG), dim3(256), 0, s>>>(a); });
            return;
        }
        if constexpr (takes_ilv8w(dbl, LM, LN)) if (SpmmKernel::ilv8w == k) {
            variant<canFirst>(a.first, [&](auto F) { k_spmm_ilv8w<LN, EPI, F><<<dim3(nWG), dim3(256), 0, s>>>(a); });
            return;
        }
        if constexpr (takes_mfma8(dbl, LM, LN)) if (SpmmKernel::mfma8 == k) {
            constexpr bool pre8 = (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT);
            static int const use_pre8 = lab_switch("TFQMRGPU_EPI_PREFETCH", 1);
            variant<pre8>(use_pre8, [&](auto PRE) { k_spmm_mfma8<R, LM, LN, EPI, PRE><<<dim3(nWG), dim3(256), 0, s>>>(a); });
        }
    }
};

bool spmm_ilv8(SpmmKernel k, bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    return spmm_switch<Ilv8Family>(k, dbl, lm, ln, epi, a, nWG, s);
}

} // namespace tfq
