// The multiply's launches: the kernel family of a launch (spmm_select), the epilogue of a user-defined operator (k_spmm_direct) and the
// multiply on caller-owned native arrays (tfqmrgpuExt_multiply, k_spmm_n16).  Contract and families: tfq_spmm.hpp.
// (timing-only variants of the kernels -- block products or fetches skipped, stamps, the shader clock under load: results wrong by
//  construction -- live in a copy of their own, scripts/lab/tfq_spmm_probes.hip, built with scripts/build_variant.sh; nothing of them is in the product sources)
#include "tfq_spmm.hpp"

namespace tfq {

// ---------------------------------------------------------------------------------------------------
// one thread per output element
template <typename R, int LM, int LN, int EPI>
__global__ __launch_bounds__(256) void k_spmm_direct(SpmmArgs a) {
    if (gate_closed(a)) return;
    constexpr int P = LM * LN;                       // elements per plane
    constexpr int NACC = (P >= 256) ? P / 256 : 1;   // outputs per thread
    constexpr int GRP = (P >= 256) ? 1 : 256 / P;    // Y blocks in flight per work group
    constexpr int NPL = EpiPlanes<EPI>::N;
    static_assert(P < 256 || P % 256 == 0, "block does not tile the work group");
    int const t = threadIdx.x;
    int const g = (P >= 256) ? 0 : t / P;
    int const e0 = (P >= 256) ? t : t % P;
    bool const active = (g < GRP);
    uint32_t const chunk = a.order ? a.order[blockIdx.x] : blockIdx.x;   // XCD-aware launch order (tfq_plan.cpp)
    uint32_t first, last, col = 0;
    if (a.chunkFirst) { first = a.chunkFirst[chunk]; last = a.chunkFirst[chunk + 1]; col = a.chunkCol[chunk]; }
    else { first = chunk * a.CH; last = min(first + a.CH, a.nY); }

    int const j = e0 % LN;                           // 256 % LN == 0 whenever NACC > 1
    R sr = 0, si = 0;
    if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
        sr = epi_scalar<R>(a, col, LN, 0, j);
        si = epi_scalar<R>(a, col, LN, 1, j);
    }
    double part[NPL > 0 ? NPL : 1] = {};

    if (active) for (uint32_t y = first + g; y < last; y += GRP) {
        R yr[NACC], yi[NACC];
#pragma unroll
        for (int n = 0; n < NACC; ++n) { yr[n] = 0; yi[n] = 0; }
        if (a.Yext) {   // product computed by a user-defined operator
            R const* Yb = (R const*)a.Yext + size_t(a.yPerm[y]) * 2 * P;
#pragma unroll
            for (int n = 0; n < NACC; ++n) { yr[n] = Yb[e0 + n * 256]; yi[n] = Yb[P + e0 + n * 256]; }
        } else
        for (uint32_t q = a.starts[y]; q < a.starts[y + 1]; ++q) {
            R const* Ab = (R const*)a.A + size_t(a.pairs[2 * size_t(q)]) * 2 * LM * LM;
            R const* Xb = (R const*)a.X + size_t(a.pairs[2 * size_t(q) + 1]) * 2 * P;
#pragma unroll
            for (int n = 0; n < NACC; ++n) {
                int const e = e0 + n * 256, i = e / LN;
                R cr = 0, ci = 0;
#pragma unroll 4
                for (int k = 0; k < LM; ++k) {
                    R const ar = Ab[k * LM + i], ai = Ab[LM * LM + k * LM + i];
                    R const xr = Xb[k * LN + j], xi = Xb[P + k * LN + j];
                    cr = fma_(-ai, xi, fma_(ar, xr, cr));
                    ci = fma_(ai, xr, fma_(ar, xi, ci));
                }
                yr[n] += cr; yi[n] += ci;
            }
        }
        uint32_t const bq = rhs_block<EPI>(a, y);
#pragma unroll
        for (int n = 0; n < NACC; ++n) {
            int const e = e0 + n * 256;
            int const el = plane_offset(a.ilv, e / LN, e % LN, LN);      // where the plan keeps element (row, column)
            epilogue<R, EPI>(a, size_t(y) * 2 * P + el, P, yr[n], yi[n], sr, si, bq, el, part);
        }
    }

    if constexpr (NPL > 0) {
        // threads that share j: rank = position among them; sum in rank order
        constexpr int RANKS = (P >= 256) ? 256 / LN : GRP * LM;
        __shared__ double s[NPL * LN * RANKS];
        int const rank = (P >= 256) ? t / LN : g * LM + e0 / LN;
        if (active)
#pragma unroll
            for (int p = 0; p < NPL; ++p) s[(p * LN + j) * RANKS + rank] = part[p];
        __syncthreads();
        for (int e = t; e < NPL * LN; e += 256) {
            double sum = 0;
#pragma unroll 1
            for (int r = 0; r < RANKS; ++r) sum += s[e * RANKS + r];
            write_record<EPI>(a, chunk, LN, e / LN, e % LN, sum);
        }
        if (a.foldPlan) spmm_fold<R, LN, EPI>(a, col);   // small systems: the column operation behind this multiply, in the last work group of the column
    }
}

// (an epilogue launch: no multiply of TFQ_SIZES takes k_spmm_direct)
template <typename R, int LM, int LN, int EPI> struct DirectEpilogue {
    static void go(SpmmKernel, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
        if constexpr (EPI != EPI_NONE) k_spmm_direct<R, LM, LN, EPI><<<dim3(nWG), dim3(256), 0, s>>>(a);
    }
};

// ---------------------------------------------------------------------------------------------------
// The kernel family of a launch: the first whose shapes (tfq_spmm.hpp: takes_*) and conditions fit.  The lab switches that steer it:
// TFQMRGPU_S4W (s4w_columns) and TFQMRGPU_M4=0 (the kernels these shapes had before k_spmm_m4: k_spmm_small4 and k_spmm_mfma8).
// The variants inside a family (first iteration, hash, streamed A, prefetch, three products, clamp, columns per lane) are its launcher's.
static SpmmKernel spmm_select(bool dbl, int lm, int ln, int epi, SpmmArgs const& a) {
    static int const use_m4 = lab_switch("TFQMRGPU_M4", 1);
    bool const pairs = a.ilv && a.chunkFirst;          // the plan keeps its blocks interleaved (tfq_plan.cpp: layoutBuffer); never the plain mode
    bool const quads = 4 == a.ilv && a.chunkFirst;     // ... in groups of four rows
    if (takes_s4w(dbl, lm, ln) && s4w_columns(ln, epi)) return SpmmKernel::s4w;
    if (takes_m4(dbl, lm, ln) && use_m4) return SpmmKernel::m4;
    if (takes_ilv16(dbl, lm, ln) && pairs) return SpmmKernel::ilv16;
    if (takes_ilv16f(dbl, lm, ln) && quads) return SpmmKernel::ilv16f;
    if (takes_ilvf(dbl, lm, ln) && quads) return SpmmKernel::ilvf;
    if (takes_ilv8(dbl, lm, ln) && pairs) return a.colBatch ? SpmmKernel::ilv8b : SpmmKernel::ilv8;
    if (takes_ilv8f(dbl, lm, ln) && quads) return SpmmKernel::ilv8f;
    if (takes_ilv8w(dbl, lm, ln) && pairs) return SpmmKernel::ilv8w;
    if (takes_mfma(dbl, lm, ln)) return SpmmKernel::mfma;
    if (takes_mfma8(dbl, lm, ln)) return SpmmKernel::mfma8;
    if (takes_small4(dbl, lm, ln)) return SpmmKernel::small4;
    return SpmmKernel::direct;
}

// the multiply: the selected family through the launcher of its file; false: the shape is not one of TFQ_SIZES
static bool spmm_go(bool dbl, int lm, int ln, int epi, SpmmArgs const& a, uint32_t nWG, hipStream_t s) {
    SpmmKernel const k = spmm_select(dbl, lm, ln, epi, a);
    switch (k) {
    case SpmmKernel::mfma:
        return spmm_mfma(k, dbl, lm, ln, epi, a, nWG, s);
    case SpmmKernel::ilv16: case SpmmKernel::ilv16f: case SpmmKernel::ilvf:
        return spmm_ilv16(k, dbl, lm, ln, epi, a, nWG, s);
    case SpmmKernel::ilv8b: case SpmmKernel::ilv8: case SpmmKernel::ilv8f: case SpmmKernel::ilv8w: case SpmmKernel::mfma8:
        return spmm_ilv8(k, dbl, lm, ln, epi, a, nWG, s);
    case SpmmKernel::s4w: case SpmmKernel::m4: case SpmmKernel::small4:
        return spmm_rows4(k, dbl, lm, ln, epi, a, nWG, s);
    case SpmmKernel::direct:   // (only shapes outside TFQ_SIZES)
        break;
    }
    return false;
}

static SpmmArgs spmm_args(int epi, DevPlan const& d) {
    SpmmArgs a{};
    a.A = d.A; a.starts = d.starts; a.pairs = d.pairs; a.nY = d.nnzbX;
    a.chunkFirst = d.chunkFirst; a.chunkCol = d.chunkCol; a.CH = 0;
    a.order = d.order;
    a.ctl = d.ctl; a.v3 = d.v3; a.B = d.R ? d.R : d.B; a.bOfX = d.R ? nullptr : d.bOfX; a.pz = d.pz; a.pd = d.pd;
    a.m3 = d.m3;
    a.foldPlan = d.fold ? d.self : nullptr;
    a.hashV3 = d.hashV3; a.origCol = d.origCol; a.rowI = d.rowI; a.ilv = d.ilv; a.aOnce = d.aOnce;
    a.colBatch = d.colBatch; a.colStart = d.colStart; a.colChunkPtr = d.colChunkPtr;
    switch (epi) {
    case EPI_XPAY_DOT:     a.X = d.v6; a.Y = d.v9; a.e0 = d.v4; a.e1 = d.v8; a.sc = d.beta; a.gate = 1; a.first = d.first; break;
    case EPI_AXPY_NRM_DOT: a.X = d.v6; a.Y = d.v8; a.e0 = d.v5; a.sc = d.alfa; a.gate = 1;
                           if (d.lateV5) { a.late = 1; a.e2 = d.v9; a.first = d.first; } break;   // (late_v5 grants the flag to plans on k_spmm_ilv16 alone)
    case EPI_RESIDUAL:     a.X = d.x;  a.Y = nullptr; a.gate = 2; break;
    default: break;
    }
    // column batches: one work group per chunk of a batch's FIRST column, in an order of its own
    if (d.colBatch && !d.fold) a.order = d.orderB; else a.colBatch = nullptr;
    return a;
}
static uint32_t work_groups(DevPlan const& d) { return (d.colBatch && !d.fold) ? d.nChunksB : d.nChunks; }

// the kernel family that spmm_launch picks for this plan
char const* spmm_kernel_family(DevPlan const& d) {
    static char const* const names[] = { "k_spmm_s4w", "k_spmm_m4", "k_spmm_ilv16", "k_spmm_ilv16f", "k_spmm_ilvf", "k_spmm_ilv8b", "k_spmm_ilv8",
                                         "k_spmm_ilv8f", "k_spmm_ilv8w", "k_spmm_mfma", "k_spmm_mfma8", "k_spmm_small4", "k_spmm_direct" };
    static_assert(sizeof(names) / sizeof(names[0]) == int(SpmmKernel::direct) + 1, "a name per family");
    return names[int(spmm_select(d.dbl, d.LM, d.LN, EPI_XPAY_DOT, spmm_args(EPI_XPAY_DOT, d)))];
}

// the multiply's side of the "late v5" slot (tfq_solve.hpp: late_v5): the second fused multiply of this plan runs on k_spmm_ilv16, the one kernel
// whose epilogue takes the pending half step.  Lab builds: TFQMRGPU_LATE_V5=0 keeps the slot in which k_v5_nrm stores v5
bool spmm_late_v5(DevPlan const& d) {
    static int const lateEnv = lab_switch("TFQMRGPU_LATE_V5", 1);
    return lateEnv && SpmmKernel::ilv16 == spmm_select(d.dbl, d.LM, d.LN, EPI_AXPY_NRM_DOT, spmm_args(EPI_AXPY_NRM_DOT, d));
}

void spmm_launch(int epi, DevPlan const& d, hipStream_t s) {
    if (epi != EPI_XPAY_DOT && epi != EPI_AXPY_NRM_DOT && epi != EPI_RESIDUAL) return;
    spmm_go(d.dbl, d.LM, d.LN, epi, spmm_args(epi, d), work_groups(d), s);
}

// Y = A * X on vectors of the plan (both in the plan's own block and element order), no epilogue, never gated
void spmm_apply(DevPlan const& d, void const* X, void* Y, hipStream_t s) {
    SpmmArgs a = spmm_args(EPI_NONE, d);
    a.X = X; a.Y = Y; a.gate = 0;
    spmm_go(d.dbl, d.LM, d.LN, EPI_NONE, a, work_groups(d), s);
}

void epilogue_launch(int epi, DevPlan const& d, void const* Yext, uint32_t const* i2u, hipStream_t s) {
    SpmmArgs a = spmm_args(epi, d);
    a.order = nullptr; a.Yext = Yext; a.yPerm = i2u;
    spmm_switch<DirectEpilogue>(SpmmKernel::direct, d.dbl, d.LM, d.LN, epi, a, d.nChunks, s);
}

// ---------------------------------------------------------------------------------------------------
// 16 x 16 blocks on the CALLER's native planes (tfqmrgpuExt_multiply: the shape of the reference's `bench multi`, whose default precision is float).  In the native order a lane
// of v_mfma_*_16x16x4 finds its operand element A[k][i] | X[k][j] 4 | 8 bytes at a time (k_spmm_mfma: 16 wave-wide loads of 256 | 512 bytes per block product, the
// memory pipe's rate -- 0.28 | 0.45 of the matrix peak on the reference's plan file).  Here a wave fetches the four planes of a product as four 16-byte-per-lane accesses
// (1 KiB each), passes them through a wave-private LDS patch and reads its operand elements from there (conflict-free: 64 consecutive floats per read).  The
// k-steps and the order of the four real products are k_spmm_mfma's: bit-identical results.  The Y block leaves through the same patch as two 1-KiB stores.
template <typename R>
__global__ __launch_bounds__(256) void k_spmm_n16(SpmmArgs a) {
    constexpr int P = 256;
    constexpr int VE = 16 / sizeof(R);               // elements of a 16-byte access: 4 | 2
    constexpr int NV = P / (64 * VE);                // accesses per lane and plane: 1 | 2
    using V = R __attribute__((ext_vector_type(VE)));
    using T4 = typename Acc<R>::T;
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const lr = lane >> 4, lc = lane & 15;
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    CU32 const pairs = (CU32)(uintptr_t)a.pairs; CU32 const starts = (CU32)(uintptr_t)a.starts; CU32 const yOrder = (CU32)(uintptr_t)a.yOrder;
    __shared__ __attribute__((aligned(16))) R patch[4][4 * P];   // per wave: A re | A im | X re | X im
    R* const my = patch[wave];
    uint32_t const chunk = a.plainPer ? (blockIdx.x & 7u) * a.plainPer + (blockIdx.x >> 3) : blockIdx.x;
    uint32_t const pos = chunk * 4 + uint32_t(wave);              // (no barrier below: a wave without a Y block just leaves)
    if (pos >= a.nY) return;
    uint32_t const y = a.yOrder ? yOrder[pos] : pos;             // (a prepared order: which Y block this position computes)
    uint32_t const q0 = starts[y], q1 = starts[y + 1];
    T4 cre = T4{0, 0, 0, 0}, cim = T4{0, 0, 0, 0};
    struct Ops { V v[4][NV]; };                      // [A re | A im | X re | X im][piece]: piece n of a plane = elements 64 VE n + VE lane ...
    auto fetch = [&](Ops& o, uint32_t q) __attribute__((always_inline)) {
        R const* Ab = (R const*)a.A + size_t(pairs[2 * size_t(q)]) * 2 * P + VE * lane;
        R const* Xb = (R const*)a.X + size_t(pairs[2 * size_t(q) + 1]) * 2 * P + VE * lane;
#pragma unroll
        for (int n = 0; n < NV; ++n) {
            o.v[0][n] = *(V const*)(Ab + 64 * VE * n); o.v[1][n] = *(V const*)(Ab + P + 64 * VE * n);
            o.v[2][n] = *(V const*)(Xb + 64 * VE * n); o.v[3][n] = *(V const*)(Xb + P + 64 * VE * n);
        }
    };
    auto mma = [&](Ops const& o) __attribute__((always_inline)) {
        __builtin_amdgcn_wave_barrier();             // LDS operations of one wave complete in order: the patch is free when these writes execute
#pragma unroll
        for (int pl = 0; pl < 4; ++pl)
#pragma unroll
            for (int n = 0; n < NV; ++n) *(V*)(my + pl * P + 64 * VE * n + VE * lane) = o.v[pl][n];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s = 0; s < 4; ++s) {                // k = 4 s + lr: lane (lr, lc) feeds A[k][i = lc] and X[k][j = lc]
            int const e = (4 * s + lr) * 16 + lc;
            R const ar = my[e], ai = my[P + e], xr = my[2 * P + e], xi = my[3 * P + e];
            cre = Acc<R>::mma(ar, xr, cre);
            cim = Acc<R>::mma(ar, xi, cim);
            cre = Acc<R>::mma(-ai, xi, cre);
            cim = Acc<R>::mma(ai, xr, cim);
        }
    };
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
    // the accumulator registers of a lane are rows Acc<R>::row(lane, r) of column lc: through the patch into 16 bytes per lane
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 4; ++r) { my[Acc<R>::row(lane, r) * 16 + lc] = cre[r]; my[P + Acc<R>::row(lane, r) * 16 + lc] = cim[r]; }
    __builtin_amdgcn_wave_barrier();
    R* const Yb = (R*)a.Y + size_t(y) * 2 * P + VE * lane;
#pragma unroll
    for (int n = 0; n < NV; ++n) {
        *(V*)(Yb + 64 * VE * n) = *(V const*)(my + 64 * VE * n + VE * lane);
        *(V*)(Yb + P + 64 * VE * n) = *(V const*)(my + P + 64 * VE * n + VE * lane);
    }
}

static MulPrec multiply_precision(char precision) {
    char const p = char(precision | 32);
    return ('z' == p || 'd' == p) ? MulPrec::z : ('m' == p) ? MulPrec::m : MulPrec::c;
}

// The kernel family of a stand-alone multiply (tfqmrgpuExt_multiply), the counterpart of spmm_select for plans and the one place that
// decides which shapes the product takes in which precision.  plan: the family spmm_select picks (k_spmm_mfma, k_spmm_mfma8, k_spmm_s4w,
// k_spmm_m4, k_spmm_small4 on the solver's shapes); wide: k_spmm_mfma on TFQ_MULTIPLY_SIZES; mfma_m: k_spmm_mfma_m (`m`, multiples of 16);
// pad: k_spmm_pad (TFQ_PAD_SIZES; in `m` also the 4- and 8-row shapes).
enum class MulKernel { missing, n16, plan, wide, mfma_m, pad };
static MulKernel multiply_select(MulPrec p, int lm, int ln) {
    bool const mfma = (lm % 16 == 0 && ln % 16 == 0);
    bool const solver = solver_shape(lm, ln), wide = wide_shape(lm, ln);
    if (pad_shape(lm, ln)) return MulKernel::pad;
    if (MulPrec::m == p) return !(solver || wide) ? MulKernel::missing : mfma ? MulKernel::mfma_m : MulKernel::pad;
    if (wide) return MulKernel::wide;
    if (!solver) return MulKernel::missing;
    // float: the reference's plan file 44.3 -> 59.2 TFLOP/s (0.28 -> 0.38 of the matrix peak), a 16 x 16 c stencil 0.360 -> 0.249 ms (0.55); double: the LDS traffic doubles with the
    // element size and the plan file LOSES 7 % (35.3 -> 32.9), P2 gains 3 %: float only (lab: TFQMRGPU_N16 bit 0 = float, bit 1 = double; profiles/r04_native_multiply.txt)
    if (16 == lm && 16 == ln && (lab_switch("TFQMRGPU_N16", 1) & ((MulPrec::z == p) ? 2 : 1))) return MulKernel::n16;
    return MulKernel::plan;
}

bool multiply_shape_allowed(char precision, int lm, int ln) {
    return MulKernel::missing != multiply_select(multiply_precision(precision), lm, ln);
}

// Y blocks per work group of the stand-alone multiply in plain mode (SpmmArgs::CH), for every family but k_spmm_pad (its own work groups:
// one Y block per wave): enough work groups to fill 256 CUs several times, at least one unit of work per wave
static uint32_t multiply_chunk(MulPrec p, int lm, int ln) {
    int const mu = mfma_units(lm, ln, (MulPrec::c == p) ? 4 : 8);   // strips per Y block
    if (lm % 16 == 0 && ln % 16 == 0) return uint32_t((mu >= 4) ? 1 : 4 / mu);   // k_spmm_mfma | k_spmm_mfma_m | k_spmm_n16: one strip per wave
    if (8 == lm) return 4;                                  // k_spmm_mfma8 (kTile8): one Y block per wave and pass
    if (MulPrec::z == p && 32 == ln) return 16;             // 4 x 32 z, k_spmm_m4: 64 items, four per Y block (and the tile kernel's 16 before it)
    return 64;                                              // the other 4-row shapes (k_spmm_small4: a few sub-blocks per thread group)
}

uint32_t multiply_blocks_per_work_group(char precision, int lm, int ln) {   // (a prepared order is honoured by k_spmm_mfma | k_spmm_mfma_m | k_spmm_n16 only)
    return (lm % 16 || ln % 16) ? 0 : multiply_chunk(multiply_precision(precision), lm, ln);
}

tfqmrgpuStatus_t launch_multiply(char precision, int lm, int ln, uint32_t nnzbY,
    uint32_t const* starts, uint32_t const* pairs, void const* A, void const* X, void* Y, hipStream_t s, uint32_t const* yOrder)
{
    MulPrec const prec = multiply_precision(precision);
    MulKernel const k = multiply_select(prec, lm, ln);
    if (MulKernel::missing == k) return err(TFQMRGPU_BLOCKSIZE_MISSING, ln, lm);
    bool const dbl = (MulPrec::z == prec);
    SpmmArgs a{};
    a.Y = Y; a.A = A; a.X = X; a.starts = starts; a.pairs = pairs; a.nY = nnzbY;
    a.chunkFirst = nullptr; a.gate = 0;
    bool const mfma = (lm % 16 == 0 && ln % 16 == 0);
    a.yOrder = mfma ? yOrder : nullptr;
    bool ok = true;
    if (MulKernel::pad == k) ok = spmm_pad(prec, lm, ln, a, s);      // (its own work groups: one Y block per wave)
    else {
        uint32_t const ch = a.CH = multiply_chunk(prec, lm, ln);
        uint32_t nWG = (nnzbY + ch - 1) / ch;
        // (lab: contiguous eighths of the caller's Y blocks per XCD instead of round-robin work groups)
        if (mfma && nWG >= 64 && lab_switch("TFQMRGPU_PLAIN_XCD", 0)) { a.plainPer = (nWG + 7) / 8; nWG = 8 * a.plainPer; }
        switch (k) {
        case MulKernel::n16:
            if (nWG) { if (dbl) k_spmm_n16<double><<<dim3(nWG), dim3(256), 0, s>>>(a); else k_spmm_n16<float><<<dim3(nWG), dim3(256), 0, s>>>(a); }
            break;
        case MulKernel::mfma_m: ok = spmm_mfma_m(lm, ln, a, nWG, s); break;     // float data, double sums
        case MulKernel::wide:   ok = spmm_mfma_wide(dbl, lm, ln, a, nWG, s); break;
        default:                ok = spmm_go(dbl, lm, ln, EPI_NONE, a, nWG, s); break;
        }
    }
    if (!ok) return err(TFQMRGPU_BLOCKSIZE_MISSING, ln, lm);
    return (hipSuccess == hipGetLastError()) ? TFQMRGPU_STATUS_SUCCESS : TFQ_ERR(TFQMRGPU_STATUS_LAUNCH_FAILED);
}

} // namespace tfq
