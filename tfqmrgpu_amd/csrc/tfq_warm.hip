// Warm start (tfqmrgpu_ext.h section 14, tfqmrgpuExt_solveFrom): the three streaming kernels around the untouched tfQMR driver.
//   k_warm_residual   per chunk:        X0 := x ; R := (B under X, or 0) - Y ; records {|r|^2, |b|^2} per right-hand side
//   k_warm_init_col   per block column: the records summed in chunk order -> tau = |r|^2, 1 / |b|^2, rho = 1, everything else 0, the
//                                       fold counters and the control block: what k_init_col (tfq_vec.hip) does from B
//   k_warm_update     per chunk:        x := X0 + x
// and for tfqmrgpuExt_refineFrom (section 16) on an 'm' plan, whose refinement then runs on A D = R: k_warm_residual and k_warm_update in double
// on the plan's double side (resolveZ: x, B, element order ilvZ; the chunk tables and the record scratch pz are the plan's own), and
//   k_warm_bn2_col    per block column: the records summed in chunk order -> |b|^2 of the refinement's stopping test
// The driver then solves A D = R from zero with R as its X-shaped right-hand side (DevPlan::R, as the inner solves of the mixed
// precision do) and never learns about X0.  Work groups, chunk tables, element order and access width are those of the vector kernels
// (tfq_vec.hip): one work group per chunk, every lane moves 16 bytes per access and keeps its right-hand side on every trip, one [LN]
// record per chunk in a fixed order, the chunks of a column added in chunk order.  No atomics.
#include "tfq_device.hpp"
#include "tfq_vec.hpp"
#include "tfq_colops.hpp"
#include "tfq_stream.hpp"

namespace tfq {
namespace {

// geometry, 16-byte accesses and the ordered sum: tfq_stream.hpp (WGeo, w_ld, w_st, w_ordered_sum)

// ---- per chunk: X0 := x, R := B - Y, {|r|^2, |b|^2} -------------------------------------------------------------------------------
// one pass: reads x, Y and the B block under each X block (where there is one), writes X0 and R.  Never gated: it runs in front of the solve
template <typename R, int LM, int LN>
__global__ __launch_bounds__(256) void k_warm_residual(DevPlan d, void const* Y_, void* X0_, void* R_) {
    using G = WGeo<R, LM, LN>;
    __shared__ double s[2 * 256 * G::VEC];
    int const t = threadIdx.x;
    uint32_t const chunk = blockIdx.x;
    uint32_t const first = d.chunkFirst[chunk];
    uint32_t const nItems = (d.chunkFirst[chunk + 1] - first) * G::IPB;
    size_t const base = size_t(first) * 2 * G::P;
    R const* x = (R const*)d.x; R const* Y = (R const*)Y_; R* X0 = (R*)X0_; R* Rv = (R*)R_;
    double acc[2][G::VEC] = {};
    if (t < G::T) for (uint32_t w = t; w < nItems; w += G::T) {
        uint32_t const blk = w / G::IPB;
        size_t const inner = size_t(w - blk * G::IPB) * G::VEC;
        size_t const re = base + size_t(blk) * 2 * G::P + inner, im = re + G::P;
        R xr[G::VEC], xi[G::VEC], yr[G::VEC], yi[G::VEC], br[G::VEC], bi[G::VEC];
        w_ld(xr, x + re); w_ld(xi, x + im); w_ld(yr, Y + re); w_ld(yi, Y + im);
        uint32_t const bq = d.bOfX[first + blk];
        if (0xffffffffu == bq) {
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) { br[v] = 0; bi[v] = 0; }
        } else {
            R const* b = (R const*)d.B + size_t(bq) * 2 * G::P + inner;
            w_ld(br, b); w_ld(bi, b + G::P);
        }
        w_st(X0 + re, xr); w_st(X0 + im, xi);
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) {
            double const b0 = br[v], b1 = bi[v];
            acc[1][v] = __builtin_fma(b1, b1, __builtin_fma(b0, b0, acc[1][v]));
            br[v] = br[v] - yr[v]; bi[v] = bi[v] - yi[v];          // r = b - A x0, in the plan's precision
            double const r0 = br[v], r1 = bi[v];
            acc[0][v] = __builtin_fma(r1, r1, __builtin_fma(r0, r0, acc[0][v]));
        }
        w_st(Rv + re, br); w_st(Rv + im, bi);
    }
    // one record {|r|^2 [LN], |b|^2 [LN]} per chunk, the terms of a right-hand side added in one fixed order
    if (t < G::T) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) s[p * (256 * G::VEC) + t * G::VEC + v] = acc[p][v];
    }
    __syncthreads();
    double* const out = d.pz + size_t(chunk) * 2 * LN;
    for (int e = t; e < 2 * LN; e += 256) {
        int const p = e / LN, j = e % LN;
        double const* sp = s + p * (256 * G::VEC);
        out[e] = (2 == d.ilv) ? w_ordered_sum<LN, G::VEC, G::T, 2>(sp, j) : (4 == d.ilv) ? w_ordered_sum<LN, G::VEC, G::T, 4>(sp, j)
                                                                                         : w_ordered_sum<LN, G::VEC, G::T, 0>(sp, j);
    }
}

// the control block at the start of a solve: what reset_ctl of tfq_vec.hip writes, with no stallStop
__device__ inline void w_reset_ctl(Ctl* c, double tol, int maxIterations) {
    double const tol2 = tol * tol;
    c->tol2 = tol2; c->target_bound2 = tol2 * 100 * 100; c->max_bound2 = 0; c->residual2_reached = 1e300; c->probe_bound2 = 0;
    for (int i = 0; i < 6; ++i) c->red[i] = 0;
    c->iteration = 0; c->maxIterations = maxIterations;
    c->state = (maxIterations > 0) ? 0 : 3;
    c->probe = 0; c->iterations_needed = maxIterations; c->nprobes = 0; c->xpend = 0; c->stallStop = 0;
}

// ---- per block column: the set-up of the correction solve -----------------------------------------------------------------------------
// tau = |r|^2 and 1 / |b|^2: the bound of decT and the residual of the probe are tau / |b|^2 and |R - A D|^2 / |b|^2 = |B - A (X0 + D)|^2 / |b|^2, so
// `threshold` and getInfo stay relative to B.  A right-hand side with b = 0 has nothing to be relative to: it is graded against its r, as a cold
// solve of the correction system would.  r = 0 gives tau = 0, which the column operations treat as they treat a zero column of B today.
template <typename R, int LN>
__global__ __launch_bounds__(256) void k_warm_init_col(DevPlan d, double tol, int maxIterations) {
    __shared__ double s[512];
    uint32_t const col = blockIdx.x;
    int const t = threadIdx.x;
    double dd[2];
    column_sum<LN, 2>(d.pz, d.colChunkPtr[col], d.colChunkPtr[col + 1], s, dd);
    if (t < LN) {
        double const r2 = dd[0], b2 = dd[1];
        size_t const ir = (size_t(col) * 2 + 0) * LN + t, ii = ir + LN, i1 = size_t(col) * LN + t;
        d.tau[i1] = r2; d.invBn2[i1] = 1. / ((b2 > 0.) ? b2 : r2); d.var[i1] = 0; d.d[i1] = 0; d.status[i1] = 0;
        ((R*)d.rho)[ir] = 1; ((R*)d.rho)[ii] = 0;
        ((R*)d.alfa)[ir] = 0; ((R*)d.alfa)[ii] = 0; ((R*)d.beta)[ir] = 0; ((R*)d.beta)[ii] = 0;
        ((R*)d.c67)[ir] = 0; ((R*)d.c67)[ii] = 0; ((R*)d.eta)[ir] = 0; ((R*)d.eta)[ii] = 0;
        ((R*)d.c67a)[ir] = 0; ((R*)d.c67a)[ii] = 0; ((R*)d.eta2)[ir] = 0; ((R*)d.eta2)[ii] = 0;
    }
    if (0 == t) {   // the arrival counters of the folded column operations start every solve at zero
        d.foldCount[col] = 0;
        if (0 == col) d.foldCount[d.nCols] = 0;
    }
    if (0 == col && 0 == t) w_reset_ctl(d.ctl, tol, maxIterations);
}

// ---- per block column, 'm' plans (tfqmrgpu_ext.h section 16): |b|^2 of the refinement -------------------------------------------------------------
// The records of k_warm_residual<double> on the plan's double side, summed in chunk order -> bn2z = |b|^2, or |r0|^2 where b = 0 (graded against
// its own r0, as above).  Cycle 0 of a cold refinement takes its |r|^2 for this (k_refine_init_col, tfq_vec.hip), which here would be |r0|^2
// for every right-hand side.  The scalars of the float solves stay with k_refine_init_col, which also forms the first residual |r0|^2 / bn2z
template <int LN>
__global__ __launch_bounds__(256) void k_warm_bn2_col(DevPlan d, double* bn2z) {
    __shared__ double s[512];
    uint32_t const col = blockIdx.x;
    int const t = threadIdx.x;
    double dd[2];
    column_sum<LN, 2>(d.pz, d.colChunkPtr[col], d.colChunkPtr[col + 1], s, dd);
    if (t < LN) bn2z[size_t(col) * LN + t] = (dd[1] > 0.) ? dd[1] : dd[0];
}

// ---- per chunk: x := X0 + x ------------------------------------------------------------------------------------------------------------
// a correction that is exactly zero leaves X0 as it is, bit for bit (-0.0 + 0.0 would be +0.0)
template <typename R, int LM, int LN>
__global__ __launch_bounds__(256) void k_warm_update(DevPlan d, void const* X0_) {
    using G = WGeo<R, LM, LN>;
    uint32_t const chunk = blockIdx.x;
    uint32_t const first = d.chunkFirst[chunk];
    uint32_t const nItems = (d.chunkFirst[chunk + 1] - first) * 2 * G::IPB;     // both planes: nothing here depends on the right-hand side
    size_t const base = size_t(first) * 2 * G::P;
    R* x = (R*)d.x; R const* X0 = (R const*)X0_;
    for (uint32_t w = threadIdx.x; w < nItems; w += 256) {
        size_t const o = base + size_t(w) * G::VEC;
        R a[G::VEC], b[G::VEC];
        w_ld(a, X0 + o); w_ld(b, x + o);
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) b[v] = (R(0) == b[v]) ? a[v] : a[v] + b[v];
        w_st(x + o, b);
    }
}

// what: 0 the residual pass and the set-up of the correction solve, 1 the update, 2 the residual pass and |b|^2 of an 'm' plan's refinement (bn2z)
template <typename R, int LM, int LN>
void warm_run(int what, DevPlan const& d, void const* Y, void* X0, void* Rv, double* bn2z, double tol, int maxIt, hipStream_t s) {
    dim3 const grid(d.nChunks), cols(d.nCols), blk(256);
    if (0 == what) {
        k_warm_residual<R, LM, LN><<<grid, blk, 0, s>>>(d, Y, X0, Rv);
        k_warm_init_col<R, LN><<<cols, blk, 0, s>>>(d, tol, maxIt);
    } else if (2 == what) {
        k_warm_residual<R, LM, LN><<<grid, blk, 0, s>>>(d, Y, X0, Rv);
        k_warm_bn2_col<LN><<<cols, blk, 0, s>>>(d, bn2z);
    } else k_warm_update<R, LM, LN><<<grid, blk, 0, s>>>(d, X0);
}

bool warm_dispatch(int what, DevPlan const& d, void const* Y, void* X0, void* Rv, double* bn2z, double tol, int maxIt, hipStream_t s) {
    // false: a missing instance is an error, never a fall-back
    return for_shape(d.dbl, d.LM, d.LN, [&](auto sh) { using S = decltype(sh); warm_run<typename S::real, S::LM, S::LN>(what, d, Y, X0, Rv, bn2z, tol, maxIt, s); });
}

} // namespace

bool warm_residual_launch(DevPlan const& d, void const* Y, void* X0, void* R, double tol, int maxIt, hipStream_t s) {
    return warm_dispatch(0, d, Y, X0, R, nullptr, tol, maxIt, s);
}
bool warm_update_launch(DevPlan const& d, void const* X0, hipStream_t s) {
    return warm_dispatch(1, d, nullptr, const_cast<void*>(X0), nullptr, nullptr, 0., 0, s);
}
bool warm_refine_residual_launch(DevPlan const& dz, void const* Y, void* X0, void* R, double* bn2z, hipStream_t s) {
    if (!dz.dbl || !bn2z) return false;     // the double side of an 'm' plan (resolveZ) and nothing else
    return warm_dispatch(2, dz, Y, X0, R, bn2z, 0., 0, s);
}

} // namespace tfq
