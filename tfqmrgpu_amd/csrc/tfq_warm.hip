// Warm start (tfqmrgpu_ext.h section 14, tfqmrgpuExt_solveFrom): the three streaming kernels around the untouched tfQMR driver.
//   k_warm_residual   per chunk:        X0 := x ; R := (B under X, or 0) - Y ; records {|r|^2, |b|^2} per right-hand side
//   k_warm_init_col   per block column: the records summed in chunk order -> tau = |r|^2, 1 / |b|^2, then the set-up of every solve
//                                       (tfq_colops.hpp: init_col_scalars, reset_ctl), as k_init_col (tfq_vec.hip) does from B
//   k_warm_update     per chunk:        x := X0 + x
// and for tfqmrgpuExt_refineFrom (section 16) on an 'm' plan, whose refinement then runs on A D = R: k_warm_residual and k_warm_update in double
// on the plan's double side (resolveZ: x, B, element order ilvZ; the chunk tables and the record scratch pz are the plan's own), and
//   k_warm_bn2_col    per block column: the records summed in chunk order -> |b|^2 of the refinement's stopping test
// The driver then solves A D = R from zero with R as its X-shaped right-hand side (DevPlan::R, as the inner solves of the mixed
// precision do) and never learns about X0.  Work groups, chunk span, accesses and the record of a chunk are the vector kernels' own
// (tfq_stream.hpp: Geo, TFQ_CHUNK_SPAN, ldv / stv, ld_b_under_x, chunk_reduce); the chunks of a column are added in chunk order.  No atomics.
#include "tfq_device.hpp"
#include "tfq_vec.hpp"
#include "tfq_colops.hpp"
#include "tfq_stream.hpp"

namespace tfq {
namespace {

// ---- per chunk: X0 := x, R := B - Y, {|r|^2, |b|^2} -------------------------------------------------------------------------------
// one pass: reads x, Y and the B block under each X block (where there is one), writes X0 and R.  Never gated: it runs in front of the solve
// (8 waves per SIMD asked for: without it the record tail's LDS offsets, held in SGPRs, take the float LN = 8 instances to 106 SGPRs and 7 waves)
template <typename R, int LM, int LN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_warm_residual(DevPlan d, void const* Y_, void* X0_, void* R_) {
    using G = Geo<R, LM, LN>;
    __shared__ double s[2 * 256 * G::VEC];
    TFQ_CHUNK_SPAN(G)
    R const* x = (R const*)d.x; R const* Y = (R const*)Y_; R* X0 = (R*)X0_; R* Rv = (R*)R_;
    double acc[2][G::VEC] = {};
    if (t < G::T) for (uint32_t w = t; w < nItems; w += G::T) {
        TFQ_ITEM_OFFSETS(G)
        R xr[G::VEC], xi[G::VEC], yr[G::VEC], yi[G::VEC], br[G::VEC], bi[G::VEC];
        ldv(xr, x + re); ldv(xi, x + im); ldv(yr, Y + re); ldv(yi, Y + im);
        ld_b_under_x<R, G::VEC>(br, bi, d, first + blk, size_t(w - blk * G::IPB) * G::VEC, G::P);
        stv(X0 + re, xr); stv(X0 + im, xi);
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) {
            double const b0 = br[v], b1 = bi[v];
            acc[1][v] = __builtin_fma(b1, b1, __builtin_fma(b0, b0, acc[1][v]));
            br[v] = br[v] - yr[v]; bi[v] = bi[v] - yi[v];          // r = b - A x0, in the plan's precision
            double const r0 = br[v], r1 = bi[v];
            acc[0][v] = __builtin_fma(r1, r1, __builtin_fma(r0, r0, acc[0][v]));
        }
        stv(Rv + re, br); stv(Rv + im, bi);
    }
    // one record {|r|^2 [LN], |b|^2 [LN]} per chunk
    chunk_reduce<LN, G::VEC, G::T, 2>(acc, s, d.pz + size_t(chunk) * 2 * LN, t, d.ilv);
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
    double const r2 = dd[0], b2 = dd[1];
    init_col_scalars<R, LN>(d, col, t, r2, 1. / ((b2 > 0.) ? b2 : r2));
    if (0 == col && 0 == t) reset_ctl(d.ctl, tol, maxIterations, 0);
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
    using G = Geo<R, LM, LN>;
    TFQ_CHUNK_SPAN(G)
    R* x = (R*)d.x; R const* X0 = (R const*)X0_;
    for (uint32_t w = t; w < 2 * nItems; w += 256) {     // both planes, all 256 lanes: nothing here depends on the right-hand side
        size_t const o = base + size_t(w) * G::VEC;
        R a[G::VEC], b[G::VEC];
        ldv(a, X0 + o); ldv(b, x + o);
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) b[v] = (R(0) == b[v]) ? a[v] : a[v] + b[v];
        stv(x + o, b);
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
