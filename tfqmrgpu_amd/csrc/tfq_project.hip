// Start projection (tfqmrgpu_ext.h section 17, tfqmrgpuExt_projectStart): the kept starts S_0 ... S_{K-1} and their images W_i = A S_i
// (the plan's own multiply, tfq_project_host.cpp) -> per (block column, right-hand side) the combination x = sum gamma_i S_i that
// minimises |B - sum gamma_i W_i|.
//   k_project_gram       per chunk:        one record of K^2 + 2K + 1 doubles per right-hand side: G_ii, Re/Im of G_il (i < l), Re/Im of g_i = <W_i, B>, |B|^2
//   k_project_solve_col  per block column: the records summed in chunk order; one lane per right-hand side runs the Cholesky factorisation of G in
//                                          the order of the starts, drops a start whose pivot is too small, writes gamma and the number of kept starts
//   k_project_combine    per chunk:        x := sum gamma_i S_i, accumulated in double in slot order, rounded once to the storage type
// Work groups, chunk span, accesses, the right-hand side of a slot and the sums of a chunk are the vector kernels' own (tfq_stream.hpp: Geo,
// TFQ_CHUNK_SPAN, ldv / stv, ld_b_under_x, slot_rhs, chunk_reduce_rounds).  The record of a chunk is kept plane by
// plane -- rec[plane][chunk][LN] -- so that every plane is summed by column_sum<LN, 1> (tfq_colops.hpp) as the records of the solver are.  No atomics.
#include "tfq_device.hpp"
#include "tfq_vec.hpp"
#include "tfq_colops.hpp"
#include "tfq_stream.hpp"
#include "tfq_project.hpp"

namespace tfq {
namespace {

// planes of a record: [0, K) G_ii | K + 2 * pair(i, l) + {0, 1} Re, Im of G_il for i < l, pairs in the order (0,1) (0,2) ... (K-2,K-1) |
// K*K + 2*i + {0, 1} Re, Im of g_i | K*K + 2*K  |B|^2
template <int K> struct PPlanes {
    static constexpr int N = project_planes(K);
    __host__ __device__ static constexpr int pair(int i, int l) { return i * K - (i * (i + 1)) / 2 + (l - i - 1); }
    __host__ __device__ static constexpr int G(int i, int l, int im) { return K + 2 * pair(i, l) + im; }
    __host__ __device__ static constexpr int g(int i, int im) { return K * K + 2 * i + im; }
    static constexpr int B2 = K * K + 2 * K;
};

// ---- per chunk: the Gram sums ---------------------------------------------------------------------------------------------------------
// one pass over W_0 ... W_{K-1} and the B block under each X block (zero where there is none, as in k_warm_residual); every product and
// every sum in double.  The planes leave through LDS in rounds of ROUND planes (all at once: 25 planes x 8 KiB for float storage), each round
// in the fixed slot order of chunk_reduce
template <typename R, int LM, int LN, int K>
__global__ __launch_bounds__(256) void k_project_gram(DevPlan d, ProjectVecs pv, double* rec) {
    using G = Geo<R, LM, LN>;
    using PL = PPlanes<K>;
    constexpr int NP = PL::N;
    constexpr int ROUND = 4096 / (256 * G::VEC);             // planes per round: 32 KiB of LDS
    __shared__ double s[ROUND * 256 * G::VEC];
    TFQ_CHUNK_SPAN(G)
    double acc[NP][G::VEC] = {};
    if (t < G::T) for (uint32_t w = t; w < nItems; w += G::T) {
        TFQ_ITEM_OFFSETS(G)
        R wr[K][G::VEC], wi[K][G::VEC], br[G::VEC], bi[G::VEC];
#pragma unroll
        for (int i = 0; i < K; ++i) { ldv(wr[i], (R const*)pv.w[i] + re); ldv(wi[i], (R const*)pv.w[i] + im); }
        ld_b_under_x<R, G::VEC>(br, bi, d, first + blk, size_t(w - blk * G::IPB) * G::VEC, G::P);
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) {
            double const b0 = br[v], b1 = bi[v];
            acc[PL::B2][v] = fma_(b1, b1, fma_(b0, b0, acc[PL::B2][v]));
#pragma unroll
            for (int i = 0; i < K; ++i) {
                double const a0 = wr[i][v], a1 = wi[i][v];
                acc[i][v] = fma_(a1, a1, fma_(a0, a0, acc[i][v]));
                // <a, c> = sum conj(a) c
                acc[PL::g(i, 0)][v] = fma_(a1, b1, fma_(a0, b0, acc[PL::g(i, 0)][v]));
                acc[PL::g(i, 1)][v] = fma_(-a1, b0, fma_(a0, b1, acc[PL::g(i, 1)][v]));
#pragma unroll
                for (int l = i + 1; l < K; ++l) {
                    double const c0 = wr[l][v], c1 = wi[l][v];
                    acc[PL::G(i, l, 0)][v] = fma_(a1, c1, fma_(a0, c0, acc[PL::G(i, l, 0)][v]));
                    acc[PL::G(i, l, 1)][v] = fma_(-a1, c0, fma_(a0, c1, acc[PL::G(i, l, 1)][v]));
                }
            }
        }
    }
    // rec[plane][chunk][LN]
    chunk_reduce_rounds<LN, G::VEC, G::T, ROUND>(acc, s, rec + size_t(chunk) * LN, size_t(d.nChunks) * LN, t, d.ilv);
}

// ---- per block column: the minimiser ---------------------------------------------------------------------------------------------------------
// G gamma = g by a Cholesky factorisation G = L L^H in the order of the starts (newest first).  Start i is dropped for this right-hand side when its
// pivot d_i = G_ii - sum_l |L_il|^2 is not greater than G_ii * pivotMin: it then takes no part in the rows behind it and gets gamma_i = 0.
// gamma [nCols][LN][4][2] (Re, Im; zeros for dropped and absent slots), nUsed [nCols][LN].  b = 0: gamma = 0, nUsed = 0
template <int LN, int K>
__global__ __launch_bounds__(256) void k_project_solve_col(DevPlan d, double const* rec, double pivotMin, double* gamma, int32_t* nUsed) {
    using PL = PPlanes<K>;
    __shared__ double s[256];
    uint32_t const col = blockIdx.x;
    int const t = threadIdx.x;
    uint32_t const c0 = d.colChunkPtr[col], c1 = d.colChunkPtr[col + 1];
    double v[PL::N];
#pragma unroll
    for (int p = 0; p < PL::N; ++p) {
        double one[1];
        column_sum<LN, 1>(rec + size_t(p) * d.nChunks * LN, c0, c1, s, one);
        v[p] = one[0];
    }
    if (t >= LN) return;
    double Lr[K][K] = {}, Li[K][K] = {}, inv[K] = {};       // L_il for l < i; 1 / L_ii, 0 for a dropped start
    bool kept[K];
    int used = 0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double dd = v[i];
#pragma unroll
        for (int l = 0; l < i; ++l) {
            // L_il = (G_il - sum_{m < l} L_im conj(L_lm)) / L_ll, with G_il = conj(G_li) of the stored upper triangle
            double xr = v[PL::G(l, i, 0)], xi = -v[PL::G(l, i, 1)];
#pragma unroll
            for (int m = 0; m < l; ++m) {
                xr = fma_(-Lr[i][m], Lr[l][m], fma_(-Li[i][m], Li[l][m], xr));
                xi = fma_(-Li[i][m], Lr[l][m], fma_(Lr[i][m], Li[l][m], xi));
            }
            Lr[i][l] = xr * inv[l]; Li[i][l] = xi * inv[l];     // (a dropped l: inv = 0, the column is empty)
            dd = fma_(-Lr[i][l], Lr[i][l], fma_(-Li[i][l], Li[i][l], dd));
        }
        kept[i] = dd > v[i] * pivotMin;                         // (G_ii = 0: 0 > 0 is false; a NaN is dropped too)
        inv[i] = kept[i] ? 1. / sqrt(dd) : 0.;
        used += kept[i] ? 1 : 0;
    }
    // L y = g, then L^H gamma = y
    double yr[K], yi[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double xr = v[PL::g(i, 0)], xi = v[PL::g(i, 1)];
#pragma unroll
        for (int l = 0; l < i; ++l) {
            xr = fma_(-Lr[i][l], yr[l], fma_(Li[i][l], yi[l], xr));
            xi = fma_(-Lr[i][l], yi[l], fma_(-Li[i][l], yr[l], xi));
        }
        yr[i] = xr * inv[i]; yi[i] = xi * inv[i];
    }
    double gr[K], gi[K];
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double xr = yr[i], xi = yi[i];
#pragma unroll
        for (int l = i + 1; l < K; ++l) {                       // conj(L_li) gamma_l
            xr = fma_(-Lr[l][i], gr[l], fma_(-Li[l][i], gi[l], xr));
            xi = fma_(-Lr[l][i], gi[l], fma_(Li[l][i], gr[l], xi));
        }
        gr[i] = xr * inv[i]; gi[i] = xi * inv[i];
    }
    bool const zeroB = !(v[PL::B2] > 0.);
    double* const out = gamma + (size_t(col) * LN + t) * 2 * kProjectMax;
#pragma unroll
    for (int i = 0; i < kProjectMax; ++i) {
        bool const on = (i < K) && !zeroB && kept[(i < K) ? i : 0];
        out[2 * i] = on ? gr[(i < K) ? i : 0] : 0.; out[2 * i + 1] = on ? gi[(i < K) ? i : 0] : 0.;
    }
    nUsed[size_t(col) * LN + t] = zeroB ? 0 : used;
}

// ---- per chunk: x := sum gamma_i S_i -------------------------------------------------------------------------------------------------------
// a lane keeps its right-hand sides on every trip, so it fetches its coefficients once.  Re and Im are accumulated in double by fused
// multiply-adds in slot order, each slot Re-part first, and rounded once to the storage type
template <typename R, int LM, int LN, int K>
__global__ __launch_bounds__(256) void k_project_combine(DevPlan d, ProjectVecs pv, double const* gamma) {
    using G = Geo<R, LM, LN>;
    TFQ_CHUNK_SPAN(G)
    if (t >= G::T) return;
    double cr[K][G::VEC], ci[K][G::VEC];
#pragma unroll
    for (int v = 0; v < G::VEC; ++v) {
        double const* const c = gamma + (size_t(col) * LN + slot_rhs<LN>(d.ilv, t * G::VEC + v)) * 2 * kProjectMax;
#pragma unroll
        for (int i = 0; i < K; ++i) { cr[i][v] = c[2 * i]; ci[i][v] = c[2 * i + 1]; }
    }
    R* const x = (R*)d.x;
    for (uint32_t w = t; w < nItems; w += G::T) {
        TFQ_ITEM_OFFSETS(G)
        double ar[G::VEC] = {}, ai[G::VEC] = {};
#pragma unroll
        for (int i = 0; i < K; ++i) {
            R sr[G::VEC], si[G::VEC];
            ldv(sr, (R const*)pv.s[i] + re); ldv(si, (R const*)pv.s[i] + im);
#pragma unroll
            for (int v = 0; v < G::VEC; ++v) {
                double const s0 = sr[v], s1 = si[v];
                ar[v] = fma_(-ci[i][v], s1, fma_(cr[i][v], s0, ar[v]));
                ai[v] = fma_(ci[i][v], s0, fma_(cr[i][v], s1, ai[v]));
            }
        }
        R xr[G::VEC], xi[G::VEC];
#pragma unroll
        for (int v = 0; v < G::VEC; ++v) { xr[v] = R(ar[v]); xi[v] = R(ai[v]); }
        stv(x + re, xr); stv(x + im, xi);
    }
}

template <typename R, int LM, int LN, int K>
void project_run(DevPlan const& d, ProjectVecs const& pv, double* rec, double pivotMin, double* gamma, int32_t* nUsed, hipStream_t s) {
    dim3 const grid(d.nChunks), cols(d.nCols), blk(256);
    k_project_gram<R, LM, LN, K><<<grid, blk, 0, s>>>(d, pv, rec);
    k_project_solve_col<LN, K><<<cols, blk, 0, s>>>(d, rec, pivotMin, gamma, nUsed);
    k_project_combine<R, LM, LN, K><<<grid, blk, 0, s>>>(d, pv, gamma);
}

} // namespace

bool project_launch(DevPlan const& d, int k, ProjectVecs const& pv, double* rec, double pivotMin, double* gamma, int32_t* nUsed, hipStream_t s) {
    if (k < 1 || k > kProjectMax) return false;
    // false: a missing instance is an error, never a fall-back
    return for_shape(d.dbl, d.LM, d.LN, [&](auto sh) {
        using S = decltype(sh); using R = typename S::real;
        switch (k) {
            case 1:  project_run<R, S::LM, S::LN, 1>(d, pv, rec, pivotMin, gamma, nUsed, s); break;
            case 2:  project_run<R, S::LM, S::LN, 2>(d, pv, rec, pivotMin, gamma, nUsed, s); break;
            case 3:  project_run<R, S::LM, S::LN, 3>(d, pv, rec, pivotMin, gamma, nUsed, s); break;
            default: project_run<R, S::LM, S::LN, 4>(d, pv, rec, pivotMin, gamma, nUsed, s); break;
        }
    });
}

} // namespace tfq
