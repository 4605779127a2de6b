// What every chunk-streaming kernel shares -- the tfQMR slot kernels and the refinement (tfq_vec.hip), the warm start (tfq_warm.hip), the start
// projection (tfq_project.hip): the geometry of one work group per chunk (Vec, Geo), the 16-byte non-temporal accesses (ldv, stv; ldf), the
// right-hand side of a slot (slot_rhs), the ordered sum of a right-hand side's terms and the way from per-lane accumulators to one [LN] record per
// plane (ordered_sum, chunk_reduce), the chunk span and the item offsets (TFQ_CHUNK_SPAN, TFQ_CHUNK_GATE, TFQ_ITEM_OFFSETS) and the B block under
// an X block (ld_b_under_x, ld_rhs).  ONE definition of each: "the sum order of the vector kernels" is this file.
// A slot kernel uses a piece from here only where its assembly stays the same (scripts/isa_compare.sh).
#pragma once
#include "tfq_device.hpp"
#include "tfq_colops.hpp"

namespace tfq {

template <typename R> struct Vec;
template <> struct Vec<double> { static constexpr int N = 2; using T = double2; };
template <> struct Vec<float>  { static constexpr int N = 4; using T = float4;  };

// T: the largest thread count <= 256 such that a thread's elements keep their RHS index j on every trip -- in the native order ((t * VEC) % LN == 0) and in
// the interleaved ones, where a thread's VEC elements are ROWS of one column and its column is (t + trip * T) % LN: T % LN == 0 (r04, for the 8 x 9 and
// 8 x 10 plans on row pairs; the only shape for which the two rules differ is LN = 10: 250 threads where 255 would do for the native order)
template <typename R, int LM, int LN>
struct Geo {
    static constexpr int VEC = Vec<R>::N;
    static constexpr int P = LM * LN;            // elements of one plane (Re or Im) of a block
    static constexpr int IPB = P / VEC;          // vector items per block plane
    static constexpr int T = (256 / LN) * LN;
    static_assert(P % VEC == 0, "block plane must be a multiple of the vector width");
};

// The vector kernels touch every element exactly once: all their accesses are non-temporal, so the streams neither
// wait for nor leave lines in the L2 that the multiply kernels want for their operand blocks (measured on P2:
// x_v6_v7 0.780 -> 0.716 ms, xpay_v6 0.316 -> 0.289 ms, and the two fused multiplies that follow 0.773/0.716 ->
// 0.743/0.681 ms).
template <typename R> __device__ inline void ldv(R (&r)[Vec<R>::N], R const* p) {
    using V = R __attribute__((ext_vector_type(Vec<R>::N)));
    auto const v = __builtin_nontemporal_load(reinterpret_cast<V const*>(p));
#pragma unroll
    for (int i = 0; i < Vec<R>::N; ++i) r[i] = v[i];
}
template <typename R> __device__ inline void stv(R* p, R const (&r)[Vec<R>::N]) {
    using V = R __attribute__((ext_vector_type(Vec<R>::N)));
    V v;
#pragma unroll
    for (int i = 0; i < Vec<R>::N; ++i) v[i] = r[i];
    __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
}
// the float shadow vector read with the vector width of R
template <int N> __device__ inline void ldf(float (&r)[N], float const* p) {
    if constexpr (N == 2) { auto const v = *reinterpret_cast<float2 const*>(p); r[0] = v.x; r[1] = v.y; }
    else { auto const v = *reinterpret_cast<float4 const*>(p); r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
}

// the right-hand side of element / LDS slot m of a work group's slice: ilv = G > 0: every G consecutive elements are rows of ONE column
// (tfq_device.hpp: ilv_offset), else consecutive columns
template <int LN> __device__ inline int slot_rhs(int ilv, int m) { return ilv ? (m / ilv) % LN : m % LN; }

// Sum the per-thread accumulators acc[NPL][VEC] of a work group into one [LN] record per plane, out[p * stride + j] (stride = LN: one record
// out[NPL][LN] per chunk).
// Fixed order => bitwise reproducible.  s is LDS of NPL*256*VEC doubles.
// The terms of one sum, in order: element m of the work group's slice belongs to column (m / G) % LN for plans that keep G rows of a
// column together (ILV = G, tfq_device.hpp: ilv_offset), to column m % LN otherwise.  (r04) ILV is a template parameter and the
// terms are fetched in batches of 16 before they are added: with the run-time `ilv` of r01-r03 every LDS read waited for the
// addition in front of it -- 32 dependent round trips by 16 threads at the end of every work group of k_v5_nrm, which is what made
// that kernel stream at 5.8 TB/s where k_xpay_v6, the same three vectors without a sum, reaches 6.6.  Same additions, same order.
template <int LN, int VEC, int T, int ILV>
__device__ inline double ordered_sum(double const* sp, int j) {
    constexpr int terms = (T * VEC) / LN, B = (terms < 16) ? terms : 16, full = terms / B * B;
    auto at = [&](int n) { return ILV ? sp[((n / ILV) * LN + j) * ILV + n % ILV] : sp[n * LN + j]; };
    double sum = 0;
    for (int n0 = 0; n0 < full; n0 += B) {
        double v[B];
#pragma unroll
        for (int i = 0; i < B; ++i) v[i] = at(n0 + i);
#pragma unroll
        for (int i = 0; i < B; ++i) sum += v[i];
    }
#pragma unroll
    for (int n = full; n < terms; ++n) sum += at(n);
    return sum;
}
// (the dispatch on ilv is written in place: as a function of its own it changes k_dot35 and k_v5_nrm)
// PLANES: plane p goes to out[p * planeStride + j] instead, for records that are kept plane by plane
template <int LN, int VEC, int T, int NPL, bool PLANES = false>
__device__ inline void chunk_reduce(double const (*acc)[VEC], double* s, double* out, int t, int ilv = 0, bool coherent = false, size_t planeStride = 0) {   // coherent: folded path, tfq_colops.hpp: co_store
    __syncthreads();
    if (t < T) {
#pragma unroll
        for (int p = 0; p < NPL; ++p)
#pragma unroll
            for (int v = 0; v < VEC; ++v) s[p * (256 * VEC) + t * VEC + v] = acc[p][v];
    }
    __syncthreads();
    for (int e = t; e < NPL * LN; e += 256) {
        int const p = e / LN, j = e % LN;
        double const* sp = s + p * (256 * VEC);
        st_record(PLANES ? out + p * planeStride + j : out + p * LN + j,
                  (2 == ilv) ? ordered_sum<LN, VEC, T, 2>(sp, j) : (4 == ilv) ? ordered_sum<LN, VEC, T, 4>(sp, j) : ordered_sum<LN, VEC, T, 0>(sp, j), coherent);
    }
}
// more planes than LDS holds at once: ROUND planes per round in plane order, s is LDS of ROUND*256*VEC doubles (the barrier in front of a round:
// the sums of the round before have been read)
template <int LN, int VEC, int T, int ROUND, int NPL, int P0 = 0>
__device__ inline void chunk_reduce_rounds(double const (&acc)[NPL][VEC], double* s, double* out, size_t planeStride, int t, int ilv) {
    if constexpr (P0 < NPL) {
        chunk_reduce<LN, VEC, T, (NPL - P0 < ROUND) ? NPL - P0 : ROUND, true>(acc + P0, s, out + P0 * planeStride, t, ilv, false, planeStride);
        chunk_reduce_rounds<LN, VEC, T, ROUND, NPL, P0 + ROUND>(acc, s, out, planeStride, t, ilv);
    }
}

// The span of this work group's chunk: blocks first ..., nItems vector items per plane, block column col, element offset base.  A statement macro,
// not a function: the slot kernels' code must not move (LABBOOK, "Grading kernels").  TFQ_CHUNK_GATE in front of it in the kernels of a solve's slot
#define TFQ_CHUNK_GATE if (d.ctl->state != 0) return;
#define TFQ_CHUNK_SPAN(G)                                                         \
    int const t = threadIdx.x;                                                    \
    uint32_t const chunk = blockIdx.x;                                            \
    uint32_t const first = d.chunkFirst[chunk];                                   \
    uint32_t const nItems = (d.chunkFirst[chunk + 1] - first) * G::IPB;           \
    uint32_t const col = d.chunkCol[chunk];                                       \
    size_t const base = size_t(first) * 2 * G::P;                                 \
    (void)col;

// item w of the span: its block blk (first + blk in the plan) and the offsets of its Re and Im piece
#define TFQ_ITEM_OFFSETS(G)                                                       \
    uint32_t const blk = w / G::IPB;                                              \
    size_t const re = base + size_t(blk) * 2 * G::P + size_t(w - blk * G::IPB) * G::VEC; \
    size_t const im = re + G::P;

// the B block under an X block (bOfX), or zeros
template <typename R, int VEC>
__device__ inline void ld_b_under_x(R (&r)[VEC], R (&i)[VEC], DevPlan const& d, uint32_t xblock, size_t inner, int P) {
    uint32_t const bq = d.bOfX[xblock];
    if (0xffffffffu == bq) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) { r[v] = 0; i[v] = 0; }
    } else {
        R const* b = (R const*)d.B + size_t(bq) * 2 * P + inner;
        ldv(r, b); ldv(i, b + P);
    }
}
// At the start of a solve v5 is B scattered onto zeros (tfqmrgpu_core.hxx:153): the kernels of the first iteration that read it
// take the B block under an X block, or zeros, directly -- v5 itself is first WRITTEN by k_v5_nrm of that iteration, or, in the "late v5"
// slot (DevPlan::lateV5), by the second fused multiply of that iteration, which reads the right-hand side the same way.
template <typename R, int VEC>
__device__ inline void ld_rhs(R (&r)[VEC], R (&i)[VEC], DevPlan const& d, uint32_t xblock, size_t inner, int P) {
    if (d.R) {   // the right-hand side of this solve is a whole X-shaped vector (mixed-precision refinement)
        R const* b = (R const*)d.R + size_t(xblock) * 2 * P + inner;
        ldv(r, b); ldv(i, b + P);
        return;
    }
    ld_b_under_x(r, i, d, xblock, inner, P);
}

} // namespace tfq
