// What the streaming kernels outside the tfQMR slot share (tfq_warm.hip, tfq_project.hip): the geometry of one work group per chunk, the
// 16-byte non-temporal accesses, and the ordered sum of a right-hand side's terms.  Geometry and access width are those of the vector
// kernels (tfq_vec.hip: Geo, ldv, stv): every lane moves 16 bytes per access and keeps its right-hand side on every trip.
#pragma once
#include "tfq_device.hpp"

namespace tfq {

template <typename R> struct WVec;
template <> struct WVec<double> { static constexpr int N = 2; };
template <> struct WVec<float>  { static constexpr int N = 4; };

template <typename R, int LM, int LN>
struct WGeo {
    static constexpr int VEC = WVec<R>::N;
    static constexpr int P = LM * LN;            // elements of one plane (Re or Im) of a block
    static constexpr int IPB = P / VEC;          // vector items per block plane
    static constexpr int T = (256 / LN) * LN;    // active threads: a multiple of LN, so that a thread keeps its right-hand side on every trip
    static_assert(P % VEC == 0, "block plane must be a multiple of the vector width");
};

template <typename R> __device__ inline void w_ld(R (&r)[WVec<R>::N], R const* p) {
    using V = R __attribute__((ext_vector_type(WVec<R>::N)));
    auto const v = __builtin_nontemporal_load(reinterpret_cast<V const*>(p));
#pragma unroll
    for (int i = 0; i < WVec<R>::N; ++i) r[i] = v[i];
}
template <typename R> __device__ inline void w_st(R* p, R const (&r)[WVec<R>::N]) {
    using V = R __attribute__((ext_vector_type(WVec<R>::N)));
    V v;
#pragma unroll
    for (int i = 0; i < WVec<R>::N; ++i) v[i] = r[i];
    __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
}

// the terms of one right-hand side in the work group's slice of LDS, added in slot order: slot m belongs to column (m / ILV) % LN for plans that keep
// ILV rows of a column together (tfq_device.hpp: ilv_offset), to column m % LN otherwise
template <int LN, int VEC, int T, int ILV>
__device__ inline double w_ordered_sum(double const* sp, int j) {
    constexpr int terms = (T * VEC) / LN;
    double sum = 0;
    for (int n = 0; n < terms; ++n) sum += ILV ? sp[((n / ILV) * LN + j) * ILV + n % ILV] : sp[n * LN + j];
    return sum;
}
// the same for the element order of the plan (DevPlan::ilv)
template <int LN, int VEC, int T>
__device__ inline double w_ordered_sum(int ilv, double const* sp, int j) {
    return (2 == ilv) ? w_ordered_sum<LN, VEC, T, 2>(sp, j) : (4 == ilv) ? w_ordered_sum<LN, VEC, T, 4>(sp, j) : w_ordered_sum<LN, VEC, T, 0>(sp, j);
}

} // namespace tfq
