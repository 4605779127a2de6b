// What the kernels on the interleaved element orders share (tfq_spmm_ilv8.hip, tfq_spmm_ilv16.hip) besides tfq_spmm.hpp: the start of a work group
// and, for the 16-byte pieces of a lane, the operands of an epilogue and the plane exchange of the 8-row kernels.  The arithmetic of an epilogue is
// epi_xpay2 | epi_axpy | epi_dot | epi_nrm of tfq_spmm.hpp per element.
// A kernel uses a piece only where every instance keeps its assembly with it (scripts/isa_compare.sh against the parent commit; the compiler
// schedules and allocates differently around an inlined call often enough); elsewhere the block stays written out in the kernel:
//   ChunkWG                k_spmm_ilv8, k_spmm_ilv8b, k_spmm_ilv8w
//   EpiPiece               k_spmm_ilv8, k_spmm_ilv8b
//   planes / xor8          k_spmm_ilv8, k_spmm_ilv8b, k_spmm_ilv8w; k_spmm_ilv8f for Y (u, v, w with its local x8; b written out)
//   epi_xpay2 | epi_axpy   k_spmm_ilv8
//   epi_dot | epi_nrm      all but k_spmm_ilvf (the residual of k_spmm_ilv16 has another form)
#pragma once
#include "tfq_spmm.hpp"

namespace tfq {

// The start of a work group of 256 threads that processes one chunk (the Y blocks [first, last) of block column col).
// The index lists through the constant address space: uniform reads become scalar loads whatever the stores around them
struct ChunkWG {
    using CU32 = __attribute__((address_space(4))) uint32_t const*;
    int lane, wave; CU32 pairs, starts; uint32_t chunk, first, last, col;
    __device__ __forceinline__ explicit ChunkWG(SpmmArgs const& a)
        : lane(threadIdx.x & 63), wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), pairs((CU32)(uintptr_t)a.pairs), starts((CU32)(uintptr_t)a.starts),
          chunk(a.order ? a.order[blockIdx.x] : blockIdx.x),   // XCD-aware launch order (tfq_plan.cpp)
          first(a.chunkFirst[chunk]), last(a.chunkFirst[chunk + 1]), col(a.chunkCol[chunk]) {}
};

// A piece: the 16 bytes of a lane, V = d2v | f4v (a pair | quad of rows of one column); its shadow-vector values are floats, f2v | f4v
template <typename V> using PieceReal = std::remove_reference_t<decltype(V{}[0])>;
template <typename V> constexpr int piece_n = sizeof(V) / sizeof(PieceReal<V>);
template <typename V> using ShadowPiece = typename VecOf<float, piece_n<V>>::T;

// The vectors an epilogue reads for the piece at `off` of a lane's plane: old v4 | v5 (u), v8 (v) and v3 (w), touched once (non-temporal).
// FIRST: the first iteration of a solve, old v4 = v8 = 0 are not read; HASH: v3 is recomputed, not read.  What is not read is zero
template <typename V>
struct EpiPiece {
    V u, v; ShadowPiece<V> w;
    template <int EPI, bool FIRST, bool HASH>
    __device__ __forceinline__ void load(SpmmArgs const& a, size_t off) {
        using R = PieceReal<V>;
        u = V{}; v = V{}; w = ShadowPiece<V>{};
        if constexpr (EPI == EPI_XPAY_DOT || EPI == EPI_AXPY_NRM_DOT) {
            if constexpr (!(EPI == EPI_XPAY_DOT && FIRST)) {
                u = __builtin_nontemporal_load((V const*)((R const*)a.e0 + off));
                if constexpr (EPI == EPI_XPAY_DOT) v = __builtin_nontemporal_load((V const*)((R const*)a.e1 + off));
            }
            if constexpr (!HASH) w = __builtin_nontemporal_load((ShadowPiece<V> const*)(a.v3 + off));
        }
    }
};

// The plane exchange of the 8-row kernels: lane (cp = 0: Re, 1: Im) holds its plane's piece `mine`, the lane 8 further the `other` plane's piece of the
// same elements (xor8); planes() is (Re, Im) of the elements from the two
template <typename V> __device__ inline V xor8(V v) {
    if constexpr (piece_n<V> == 2) return V{__shfl_xor(v[0], 8), __shfl_xor(v[1], 8)};
    else return V{__shfl_xor(v[0], 8), __shfl_xor(v[1], 8), __shfl_xor(v[2], 8), __shfl_xor(v[3], 8)};
}
template <typename V> struct ReIm { V r, i; };
template <typename V> __device__ __forceinline__ ReIm<V> planes(V mine, V other, int cp) { return { cp ? other : mine, cp ? mine : other }; }

} // namespace tfq
