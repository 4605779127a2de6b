// Block layout conversion between TWO shapes (padded plans, tfqmrgpu_ext.h section 18): the caller's compact blocks of uR x uC on one side,
// the plan's blocks of nR x nC (nR >= uR, nC >= uC; one of the fifteen listed shapes) on the other.  The two-shape counterparts of k_convert /
// k_convert_list (tfq_layout.hip): the same way to a block (firstUser / list, u2n), the same place of an element on the library's side
// (plane_offset with the plan's nC), the same user_offset on the caller's side, with the caller's shape and a block stride of 2 uR uC.
//
// Setting (direction 0) writes EVERY element of the library's block: the caller's value inside, +0.0 in the padding, and 1.0 in the real
// plane of the padded diagonal where the block is a diagonal block of A (unit[ub] != 0) -- A (+) 1 is as regular as A, and its inverse in
// the block-Jacobi set-up is A^-1 (+) 1.  Getting (direction 1) reads the inside only.
// Accesses are element-wise, as in convert_block: the caller's side of a 25 x 25 block is not 16-byte aligned from block to block.
#include "tfq_convert.hpp"

namespace tfq {

// one block, by the 256 threads of a work group; unit: this is a diagonal block of A
template <typename R, typename U>   // R: library side, U: caller's side
__device__ inline void convert_block_pad(int direction, R* nblock, U* ublock, int nR, int nC, int uR, int uC, int layout, bool trans, bool conj,
    int ilv, bool unit)
{
    if (0 == direction) {
        int const P = nR * nC, E = 2 * P;
        for (int e = threadIdx.x; e < E; e += 256) {      // every element of the library's block
            int const c = e / P, r = (e % P) / nC, s = e % nC;
            R v = (unit && 0 == c && r == s) ? R(1) : R(0);
            if (r < uR && s < uC) {
                v = R(ublock[user_offset(layout, trans, uR, uC, r, s, c)]);
                if (conj && c) v = -v;
            }
            nblock[c * P + plane_offset(ilv, r, s, nC)] = v;
        }
    } else {
        int const P = uR * uC, E = 2 * P;
        for (int e = threadIdx.x; e < E; e += 256) {      // the caller's elements only
            int const c = e / P, r = (e % P) / uC, s = e % uC;
            U const v = U(nblock[c * nR * nC + plane_offset(ilv, r, s, nC)]);
            ublock[user_offset(layout, trans, uR, uC, r, s, c)] = (conj && c) ? -v : v;
        }
    }
}

// One work group per USER block ub = firstUser + blockIdx.x; block 0 of `stage` is user block firstUser (k_convert)
template <typename R, typename U>
__global__ __launch_bounds__(256) void k_convert_pad(int direction, R* native, U* stage, uint32_t const* u2n, uint8_t const* unit,
    uint32_t firstUser, int nR, int nC, int uR, int uC, int layout, bool trans, bool conj, int ilv)
{
    uint32_t const ub = firstUser + blockIdx.x;
    uint32_t const nb = u2n ? u2n[ub] : ub;
    convert_block_pad(direction, native + size_t(nb) * 2 * nR * nC, stage + size_t(blockIdx.x) * 2 * uR * uC, nR, nC, uR, uC, layout, trans, conj,
                      ilv, unit && unit[ub]);
}

// One work group per entry k = blockIdx.x of `list`; block k of `stage` is the caller's side of user block list[k] (k_convert_list)
template <typename R, typename U>
__global__ __launch_bounds__(256) void k_convert_pad_list(int direction, R* native, U* stage, uint32_t const* list, uint32_t const* u2n,
    uint8_t const* unit, int nR, int nC, int uR, int uC, int layout, bool trans, bool conj, int ilv)
{
    uint32_t const ub = list[blockIdx.x];
    uint32_t const nb = u2n ? u2n[ub] : ub;
    convert_block_pad(direction, native + size_t(nb) * 2 * nR * nC, stage + size_t(blockIdx.x) * 2 * uR * uC, nR, nC, uR, uC, layout, trans, conj,
                      ilv, unit && unit[ub]);
}

// as launch_convert, with the caller's shape uR x uC next to the plan's and the flags of A's diagonal blocks (device memory, by the caller's
// block index; nullptr for B and X)
void launch_convert_pad(int direction, bool userDbl, bool nativeDbl, void* native, void* stage, uint32_t const* u2n, uint8_t const* unit,
    uint32_t firstUser, uint32_t nBlocks, int nR, int nC, int uR, int uC, int layout, bool trans, bool conj, int ilv, hipStream_t s, uint32_t const* list)
{
    if (0 == nBlocks) return;
    dim3 const g(nBlocks), b(256);
#define TFQ_CONVERT(R, U) { \
        if (list) k_convert_pad_list<R, U><<<g, b, 0, s>>>(direction, (R*)native, (U*)stage, list, u2n, unit, nR, nC, uR, uC, layout, trans, conj, ilv); \
        else      k_convert_pad<R, U><<<g, b, 0, s>>>(direction, (R*)native, (U*)stage, u2n, unit, firstUser, nR, nC, uR, uC, layout, trans, conj, ilv); }
    if (nativeDbl) { if (userDbl) TFQ_CONVERT(double, double) else TFQ_CONVERT(double, float) }
    else           { if (userDbl) TFQ_CONVERT(float, double)  else TFQ_CONVERT(float, float) }
#undef TFQ_CONVERT
}

} // namespace tfq
