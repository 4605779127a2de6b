// What the layout conversions of one shape (tfq_layout.hip) and of two shapes (tfq_pad.hip) share: where an element lies in the CALLER's block.
#pragma once
#include "tfq_device.hpp"

namespace tfq {

// offset of part c of element (r, s) of an nR x nC block in the USER's array
__device__ inline uint32_t user_offset(int layout, bool trans, int nR, int nC, int r, int s, int c) {
    int const rows = trans ? nC : nR, cols = trans ? nR : nC;   // shape of the user's array
    int const i = trans ? s : r, j = trans ? r : s;              // position inside it
    (void)rows;
    switch (layout) {
        case TFQMRGPU_LAYOUT_RRRRIIII: return uint32_t(c * nR * nC + i * cols + j);
        case TFQMRGPU_LAYOUT_RRIIRRII: return uint32_t(i * 2 * cols + c * cols + j);
        default:                       return uint32_t((i * cols + j) * 2 + c);  // RIRIRIRI
    }
}

} // namespace tfq
