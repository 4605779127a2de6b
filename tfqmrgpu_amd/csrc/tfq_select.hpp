// internal launch interface of the selection kernels (tfq_select.hip; tfqmrgpuExt_selectDrop and tfqmrgpuExt_selectLeak, tfqmrgpu_ext.h
// section 20; host side tfq_grade_host.cpp).  An ITEM is a block of X in the caller's order (selectDrop) or a leak position (selectLeak);
// its record is [LN] doubles as tfq_drop_cost.hip / tfq_leak_map.hip wrote it.  All pointers are device memory that the library owns.
#pragma once
#include <cstdint>
#include <hip/hip_runtime_api.h>

namespace tfq {

constexpr uint32_t kSelTile = 256;                 // items per compaction tile: one work group, one item per thread in the scatter
constexpr uint32_t kSelExcluded = 0xffffffffu;     // in colOf: this item is never selected (a block of X that carries a block of B)
inline uint32_t select_tiles(uint32_t nItems) { return (nItems + kSelTile - 1) / kSelTile; }

// flag[n] = 1 where item n is selected, else 0, and tileCount[tile] = the flags set among the items of the tile (the first pass of the
// compaction).  rec [nItems][LN]; bnorm2 of column c and right-hand side j at bnorm2[c * bStride + j]; colOf [nItems] the compressed block
// column of every item or kSelExcluded.  eta2 = eta * eta as the host rounded it; the product eta2 * bnorm2 is rounded once.
//   leak == false (selectDrop): selected where rec <= eta2 * bnorm2 for EVERY j        (a comparison with a NaN is false)
//   leak == true  (selectLeak): selected where bnorm2 > 0 and rec > eta2 * bnorm2 for SOME j
void select_flag_launch(uint32_t nItems, int LN, double const* rec, double const* bnorm2, uint32_t bStride, uint32_t const* colOf,
    double eta2, bool leak, uint8_t* flag, uint32_t* tileCount, hipStream_t s);

// the second and third pass: tileCount [nTiles + 1] becomes the exclusive prefix sums of the counts (one work group), entry nTiles the
// number selected; list [0 .. that number) = the selected items, ascending (one work group per tile)
void select_compact_launch(uint32_t nItems, uint8_t const* flag, uint32_t* tileCount, uint32_t* list, hipStream_t s);

// out[c * LN + j] = the sum over the entries i in start[c] .. start[c + 1] whose item n = order[i] (order == nullptr: n = i) has
// flag[n] == keep of rec[n * LN + j], or of its square root (root).  One work group per column, one fixed order, no atomics
void select_sum_launch(uint32_t nCols, int LN, double const* rec, uint8_t const* flag, uint32_t const* start, uint32_t const* order,
    bool keep, bool root, double* out, hipStream_t s);

} // namespace tfq
