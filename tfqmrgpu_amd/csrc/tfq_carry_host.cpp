// Carry an operand from one plan to another (tfqmrgpu_ext.h section 15), host side: the checks of the caller's block map and the
// composition of the list the kernel reads (tfq_carry.hip: k_carry).  Plain C++ on plain index arrays -- no Plan, no device:
// scripts/carry_map_check.cpp runs it under the sanitizers.
//
// The caller's map is in the caller's block orders of BOTH plans: block n of the destination takes block oldBlock[n] of the source, -1 a
// zero block, no list the identity.  The kernel walks the destination window as it lies in the buffer, so it needs the map in the stored
// orders: A and B are stored in the caller's order, the X-shaped vectors in each plan's internal order (Plan::u2i, Plan::i2u).  One pass
// over the destination's blocks, O(nnzb): nothing is searched or sorted.
#include "tfq_plan.hpp"

namespace tfq {

bool carry_map_ok(int64_t nBlocks, int32_t const* oldBlock, uint32_t nnzbDst, uint32_t nnzbSrc) {
    if (nBlocks < 0 || uint64_t(nBlocks) != uint64_t(nnzbDst)) return false;
    if (nullptr == oldBlock) return nnzbDst == nnzbSrc;             // the identity needs as many blocks on either side
    for (int64_t n = 0; n < nBlocks; ++n) {
        int32_t const o = oldBlock[n];
        if (o < -1) return false;
        if (o >= 0 && uint32_t(o) >= nnzbSrc) return false;
    }
    return true;
}

void carry_compose(std::vector<uint32_t>& out, uint32_t nnzbDst, int32_t const* oldBlock, uint32_t const* dstI2U, uint32_t const* srcU2I) {
    out.resize(nnzbDst);
    for (uint32_t n = 0; n < nnzbDst; ++n) {
        uint32_t const u = dstI2U ? dstI2U[n] : n;                  // the caller's index of stored block n of the destination
        int64_t const o = oldBlock ? int64_t(oldBlock[u]) : int64_t(u);
        out[n] = (o < 0) ? kCarryZero : (srcU2I ? srcU2I[o] : uint32_t(o));
    }
}

} // namespace tfq
