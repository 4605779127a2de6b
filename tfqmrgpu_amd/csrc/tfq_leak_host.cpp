// Truncation leak (tfqmrgpu_ext.h section 11), host side: which block products A_ik X_kc land on a block row i that block column c of X
// does NOT hold; the pattern of X grown by chosen ones of those positions (section 12, grow_pattern); and, at the end of the file, the
// plan's products grouped by X block and the pattern of X without chosen blocks (section 13, drop_listing and shrink_pattern).  Plain C++ on
// plain index arrays -- no Plan, no device: scripts/leak_listing_check.cpp, scripts/grow_pattern_check.cpp and
// scripts/shrink_pattern_check.cpp run it under the sanitizers.
//
// One pass over the block rows i of A.  Row i of X is stamped into a [nCols] array, so that "(i, c) is in the pattern of X" is one
// comparison; for every A block (i, k) of the row, in ascending k, every X block (k, c) of row k whose column is not stamped is a product
// of the leak position (c, i).  The products come out sorted by (i, k); one stable counting sort by c makes that (c, i, k).  A's rows
// in ascending k come from A by block column (a_by_column, built once per plan): walking the columns in order and dealing every block to
// its row leaves each row sorted.  Cost: O(nPairs + nLeakPairs + nnzbA + nnzbX + nRows + nCols) -- every product of A X is looked at
// once, inside the pattern or not; nothing is searched.
#include "tfq_plan.hpp"

#include <algorithm>

namespace tfq {

void a_by_column(uint32_t nRows, std::vector<uint32_t> const& colOfA, std::vector<uint32_t>& cscPtr, std::vector<uint32_t>& cscBlock) {
    uint32_t const nnzbA = uint32_t(colOfA.size());
    cscPtr.assign(size_t(nRows) + 1, 0u);
    for (auto const c : colOfA) ++cscPtr[c + 1];
    for (uint32_t c = 0; c < nRows; ++c) cscPtr[c + 1] += cscPtr[c];
    cscBlock.resize(nnzbA);
    std::vector<uint32_t> fill(cscPtr.begin(), cscPtr.end() - 1);
    for (uint32_t q = 0; q < nnzbA; ++q) cscBlock[fill[colOfA[q]]++] = q;
}

uint32_t leak_unit_products(int LM, int LN) {
    return uint32_t(std::min(64, std::max(16, 4096 / (LM * LN))));
}

bool leak_listing(LeakListing& out, uint32_t nRows, uint32_t nCols,
    uint32_t nnzbA, uint32_t const* rowOfA, uint32_t const* colOfA, uint32_t const* cscPtr, uint32_t const* cscBlock,
    uint32_t nnzbX, uint32_t const* rowOfX, uint32_t const* colOfX, uint32_t const* u2i, uint32_t maxProducts)
{
    out = LeakListing{};
    // blocks of A by block row in ascending block column, blocks of X by block row in the caller's order
    std::vector<uint32_t> aPtr(size_t(nRows) + 1, 0u), aByRow(nnzbA), xPtr(size_t(nRows) + 1, 0u), xByRow(nnzbX);
    for (uint32_t q = 0; q < nnzbA; ++q) ++aPtr[rowOfA[q] + 1];
    for (uint32_t x = 0; x < nnzbX; ++x) ++xPtr[rowOfX[x] + 1];
    for (uint32_t r = 0; r < nRows; ++r) { aPtr[r + 1] += aPtr[r]; xPtr[r + 1] += xPtr[r]; }
    {
        std::vector<uint32_t> fill(aPtr.begin(), aPtr.end() - 1);
        for (uint32_t k = 0; k < nRows; ++k)
            for (uint32_t n = cscPtr[k]; n < cscPtr[k + 1]; ++n) { auto const q = cscBlock[n]; aByRow[fill[rowOfA[q]]++] = q; }
        fill.assign(xPtr.begin(), xPtr.end() - 1);
        for (uint32_t x = 0; x < nnzbX; ++x) xByRow[fill[rowOfX[x]]++] = x;
    }
    // (k, c) is in the pattern of X once: of two X blocks with the same row and column the solver's pair list knows the first only
    std::vector<uint32_t> stamp(nCols, 0u);
    std::vector<uint8_t> isFirst(nnzbX, uint8_t(0));
    for (uint32_t r = 0; r < nRows; ++r)
        for (uint32_t n = xPtr[r]; n < xPtr[r + 1]; ++n) {
            auto const x = xByRow[n];
            if (stamp[colOfX[x]] != r + 1) { stamp[colOfX[x]] = r + 1; isFirst[x] = 1; }
        }
    std::fill(stamp.begin(), stamp.end(), 0u);

    struct Product { uint32_t col, row, a, x; };
    std::vector<Product> found;
    std::vector<size_t> colCount(size_t(nCols) + 1, 0);
    for (uint32_t i = 0; i < nRows; ++i) {
        for (uint32_t n = xPtr[i]; n < xPtr[i + 1]; ++n) stamp[colOfX[xByRow[n]]] = i + 1;
        for (uint32_t m = aPtr[i]; m < aPtr[i + 1]; ++m) {
            auto const q = aByRow[m];
            auto const k = colOfA[q];
            for (uint32_t n = xPtr[k]; n < xPtr[k + 1]; ++n) {
                auto const x = xByRow[n];
                auto const c = colOfX[x];
                if (!isFirst[x] || stamp[c] == i + 1) continue;
                found.push_back(Product{c, i, q, u2i[x]});
                ++colCount[c + 1];
            }
        }
    }
    if (found.size() > size_t(0x7fffffff)) return false;            // the device lists are 32 bit
    for (uint32_t c = 0; c < nCols; ++c) colCount[c + 1] += colCount[c];

    // stable by column: (column, row, k)
    std::vector<uint32_t> order(found.size());
    {
        std::vector<size_t> fill(colCount.begin(), colCount.end() - 1);
        for (size_t n = 0; n < found.size(); ++n) order[fill[found[n].col]++] = uint32_t(n);
    }
    out.pairs.resize(2 * found.size());
    out.posStart.push_back(0u);
    for (size_t n = 0; n < order.size(); ++n) {
        auto const& f = found[order[n]];
        if (0 == n || f.col != out.posCol.back() || f.row != out.posRow.back()) {
            if (n) out.posStart.push_back(uint32_t(n));
            out.posCol.push_back(f.col); out.posRow.push_back(f.row);
        }
        out.pairs[2 * n] = f.a; out.pairs[2 * n + 1] = f.x;
    }
    if (!order.empty()) out.posStart.push_back(uint32_t(order.size()));

    // work units: runs of positions of ONE column with at most maxProducts products (a position is never cut)
    uint32_t const nPos = uint32_t(out.posCol.size());
    out.colUnitPtr.assign(size_t(nCols) + 1, 0u);
    for (uint32_t pos = 0, c = 0; c < nCols; ++c) {
        out.colUnitPtr[c] = uint32_t(out.unitFirst.size());
        uint32_t inUnit = 0;
        for (; pos < nPos && out.posCol[pos] == c; ++pos) {
            uint32_t const n = out.posStart[pos + 1] - out.posStart[pos];
            if (0 == inUnit || inUnit + n > maxProducts) { out.unitFirst.push_back(pos); inUnit = 0; }
            inUnit += n;
        }
    }
    out.colUnitPtr[nCols] = uint32_t(out.unitFirst.size());
    out.unitFirst.push_back(nPos);
    out.built = true;
    return true;
}

// The grown pattern (tfqmrgpu_ext.h section 12).  The taken positions are dealt to their block rows in ascending compressed column -- the
// order of the caller's column indices, createPlan numbers the columns that way --: all positions are in that order already, a list is
// brought into it by one stable counting sort by column.  A position named twice arrives twice in a row at its block row: one comparison
// with the column that row took last.  Cost: O(nnzbX + nTake + nRows + nCols), nothing is searched.
int grow_pattern(GrownPattern& out, uint32_t nRows, uint32_t nCols, uint32_t nnzbX, uint32_t const* rowOfX, uint32_t const* colOfX,
    int32_t const* callersCol, int indexOffset, size_t nPos, uint32_t const* posRow, uint32_t const* posCol, uint64_t nTake, uint64_t const* take)
{
    out = GrownPattern{};
    size_t const nAdd = take ? size_t(nTake) : nPos;
    if (take && nTake > nPos) return 1;                              // more indices than positions: one is out of range or named twice
    if (size_t(nnzbX) + nAdd >= size_t(0x7fffffff)) return 2;        // (room for an index offset of 1)
    std::vector<uint32_t> add(nAdd);                                 // the taken positions, ascending by column
    if (take) {
        std::vector<size_t> fill(size_t(nCols) + 1, 0);
        for (size_t n = 0; n < nAdd; ++n) {
            if (take[n] >= nPos) return 1;
            ++fill[posCol[take[n]] + 1];
        }
        for (uint32_t c = 0; c < nCols; ++c) fill[c + 1] += fill[c];
        for (size_t n = 0; n < nAdd; ++n) add[fill[posCol[take[n]]]++] = uint32_t(take[n]);
    } else {
        for (size_t n = 0; n < nAdd; ++n) add[n] = uint32_t(n);
    }
    GrownPattern g;
    g.rowPtr.assign(size_t(nRows) + 1, 0);
    for (uint32_t x = 0; x < nnzbX; ++x) ++g.rowPtr[rowOfX[x] + 1];
    for (auto const p : add) ++g.rowPtr[posRow[p] + 1];
    for (uint32_t r = 0; r < nRows; ++r) g.rowPtr[r + 1] += g.rowPtr[r];
    size_t const nnzb = size_t(nnzbX) + nAdd;
    g.colInd.resize(nnzb); g.oldBlock.resize(nnzb);
    std::vector<int32_t> fill(g.rowPtr.begin(), g.rowPtr.end() - 1);
    for (uint32_t x = 0; x < nnzbX; ++x) {                           // the old blocks first, in the caller's order
        auto const at = fill[rowOfX[x]]++;
        g.colInd[at] = callersCol[colOfX[x]]; g.oldBlock[at] = int32_t(x);
    }
    std::vector<uint32_t> lastCol(nRows, ~0u);                       // the column of the position that each block row took last
    for (auto const p : add) {
        auto const r = posRow[p], c = posCol[p];
        if (lastCol[r] == c) return 1;                               // named twice
        lastCol[r] = c;
        auto const at = fill[r]++;
        g.colInd[at] = callersCol[c]; g.oldBlock[at] = -1;
    }
    for (auto& v : g.rowPtr) v += indexOffset;
    out = std::move(g);
    return 0;
}

// The listing of the drop cost (tfqmrgpu_ext.h section 13): the plan's pair list comes grouped by the block of A X that a product lands
// on; one stable counting sort by the X operand groups it by X block and keeps the order of the pair list inside a block
void drop_listing(DropListing& out, uint32_t nnzbX, size_t nPairs, uint32_t const* pairs, uint32_t const* u2i) {
    out = DropListing{};
    out.start.assign(size_t(nnzbX) + 1, 0u);
    for (size_t q = 0; q < nPairs; ++q) ++out.start[pairs[2 * q + 1] + 1];
    for (uint32_t x = 0; x < nnzbX; ++x) out.start[x + 1] += out.start[x];
    out.aOf.resize(nPairs);
    std::vector<uint32_t> fill(out.start.begin(), out.start.end() - 1);
    for (size_t q = 0; q < nPairs; ++q) out.aOf[fill[pairs[2 * q + 1]]++] = pairs[2 * q];
    out.xOf.assign(u2i, u2i + nnzbX);
    out.built = true;
}

// The shrunk pattern (section 13): one mark per old block, so that a block named twice is one comparison; the blocks that stay are
// written in the caller's order, which is the order inside every block row.  Cost: O(nnzbX + nDrop + nRows), nothing is searched
int shrink_pattern(GrownPattern& out, uint32_t nRows, uint32_t nnzbX, uint32_t const* rowOfX, uint32_t const* colOfX,
    int32_t const* callersCol, int indexOffset, uint8_t const* hasB, uint64_t nDrop, int32_t const* drop)
{
    out = GrownPattern{};
    if (nDrop > uint64_t(nnzbX)) return 1;                           // more indices than blocks: one is out of range or named twice
    std::vector<uint8_t> gone(nnzbX, uint8_t(0));
    for (uint64_t n = 0; n < nDrop; ++n) {
        if (drop[n] < 0 || uint32_t(drop[n]) >= nnzbX || gone[drop[n]]) return 1;
        gone[drop[n]] = 1;
    }
    for (uint64_t n = 0; n < nDrop; ++n) if (hasB[drop[n]]) return 2;  // (behind the look at every index: a bad list is a bad list first)
    GrownPattern g;
    g.rowPtr.assign(size_t(nRows) + 1, 0);
    size_t const nnzb = size_t(nnzbX) - size_t(nDrop);
    g.colInd.reserve(nnzb); g.oldBlock.reserve(nnzb);
    for (uint32_t x = 0; x < nnzbX; ++x) {
        if (gone[x]) continue;
        ++g.rowPtr[rowOfX[x] + 1];
        g.colInd.push_back(callersCol[colOfX[x]]); g.oldBlock.push_back(int32_t(x));
    }
    for (uint32_t r = 0; r < nRows; ++r) g.rowPtr[r + 1] += g.rowPtr[r];
    for (auto& v : g.rowPtr) v += indexOffset;
    out = std::move(g);
    return 0;
}

} // namespace tfq
