// The listing of the drop cost and the shrunk pattern (tfqmrgpu_amd/csrc/tfq_leak_host.cpp: drop_listing, shrink_pattern; tfqmrgpu_ext.h
// section 13) as a stand-alone host program, for a sanitizer build:
//   shrink_pattern_check <file> [<file> ...]       (scripts/check_sanitize.sh shrink_pattern builds it with -fsanitize=address,undefined and runs it)
// The files are those of scripts/leak_listing_check.cpp (scripts/leak_listing_inputs.py writes them).  For every file the pair list of
// the plan is written down by brute force -- per block (i, c) of X in the caller's order, per A block (i, k) of that row, the X block
// (k, c) --, the listing is built from it and compared with the pairs picked out per X block; the pattern is shrunk by: no block (NULL
// list), one block, every third block backwards, every block that carries no B, and -- with B taken out of the last column -- that whole
// column, which vanishes; and refused for an index out of range, a negative one, one named twice, more indices than blocks, and a block
// that carries B.
// Checked: start, aOf and xOf of the listing; the counts of the shrunk pattern, its row pointers with the index offset, that the blocks
// that stay keep their order and their column index and that oldBlock names them; a refusal leaves `out` empty.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <utility>

#include "tfq_plan.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("%s: FAILED %s (line %d)\n", path, #cond, __LINE__); return 1; } } while (0)

static int shrunk_ok(char const* path, tfq::GrownPattern const& g, uint32_t nRows, std::vector<uint32_t> const& rowOfX,
    std::vector<uint32_t> const& colOfX, std::vector<int32_t> const& callersCol, int off, std::vector<int32_t> const& dropped)
{
    size_t const nnzbX = rowOfX.size(), nnzb = nnzbX - dropped.size();
    CHECK(g.rowPtr.size() == size_t(nRows) + 1 && g.colInd.size() == nnzb && g.oldBlock.size() == nnzb);
    CHECK(g.rowPtr[0] == off && size_t(g.rowPtr[nRows] - off) == nnzb);
    std::vector<uint8_t> gone(nnzbX, 0);
    for (auto const d : dropped) gone[d] = 1;
    size_t n = 0;
    for (size_t x = 0; x < nnzbX; ++x) {
        if (gone[x]) continue;
        CHECK(n < nnzb && g.oldBlock[n] == int32_t(x) && g.colInd[n] == callersCol[colOfX[x]]);
        CHECK(g.rowPtr[rowOfX[x]] - off <= int32_t(n) && int32_t(n) < g.rowPtr[rowOfX[x] + 1] - off);
        ++n;
    }
    CHECK(n == nnzb);
    return 0;
}

static int run(char const* path) {
    std::ifstream in(path);
    CHECK(in.good());
    uint64_t nRows, nCols, nnzbA, nnzbX, maxProducts, wantBlocks, wantPairs;
    in >> nRows >> nCols >> nnzbA >> nnzbX >> maxProducts >> wantBlocks >> wantPairs;
    auto read = [&](size_t n) { std::vector<uint32_t> v(n); for (auto& x : v) in >> x; return v; };
    auto const rowOfA = read(nnzbA), colOfA = read(nnzbA), rowOfX = read(nnzbX), colOfX = read(nnzbX), u2i = read(nnzbX);
    CHECK(!in.fail());

    // the plan's pair list, by brute force
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> xAt;
    for (uint32_t x = uint32_t(nnzbX); x > 0; --x) xAt[{rowOfX[x - 1], colOfX[x - 1]}] = x - 1;       // of two blocks on one place the first
    std::vector<uint32_t> pairs;
    for (uint32_t y = 0; y < nnzbX; ++y)
        for (uint32_t q = 0; q < nnzbA; ++q) {
            if (rowOfA[q] != rowOfX[y]) continue;
            auto const hit = xAt.find({colOfA[q], colOfX[y]});
            if (hit != xAt.end()) { pairs.push_back(q); pairs.push_back(hit->second); }
        }
    size_t const nPairs = pairs.size() / 2;
    tfq::DropListing l;
    tfq::drop_listing(l, uint32_t(nnzbX), nPairs, pairs.data(), u2i.data());
    CHECK(l.built && l.start.size() == nnzbX + 1 && l.aOf.size() == nPairs && l.xOf == u2i);
    CHECK(0 == l.start[0] && l.start[nnzbX] == nPairs);
    for (uint32_t x = 0; x < nnzbX; ++x) {
        std::vector<uint32_t> want;
        for (size_t q = 0; q < nPairs; ++q) if (pairs[2 * q + 1] == x) want.push_back(pairs[2 * q]);
        CHECK(l.start[x] <= l.start[x + 1] && l.start[x + 1] - l.start[x] == want.size());
        CHECK(std::equal(want.begin(), want.end(), l.aOf.begin() + l.start[x]));
    }
    tfq::drop_listing(l, 0, 0, nullptr, nullptr);                   // nothing at all
    CHECK(l.built && l.start.size() == 1 && l.aOf.empty() && l.xOf.empty());

    int const off = 1;                                               // the caller's indices: 1-based, and not the compressed ones
    std::vector<int32_t> callersCol(nCols);
    for (uint32_t c = 0; c < nCols; ++c) callersCol[c] = int32_t(3 * c + 5 + off);
    std::vector<uint8_t> hasB(nnzbX, 0);                             // B: the first block of every block column
    {
        std::vector<uint8_t> seen(nCols, 0);
        for (uint32_t x = 0; x < nnzbX; ++x) if (!seen[colOfX[x]]) { seen[colOfX[x]] = 1; hasB[x] = 1; }
    }
    auto shrink = [&](tfq::GrownPattern& g, std::vector<int32_t> const& drop, bool null = false) {
        return tfq::shrink_pattern(g, uint32_t(nRows), uint32_t(nnzbX), rowOfX.data(), colOfX.data(), callersCol.data(), off, hasB.data(),
                                   drop.size(), null ? nullptr : drop.data());
    };
    std::vector<int32_t> freeBlocks, third, lastColumn;
    for (uint32_t x = 0; x < nnzbX; ++x) if (!hasB[x]) freeBlocks.push_back(int32_t(x));
    for (size_t p = freeBlocks.size(); p > 0; p = (p > 3 ? p - 3 : 0)) third.push_back(freeBlocks[p - 1]);
    for (uint32_t x = 0; x < nnzbX; ++x) if (colOfX[x] + 1 == nCols) lastColumn.push_back(int32_t(x));
    CHECK(!freeBlocks.empty() && !lastColumn.empty());
    tfq::GrownPattern g;
    CHECK(0 == shrink(g, {}, true) && !shrunk_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, {}));
    CHECK(0 == shrink(g, {freeBlocks[freeBlocks.size() / 2]}) && !shrunk_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, {freeBlocks[freeBlocks.size() / 2]}));
    CHECK(0 == shrink(g, third) && !shrunk_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, third));
    CHECK(0 == shrink(g, freeBlocks) && !shrunk_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, freeBlocks));
    size_t const smallest = g.colInd.size();
    CHECK(smallest == nCols);

    auto refused = [&](std::vector<int32_t> const& drop, int code) { return code == shrink(g, drop) && g.rowPtr.empty() && g.colInd.empty() && g.oldBlock.empty(); };
    CHECK(refused({int32_t(nnzbX)}, 1));
    CHECK(refused({-1}, 1));
    CHECK(refused({0x7fffffff}, 1));
    CHECK(refused({freeBlocks[0], freeBlocks[0]}, 1));
    CHECK(refused({freeBlocks.back(), freeBlocks[0], freeBlocks.back()}, 1));
    {
        std::vector<int32_t> tooMany(nnzbX + 1, 0);
        for (uint32_t x = 0; x < nnzbX; ++x) tooMany[x] = int32_t(x);
        CHECK(refused(tooMany, 1));
        tooMany.pop_back();
        CHECK(refused(tooMany, 2));                                  // every block: the ones with B are among them
    }
    CHECK(refused(lastColumn, 2));
    CHECK(refused({freeBlocks[0], lastColumn[0]}, 2));

    // a column without B loses all its blocks: it vanishes from the pattern (createPlan admits no such column; the plain function does)
    for (auto const x : lastColumn) hasB[x] = 0;
    CHECK(0 == shrink(g, lastColumn) && !shrunk_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, lastColumn));
    CHECK(g.colInd.end() == std::find(g.colInd.begin(), g.colInd.end(), callersCol[nCols - 1]));
    std::printf("%s: %zu products grouped by %llu blocks of X; shrunk by none, one, every third, all without B (%zu blocks left), a whole column: ok\n",
                path, nPairs, (unsigned long long)nnzbX, smallest);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <file> [<file> ...]\n", argv[0]); return 2; }
    for (int k = 1; k < argc; ++k) if (run(argv[k])) return 1;
    return 0;
}
