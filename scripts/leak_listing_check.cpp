// The leak listing (tfqmrgpu_amd/csrc/tfq_leak_host.cpp, tfqmrgpu_ext.h section 11) as a stand-alone host program, for a sanitizer build:
//   leak_listing_check <file> [<file> ...]         (scripts/check_sanitize.sh leak_listing builds it with -fsanitize=address,undefined and runs it)
// A file holds plain index arrays, all zero based, white-space separated (scripts/leak_listing_inputs.py writes them):
//   nRows nCols nnzbA nnzbX maxProducts expectedLeakBlocks expectedLeakPairs
//   rowOfA[nnzbA]  colOfA[nnzbA]  rowOfX[nnzbX]  colOfX[nnzbX] (compressed)  u2i[nnzbX]
// Checked: positions strictly ascending by (column, row) and none inside the pattern of X; every product's A block lies in the position's
// row, its X block in the position's column and in the A block's column, ascending inside a position; the work units tile the
// positions, none spans two columns, none with more than one position exceeds maxProducts; the counts are the expected ones.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <utility>

#include "tfq_plan.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("%s: FAILED %s (line %d)\n", path, #cond, __LINE__); return 1; } } while (0)

static int run(char const* path) {
    std::ifstream in(path);
    CHECK(in.good());
    uint64_t nRows, nCols, nnzbA, nnzbX, maxProducts, wantBlocks, wantPairs;
    in >> nRows >> nCols >> nnzbA >> nnzbX >> maxProducts >> wantBlocks >> wantPairs;
    auto read = [&](size_t n) { std::vector<uint32_t> v(n); for (auto& x : v) in >> x; return v; };
    auto const rowOfA = read(nnzbA), colOfA = read(nnzbA), rowOfX = read(nnzbX), colOfX = read(nnzbX), u2i = read(nnzbX);
    CHECK(!in.fail());
    std::vector<uint32_t> cscPtr, cscBlock;
    tfq::a_by_column(uint32_t(nRows), colOfA, cscPtr, cscBlock);
    tfq::LeakListing l;
    CHECK(tfq::leak_listing(l, uint32_t(nRows), uint32_t(nCols), uint32_t(nnzbA), rowOfA.data(), colOfA.data(), cscPtr.data(), cscBlock.data(),
                            uint32_t(nnzbX), rowOfX.data(), colOfX.data(), u2i.data(), uint32_t(maxProducts)));
    CHECK(l.built && l.nPositions() == wantBlocks && l.nProducts() == wantPairs);

    std::set<std::pair<uint32_t, uint32_t>> pattern;                 // (row, column) of X
    std::vector<uint32_t> i2u(nnzbX);
    for (uint32_t x = 0; x < nnzbX; ++x) { pattern.insert({rowOfX[x], colOfX[x]}); CHECK(u2i[x] < nnzbX); i2u[u2i[x]] = x; }
    size_t const nPos = l.nPositions();
    CHECK(l.posStart.size() == nPos + 1 && l.posRow.size() == nPos && 0 == l.posStart[0] && l.posStart[nPos] == l.nProducts());
    for (size_t n = 0; n < nPos; ++n) {
        uint32_t const c = l.posCol[n], i = l.posRow[n];
        CHECK(c < nCols && i < nRows && 0 == pattern.count({i, c}));
        if (n) CHECK(l.posCol[n - 1] < c || (l.posCol[n - 1] == c && l.posRow[n - 1] < i));
        CHECK(l.posStart[n] < l.posStart[n + 1]);
        for (uint32_t q = l.posStart[n]; q < l.posStart[n + 1]; ++q) {
            uint32_t const a = l.pairs[2 * size_t(q)], xi = l.pairs[2 * size_t(q) + 1];
            CHECK(a < nnzbA && xi < nnzbX);
            uint32_t const x = i2u[xi];
            CHECK(rowOfA[a] == i && colOfX[x] == c && rowOfX[x] == colOfA[a]);
            if (q > l.posStart[n]) CHECK(colOfA[l.pairs[2 * size_t(q) - 2]] <= colOfA[a]);
        }
    }
    size_t const nUnits = l.nUnits();
    CHECK(l.unitFirst.size() == nUnits + 1 && l.unitFirst[nUnits] == nPos && l.colUnitPtr.size() == nCols + 1 && l.colUnitPtr[nCols] == nUnits);
    CHECK(0 == nUnits || 0 == l.unitFirst[0]);
    for (uint32_t c = 0; c < nCols; ++c) {
        CHECK(l.colUnitPtr[c] <= l.colUnitPtr[c + 1]);
        for (uint32_t u = l.colUnitPtr[c]; u < l.colUnitPtr[c + 1]; ++u) {
            uint32_t const p0 = l.unitFirst[u], p1 = l.unitFirst[u + 1];
            CHECK(p0 < p1 && p1 <= nPos);
            for (uint32_t n = p0; n < p1; ++n) CHECK(l.posCol[n] == c);
            CHECK(p1 - p0 == 1 || l.posStart[p1] - l.posStart[p0] <= maxProducts);
        }
    }
    std::printf("%s: %zu leak positions, %zu products, %zu work units of at most %llu products: ok\n", path, nPos, l.nProducts(), nUnits,
                (unsigned long long)maxProducts);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <file> [<file> ...]\n", argv[0]); return 2; }
    for (int k = 1; k < argc; ++k) if (run(argv[k])) return 1;
    return 0;
}
