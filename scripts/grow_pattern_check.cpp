// The grown pattern (tfqmrgpu_amd/csrc/tfq_leak_host.cpp: grow_pattern, tfqmrgpu_ext.h section 12) as a stand-alone host program, for a
// sanitizer build:
//   grow_pattern_check <file> [<file> ...]         (scripts/check_sanitize.sh grow_pattern builds it with -fsanitize=address,undefined and runs it)
// The files are those of scripts/leak_listing_check.cpp (scripts/leak_listing_inputs.py writes them).  For every file the listing is
// built and the pattern grown by: no position, all (NULL list), all (as a list, backwards), every third position backwards; and refused
// for an index out of range, an index named twice, and more indices than positions.
// Checked: the counts; as a multiset the new pattern is the old one and the taken positions; every block row keeps its old blocks in
// their order, the added ones follow in ascending column; oldBlock numbers the old blocks 0, 1, 2, ...; a refusal leaves `out` empty.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <utility>

#include "tfq_plan.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("%s: FAILED %s (line %d)\n", path, #cond, __LINE__); return 1; } } while (0)

static int grown_ok(char const* path, tfq::GrownPattern const& g, uint32_t nRows, std::vector<uint32_t> const& rowOfX,
    std::vector<uint32_t> const& colOfX, std::vector<int32_t> const& callersCol, int off, tfq::LeakListing const& l,
    std::vector<uint64_t> const& taken)
{
    size_t const nnzbX = rowOfX.size(), nnzb = nnzbX + taken.size();
    CHECK(g.rowPtr.size() == size_t(nRows) + 1 && g.colInd.size() == nnzb && g.oldBlock.size() == nnzb);
    CHECK(g.rowPtr[0] == off && size_t(g.rowPtr[nRows] - off) == nnzb);
    std::vector<std::pair<uint32_t, int32_t>> want, got;
    for (size_t x = 0; x < nnzbX; ++x) want.push_back({rowOfX[x], callersCol[colOfX[x]]});
    for (auto const p : taken) want.push_back({l.posRow[p], callersCol[l.posCol[p]]});
    int32_t nextOld = 0;
    for (uint32_t r = 0; r < nRows; ++r) {
        CHECK(g.rowPtr[r] <= g.rowPtr[r + 1]);
        bool added = false;
        for (int32_t n = g.rowPtr[r] - off; n < g.rowPtr[r + 1] - off; ++n) {
            got.push_back({r, g.colInd[n]});
            if (g.oldBlock[n] >= 0) {
                CHECK(!added && g.oldBlock[n] == nextOld && rowOfX[nextOld] == r && g.colInd[n] == callersCol[colOfX[nextOld]]);
                ++nextOld;
            } else {
                CHECK(-1 == g.oldBlock[n]);
                if (added) CHECK(g.colInd[n - 1] < g.colInd[n]);
                added = true;
            }
        }
    }
    CHECK(size_t(nextOld) == nnzbX);
    std::sort(want.begin(), want.end()); std::sort(got.begin(), got.end());
    CHECK(want == got);
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
    std::vector<uint32_t> cscPtr, cscBlock;
    tfq::a_by_column(uint32_t(nRows), colOfA, cscPtr, cscBlock);
    tfq::LeakListing l;
    CHECK(tfq::leak_listing(l, uint32_t(nRows), uint32_t(nCols), uint32_t(nnzbA), rowOfA.data(), colOfA.data(), cscPtr.data(), cscBlock.data(),
                            uint32_t(nnzbX), rowOfX.data(), colOfX.data(), u2i.data(), uint32_t(maxProducts)));
    size_t const nPos = l.nPositions();
    CHECK(nPos == wantBlocks);
    int const off = 1;                                               // the caller's indices: 1-based, and not the compressed ones
    std::vector<int32_t> callersCol(nCols);
    for (uint32_t c = 0; c < nCols; ++c) callersCol[c] = int32_t(3 * c + 5 + off);

    auto grow = [&](tfq::GrownPattern& g, uint64_t nTake, uint64_t const* take) {
        return tfq::grow_pattern(g, uint32_t(nRows), uint32_t(nCols), uint32_t(nnzbX), rowOfX.data(), colOfX.data(), callersCol.data(), off,
                                 nPos, l.posRow.data(), l.posCol.data(), nTake, take);
    };
    std::vector<uint64_t> all(nPos), backwards, third;
    for (size_t p = 0; p < nPos; ++p) all[p] = p;
    backwards.assign(all.rbegin(), all.rend());
    for (size_t p = nPos; p > 0; p = (p > 3 ? p - 3 : 0)) third.push_back(p - 1);
    tfq::GrownPattern g;
    uint64_t const none = 0;
    CHECK(0 == grow(g, 0, &none) && !grown_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, l, {}));
    CHECK(0 == grow(g, 12345, nullptr) && !grown_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, l, all));
    CHECK(0 == grow(g, backwards.size(), backwards.data()) && !grown_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, l, all));
    CHECK(0 == grow(g, third.size(), third.data()) && !grown_ok(path, g, uint32_t(nRows), rowOfX, colOfX, callersCol, off, l, third));
    size_t const grownBlocks = g.colInd.size();
    auto refused = [&](std::vector<uint64_t> const& take) { return 1 == grow(g, take.size(), take.data()) && g.rowPtr.empty() && g.colInd.empty() && g.oldBlock.empty(); };
    CHECK(refused({uint64_t(nPos)}));
    CHECK(refused({~uint64_t(0)}));
    if (nPos) {
        CHECK(refused({0, 0}));
        CHECK(refused({uint64_t(nPos - 1), 0, uint64_t(nPos - 1)}));
        auto tooMany = all; tooMany.push_back(0);
        CHECK(refused(tooMany));
    }
    std::printf("%s: %zu leak positions; grown by none, all, every third (%zu blocks from %llu): ok\n", path, nPos, grownBlocks,
                (unsigned long long)nnzbX);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <file> [<file> ...]\n", argv[0]); return 2; }
    for (int k = 1; k < argc; ++k) if (run(argv[k])) return 1;
    return 0;
}
