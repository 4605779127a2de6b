// The block map of tfqmrgpuExt_carry (tfqmrgpu_amd/csrc/tfq_carry_host.cpp: carry_map_ok, carry_compose; tfqmrgpu_ext.h section 15) as a
// stand-alone host program, for a sanitizer build:
//   carry_map_check <file> [<file> ...]            (scripts/check_sanitize.sh carry_map builds it with -fsanitize=address,undefined and runs it)
// The files are those of scripts/leak_listing_check.cpp (scripts/leak_listing_inputs.py writes them).  For every file the source plan is
// the file's pattern of X with its internal order (u2i); the destination is that pattern grown by all leak positions (grow_pattern, so the
// map has -1 entries), by none, and a destination of arbitrary size whose map is random with repeats and -1 entries, and all -1.
// Checked: the composed list against the definition, entry by entry, through the internal orders of BOTH plans (X) and in the caller's
// order (A, B); the identity without a list; and that carry_map_ok refuses a wrong block count, a missing list with unequal counts,
// entries below -1 and entries at or above the source's count -- and accepts every map that is composed here.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>

#include "tfq_plan.hpp"

#define CHECK(cond) do { if (!(cond)) { std::printf("%s: FAILED %s (line %d)\n", path, #cond, __LINE__); return 1; } } while (0)

// the internal order of a pattern: by (column, row), stable -- what Plan::i2u holds
static std::vector<uint32_t> internal_order(std::vector<uint32_t> const& row, std::vector<int32_t> const& col) {
    std::vector<uint32_t> i2u(row.size());
    std::iota(i2u.begin(), i2u.end(), 0u);
    std::stable_sort(i2u.begin(), i2u.end(), [&](uint32_t a, uint32_t b) { return col[a] != col[b] ? col[a] < col[b] : row[a] < row[b]; });
    return i2u;
}

static int composed_ok(char const* path, std::vector<int32_t> const& map, bool useList, std::vector<uint32_t> const& dstI2U,
    std::vector<uint32_t> const& srcU2I, bool xShaped)
{
    uint32_t const nDst = uint32_t(dstI2U.size()), nSrc = uint32_t(srcU2I.size());
    CHECK(tfq::carry_map_ok(int64_t(nDst), useList ? map.data() : nullptr, nDst, nSrc));
    std::vector<uint32_t> out(3, 12345u);                            // (whatever was in it goes)
    tfq::carry_compose(out, nDst, useList ? map.data() : nullptr, xShaped ? dstI2U.data() : nullptr, xShaped ? srcU2I.data() : nullptr);
    CHECK(out.size() == nDst);
    for (uint32_t n = 0; n < nDst; ++n) {
        uint32_t const u = xShaped ? dstI2U[n] : n;
        int32_t const o = useList ? map[u] : int32_t(u);
        uint32_t const want = (o < 0) ? tfq::kCarryZero : (xShaped ? srcU2I[o] : uint32_t(o));
        CHECK(out[n] == want);
        CHECK(tfq::kCarryZero == out[n] || out[n] < nSrc);
    }
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
    uint32_t const nSrc = uint32_t(nnzbX);

    // the destination patterns: grown by every leak position, and by none
    std::vector<uint32_t> cscPtr, cscBlock;
    tfq::a_by_column(uint32_t(nRows), colOfA, cscPtr, cscBlock);
    tfq::LeakListing l;
    CHECK(tfq::leak_listing(l, uint32_t(nRows), uint32_t(nCols), uint32_t(nnzbA), rowOfA.data(), colOfA.data(), cscPtr.data(), cscBlock.data(),
                            nSrc, rowOfX.data(), colOfX.data(), u2i.data(), uint32_t(maxProducts)));
    std::vector<int32_t> callersCol(nCols);
    for (uint32_t c = 0; c < nCols; ++c) callersCol[c] = int32_t(3 * c + 5);
    size_t added = 0;
    for (int all = 0; all < 2; ++all) {
        tfq::GrownPattern g;
        uint64_t const none = 0;
        CHECK(0 == tfq::grow_pattern(g, uint32_t(nRows), uint32_t(nCols), nSrc, rowOfX.data(), colOfX.data(), callersCol.data(), 0,
                                     l.nPositions(), l.posRow.data(), l.posCol.data(), 0, all ? nullptr : &none));
        std::vector<uint32_t> row(g.colInd.size());
        for (uint32_t r = 0; r < nRows; ++r) for (int32_t n = g.rowPtr[r]; n < g.rowPtr[r + 1]; ++n) row[n] = r;
        auto const dstI2U = internal_order(row, g.colInd);
        if (all) added = g.colInd.size() - nSrc;
        CHECK(!composed_ok(path, g.oldBlock, true, dstI2U, u2i, true));
        CHECK(!composed_ok(path, g.oldBlock, true, dstI2U, u2i, false));
        if (!all) CHECK(!composed_ok(path, g.oldBlock, false, dstI2U, u2i, true));   // the same pattern: the identity without a list
        // the grown pattern back onto the old one: every old block from its new place (a shrunk pattern's map)
        if (all) {
            std::vector<int32_t> back(nSrc, -1);
            for (size_t n = 0; n < g.oldBlock.size(); ++n) if (g.oldBlock[n] >= 0) back[g.oldBlock[n]] = int32_t(n);
            std::vector<uint32_t> grownU2I(dstI2U.size());
            for (uint32_t i = 0; i < dstI2U.size(); ++i) grownU2I[dstI2U[i]] = i;
            std::vector<uint32_t> srcI2U(nSrc);
            for (uint32_t u = 0; u < nSrc; ++u) srcI2U[u2i[u]] = u;
            for (auto const b : back) CHECK(b >= 0);
            // (here the file's pattern is the destination and the grown one the source)
            uint32_t const nDst = nSrc;
            CHECK(tfq::carry_map_ok(nDst, back.data(), nDst, uint32_t(grownU2I.size())));
            std::vector<uint32_t> out;
            tfq::carry_compose(out, nDst, back.data(), srcI2U.data(), grownU2I.data());
            for (uint32_t n = 0; n < nDst; ++n) CHECK(out[n] == grownU2I[back[srcI2U[n]]]);
        }
    }

    // a destination of another size: random entries with repeats and zero blocks; all zero blocks
    uint32_t const nDst = nSrc / 2 + 7;
    std::vector<uint32_t> dstI2U(nDst);
    std::iota(dstI2U.begin(), dstI2U.end(), 0u);
    uint32_t seed = 12345u + nSrc;
    auto next = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    for (uint32_t n = nDst; n > 1; --n) std::swap(dstI2U[n - 1], dstI2U[next() % n]);
    std::vector<int32_t> map(nDst);
    for (auto& m : map) { uint32_t const v = next() % (nSrc + 3); m = (v >= nSrc) ? -1 : int32_t(v); }
    CHECK(!composed_ok(path, map, true, dstI2U, u2i, true));
    CHECK(!composed_ok(path, map, true, dstI2U, u2i, false));
    std::vector<int32_t> const zeros(nDst, -1);
    CHECK(!composed_ok(path, zeros, true, dstI2U, u2i, true));

    // refusals
    CHECK(!tfq::carry_map_ok(int64_t(nDst) - 1, map.data(), nDst, nSrc));
    CHECK(!tfq::carry_map_ok(int64_t(nDst) + 1, map.data(), nDst, nSrc));
    CHECK(!tfq::carry_map_ok(-1, map.data(), nDst, nSrc));
    CHECK(!tfq::carry_map_ok(0, map.data(), nDst, nSrc));
    CHECK(tfq::carry_map_ok(0, nullptr, 0, 0) && tfq::carry_map_ok(0, map.data(), 0, nSrc));
    CHECK(!tfq::carry_map_ok(nDst, nullptr, nDst, nSrc));             // no list: the counts differ
    CHECK(tfq::carry_map_ok(nSrc, nullptr, nSrc, nSrc));
    for (int32_t const bad : {int32_t(nSrc), int32_t(nSrc) + 1, -2, INT_MIN, INT_MAX}) {
        for (uint32_t const at : {0u, nDst / 2, nDst - 1}) {
            auto m = map;
            m[at] = bad;
            CHECK(!tfq::carry_map_ok(nDst, m.data(), nDst, nSrc));
        }
    }
    std::printf("%s: %u source blocks; grown by %zu, the same pattern, back again, %u random entries: ok\n", path, nSrc, added, nDst);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <file> [<file> ...]\n", argv[0]); return 2; }
    for (int k = 1; k < argc; ++k) if (run(argv[k])) return 1;
    return 0;
}
