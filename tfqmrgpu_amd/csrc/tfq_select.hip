// Selection on the device (tfqmrgpu_ext.h section 20): which blocks of X to drop, which leak positions to take.  The records are those of
// tfq_drop_cost.hip and tfq_leak_map.hip, bnorm2 that of tfq_residual.hip; nothing here forms a block product.  Not part of a solve: every
// kernel reads and writes memory that the library owns.
//   k_select_flag     one flag per item (a block of X in the caller's order, or a leak position) from its [LN] record and bnorm2 of its
//                     column, and the count of the flags of its tile.  2^k lanes share an item, so that a wave reads runs of whole records;
//                     16-byte loads where LN is even (records and bnorm2 rows then start on 16-byte boundaries)
//   k_select_scan     ONE work group turns the tile counts into exclusive prefix sums, 256 tiles per trip, and leaves the total
//   k_select_scatter  one work group per tile: the rank of a set flag inside its tile by a ballot per wave, its place = the tile's prefix + rank
//   k_select_sum      one work group per block column: the records of the column's items with the wanted flag, added per right-hand side
// The compaction is three plain passes on one stream -- count, scan, scatter.  No work group waits for another one: no look-back, no
// spinning, no atomics, no barrier across the grid.  The items are walked in ascending order, so the list ascends by construction.
// Every sum has one fixed order: two calls on the same data give the same bits.
#include <cassert>
#include <hip/hip_runtime.h>
#include "tfq_select.hpp"

namespace tfq {

struct SelFlagArgs {
    double const *rec, *bnorm2;
    uint32_t const* colOf;
    uint8_t* flag;
    uint32_t* tileCount;
    uint32_t nItems, bStride;
    int LN, lgLanes;                        // 2^lgLanes lanes share an item
    int leak;
    double eta2;
};

// the sum of v over the 64 lanes of the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += uint32_t(__shfl_xor(int(v), o, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_select_flag(SelFlagArgs a) {
    __shared__ uint32_t sWave[4];
    int const t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int const G = 1 << a.lgLanes, g = t & (G - 1);
    uint32_t const perRound = kSelTile >> a.lgLanes;
    uint32_t const tile0 = blockIdx.x * kSelTile;
    bool const pairs = (0 == (a.LN & 1));
    int const units = pairs ? a.LN / 2 : a.LN;          // loads per record
    bool const leak = (0 != a.leak);
    uint32_t count = 0;
    // (the trip count and the shuffles are the same for every lane; only the loads are predicated)
    for (int round = 0; round < G; ++round) {
        uint32_t const n = tile0 + uint32_t(round) * perRound + uint32_t(t >> a.lgLanes);
        bool const live = (n < a.nItems);
        uint32_t const c = live ? a.colOf[n] : kSelExcluded;
        bool hit = !leak;                               // drop: every j passes; leak: some j exceeds
        if (kSelExcluded == c) {
            hit = false;
        } else {
            double const* const r = a.rec + size_t(n) * a.LN;
            double const* const b = a.bnorm2 + size_t(c) * a.bStride;
            for (int u = g; u < units; u += G) {
                double r0, r1, b0, b1;
                if (pairs) {
                    double2 const rv = *reinterpret_cast<double2 const*>(r + 2 * u), bv = *reinterpret_cast<double2 const*>(b + 2 * u);
                    r0 = rv.x; r1 = rv.y; b0 = bv.x; b1 = bv.y;
                } else {
                    r0 = r[u]; b0 = b[u]; r1 = r0; b1 = b0;
                }
                double const lim0 = __dmul_rn(a.eta2, b0), lim1 = __dmul_rn(a.eta2, b1);
                if (leak) hit = hit || (b0 > 0 && r0 > lim0) || (b1 > 0 && r1 > lim1);
                else      hit = hit && (r0 <= lim0) && (r1 <= lim1);
            }
        }
        for (int o = G >> 1; o > 0; o >>= 1) {
            bool const other = (0 != __shfl_xor(int(hit), o, 64));
            hit = leak ? (hit || other) : (hit && other);
        }
        if (0 == g && live) { a.flag[n] = uint8_t(hit); count += uint32_t(hit); }
    }
    count = wave_sum(count);
    if (0 == lane) sWave[wave] = count;
    __syncthreads();
    if (0 == t) a.tileCount[blockIdx.x] = sWave[0] + sWave[1] + sWave[2] + sWave[3];
}

__global__ __launch_bounds__(256) void k_select_scan(uint32_t* tileCount, uint32_t nTiles) {
    __shared__ uint32_t sWave[4];
    int const t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t carry = 0;                                 // the same in every thread
    for (uint32_t base = 0; base < nTiles; base += 256) {
        uint32_t const i = base + uint32_t(t);
        uint32_t const v = (i < nTiles) ? tileCount[i] : 0u;
        uint32_t x = v;                                 // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            uint32_t const y = uint32_t(__shfl_up(int(x), o, 64));
            if (lane >= o) x += y;
        }
        if (63 == lane) sWave[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) before += sWave[w]; all += sWave[w]; }
        if (i < nTiles) tileCount[i] = carry + before + x - v;
        carry += all;
        __syncthreads();                                // sWave is written again in the next trip
    }
    if (0 == t) tileCount[nTiles] = carry;
}

__global__ __launch_bounds__(256) void k_select_scatter(uint8_t const* flag, uint32_t const* tileOffset, uint32_t nItems, uint32_t* list) {
    __shared__ uint32_t sWave[4];
    int const t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t const n = blockIdx.x * kSelTile + uint32_t(t);
    bool const set = (n < nItems) && (0 != flag[n]);
    uint64_t const ballot = __ballot(set);
    if (0 == lane) sWave[wave] = uint32_t(__popcll(ballot));
    __syncthreads();
    if (set) {
        uint32_t at = tileOffset[blockIdx.x] + uint32_t(__popcll(ballot & ((uint64_t(1) << lane) - 1)));
        for (int w = 0; w < wave; ++w) at += sWave[w];
        list[at] = n;                                   // at < the total <= nItems
    }
}

struct SelSumArgs {
    double const* rec;
    uint8_t const* flag;
    uint32_t const *start, *order;
    double* out;
    int LN, keep, root;
};

// Lane t has right-hand side t % LN and is number t / LN of the 256 / LN lanes of that right-hand side: it adds the entries t / LN,
// t / LN + 256 / LN, ... of the column in that order; the lanes of a right-hand side are then added in ascending number
// (LN <= 256, which select_sum_launch asserts: with more right-hand sides than lanes R would be 0 and nothing would be added)
__global__ __launch_bounds__(256) void k_select_sum(SelSumArgs a) {
    __shared__ double s[256];
    int const t = threadIdx.x, LN = a.LN, R = 256 / LN, j = t % LN, r = t / LN;
    uint32_t const c = blockIdx.x, i0 = a.start[c], i1 = a.start[c + 1];
    if (r < R) {
        double acc = 0;
        for (uint32_t i = i0 + uint32_t(r); i < i1; i += uint32_t(R)) {
            uint32_t const n = a.order ? a.order[i] : i;
            if (int(a.flag[n]) == a.keep) {
                double const v = a.rec[size_t(n) * LN + j];
                acc += a.root ? sqrt(v) : v;
            }
        }
        s[j * R + r] = acc;
    }
    __syncthreads();
    if (t < LN) {
        double sum = 0;
#pragma unroll 1
        for (int q = 0; q < R; ++q) sum += s[t * R + q];
        a.out[size_t(c) * LN + t] = sum;
    }
}

void select_flag_launch(uint32_t nItems, int LN, double const* rec, double const* bnorm2, uint32_t bStride, uint32_t const* colOf,
    double eta2, bool leak, uint8_t* flag, uint32_t* tileCount, hipStream_t s)
{
    if (0 == nItems) return;
    int const units = (LN % 2) ? LN : LN / 2;
    int lg = 0;
    while (lg < 4 && (2 << lg) <= units) ++lg;          // the largest power of two <= min(16, units)
    SelFlagArgs a{};
    a.rec = rec; a.bnorm2 = bnorm2; a.colOf = colOf; a.flag = flag; a.tileCount = tileCount;
    a.nItems = nItems; a.bStride = bStride; a.LN = LN; a.lgLanes = lg; a.leak = leak ? 1 : 0; a.eta2 = eta2;
    k_select_flag<<<dim3(select_tiles(nItems)), dim3(256), 0, s>>>(a);
}

void select_compact_launch(uint32_t nItems, uint8_t const* flag, uint32_t* tileCount, uint32_t* list, hipStream_t s) {
    if (0 == nItems) return;
    uint32_t const nTiles = select_tiles(nItems);
    k_select_scan<<<dim3(1), dim3(256), 0, s>>>(tileCount, nTiles);
    k_select_scatter<<<dim3(nTiles), dim3(256), 0, s>>>(flag, tileCount, nItems, list);
}

void select_sum_launch(uint32_t nCols, int LN, double const* rec, uint8_t const* flag, uint32_t const* start, uint32_t const* order,
    bool keep, bool root, double* out, hipStream_t s)
{
    if (0 == nCols) return;
    assert(LN >= 1 && LN <= 256);                       // one lane per right-hand side at least (k_select_sum: R = 256 / LN >= 1); the listed shapes end at 64
    SelSumArgs a{};
    a.rec = rec; a.flag = flag; a.start = start; a.order = order; a.out = out;
    a.LN = LN; a.keep = keep ? 1 : 0; a.root = root ? 1 : 0;
    k_select_sum<<<dim3(nCols), dim3(256), 0, s>>>(a);
}

} // namespace tfq
