// Carry an operand from one plan to another on the device (tfqmrgpu_ext.h section 15, tfqmrgpuExt_carry): one kernel family,
//   k_carry<Tsrc, Tdst, REMAP>   stored block n of the destination := stored block list[n] of the source, or zeros
// The grid runs over the DESTINATION window in spans of 16 KiB (the size of a chunk): a work group of 256 lanes makes four trips, every
// lane writes 16 bytes per trip, so the stores are sequential and coalesced whatever the block shape -- a 4 x 4 float block is 128 bytes
// and a span holds 128 of them, a 64 x 64 double block is four spans.  Every block is a multiple of 16 bytes and every window starts on
// a 256-byte boundary, so the lane pattern is the same for all shapes and for A (LM x LM) as for B and X (LM x LN).
//   REMAP = false (same storage type, same element order): the 16 bytes are the source block's 16 bytes at the same place, non-temporal
//     both ways -- each byte is read once and written once.
//   REMAP = true: the lane forms its 16 bytes (2 doubles | 4 floats) element by element: the destination's element order says which
//     (plane, row, column) each one is, the source's order where that lies in the source block (tfq_device.hpp: ilv_offset); float -> double
//     is exact, double -> float rounds to nearest, once.  The source reads are plain loads: the 4 or 8 bytes a lane takes share their
//     cache line with the lanes around it, which the first-level cache serves; the stores are the same 16-byte non-temporal ones.
// The four loads of a lane are issued before its four stores.  No LDS, no atomics, no barrier; the list is read through the caches
// (consecutive lanes read the same entry).
#include "tfq_device.hpp"
#include "tfq_carry.hpp"

namespace tfq {
namespace {

constexpr uint32_t kCarryLanes = 256, kCarryTrips = 4;
constexpr uint32_t kCarrySpan = kCarryLanes * kCarryTrips;       // 16-byte pieces per work group: 16 KiB

struct CarryArgs {
    void* dst; void const* src; uint32_t const* list;
    uint32_t nBlocks;
    uint32_t piecesDst;          // 16-byte pieces per block of the destination
    int nR, nC, ilvDst, ilvSrc;
};

template <typename T> struct Piece;
template <> struct Piece<double> { static constexpr int N = 2; using V = double __attribute__((ext_vector_type(2))); };
template <> struct Piece<float>  { static constexpr int N = 4; using V = float  __attribute__((ext_vector_type(4))); };

// (row, column) of element q of a block plane in element order ilv: the inverse of plane_offset
__device__ inline void plane_position(int ilv, int q, int nC, int& r, int& s) {
    if (0 == ilv) { r = q / nC; s = q % nC; return; }
    int const t = q / ilv;
    s = t % nC; r = (t / nC) * ilv + q % ilv;
}

template <typename Ts, typename Td, bool REMAP>
__global__ __launch_bounds__(256) void k_carry(CarryArgs a) {
    using VD = typename Piece<Td>::V;
    constexpr int K = Piece<Td>::N;
    static_assert(REMAP || sizeof(Ts) == sizeof(Td), "a plain copy keeps the storage type");
    uint64_t const total = uint64_t(a.nBlocks) * a.piecesDst;       // pieces of the destination window
    uint64_t const base = uint64_t(blockIdx.x) * kCarrySpan;
    uint64_t const block0 = base / a.piecesDst;                     // uniform: once per work group
    uint32_t const rem0 = uint32_t(base - block0 * a.piecesDst);
    int const P = a.nR * a.nC;                                      // elements of one plane
    VD v[kCarryTrips];
#pragma unroll
    for (uint32_t trip = 0; trip < kCarryTrips; ++trip) {
        uint32_t const l = trip * kCarryLanes + threadIdx.x;
        VD z; for (int k = 0; k < K; ++k) z[k] = Td(0);
        v[trip] = z;
        if (base + l >= total) continue;
        uint32_t const q = rem0 + l, db = q / a.piecesDst, within = q - db * a.piecesDst;
        uint32_t const sb = a.list ? a.list[block0 + db] : uint32_t(block0 + db);
        if (kCarryZero == sb) continue;
        if constexpr (!REMAP) {
            VD const* const from = reinterpret_cast<VD const*>(a.src) + (uint64_t(sb) * a.piecesDst + within);
            v[trip] = __builtin_nontemporal_load(from);
        } else {
            Ts const* const from = reinterpret_cast<Ts const*>(a.src) + uint64_t(sb) * 2 * P;
            int const e0 = int(within) * K;                         // the lane's first element of the destination block
            int const plane = (e0 >= P) ? 1 : 0;                    // (a plane is a multiple of 16 bytes: a piece lies in one)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                int r, s;
                plane_position(a.ilvDst, e0 - plane * P + k, a.nC, r, s);
                v[trip][k] = Td(from[plane * P + plane_offset(a.ilvSrc, r, s, a.nC)]);
            }
        }
    }
    VD* const to = reinterpret_cast<VD*>(a.dst) + base;
#pragma unroll
    for (uint32_t trip = 0; trip < kCarryTrips; ++trip) {
        uint32_t const l = trip * kCarryLanes + threadIdx.x;
        if (base + l < total) __builtin_nontemporal_store(v[trip], to + l);
    }
}

} // namespace

bool carry_launch(CarrySide const& dst, CarrySide const& src, uint32_t const* list, uint32_t nBlocks, int nR, int nC, hipStream_t s) {
    if (0 == nBlocks) return true;
    CarryArgs a{};
    a.dst = dst.data; a.src = src.data; a.list = list; a.nBlocks = nBlocks;
    a.piecesDst = uint32_t(size_t(2) * nR * nC * (dst.dbl ? 8 : 4) / 16);
    a.nR = nR; a.nC = nC; a.ilvDst = dst.ilv; a.ilvSrc = src.ilv;
    uint64_t const groups = (uint64_t(nBlocks) * a.piecesDst + kCarrySpan - 1) / kCarrySpan;
    if (groups > 0x7fffffffull) return false;
    dim3 const g{uint32_t(groups)}, b{kCarryLanes};
    bool const remap = (dst.dbl != src.dbl) || (dst.ilv != src.ilv);
    if (!remap) {
        if (dst.dbl) k_carry<double, double, false><<<g, b, 0, s>>>(a);
        else         k_carry<float, float, false><<<g, b, 0, s>>>(a);
    } else if (dst.dbl) {
        if (src.dbl) k_carry<double, double, true><<<g, b, 0, s>>>(a);
        else         k_carry<float, double, true><<<g, b, 0, s>>>(a);
    } else {
        if (src.dbl) k_carry<double, float, true><<<g, b, 0, s>>>(a);
        else         k_carry<float, float, true><<<g, b, 0, s>>>(a);
    }
    return true;
}

} // namespace tfq
