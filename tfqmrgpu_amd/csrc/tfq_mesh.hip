// Energy mesh on the device (tfqmrgpu_ext.h section 19): the kernels of tfqmrgpuExt_shiftDiagonal and tfqmrgpuExt_addToSum.
//   k_diag_capture<R>      base[r][i] := A_rr(i, i)                         one thread per diagonal element, mb * lm threads (or of the listed rows)
//   k_diag_shift<RB, RT>   A_rr(i, i) := RT(base[r][i] + sigma)             the same traversal, writing
//   k_sum_add<R>           S[b](r, s) += w * X[subset[b]](r, s)             one thread per complex element of the nnzbB blocks
// A block of A is stored transposed, which its diagonal does not notice; where element (i, i) lies inside a stored block is plane_offset
// (tfq_device.hpp), the helper of k_convert.  Elementwise, memory bound and tiny next to a solve: plain loads and stores, no LDS, no
// atomics, no barrier.  Every arithmetic operation here is ONE rounding that a host restatement can repeat: nothing may be contracted.
#include "tfq_mesh.hpp"

namespace tfq {
namespace {

template <typename R>
__global__ __launch_bounds__(256) void k_diag_capture(R const* A, R* base, uint32_t const* diagOfRow, uint32_t const* rows, uint32_t nListed,
    int LM, int lm, int ilv)
{
    uint32_t const idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= nListed * uint32_t(lm)) return;
    uint32_t const k = idx / uint32_t(lm); int const i = int(idx % uint32_t(lm));
    uint32_t const r = rows ? rows[k] : k;          // (the host lists block rows of the plan only)
    uint32_t const q = diagOfRow[r];
    if (~0u == q) return;                           // (the host has refused such a pattern)
    size_t const P = size_t(LM) * LM;
    R const* const block = A + size_t(q) * 2 * P + plane_offset(ilv, i, i, LM);
    R* const out = base + (size_t(r) * LM + i) * 2;
    out[0] = block[0]; out[1] = block[P];
}

__device__ inline double add_rn(double a, double b) { return __dadd_rn(a, b); }
__device__ inline float  add_rn(float a, float b)   { return __fadd_rn(a, b); }

template <typename RB, typename RT>   // RB: the base's real type, in which the sum is formed; RT: the stored type
__global__ __launch_bounds__(256) void k_diag_shift(RT* A, RB const* base, uint32_t const* diagOfRow, uint32_t mb, int LM, int lm, int ilv,
    RB sigmaRe, RB sigmaIm)
{
    uint32_t const idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= mb * uint32_t(lm)) return;
    uint32_t const r = idx / uint32_t(lm); int const i = int(idx % uint32_t(lm));
    uint32_t const q = diagOfRow[r];
    if (~0u == q) return;
    size_t const P = size_t(LM) * LM;
    RT* const block = A + size_t(q) * 2 * P + plane_offset(ilv, i, i, LM);
    RB const* const in = base + (size_t(r) * LM + i) * 2;
    block[0] = RT(add_rn(in[0], sigmaRe));          // (double -> float: round to nearest, once, as k_convert<float, double> does)
    block[P] = RT(add_rn(in[1], sigmaIm));
}

template <typename R>
__global__ __launch_bounds__(256) void k_sum_add(R const* x, uint32_t const* subset, double* sum, uint64_t total, int LM, int LN, int ilv,
    double wRe, double wIm)
{
#pragma clang fp contract(off)
    uint64_t const idx = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    if (idx >= total) return;
    uint32_t const P = uint32_t(LM) * uint32_t(LN);
    uint32_t const b = uint32_t(idx / P), e = uint32_t(idx - uint64_t(b) * P);
    int const r = int(e / uint32_t(LN)), s = int(e % uint32_t(LN));
    R const* const block = x + size_t(subset[b]) * 2 * P + plane_offset(ilv, r, s, LN);
    double const xRe = double(block[0]), xIm = double(block[P]);
    double* const S = sum + idx * 2;
    // __dmul_rn, __dadd_rn and __dsub_rn of the compiler's header are the plain operators compiled under ITS contraction setting: two of
    // the four products came out as v_fma_f64 with them.  The plain operators under the pragma above are the four v_mul_f64 and four
    // v_add_f64 that the section names
    double const t1 = wRe * xRe, t2 = wIm * xIm;
    double const t3 = wRe * xIm, t4 = wIm * xRe;
    double const dRe = t1 - t2, dIm = t3 + t4;
    S[0] = S[0] + dRe;
    S[1] = S[1] + dIm;
}

inline dim3 groups_of(uint64_t threads) { return dim3(uint32_t((threads + 255) / 256)); }

} // namespace

void diag_capture_launch(DiagSide const& from, void* base, uint32_t const* diagOfRow, uint32_t const* rows, uint32_t nListed, int LM, int lm,
                         hipStream_t s)
{
    uint64_t const n = uint64_t(nListed) * uint32_t(lm);
    if (0 == n) return;
    if (from.dbl) k_diag_capture<double><<<groups_of(n), dim3(256), 0, s>>>((double const*)from.a, (double*)base, diagOfRow, rows, nListed, LM, lm, from.ilv);
    else          k_diag_capture<float><<<groups_of(n), dim3(256), 0, s>>>((float const*)from.a, (float*)base, diagOfRow, rows, nListed, LM, lm, from.ilv);
}

void diag_shift_launch(DiagSide const& to, void const* base, bool baseDbl, uint32_t const* diagOfRow, uint32_t mb, int LM, int lm,
                       double sigmaRe, double sigmaIm, hipStream_t s)
{
    uint64_t const n = uint64_t(mb) * uint32_t(lm);
    if (0 == n) return;
    dim3 const g = groups_of(n), b(256);
    if (baseDbl) {
        if (to.dbl) k_diag_shift<double, double><<<g, b, 0, s>>>((double*)to.a, (double const*)base, diagOfRow, mb, LM, lm, to.ilv, sigmaRe, sigmaIm);
        else        k_diag_shift<double, float><<<g, b, 0, s>>>((float*)to.a, (double const*)base, diagOfRow, mb, LM, lm, to.ilv, sigmaRe, sigmaIm);
    } else {        // a float base belongs to a float A ('c'): sigma is rounded to float here, once
        k_diag_shift<float, float><<<g, b, 0, s>>>((float*)to.a, (float const*)base, diagOfRow, mb, LM, lm, to.ilv, float(sigmaRe), float(sigmaIm));
    }
}

bool sum_add_launch(DevPlan const& d, double* sum, double wRe, double wIm, hipStream_t s) {
    uint64_t const total = uint64_t(d.nnzbB) * uint32_t(d.LM) * uint32_t(d.LN);
    if (0 == total) return true;
    if ((total + 255) / 256 > 0x7fffffffull) return false;
    if (d.dbl) k_sum_add<double><<<groups_of(total), dim3(256), 0, s>>>((double const*)d.x, d.subset, sum, total, d.LM, d.LN, d.ilv, wRe, wIm);
    else       k_sum_add<float><<<groups_of(total), dim3(256), 0, s>>>((float const*)d.x, d.subset, sum, total, d.LM, d.LN, d.ilv, wRe, wIm);
    return true;
}

} // namespace tfq
