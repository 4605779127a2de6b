// internal launch interface of the vector / column kernels (tfq_vec.hip), the multiply (tfq_spmm.hip, tfq_spmm.hpp), the grading kernels
// (tfq_residual.hip, tfq_leak.hip, tfq_leak_map.hip, tfq_drop_cost.hip, tfq_select.hip; device helpers tfq_grade.hpp, host side tfq_grade_host.cpp) and the warm start
// (tfq_warm.hip).  Device pieces that the chunk-streaming kernels share: tfq_stream.hpp; column operations and the set-up of a solve: tfq_colops.hpp
#pragma once
#include "tfq_device.hpp"

namespace tfq {

enum {
    VEC_SETUP = 0,     // clear vectors, v5 := B, tau := |b|^2, rho := 1, pz <- v3.v5
    VEC_DEC35,         // beta, rho from pz
    VEC_XPAY_V6,       // v6 := v5 + beta v6
    VEC_DEC34,         // alfa, c67 from pz
    VEC_V5_NRM,        // v5 += alfa v9 ; pd <- |v5|^2   (DevPlan::lateV5: the sum alone, the second fused multiply stores v5)
    VEC_DECT_C67,      // tau, var, eta, c67 from pd
    VEC_X_V6_V7,       // [x += eta2 v7] ; v7 := v6 + c67a v7 ; x += eta v7 ; v6 += alfa v4 ; v7 := v6 + c67 v7
    VEC_DECT_FIN,      // tau, var, eta from pd + per-column stopping record
    VEC_X_FLUSH,       // x += eta2 v7, only in front of a residual probe
    VEC_PROBE_COL      // per-column residual record from pd
};

hipError_t vec_launch(int op, DevPlan const& d, double tol, int maxIt, hipStream_t s);   // the runtime call of VEC_SETUP may fail

// Y = A*X over the plan's pair list with a fused epilogue (EPI_* in tfq_device.hpp)
void spmm_launch(int epi, DevPlan const& d, hipStream_t s);

// the kernel family spmm_launch runs for this plan (tfqmrgpuExt_getMultiplyKernel)
char const* spmm_kernel_family(DevPlan const& d);
// whether the second fused multiply of this plan runs on the kernel that can take k_v5_nrm's half step (one condition of tfq_solve.hpp: late_v5)
bool spmm_late_v5(DevPlan const& d);

// Y = A*X on two X-shaped vectors of the plan, no epilogue (tfqmrgpuExt_applyOperator)
void spmm_apply(DevPlan const& d, void const* X, void* Y, hipStream_t s);

// the epilogue of spmm_launch alone, for a product Y that a user-defined operator has already written:
// Yext holds the blocks in the caller's order, i2u[internal block] = caller's block
void epilogue_launch(int epi, DevPlan const& d, void const* Yext, uint32_t const* i2u, hipStream_t s);

// |B - A X|^2 and |B|^2 per (block column, right-hand side) of the plan's X and B and the operator A (the plan's storage type, block and
// element order; d.A is NOT read), every product and sum in double (tfq_residual.hip; tfqmrgpuExt_residual).
// rec [nChunks][2][LN] and col [nCols][2][LN] (the result) are the caller's scratch; nothing else is written
void residual_launch(DevPlan const& d, void const* A, double* rec, double* col, hipStream_t s);

// |.|^2 per (block column, right-hand side) of the block products of the leak listing (tfq_plan.hpp: LeakListing; all four lists in device
// memory) of the plan's X and the operator A, as above (tfq_leak.hip; tfqmrgpuExt_truncationLeak).
// rec [nUnits][LN] and col [nCols][LN] (the result) are the caller's scratch; nothing else is written
void leak_launch(DevPlan const& d, void const* A, uint32_t nUnits, uint32_t const* pairs, uint32_t const* posStart,
    uint32_t const* unitFirst, uint32_t const* colUnitPtr, double* rec, double* col, hipStream_t s);

// the same products per leak POSITION: |.|^2 per (position, right-hand side), one [LN] record per position of the listing into
// rec [nPos][LN], the caller's scratch; nothing else is written (tfq_leak_map.hip; tfqmrgpuExt_leakMap)
void leak_map_launch(DevPlan const& d, void const* A, uint32_t nPos, uint32_t const* pairs, uint32_t const* posStart, double* rec, hipStream_t s);

// per block n of the plan's X (the caller's block order, nX blocks) and right-hand side: cost [nX][LN] = the sum over the products
// start[n] .. start[n + 1] of the listing (tfq_plan.hpp: DropListing, all three lists in device memory) of |A_aOf[q] X_n (:, j)|^2, every
// product squared on its own, and weight [nX][LN] = |X_n (:, j)|^2, in double (tfq_drop_cost.hip; tfqmrgpuExt_dropCost).  cost or weight
// may be nullptr (cost == nullptr: A is not read); both are the caller's scratch; nothing else is written
void drop_cost_launch(DevPlan const& d, void const* A, uint32_t nX, uint32_t const* start, uint32_t const* aOf, uint32_t const* xOf,
    double* cost, double* weight, hipStream_t s);

// warm start (tfq_warm.hip; tfqmrgpuExt_solveFrom).  X0, R: X-shaped vectors of the plan's storage type, block and element order; Y = A * x.
// In front of the correction solve: X0 := x, R := (B under X, or 0) - Y, and the set-up that VEC_SETUP leaves to whoever brings d.R: tau = |r|^2,
// 1 / |b|^2, rho = 1, every other scalar 0, the fold counters and the control block.  Writes d.pz (chunk records), the scalars, X0 and R
bool warm_residual_launch(DevPlan const& d, void const* Y, void* X0, void* R, double tol, int maxIt, hipStream_t s);
// behind it: x := X0 + x.  false (both): no instance for this block shape
bool warm_update_launch(DevPlan const& d, void const* X0, hipStream_t s);
// the residual pass for the refinement of an 'm' plan (tfqmrgpuExt_refineFrom): dz is the plan's double side (resolveZ), X0, R and Y = A * x
// X-shaped vectors of doubles in element order ilvZ.  X0 := x, R := (B under X, or 0) - Y, bn2z [nCols][LN] := |b|^2, or |r|^2 where b = 0.
// Writes dz.pz (chunk records), bn2z, X0 and R; no scalar of the float solves.  false: no instance for this block shape, or dz is no double side
bool warm_refine_residual_launch(DevPlan const& dz, void const* Y, void* X0, void* R, double* bn2z, hipStream_t s);

} // namespace tfq
