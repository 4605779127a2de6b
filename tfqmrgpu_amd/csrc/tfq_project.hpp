// Start projection (tfqmrgpu_ext.h section 17): the launch interface of its kernels (tfq_project.hip) and its host side (tfq_project_host.cpp)
#pragma once
#include "tfq_device.hpp"

namespace tfq {

constexpr int kProjectMax = 4;                                      // the deepest ring of starts (tfqmrgpuExt_keepStarts)
constexpr int project_planes(int k) { return k * k + 2 * k + 1; }   // doubles per right-hand side in a chunk's record

// the k starts (newest first) and their images W_i = A S_i: X-shaped vectors of the plan's storage type, block and element order
struct ProjectVecs { void const* s[kProjectMax]; void const* w[kProjectMax]; };

// d.x := sum gamma_i S_i with the gamma that minimises |B - sum gamma_i W_i| per (block column, right-hand side); d: where the caller's X and B
// are (resolve_callers).  rec [project_planes(k)][nChunks][LN], gamma [nCols][LN][kProjectMax][2] and nUsed [nCols][LN] are the caller's
// scratch; pivotMin: the smallest pivot ratio d_i / G_ii of a kept start.  false: no instance for this block shape or this k
bool project_launch(DevPlan const& d, int k, ProjectVecs const& pv, double* rec, double pivotMin, double* gamma, int32_t* nUsed, hipStream_t s);

#pragma GCC visibility push(hidden)
// the host side of the four calls, behind the pointer checks of the C-ABI
tfqmrgpuStatus_t starts_keep(Plan& p, int depth);
tfqmrgpuStatus_t starts_push(Handle& h, Plan& p);
tfqmrgpuStatus_t starts_project(Handle& h, Plan& p, double* coefficients, int32_t* nUsed);
#pragma GCC visibility pop

} // namespace tfq
