// Energy mesh (tfqmrgpu_ext.h section 19): the launch interface of its kernels (tfq_mesh.hip) and its host side (tfq_mesh_host.cpp)
#pragma once
#include "tfq_device.hpp"

namespace tfq {

// one copy of A as it is stored (the buffer's window or the kept copy): blocks of LM x LM, transposed, element order ilv
struct DiagSide { void* a; bool dbl; int ilv; };

// base[r][i] := element (i, i) of block diagOfRow[r] of `from`, (Re, Im), for i < lm and the block rows r = rows[k], k < nListed (device
// memory; rows == nullptr: r = k, and nListed = mb is all of them); base is [mb][LM][2] of from's real type
void diag_capture_launch(DiagSide const& from, void* base, uint32_t const* diagOfRow, uint32_t const* rows, uint32_t nListed, int LM, int lm,
                         hipStream_t s);
// element (i, i) of block diagOfRow[r] of `to` := base[r][i] + sigma, componentwise in base's real type (baseDbl; float: sigma rounded to
// float once), then rounded to to's real type where that is float and the base's is double (the float A of an 'm' plan)
void diag_shift_launch(DiagSide const& to, void const* base, bool baseDbl, uint32_t const* diagOfRow, uint32_t mb, int LM, int lm,
                       double sigmaRe, double sigmaIm, hipStream_t s);
// sum[b][r][s] += w * X[subset[b]][r][s] for the nnzbB blocks of d.x that carry a block of B; sum is [nnzbB][LM][LN][2] of double, d.x as
// resolve_callers gives it.  Products and sums are rounded one by one, in the order of section 19b.  false: more work groups than a grid has
bool sum_add_launch(DevPlan const& d, double* sum, double wRe, double wIm, hipStream_t s);

#pragma GCC visibility push(hidden)
// the host side of the calls, behind the pointer checks of the C-ABI
tfqmrgpuStatus_t mesh_shift(Handle& h, Plan& p, double sigmaRe, double sigmaIm);
tfqmrgpuStatus_t sum_keep(Plan& p, bool on);
tfqmrgpuStatus_t sum_add(Handle& h, Plan& p, double wRe, double wIm);
tfqmrgpuStatus_t sum_get(Handle& h, Plan& p, double* values, int32_t* nTerms);
tfqmrgpuStatus_t sum_clear(Handle& h, Plan& p);
#pragma GCC visibility pop

} // namespace tfq
