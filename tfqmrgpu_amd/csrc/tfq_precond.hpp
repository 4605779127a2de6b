// The block-Jacobi right preconditioner (tfqmrgpu_ext.h sections 7 and 9): the launch interface of its kernels (tfq_precond.hip), and its
// host side (tfq_precond_host.cpp): the plan's memory for it, the set-up in front of a solve, and the state of the A in the buffer
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

#include "tfq_plan.hpp"

namespace tfq {

#pragma GCC visibility push(hidden)   // the host side is shared by files of the library and no part of its symbol list

// ---- the library-owned memory of a plan: one function says how large, one where
struct PrecondMem { char* minv; uint32_t* diag; uint32_t* colA; uint32_t* counter; uint32_t* identity; size_t minvBytes; };
size_t precond_bytes(Plan const& p);
PrecondMem precond_mem(Plan const& p);      // the pieces of Plan::layout.precond (allocated)

// the kept copy of the caller's A (section 9): Plan::held.aKept holds the A window of the buffer, for 'm' the double A (`a`) followed by the float A (`aFloat`)
struct KeptA { char* a; char* aFloat; size_t aBytes, aFloatBytes; };
size_t kept_a_bytes(Plan const& p);
KeptA kept_a(Plan const& p);                // the pieces of Plan::held.aKept (allocated)
inline bool kept_is_callers_a(Plan const& p) { return p.keepA && p.held.aKept && TFQMRGPU_PRECOND_NONE != p.held.precondInA; }

// ---- the caller's operands, for the calls that read them outside of a solve (tfq_grade_host.cpp; solveFrom, refineFrom and carry of tfq_api.hip)
// their checks in front of the first device call, in the documented order: no buffer | user-defined operator | and where the call reads A
// (needA): A never set | A scaled and not kept
tfqmrgpuStatus_t operands_ready(Plan const& p, bool needA);                     // tfq_grade_host.cpp
// the caller's A: the buffer's (d.A), or the kept copy while the buffer holds A M^-1 ('m': its double part) -- a patch of setBlocks('A')
// that no set-up has seen yet is in the copy already
void const* callers_a(Plan const& p, struct DevPlan const& d);                    // tfq_grade_host.cpp
// host -> device on the stream, not waited for; nothing for no bytes or no source (tfq_api.hip)
tfqmrgpuStatus_t upload(void* dst, void const* src, size_t bytes, hipStream_t s);

// ---- what a solve needs before its first iteration, and behind its last
tfqmrgpuStatus_t precond_prepare(Handle& h, Plan& p);
tfqmrgpuStatus_t precond_back(Handle& h, Plan& p);      // X := M^-1 Y

// ---- the state of the A in the buffer (Plan::held, precondIdentity, mixedFloor, cscPtr, cscBlock): every transition, by the call that causes it
void a_new_layout(Plan& p);                             // bufferSize: ends Plan::layout and Plan::held
void a_new_buffer(Plan& p);                             // setBuffer: ends Plan::held
void a_named(Plan& p);                                  // setMatrix('A'), before its argument checks
void a_set_whole(Plan& p, bool ok);                     // setMatrix('A'), behind its transfer
tfqmrgpuStatus_t a_patched(Plan& p, int32_t const* blocks, int32_t nBlocks, bool& intoKept);   // setBlocks('A'), behind its argument checks
void a_patch_written(Plan& p, int32_t const* blocks, int32_t nBlocks);   // setBlocks('A'), behind its transfer, which succeeded
tfqmrgpuStatus_t a_keep(Plan& p, bool on);              // keepOperator

#pragma GCC visibility pop

// Minv[row] := inverse of the diagonal block of block row `row` of A, [nRows][2][LM][LM] (Re plane, Im plane, row-major, NOT transposed),
// in double (wDbl) or float.  A: the plan's operator as it sits in the buffer (blocks transposed, element order ilv), double (aDbl) or
// float; diagOfRow[row]: its diagonal block, ~0u when the pattern has none.  Rows without a diagonal block and rows whose block is
// singular get the unit matrix and add one to *nIdentity.  The arithmetic is double whatever the two precisions.
void launch_precond_invert(bool aDbl, bool wDbl, void const* A, uint32_t const* diagOfRow, void* Minv, uint32_t* nIdentity,
                           uint32_t nRows, int LM, int ilv, hipStream_t s);

// in place, block b of `data` (LM x nC complex, planes Re | Im, element order ilv):  block := W * block  with W = Minv[wOfBlock[b]],
// or its transpose (transW).  With the transposed blocks of A and wOfBlock = the block column this is A_ij := A_ij * Minv_j; with an
// X-shaped vector and wOfBlock = the block row it is X_ic := Minv_i * X_ic.  Sums are accumulated in double.
void launch_precond_apply(bool dataDbl, bool wDbl, bool transW, void* data, uint32_t nBlocks, uint32_t const* wOfBlock,
                          void const* Minv, int LM, int nC, int ilv, hipStream_t s);

// ---- the listed, out-of-place forms (tfqmrgpu_ext.h section 9: a kept copy of the caller's A) -- the same arithmetic, element by element
// work group k inverts block row rows[k] (rows == nullptr: row k) for k < nListed; A may be the kept copy.  isIdentity [nRows]: 1 where
// the row got the unit matrix, 0 where not -- written for the listed rows only
void launch_precond_invert_listed(bool aDbl, bool wDbl, void const* A, uint32_t const* diagOfRow, void* Minv, uint32_t* isIdentity,
                                  uint32_t const* rows, uint32_t nListed, int LM, int ilv, hipStream_t s);

// block list[k] of `dst` := W * block list[k] of `src` for k < nListed, W = Minv[wOfBlock[list[k]]] or its transpose; no block twice in the list
void launch_precond_apply_listed(bool dataDbl, bool wDbl, bool transW, void const* src, void* dst, uint32_t nListed, uint32_t const* list,
                                 uint32_t const* wOfBlock, void const* Minv, int LM, int nC, int ilv, hipStream_t s);

} // namespace tfq
