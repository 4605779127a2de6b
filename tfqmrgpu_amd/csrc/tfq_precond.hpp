// launch interface of the block-Jacobi right preconditioner (tfq_precond.hip; tfqmrgpu_ext.h section 7)
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace tfq {

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
