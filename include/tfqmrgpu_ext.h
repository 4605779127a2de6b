/*
 * tfqmrgpu_ext.h -- additive extensions of the MI355X build of libtfQMRgpu.so.
 *
 * Nothing in here exists in the reference (real-space/tfQMRgpu); existing callers never
 * need it.  It adds (1) read-only views for parity tests, (2) control over the shadow
 * vector v3 so that iteration counts can be compared with the reference CPU path,
 * (3) a stand-alone BSR multiply on device-resident data (what the reference times in
 * `bench_tfqmrgpu multi`, bench_tfqmrgpu.cu:289-440) and (4) the multi-GPU mode: right
 * hand side block columns sharded over ranks, one tiny RCCL all-reduce per stopping test.
 */
#ifndef TFQMRGPU_EXT_H
#define TFQMRGPU_EXT_H

#include "tfqmrgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) plan introspection ------------------------------------------------------------ */
/* The arrays are exactly the analysis results of the reference createPlan
 * (tfqmrgpu.cu:183-339, members of bsrsv_plan_t, tfqmrgpu_plan.hxx:21-49): same order,
 * same integer types, 0-based.  Pointers stay valid until destroyPlan. */
typedef struct {
    uint32_t nRows;                        /* mb                                            */
    uint32_t nCols;                        /* non-empty block columns of X                  */
    uint32_t nnzbA, nnzbX, nnzbB;
    uint64_t nPairs;                       /* block products in Y = A*X                     */
    uint32_t const *pairs;                 /* [2*nPairs]  (inzA, inzX)                      */
    uint32_t const *starts;                /* [nnzbX + 1] first pair of each Y block        */
    uint32_t const *subset;                /* [nnzbB]     X block that holds each B block   */
    uint16_t const *colindx;               /* [nnzbX]     compressed block column           */
    int32_t  const *original_bsrColIndX;   /* [nCols]     user column index per compressed  */
    int32_t  LM, LN;                       /* block shape, 0 before bufferSize              */
    char     precision;                    /* 'c' / 'z', 0 before bufferSize                */
} tfqmrgpuPlanView_t;

tfqmrgpuStatus_t tfqmrgpuExt_planView(tfqmrgpuBsrsvPlan_t plan, tfqmrgpuPlanView_t *view);

/* per-iteration trace of the last solve: bound2[it] = max_rhs(tau*invBn2)*(2*it+1) as the
 * stopping test saw it (reference tfqmrgpu_core.hxx:239-252).  Returns how many entries
 * exist; copies at most `capacity`. */
int32_t tfqmrgpuExt_getBoundHistory(tfqmrgpuBsrsvPlan_t plan, double *bound2, int32_t capacity);

/* per-kernel timing of the last solve, measured with HIP events on the solver's own stream.
 * Switch on before solve; afterwards read, for each kernel class k < TFQMRGPU_PROFILE_CLASSES,
 * the number of launches that did work and their summed duration in milliseconds. */
enum {
    TFQMRGPU_PROF_DEC35 = 0, TFQMRGPU_PROF_XPAY_V6, TFQMRGPU_PROF_SPMM_V4_DOT, TFQMRGPU_PROF_DEC34,
    TFQMRGPU_PROF_V5_NRM, TFQMRGPU_PROF_DECT_C67, TFQMRGPU_PROF_X_V6_V7, TFQMRGPU_PROF_SPMM_V5_NRM_DOT,
    TFQMRGPU_PROF_DECT_FINAL, TFQMRGPU_PROF_DECIDE, TFQMRGPU_PROF_PROBE,
    TFQMRGPU_PROFILE_CLASSES
};
/* on = 1: events around every kernel class (176 events per 16 iterations: costs a 37 ms solve 0.6 ms);
 * on = 2: only around the two fused multiplies SPMM_V4_DOT and SPMM_V5_NRM_DOT (the other classes report 0 launches) */
tfqmrgpuStatus_t tfqmrgpuExt_setProfiling(tfqmrgpuBsrsvPlan_t plan, int on);
tfqmrgpuStatus_t tfqmrgpuExt_getProfile(tfqmrgpuBsrsvPlan_t plan, int64_t *launches, double *milliseconds);
/* the launches that were enqueued ahead of the stopping decision and returned without doing work
 * (a profiler counts them as calls of the same kernels) */
tfqmrgpuStatus_t tfqmrgpuExt_getProfileGated(tfqmrgpuBsrsvPlan_t plan, int64_t *launches, double *milliseconds);
/* of the launches that getProfile counts: those of the FIRST iteration of the solve.  v4, v6, v7, v8 and x are zero there and v5 is
 * B scattered onto zeros by definition (tfqmrgpu_core.hxx:125,147-153); they are neither written at the start of a solve nor
 * read: XPAY_V6, SPMM_V4_DOT, V5_NRM and X_V6_V7 move 2, 2, 1 and 2 vectors less in that launch -- price a kernel against its
 * roof on the other launches. */
tfqmrgpuStatus_t tfqmrgpuExt_getProfileFirst(tfqmrgpuBsrsvPlan_t plan, int64_t *launches, double *milliseconds);
/* the kernel family that the fused multiplies of this plan run (needs the buffer: the element order and the column batches are fixed
 * by bufferSize / setBuffer), e.g. "k_spmm_ilv16" -- so that kept profiler figures (profiles/pmc_traffic.json) can be told apart from
 * figures of a kernel that no longer runs.  Writes at most `capacity` bytes including the terminating 0. */
tfqmrgpuStatus_t tfqmrgpuExt_getMultiplyKernel(tfqmrgpuBsrsvPlan_t plan, char *name, int32_t capacity);
/* *on = 1: a solve of this plan on one rank runs the "late v5" form of the iteration slot -- V5_NRM sums |v5 + alfa v9|^2 without storing v5 and
 * SPMM_V5_NRM_DOT applies that half step in its epilogue (2 and 5 vectors moved where the other form moves 3 and 4; the same bits).  Plans whose
 * fused multiplies run on k_spmm_ilv16 with the built-in operator and that do not fold their column operations; 0 for every other plan.  On
 * several ranks (section 4) no plan folds, so there every such plan takes this form, also one for which this call answers 0 because it folds on
 * one rank.  Needs the buffer, as getMultiplyKernel does. */
tfqmrgpuStatus_t tfqmrgpuExt_getLateV5(tfqmrgpuBsrsvPlan_t plan, int32_t *on);

/* ---- (2) shadow vector v3 -------------------------------------------------------------- */
enum {
    TFQMRGPU_SHADOW_HASH       = 0, /* default: counter-based hash of (block row, block column,
                                       element), uniform (0,1]; independent of the GPU count  */
    TFQMRGPU_SHADOW_GLIBC_RAND = 1  /* the sequence the reference CPU path uses: glibc rand()
                                       from seed 1, /RAND_MAX, flat over [nnzbX][2][LM][LN]
                                       (tfqmrgpu_linalg.hxx:799-802)                          */
};
/* call after createPlan and before setBuffer */
tfqmrgpuStatus_t tfqmrgpuExt_setShadowMode(tfqmrgpuBsrsvPlan_t plan, int mode);
/* user-supplied v3, host array float[nnzbX][2][LM][LN] in the caller's BSR order; call after setBuffer */
tfqmrgpuStatus_t tfqmrgpuExt_setShadowVector(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, float const *v3);
/* the vector in use, same shape and order (for parity tests: feed it to a CPU implementation); call after setBuffer,
 * not during a solve.  In hash mode the four reals (Re, Im) x (row 2m, row 2m+1) of column j of the block in block row r,
 * ORIGINAL block column c (0-based) come from one 64-bit hash, 16 bits each:
 *   h = splitmix64(key + (m * ln + j) * 0xd1342543de82ef95),  key = splitmix64(c << 32 | r) ^ 1234,
 *   value = float(((h >> 16 * (2 * (row & 1) + (Im ? 1 : 0))) & 0xffff) + 1) / 2^16   in (0, 1]
 * (tfq_device.hpp), whatever the block order and however the columns are sharded over GPUs. */
tfqmrgpuStatus_t tfqmrgpuExt_getShadowVector(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, float *v3);

/* Debug getter for kernel-level parity tests: one of the solver's X-shaped work vectors as the last solve left it --
 * which = 1: the solution X, 4 ... 9: v4 ... v9 in the reference's numbering (tfqmrgpu_core.hxx:52-59; v4 = A-image
 * recurrence, v5 = residual-like vector, v6/v7 = search directions, v8 = A v6 of the second half step, v9 = A v6 of the
 * first) -- to host memory, native layout [nnzbX][2][lm][ln], caller's block order, plan precision.  Non-destructive;
 * call it before the next set/getMatrix, which stage the caller's blocks through v4 ... v9.
 * After a solve that stopped at iteration k the vectors are those of the reference at the end of iteration k, except
 * that the residual probe of this library does not overwrite v9 (the reference's does, tfqmrgpu_core.hxx:265). */
tfqmrgpuStatus_t tfqmrgpuExt_getWorkVector(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int which, void *values);

/* ---- (3) stand-alone block-sparse multiply --------------------------------------------- */
/* Y[iY] = sum over pairs p in [starts[iY], starts[iY+1]) of A[pairs[2p]] * X[pairs[2p+1]]
 * All pointers are DEVICE pointers.  Blocks are in the native layout RRRRIIII:
 * A[nnzbA][2][lm(k)][lm(i)] (transposed), X|Y[nnzb][2][lm][ln].
 * Same contract as the reference kernel gemmNxNf (tfqmrgpu_blockmult.hxx:9-93).
 * Four real products per complex one, as the reference (the three-product form is an option of a PLAN, section 6).
 * precision: 'z' (or 'd') complex<double>; 'm' float data summed in double -- operands and Y are float, every sum is
 * accumulated in double and rounded to float once, when Y is stored (the reference's gemmNxNf<float, ..., double>); every
 * other letter complex<float> ('c', 'f').
 * Shapes (lm x ln), the 21 of the reference's `bench multi`, in every precision: the solver's 15 (4x4, 4x5, 4x8, 4x32, 8x8,
 * 8x9, 8x10, 8x32, 8x64, 16x16, 16x32, 16x64, 32x32, 32x64, 64x64) and 6x6, 12x12, 24x24, 48x48, 96x96, 128x128.  Any other
 * shape returns TFQMRGPU_BLOCKSIZE_MISSING.  The further shapes belong to this product only: the block
 * sizes of the solver (tfqmrgpu_bsrsv_bufferSize, tfqmrgpu_bsrsv_allowedBlockSizes) do not change, as in the reference
 * (allowed_block_sizes.h). */
tfqmrgpuStatus_t tfqmrgpuExt_multiply(tfqmrgpuHandle_t handle,
    char precision, int lm, int ln,
    uint32_t nnzbY, uint32_t const *starts_d, uint32_t const *pairs_d,
    void const *A_d, void const *X_d, void *Y_d);

/* A PREPARED launch order for that product (r04).  The listing stays the caller's; which work group computes which Y block is the library's to
 * choose, and for a listing that is multiplied many times it is chosen once, outside the caller's timed loop -- as the reference's own
 * benchmark prepares its launch (bench_tfqmrgpu.cu:442-556 in front of the timed loop :289-440).  multiplyPrepare reads the two lists
 * back from the device, finds block columns (Y blocks that share X blocks) and row bands (by the A indices) and leaves an XCD-aware order
 * in device memory: mode 1 = neighbouring work groups share X and A blocks, the 8 XCDs split the block COLUMNS (every L2 sees all of A and an
 * eighth of X); mode 3 = the XCDs split the block ROWS (an eighth of A, all of X); mode 4 = 1 or 3, whichever keeps the larger operand split
 * (the recommended one); mode 2 = mode 1 with the work groups of most block products first; mode 0 or a shape whose kernel takes no order (lm or ln
 * not a multiple of 16): *order = NULL,
 * which multiplyOrdered treats as the caller's order.  Results are those of tfqmrgpuExt_multiply bit for bit (the same kernel computes
 * every Y block from the same pair list).  An order belongs to ONE listing (nnzbY, starts, pairs): release it with multiplyRelease. */
tfqmrgpuStatus_t tfqmrgpuExt_multiplyPrepare(tfqmrgpuHandle_t handle, char precision, int lm, int ln,
    uint32_t nnzbY, uint32_t const *starts_d, uint32_t const *pairs_d, int mode, void **order);
tfqmrgpuStatus_t tfqmrgpuExt_multiplyOrdered(tfqmrgpuHandle_t handle,
    char precision, int lm, int ln,
    uint32_t nnzbY, uint32_t const *starts_d, uint32_t const *pairs_d,
    void const *A_d, void const *X_d, void *Y_d, void const *order);
tfqmrgpuStatus_t tfqmrgpuExt_multiplyRelease(void *order);

/* The same product on the data of a plan: X := A * X for the plan's operator A (as given to setMatrix('A')) and the
 * plan's X (setMatrix('X') before, getMatrix('X') afterwards), truncated to the pattern of X like every product of the
 * solver.  Uses the multiply kernel and the block / element order of the solver itself -- for 16 x 16
 * complex<double> plans the row-pair-interleaved one -- so it is also what bench.py times as "the BSR multiply".
 * `repetitions` > 1 computes the product that many times from the same X (timing); `repetitions` < 0: that many launches and NO copy
 * of the product back into X (a timed region then holds the multiply kernel alone); asynchronous on the handle's stream. */
tfqmrgpuStatus_t tfqmrgpuExt_applyOperator(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int repetitions);

/* ---- (4) multi-GPU: one process per GPU, block columns of X/B sharded ------------------- */
/* Splits the compressed block columns of X into `nranks` contiguous ranges with balanced
 * block counts and extracts the sub-patterns of X and B that belong to `rank`.
 * Outputs are malloc'ed by the library; release with tfqmrgpuExt_freeShard.
 * xBlocks/bBlocks list, for every block of the shard, its index in the unsharded operator
 * (so that values can be scattered/gathered).  Index arrays are 0-based regardless of
 * indexOffset of the input. */
typedef struct {
    int32_t  mb;
    int32_t  nnzbX, nnzbB;
    int32_t *rowPtrX, *colIndX;  /* [mb+1], [nnzbX] */
    int32_t *rowPtrB, *colIndB;  /* [mb+1], [nnzbB] */
    int32_t *xBlocks, *bBlocks;  /* [nnzbX], [nnzbB] indices into the global value arrays   */
    int32_t  firstCol, nCols;    /* range of compressed block columns owned by this rank     */
} tfqmrgpuShard_t;

tfqmrgpuStatus_t tfqmrgpuExt_shardColumns(int mb,
    int32_t const *rowPtrX, int nnzbX, int32_t const *colIndX,
    int32_t const *rowPtrB, int nnzbB, int32_t const *colIndB,
    int indexOffset, int nranks, int rank, tfqmrgpuShard_t *shard);
void tfqmrgpuExt_freeShard(tfqmrgpuShard_t *shard);

/* RCCL communicator for the stopping test.  rank 0 creates the id, the caller broadcasts the
 * 128 bytes by any means (torch.distributed, MPI, a file), every rank calls commInit. */
tfqmrgpuStatus_t tfqmrgpuExt_commUniqueId(char id[128]);
tfqmrgpuStatus_t tfqmrgpuExt_commInit(tfqmrgpuHandle_t handle, int nranks, int rank, char const id[128]);
tfqmrgpuStatus_t tfqmrgpuExt_commDestroy(tfqmrgpuHandle_t handle);
/* Instead of RCCL: a host callback that max-reduces `n` doubles in place over all ranks
 * (used by the CPU/gloo tests of the sharding logic and by MPI-based callers). */
typedef void (*tfqmrgpuReduceMax_t)(void *ctx, double *values, int n);
tfqmrgpuStatus_t tfqmrgpuExt_setReduceCallback(tfqmrgpuHandle_t handle, tfqmrgpuReduceMax_t fn, void *ctx);

/* ---- (6) precision options -------------------------------------------------------------- */
/* Mixed precision: tfqmrgpu_bsrsv_bufferSize(..., 'm', ...) -- dormant in the reference (tfqmrgpu.cu:42, "load float, multiply-
 * accumulate double, store float"; tfqmrgpu.h:72 "start with float and converge double"), built here as iterative refinement:
 * x, B and A are kept in double, every cycle computes r = b - A x in double, solves A d = r with the complex<float> tfQMR and adds
 * d to x in double.  setMatrix / getMatrix of such a plan accept 'c' AND 'z' data (converted on the way); solve's threshold is
 * max_rhs |b - A x| / |b| in double arithmetic, maxIterations bounds the sum of the float iterations; getInfo reports that sum.
 * The buffer is 11 float-sized vectors against 15 for 'z'.  Where float iterations cannot reduce the residual (systems on which
 * the 'c' solver stagnates above ~0.1) solve returns TFQMRGPU_STATUS_MAX_ITERATIONS with the best x.
 * getRefinementHistory: residual[i] = the relative residual (double arithmetic) in front of float solve i, the last entry the final
 * one; iterations[i] = the float iterations of solve i (0 in the last entry); either array may be NULL; returns the count. */
int32_t tfqmrgpuExt_getRefinementHistory(tfqmrgpuBsrsvPlan_t plan, double *residual, int32_t *iterations, int32_t capacity);
/* Three real products per complex one (Gauss) in the complex<double> multiplies of the block shapes above 16 x 16: a quarter fewer
 * matrix instructions (64 x 64: iteration -7 %), but Im = P3 - P1 - P2 is accurate relative to |A||X| only -- an imaginary part
 * 10^-k times smaller than the real part loses k digits against the reference's four products.  OFF unless switched on here
 * (it was the default until round 2); call before solve. */
tfqmrgpuStatus_t tfqmrgpuExt_setThreeProductMultiply(tfqmrgpuBsrsvPlan_t plan, int on);

/* ---- (5) user-defined linear operator --------------------------------------------------- */
/* The reference lets C++ users replace the block-sparse operator by their own `action_t` class whose
 * `multiply(y, x, colindx, nnzbX, nCols, l2nX, streamId)` returns the flop count (README.md:110-117,
 * tfqmrgpu_blocksparse.hxx:71-199, called at tfqmrgpu_core.hxx:134).  The C-ABI counterpart: a callback
 * that ENQUEUES Y = A*X on `stream` (no synchronisation) for device vectors in the caller's own BSR block
 * order of X and the native layout Y|X[nnzbX][2][lm][ln]; colindx_d[nnzbX] is the compressed block column
 * of every block (what the reference hands over).  *flops receives the operation count of the call.
 * A non-zero return value aborts the solve and is returned by tfqmrgpu_bsrsv_solve.
 * With an operator installed the solver runs its un-fused schedule (gather into the caller's order,
 * callback, vector-update kernel) and synchronises with the host once per iteration, like the reference;
 * createPlan still needs a pattern for A (any valid one, e.g. block-diagonal), its values are not used.
 * Two X-shaped scratch vectors are allocated by the library at the first solve and released by
 * destroyPlan.  multiply == NULL restores the built-in block-sparse operator. */
typedef tfqmrgpuStatus_t (*tfqmrgpuOperator_t)(void *ctx, void *Y_d, void const *X_d,
    uint16_t const *colindx_d, uint32_t nnzbX, uint32_t nCols, int lm, int ln, char precision,
    tfqmrgpuStream_t stream, double *flops);
tfqmrgpuStatus_t tfqmrgpuExt_setOperator(tfqmrgpuBsrsvPlan_t plan, tfqmrgpuOperator_t multiply, void *ctx);

/* ---- (7) preconditioner ------------------------------------------------------------------ */
/* The reference has the hook and never filled it (has_preconditioner() returns false, tfqmrgpu_blocksparse.hxx:68,79;
 * tfqmrgpu_core.hxx:37,57).  Here: block Jacobi applied from the RIGHT.  With M = blockdiag(A) the solver iterates on
 * (A M^-1) Y = B and returns X = M^-1 Y.  A M^-1 has the block pattern of A (block (i,j) becomes A_ij M_jj^-1) and M^-1 Y the
 * pattern of Y (block (i,c) becomes M_ii^-1 Y_ic), so the truncation of every product to the pattern of X
 * commutes with it: the truncated problem that is solved is exactly the caller's.  The residual B - (A M^-1) Y equals B - A X:
 * `threshold`, the bound history and getInfo's residuum_reached keep their meaning.  It costs nothing per iteration.
 *
 * setPreconditioner: kind NONE (the default) or BLOCK_JACOBI; any other kind returns TFQMRGPU_UNDOCUMENTED_ERROR.  Call it after
 *   bufferSize; it takes effect at the next solve.  A plan that never calls it, or sets NONE, behaves bit for bit as without this
 *   section: same buffer size, same launches, same results.
 * setMatrix('A') marks the preconditioner stale.  The first solve after it inverts the diagonal blocks (Gauss-Jordan with row
 *   exchanges, double arithmetic in every precision) and scales A IN PLACE in the buffer; later solves of the same A (new B) reuse
 *   both.  M^-1 lives in device memory that the library owns, allocated at the first preconditioned solve and released by destroyPlan;
 *   bufferSize and the buffer layout do not change.
 * Switching the kind after A has been scaled needs a fresh setMatrix('A'): until then solve returns TFQMRGPU_UNDOCUMENTED_ERROR
 *   with the key character 'A' (status = 14 + 1000 * line + 10^7 * 'A') instead of solving with a half-scaled operator.  The same
 *   status when A has never been set.
 * A block row without a diagonal block in the pattern of A, or whose diagonal block is singular (a pivot that is zero or not
 *   finite; pivots are chosen by max(|Re|, |Im|)) or whose inverse is not finite in the precision it is stored in, gets M_ii = 1;
 *   the solve runs all the same.  M^-1 never holds anything but finite numbers.
 * getMatrix('X') and tfqmrgpuExt_getWorkVector(.., 1, ..) return X, not Y: the back transform runs at the end of solve, on the
 *   solver's stream, also when the solve ends at maxIterations or in a breakdown.  The other work vectors (4 ... 9) are those of the
 *   scaled system.  tfqmrgpuExt_applyOperator on such a plan multiplies with what is in the buffer: A M^-1 once a solve (or
 *   getPreconditioner) has scaled A, the caller's A before.  The caller's A itself is not kept (unless section 9 is switched on): whoever reads the A window of the
 *   buffer directly finds A M^-1 there (getMatrix hands out X only, as in the reference).  setBuffer starts afresh: the new buffer
 *   holds no A, so setMatrix('A') has to follow it and is inverted and scaled at the next solve; bufferSize does the same.
 * Precisions 'z', 'c' and 'm'.  'm': both copies of A (double and float) are scaled, M^-1 is kept in double and the back transform
 *   is applied once, in double, to the refined solution.
 * A plan with a user-defined operator (section 5) refuses: solve returns TFQMRGPU_NO_IMPLEMENTATION, on several ranks through the
 *   vote in front of the solve, so that all ranks leave together.
 *   With kind NONE such a plan solves whatever state the A in the buffer is in: the operator never reads it.
 * Several ranks (section 4): every rank holds all of A and computes the same M^-1; the back transform is local to a rank's block
 *   columns.  X does not depend on the number of ranks.
 * getInfo: iterations and residual as always; flops_performed includes the back transform, 8 LM LM LN nnzbX; the set-up is not
 *   counted (it belongs to setMatrix('A')).
 * getPreconditioner: M^-1 as the solver uses it, to host memory, [mb][2][LM][LM] (Re plane, Im plane, row-major), in the plan's
 *   precision ('m': double), and the number of block rows whose M_ii is the unit matrix.  Either pointer may be NULL.  Needs kind
 *   BLOCK_JACOBI (else TFQMRGPU_UNDOCUMENTED_ERROR); called between setMatrix('A') and the first solve it performs the set-up
 *   itself, so that the solve finds it done. */
enum { TFQMRGPU_PRECOND_NONE = 0, TFQMRGPU_PRECOND_BLOCK_JACOBI = 1 };
tfqmrgpuStatus_t tfqmrgpuExt_setPreconditioner(tfqmrgpuBsrsvPlan_t plan, int kind);
tfqmrgpuStatus_t tfqmrgpuExt_getPreconditioner(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
                                               void *Minv /* host, [mb][2][LM][LM], plan precision ('m': double) */,
                                               int32_t *nIdentity);

/* ---- (8) listed blocks ------------------------------------------------------------------- */
/* setMatrix and getMatrix move an operand whole.  Along an energy loop only the diagonal blocks of A change, and a Green-function
 * caller reads only the X blocks that sit on B's pattern: setBlocks / getBlocks convert the blocks that a list names and leave every
 * other block of the operand untouched, bit for bit.
 *
 * blocks[k] is the 0-based position of a block in the caller's own block order of that operand -- the order of the bsrColInd array
 *   given to createPlan, whatever indexOffset was.  `values` holds nBlocks blocks, compact: block k of `values` is block blocks[k] of
 *   the operand.  `blocks` is always a HOST array and is the caller's again when the call returns; `values` may be host or device memory,
 *   told apart as in setMatrix / getMatrix (device memory: one conversion kernel on the handle's stream, no staging).
 * Layout, trans, precision and the rule that A is stored transposed are exactly those of setMatrix / getMatrix, and so is the rule
 *   that an 'm' plan takes 'c' or 'z' data; setBlocks('A') on an 'm' plan writes both its copies of A, the double and the float one.
 * getBlocks reads X only, as getMatrix: any other `var` returns the status that getMatrix returns for it.
 *   blocks == NULL: the X blocks on B's pattern, in B's block order (tfqmrgpuPlanView_t::subset); it needs nBlocks == nnzbB, anything
 *   else returns TFQMRGPU_POINTER_INVALID.  After a preconditioned solve (section 7) getBlocks returns X, the back-transformed
 *   solution, as getMatrix does.
 * setBlocks takes no NULL list: TFQMRGPU_POINTER_INVALID (so does getBlocks of an `nBlocks` that is not nnzbB).
 * nBlocks == 0 returns success and touches nothing.
 * All checks come before the first device call, in this order: layout, trans and the plan / handle pointers as in setMatrix; no
 *   bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; `var`; the list -- an index < 0 or >= nnzb of that operand, or in setBlocks an
 *   index that occurs twice, returns TFQMRGPU_UNDOCUMENTED_ERROR with the key character `var` (status = 14 + 1000 * line + 10^7 * var);
 *   getBlocks may name a block twice; the check takes O(nBlocks + nnzb) --; no buffer: TFQMRGPU_POINTER_INVALID; precision mismatch;
 *   values == NULL.  After any error the buffer is what it was.
 * setBlocks('A') and the state of the plan: like setMatrix('A') it forgets the float floor that an 'm' plan remembers.  It does NOT
 *   make a plan whose A was never set whole have an A: the first A comes from setMatrix('A').  If the A in the buffer has been scaled
 *   by the preconditioner (section 7: a preconditioned solve or getPreconditioner since the last setMatrix('A')) it returns
 *   TFQMRGPU_NO_IMPLEMENTATION and writes nothing: the buffer holds A M^-1, and M changes with the diagonal blocks, so a patch of
 *   A M^-1 is not a patch of A.  A whole setMatrix('A') makes partial updates possible again until the next preconditioned solve;
 *   a plan that keeps the caller's A (section 9) takes the patch at any time.
 *   With kind BLOCK_JACOBI chosen but A not yet scaled setBlocks('A') is allowed: the next solve inverts and scales what is then in
 *   the buffer.
 * As setMatrix / getMatrix: host arrays are staged through the work vectors v4 ... v9 (call tfqmrgpuExt_getWorkVector first), a list
 *   of any length in as many batches as the stage needs, one stream synchronisation per batch; do not call during a solve.  The device
 *   copy of the list is memory that the library owns, grown on demand and released by destroyPlan; bufferSize and the buffer layout do
 *   not change.  Uploading the list synchronises the handle's stream once; with blocks == NULL nothing is uploaded (the plan's own list
 *   is on the device), and with device `values` such a call does not synchronise at all.
 * Several ranks (section 4): the list refers to the rank's own plan.  There are no Fortran wrappers, as for every call of this file. */
tfqmrgpuStatus_t tfqmrgpuExt_setBlocks(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char var /* 'A', 'B', 'X' */,
    int32_t nBlocks, int32_t const *blocks /* host */, void const *values,
    char precision, char trans, tfqmrgpuDataLayout_t layout);
tfqmrgpuStatus_t tfqmrgpuExt_getBlocks(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, char var /* 'X' only, as getMatrix */,
    int32_t nBlocks, int32_t const *blocks /* host, or NULL */, void *values,
    char precision, char trans, tfqmrgpuDataLayout_t layout);

/* ---- (9) keeping the caller's A on a preconditioned plan --------------------------------- */
/* The first preconditioned solve (section 7) overwrites the A in the buffer with A M^-1, so that setBlocks('A') (section 8) has nothing
 * left to patch and a change of kind needs a whole setMatrix('A').  keepOperator(plan, 1) makes the plan keep the caller's own A next to
 * the scaled one: a patch of A is then a patch of the copy, and the set-up is redone for the block rows and block columns that the patch
 * touched.  This is what lets an energy loop -- only the diagonal blocks of A change -- run with the preconditioner.
 *
 * keepOperator: off is the default.  A plan that never calls it, or calls it with 0, behaves bit for bit as without this section: same
 *   buffer size, same launches, same results, same statuses (TFQMRGPU_NO_IMPLEMENTATION of setBlocks('A') on a scaled plan, the status
 *   with the key character 'A' after a change of kind).  Call it after bufferSize, like setPreconditioner; it survives bufferSize and
 *   setBuffer as the kind does.  Switching it ON while the A in the buffer has been scaled already and the plan has no copy returns
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A' (status = 14 + 1000 * line + 10^7 * 'A'): the caller's A is gone, setMatrix('A')
 *   brings one.  Switching it OFF releases the copy; the plan then behaves as if it had never been on.
 * The copy: made at the set-up (the first preconditioned solve, or getPreconditioner, after setMatrix('A')) from the A window of the
 *   buffer, device to device, before that window is scaled in place -- the buffer's own block order, transposition and element order; an
 *   'm' plan keeps both its copies of A, the double and the float one.  It is device memory that the library owns (the size of the A
 *   window(s)), allocated at the first such set-up and released by destroyPlan, by keepOperator(plan, 0), by setBuffer and by bufferSize;
 *   bufferSize and the buffer layout do not change.  The first preconditioned solve gives the bits it gives without the switch.
 * setBlocks('A') while the A in the buffer is scaled writes the listed blocks into the copy and returns success.  Arguments and list
 *   are checked as in section 8, in the same order; after an error nothing has changed.  Like every setBlocks('A') it forgets the float
 *   floor of an 'm' plan.  The library remembers the block columns that hold a listed block and the block rows whose diagonal block is
 *   listed; several calls before a solve add up.  While the A in the buffer is NOT scaled (kind NONE, or between setMatrix('A') and
 *   the set-up) setBlocks('A') writes the buffer, as in section 8.
 * The next set-up (solve or getPreconditioner) redoes what was touched: M_ii^-1 for the remembered rows, from the copy; every block
 *   A_ij M_jj^-1 of the remembered columns, from the copy into the buffer ('m': both copies); the count of unit matrices (a diagonal
 *   block can become singular, or stop being so).  Each block has the bits that a whole setMatrix('A') of the patched matrix and a whole
 *   set-up give it, so the solve is that solve, bit for bit.  The lists of the partial set-up live in library-owned device memory, grown
 *   on demand and released by destroyPlan; uploading them synchronises the handle's stream once.
 * setPreconditioner(plan, NONE) on a scaled plan needs no new matrix: the next solve copies the caller's A back into the buffer and
 *   solves without a preconditioner; BLOCK_JACOBI again scales it again.
 * setMatrix('A') whole works as always: it writes the buffer; the copy is taken again at the next set-up, patches that no set-up has
 *   seen are forgotten.
 * tfqmrgpuExt_applyOperator multiplies with what is in the buffer (A M^-1 once scaled), not with the copy; getWorkVector, the back
 *   transform and flops_performed are those of section 7 (the partial set-up is not counted, like the whole one).  A plan with a
 *   user-defined operator (section 5) accepts the switch and keeps nothing: it has no blocks to scale.
 * Several ranks (section 4): every rank holds all of A, and everything above is local to a rank. */
tfqmrgpuStatus_t tfqmrgpuExt_keepOperator(tfqmrgpuBsrsvPlan_t plan, int on);

/* ---- (10) per-right-hand-side residual of the caller's system ---------------------------- */
/* getInfo gives ONE residual, the maximum over all right-hand sides of all block columns, and solve ONE status.  After
 * TFQMRGPU_STATUS_MAX_ITERATIONS or TFQMRGPU_STATUS_BREAKDOWN the caller cannot tell which right-hand sides are good; the solver's own
 * probe sums in the plan's precision (float on a 'c' plan and inside the float solves of an 'm' plan); and nothing grades an X that the
 * caller brought.  residual computes |B - A X|^2 and |B|^2 per (block column, right-hand side) on the device, in double, without
 * fetching X.
 *
 * residual2[c*LN + j] = sum over the blocks of compressed block column c of |(B - A X)(:, j)|^2,
 * bnorm2[c*LN + j]    = the same sum of |B(:, j)|^2,           both HOST arrays [nCols][LN] of double, either may be NULL;
 * columns[c]          = the caller's block column index of compressed column c (tfqmrgpuPlanView_t::original_bsrColIndX, incl. indexOffset),
 *                       a HOST array [nCols], may be NULL;
 * *worst              = sqrt(max over c, j of residual2 / bnorm2), may be NULL.  All four NULL: TFQMRGPU_STATUS_NO_INFO_PASSED.
 *
 * Operands: A is the caller's A; B what the last setMatrix('B') / setBlocks('B') left; X what getMatrix('X') would return at that
 *   moment -- after a solve the solution (back-transformed on a preconditioned plan, section 7), after setMatrix('X') / setBlocks('X')
 *   the caller's X.
 * The product A X is truncated to the pattern of X, as every product of the solver is; blocks of X that carry no B
 *   block contribute |A X|^2.  This is the quantity `threshold` is defined on.
 * Arithmetic: every product and every sum runs in double, whatever the plan's precision.  'z': double data.  'c': float data converted
 *   on load, so that each float x float product is exact in double.  'm': the plan's double copies of X, B and A.  Always four real
 *   products per complex one, whatever setThreeProductMultiply says.
 * Deterministic: one [LN] record per chunk of a block column, written by one work group; the chunks of a column are added in chunk
 *   order by one work group per column; no atomics.  Two calls on the same data give the same bits.
 * The quotient is the IEEE one: a right-hand side with b = 0 gives NaN if r = 0, else +inf.  *worst ignores NaN entries; it is NaN only
 *   if every entry is.
 * Non-destructive: the call writes nothing into the caller's buffer -- not the work vectors v4 ... v9, not the partial sums and
 *   records of a solve, not its control block.  tfqmrgpuExt_getWorkVector and getBoundHistory behind it return what they returned in
 *   front of it, and a following solve is the solve it would have been.  Its scratch ([nChunks][2][LN] + [nCols][2][LN] doubles) is
 *   device memory that the library owns, allocated at the first call and released by destroyPlan and by bufferSize; bufferSize and the
 *   buffer layout do not change.  A plan that never calls it runs the launches it ran before.
 * Stream: asynchronous on the handle's stream up to the copy-out; it synchronises that stream once to fill the host arrays.  Do not
 *   call it during a solve.
 * All checks come before the first device call, in this order: plan / handle pointers as in getMatrix; no bufferSize yet:
 *   TFQMRGPU_UNDOCUMENTED_ERROR; all four outputs NULL: TFQMRGPU_STATUS_NO_INFO_PASSED; no buffer: TFQMRGPU_POINTER_INVALID; a plan with a
 *   user-defined operator (section 5): TFQMRGPU_NO_IMPLEMENTATION, the operator is the caller's to apply; A never set whole on this
 *   buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A' (status = 14 + 1000 * line + 10^7 * 'A'); the A in the buffer has been
 *   scaled by the preconditioner (section 7) and the plan keeps no copy: TFQMRGPU_NO_IMPLEMENTATION -- the caller's A is gone;
 *   `keepOperator` keeps it.  After any error nothing has been written, neither device nor host arrays.
 * With keepOperator (section 9) and a scaled buffer the kernel reads the kept copy ('m': its double part).  Patches of setBlocks('A')
 *   that no set-up has seen yet are in the copy already, so they count.
 * Several ranks (section 4): local to the rank's own block columns, no collective.  getInfo: nothing in it changes. */
tfqmrgpuStatus_t tfqmrgpuExt_residual(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double *residual2, double *bnorm2, int32_t *columns, double *worst);

/* ---- (11) truncation leak: what A X puts outside the pattern of X ------------------------------------------------------------- */
/* Every product of this library is truncated to the block pattern of X: solve, `threshold`, getInfo and residual
 * (section 10) all grade the TRUNCATED problem.  The pattern is the caller's choice -- a truncation radius around each source --, and
 * nothing above tells whether it was large enough.  What does is the part of A X that falls on block rows OUTSIDE a block column's
 * pattern: each of those missing blocks is a term of the untruncated residual B - A X~ (X~: X padded with zero blocks to full columns)
 * that section 10 leaves out.  With X~ zero there and B inside the pattern,
 *     |B - A X~|^2 (:, j) of block column c  =  residual2[c*LN + j] (section 10)  +  leak2[c*LN + j],
 * per right-hand side, so that a caller can widen or shrink the radius column by column.
 *
 * leak2[c*LN + j] = sum over the block rows i with (i, c) NOT in the pattern of X
 *                   of | sum over k with (i, k) in the pattern of A and (k, c) in the pattern of X of  A_ik X_kc  (:, j) |^2,
 *                   a HOST array [nCols][LN] of double, may be NULL; c is the compressed block column, as in section 10.  A block column
 *                   with no such row (a full column, say) gets exactly 0.0;
 * columns[c]      = the caller's block column index of compressed column c, a HOST array [nCols], may be NULL: as in section 10;
 * *nLeakBlocks    = the number of (block row, block column) positions outside the pattern of X that receive a product, may be NULL;
 * *nLeakPairs     = the number of block products that land there, may be NULL (the products inside the pattern: tfqmrgpuPlanView_t::nPairs).
 *
 * Operands: A is the caller's A -- the buffer's, or the kept copy (section 9) while the buffer holds A M^-1, patches of setBlocks('A')
 *   that no set-up has seen yet included; X what getMatrix('X') would return at that moment.  B is not read.
 * Arithmetic: every product and every sum runs in double, whatever the plan's precision.  'z': double data.  'c': float data converted
 *   on load, so that each float x float product is exact in double.  'm': the plan's double copies of X and A.  Always four real
 *   products per complex one, whatever setThreeProductMultiply says.
 * Deterministic: one [LN] record per work unit (a run of leak positions of one block column, cut by the number of products, so that a
 *   long shell is summed by several units), written by one work group; the units of a column are added in unit order by one work group
 *   per column, which writes 0 for a column without units; no atomics.  Two calls on the same data give the same bits.
 * Non-destructive: the call writes nothing into the caller's buffer -- not the work vectors v4 ... v9, not the partial sums and records
 *   of a solve, not its control block; a following solve is the solve it would have been.  bufferSize and the buffer layout do not change.
 * The listing of the leak positions and their products is built on the host from the plan's patterns at the first call, in time linear
 *   in the products of A X, the blocks of A and the blocks of X, and kept in the plan; its device copy and the records are device memory
 *   that the library owns, allocated by the first call that asks for leak2.  Both are released by destroyPlan and by bufferSize.  A plan
 *   that never makes the call runs the launches it ran before and allocates nothing.
 * Stream: the first call that asks for leak2 uploads the listing on the handle's stream and synchronises it once; every such call is
 *   asynchronous on that stream up to the copy-out and synchronises it once to fill leak2.  Do not call it during a solve.
 * All checks come before the first device call, in the order of section 10: plan / handle pointers; no bufferSize yet:
 *   TFQMRGPU_UNDOCUMENTED_ERROR; all four outputs NULL: TFQMRGPU_STATUS_NO_INFO_PASSED.  columns, nLeakBlocks and nLeakPairs depend on the
 *   patterns alone: with leak2 == NULL the call does the host analysis, launches nothing and returns HERE -- it needs the plan and
 *   bufferSize only, no buffer and no A.  With leak2: no buffer: TFQMRGPU_POINTER_INVALID; a plan with a user-defined operator:
 *   TFQMRGPU_NO_IMPLEMENTATION; A never set whole on this buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; the A in the
 *   buffer has been scaled by the preconditioner and the plan keeps no copy: TFQMRGPU_NO_IMPLEMENTATION.  After any error nothing has been
 *   written, neither device nor host arrays.
 * Several ranks (section 4): local to the rank's own block columns, no collective; every rank holds all of A, so its listing is complete. */
tfqmrgpuStatus_t tfqmrgpuExt_truncationLeak(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double *leak2, int32_t *columns, uint64_t *nLeakBlocks, uint64_t *nLeakPairs);
/* How the listing of truncationLeak is cut: the number of work units of every compressed block column into unitsPerColumn (a HOST array
 * [nCols], may be NULL); returns the number of work units of the plan, 0 while the listing has not been built. */
int64_t tfqmrgpuExt_leakUnits(tfqmrgpuBsrsvPlan_t plan, uint32_t *unitsPerColumn);

/* ---- (12) leak map: the truncation leak per position, and the pattern of X grown where it leaks ------------------------------------- */
/* Section 11 tells per block column how much of A X the truncation cut off.  A caller who sees a large leak2[c] still cannot tell WHICH
 * block rows to add to column c; all that is left is a larger geometric radius.  leakMap gives the leak of every single leak position
 * -- a (block row i, block column c) outside the pattern of X that receives a product --, and growPattern turns a chosen set of positions
 * into the BSR pattern of X for the next createPlan: solve, residual, truncationLeak, leakMap, growPattern, createPlan.  The pattern
 * grows where the operator carries weight out of it, not isotropically.
 *
 * rows[p]          = the block row of leak position p, 0-based whatever the plan's indexOffset, a HOST array [capacity], may be NULL;
 * cols[p]          = its COMPRESSED block column, as c in sections 10 and 11 (columns[] there gives the caller's index), a HOST array
 *                    [capacity], may be NULL;
 * pos2[p*LN + j]   = | sum over k with (i, k) in the pattern of A and (k, c) in the pattern of X of  A_ik X_kc  (:, j) |^2  for
 *                    (i, c) = (rows[p], cols[p]), a HOST array [capacity][LN] of double, may be NULL;
 * *nLeakBlocks     = the number of positions, nLeakBlocks of section 11, may be NULL.  All four NULL: TFQMRGPU_STATUS_NO_INFO_PASSED.
 *                    Only the first *nLeakBlocks entries of the arrays are written.
 *
 * The order of the positions is part of the interface: ascending compressed block column, then ascending block row.  Position p of
 *   leakMap is position p of growPattern.  The positions of block column c are consecutive; added up per right-hand side they are
 *   leak2[c*LN + j] of section 11, up to the rounding of a sum in another order.
 * Operands and arithmetic are section 11's: the caller's A -- the buffer's, or the kept copy (section 9) while the buffer holds A M^-1,
 *   patches of setBlocks('A') that no set-up has seen yet included --; X what getMatrix('X') would return at that moment; every product
 *   and every sum in double whatever the plan's precision ('c': float data converted on load, 'm': the plan's double copies), always
 *   four real products per complex one.
 * Deterministic: the [LN] record of a position is written by one wave (block shapes that are multiples of 16: the wave forms the whole
 *   block of A X of the position and adds its rows in one fixed order) or by one work group (4- and 8-row shapes: the rows are added in
 *   row order); no atomics, nothing is added across positions.  Two calls on the same data give the same bits.
 * Non-destructive: the call writes nothing into the caller's buffer; a following solve, residual or truncationLeak is the one it would
 *   have been.  bufferSize and the buffer layout do not change.
 * Memory: the listing of the positions is section 11's, built on the host at the first call of either section and uploaded ONCE, by the
 *   first call of either that needs it on the device.  The records, [nLeakBlocks][LN] doubles, are device memory that the library owns,
 *   allocated by the first call that asks for pos2, released by destroyPlan and by bufferSize.  A plan that never makes the call runs
 *   the launches it ran before and allocates nothing.
 * Stream: asynchronous on the handle's stream up to the copy-out ([nLeakBlocks][LN] doubles), then one synchronise (one more at the
 *   upload of the listing).  Do not call it during a solve.
 * All checks come before the first device call, those of section 11 in its order: plan / handle pointers; no bufferSize yet:
 *   TFQMRGPU_UNDOCUMENTED_ERROR; all four outputs NULL: TFQMRGPU_STATUS_NO_INFO_PASSED.  rows, cols and *nLeakBlocks depend on the patterns
 *   alone: with pos2 == NULL the call does the host analysis, launches nothing and needs the plan and bufferSize only.  With pos2: no
 *   buffer: TFQMRGPU_POINTER_INVALID; a plan with a user-defined operator: TFQMRGPU_NO_IMPLEMENTATION; A never set whole on this buffer:
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; the A in the buffer has been scaled by the preconditioner and the plan keeps no
 *   copy: TFQMRGPU_NO_IMPLEMENTATION.  Then, with any of the three arrays given, capacity < the number of positions:
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'; *nLeakBlocks (if given) HAS been filled in -- the room to come back with --
 *   and nothing else.  After any other error nothing has been written, neither device nor host arrays.
 * Several ranks (section 4): local to the rank's own block columns, as section 11. */
tfqmrgpuStatus_t tfqmrgpuExt_leakMap(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    uint64_t capacity,            /* positions the three arrays have room for */
    int32_t *rows,                /* HOST [capacity]      block row of each leak position, 0-based, may be NULL */
    int32_t *cols,                /* HOST [capacity]      COMPRESSED block column of each position, may be NULL */
    double  *pos2,                /* HOST [capacity][LN]  |(A X)(i,c)(:, j)|^2 per position and right-hand side, may be NULL */
    uint64_t *nLeakBlocks);       /* may be NULL; all four NULL: TFQMRGPU_STATUS_NO_INFO_PASSED */

/* The pattern of X with the leak positions take[0 .. nTake) added (indices into the order of leakMap; take == NULL: every position,
 * nTake is ignored), in the form createPlan reads: host only, it needs the plan and bufferSize.
 * Every block row keeps its old blocks in their old order; the added blocks of a row follow them, ascending by the caller's block column
 *   index.  oldBlock maps the values over: new block n holds old block oldBlock[n] of the caller's order, or is new (-1: zero, or a guess).
 *   nTake == 0 with a non-NULL list reproduces the old pattern (oldBlock = 0, 1, 2, ...).
 * The arrays are malloc'ed by the library (tfqmrgpuExt_freeGrownPattern releases them and zeroes the struct), as in section 4.
 * Cost: O(nnzbX + nTake + mb + nCols) behind the listing, which is built at the first call of this section or of section 11; nothing
 *   is searched.
 * plan or grown NULL: TFQMRGPU_POINTER_INVALID; no bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; an index >= nLeakBlocks or an index named
 *   twice: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'.  After any error *grown is zeroed (NULL arrays). */
typedef struct {
    int32_t  mb, nnzbX;
    int32_t *rowPtrX, *colIndX;   /* [mb+1], [nnzbX], with the plan's indexOffset and the CALLER'S block column indices */
    int32_t *oldBlock;            /* [nnzbX] position of the block in the old plan's caller order, -1 for an added block */
} tfqmrgpuGrownPattern_t;
tfqmrgpuStatus_t tfqmrgpuExt_growPattern(tfqmrgpuBsrsvPlan_t plan,
    uint64_t nTake, uint64_t const *take /* HOST, leak-map position indices; NULL: all positions (nTake ignored) */,
    tfqmrgpuGrownPattern_t *grown);
void tfqmrgpuExt_freeGrownPattern(tfqmrgpuGrownPattern_t *grown);

/* ---- (13) drop cost: what each block of X carries, and the pattern of X without chosen blocks ----------------------------------------- */
/* Sections 10 to 12 let a pattern grow where the operator carries weight out of it; nothing there tells which blocks the pattern holds
 * for nothing.  The pattern is the cost of everything: the buffer, every vector kernel and every block product scale with nnzbX.
 * dropCost gives per block of X how much of the residual rests on it, and shrinkPattern turns a list of blocks to drop into the BSR
 * pattern of X for the next createPlan: solve, residual, truncationLeak, leakMap, growPattern, dropCost, shrinkPattern, createPlan.
 *
 * For block n of X at (block row k, compressed block column c) and right-hand side j:
 * cost2[n*LN + j]   = sum over the block rows i with (i, k) in the pattern of A and (i, c) in the pattern of X of | A_ik X_kc (:, j) |^2,
 *                     a HOST array [nnzbX][LN] of double, may be NULL;
 * weight2[n*LN + j] = | X_kc (:, j) |^2, a HOST array [nnzbX][LN] of double, may be NULL;
 * *nProducts        = the number of block products, tfqmrgpuPlanView_t::nPairs, may be NULL.  All three NULL: TFQMRGPU_STATUS_NO_INFO_PASSED.
 *
 * The terms of cost2 are exactly the plan's own block products (tfqmrgpuPlanView_t::pairs) whose X operand is block n; every such
 *   product lands on a different block of A X, and each is squared ON ITS OWN.
 * What it says: let X' be X with block n set to zero.  A X' differs from A X, on the pattern, by exactly the blocks A_ik X_kc, so that
 *   for block column c and right-hand side j
 *       |B - A X'|  <=  sqrt(residual2[c*LN + j]) (section 10)  +  sqrt(cost2[n*LN + j]),     and
 *       |B - A X'|^2 =  cost2[n*LN + j]  where the residual is zero.
 *   For a SET of dropped blocks the square roots add (triangle inequality).  A caller drops block n when sqrt(cost2) is small against
 *   threshold * sqrt(bnorm2) of section 10.
 * What it does not say: a new solve on the shrunk pattern is a different truncated problem, not X'.  The dropped position becomes a leak
 *   position of the new plan, and section 11 measures it there.
 * Index and order: n is the caller's block order of X -- the order of bsrColIndX given to createPlan, whatever indexOffset was --, as in
 *   getWorkVector and setBlocks.  Of two blocks of X on the same (block row, block column) the pair list knows the first only; the
 *   second has no product.
 * Operands: A is chosen as in section 11 -- the buffer's, or the kept copy (section 9) while the buffer holds A M^-1, patches of
 *   setBlocks('A') that no set-up has seen yet included --; X what getMatrix('X') would return at that moment: after a solve the
 *   solution (back-transformed on a preconditioned plan), after setMatrix('X') / setBlocks('X') the caller's X.  B is not read.
 * Arithmetic: every product and every sum runs in double, whatever the plan's precision.  'z': double data.  'c': float data converted
 *   on load.  'm': the plan's double copies of X and A.  Always four real products per complex one.
 * Deterministic: one [LN] record per X block, written by one wave (block shapes that are multiples of 16) or by one work group (4- and
 *   8-row shapes: the rows are added in row order); the products of a block are added in the order of the pair list; no atomics,
 *   nothing is added across blocks.  Two calls on the same data give the same bits.
 * An X block with no product gets exactly 0.0 in cost2: its block row holds no A block in a row of the column's pattern.
 * Non-destructive: the call writes nothing into the caller's buffer; work vectors, bound history, residual, truncationLeak, leakMap and
 *   a following solve are bit for bit what they would have been.  bufferSize and the buffer layout do not change.
 * Memory: the listing -- the plan's pairs grouped by X block -- is built on the host in O(nPairs + nnzbX) by one stable counting sort at
 *   the first call that asks for an array, and uploaded once.  Its device copy and the records (2 x [nnzbX][LN] doubles) are device
 *   memory that the library owns, allocated by the first call that asks for an array, released by destroyPlan and by bufferSize.  The
 *   kernel writes each record at the caller's block index, so the copy-out is a plain copy.  A plan that never makes the call runs the
 *   launches it ran before and allocates nothing.
 * Stream: asynchronous on the handle's stream up to the copy-out (nnzbX * LN doubles per array), then one synchronise (one more at the
 *   upload of the listing).  Do not call it during a solve.
 * All checks come before the first device call, in the order of section 11: plan / handle pointers; no bufferSize yet:
 *   TFQMRGPU_UNDOCUMENTED_ERROR; all three outputs NULL: TFQMRGPU_STATUS_NO_INFO_PASSED; both arrays NULL with nProducts given: it is filled
 *   in from the plan alone and the call returns HERE -- no buffer and no A needed.  Then: no buffer: TFQMRGPU_POINTER_INVALID; a plan with
 *   a user-defined operator: TFQMRGPU_NO_IMPLEMENTATION; and with cost2 given: A never set whole on this buffer:
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; the A in the buffer has been scaled by the preconditioner and the plan keeps no
 *   copy: TFQMRGPU_NO_IMPLEMENTATION.  With weight2 only, A is not needed and the last two checks are skipped.  After any error nothing
 *   has been written, neither device nor host arrays nor *nProducts.
 * Several ranks (section 4): local to the rank's plan, no collective. */
tfqmrgpuStatus_t tfqmrgpuExt_dropCost(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double *cost2,                /* HOST [nnzbX][LN], may be NULL */
    double *weight2,              /* HOST [nnzbX][LN], may be NULL */
    uint64_t *nProducts);         /* = tfqmrgpuPlanView_t::nPairs, may be NULL */

/* The pattern of X without the blocks drop[0 .. nDrop) (block positions of X in the caller's order, 0-based whatever indexOffset), in
 * the form createPlan reads: host only, it needs the plan alone, not bufferSize.
 * Every block row keeps its other blocks in their old order.  rowPtrX and colIndX carry the plan's indexOffset and the caller's block
 *   column indices; oldBlock[n] is the old position of new block n, as in growPattern -- it is never -1 here.  Growing and shrinking
 *   compose through the two oldBlock maps.  nDrop == 0 reproduces the old pattern (drop may be NULL then).
 * A block column of X that loses all its blocks would vanish from the new pattern.  It would have held no B, and createPlan admits no
 *   such column (TFQMRGPU_B_HAS_A_ZERO_COLUMN): on a plan every block column keeps at least its blocks of B.
 * The arrays are malloc'ed by the library; tfqmrgpuExt_freeGrownPattern releases them.  Cost: O(nnzbX + nDrop + mb), no search.
 * plan or shrunk NULL, or drop NULL with nDrop > 0: TFQMRGPU_POINTER_INVALID; an index < 0, an index >= nnzbX or an index named twice:
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'; a listed block that carries a block of B (tfqmrgpuPlanView_t::subset):
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'B' -- createPlan needs B's pattern inside X's.  After any error *shrunk is zeroed. */
tfqmrgpuStatus_t tfqmrgpuExt_shrinkPattern(tfqmrgpuBsrsvPlan_t plan,
    uint64_t nDrop, int32_t const *drop /* HOST, block positions of X in the caller's order */,
    tfqmrgpuGrownPattern_t *shrunk);   /* released by tfqmrgpuExt_freeGrownPattern */

/* ---- (14) warm start: solve from the X in the plan --------------------------------------------------------------------------------- */
/* tfqmrgpu_bsrsv_solve zeroes X, as the reference does (tfqmrgpu_core.hxx:125): whatever setMatrix('X') brought, or the last solve left,
 * is ignored.  The loops that sections 8 to 13 serve all end in a solve that has a good X at hand: the re-solve on a grown or shrunk
 * pattern (sections 12, 13: the old values mapped through oldBlock), the next energy of a loop that patches the diagonal blocks of A
 * (sections 8, 9), and a solve that ended at TFQMRGPU_STATUS_MAX_ITERATIONS.  solveFrom solves A X = B starting from X0, the X in the
 * plan; tfqmrgpu_bsrsv_solve itself is unchanged and still ignores X.
 *
 * X0 is what getMatrix('X') would return at that moment: after a solve the solution (back-transformed on a preconditioned plan,
 *   section 7), after setMatrix('X') / setBlocks('X') the caller's X.
 * It runs as a correction solve: R = B - A X0, truncated to the pattern of X as every product is and formed in the
 *   plan's precision; tfQMR solves A D = R from zero with the kernels and the driver of tfqmrgpu_bsrsv_solve; then X = X0 + D.
 * threshold and getInfo keep their meaning: every residual is RELATIVE TO |B| per right-hand side, not to |R|; the bound of the
 *   recurrence starts at |r|^2 / |b|^2 instead of 1.  A solve from a converged X0 stops after its first iteration, whose probe confirms it.
 * Afterwards getBoundHistory, getInfo and getWorkVector(.., 1) are as after solve: the iterations are those of the correction solve,
 *   flops_performed includes the product A X0, the residual pass and the update.  getWorkVector(.., 4 ... 9) return the vectors of the
 *   CORRECTION solve A D = R, started from D = 0 with R as its right-hand side: they belong to D, not to X.
 * A right-hand side whose R is exactly zero keeps its X0 bit for bit: it is neither a breakdown nor a NaN, and takes no part in the
 *   status (it is treated as a zero column of B is in solve).  A right-hand side with b = 0 has nothing to be relative to and is graded
 *   against |r|, as in a cold solve of the correction system.
 * maxIterations <= 0: X = X0 is left untouched; the status is TFQMRGPU_STATUS_MAX_ITERATIONS, as solve returns for it.
 * tfqmrgpu_bsrsv_solve on the same plan, before or after, is bit for bit the solve it was: the same launches, the same buffer.
 * Precisions: 'z' and 'c'.  'm': TFQMRGPU_NO_IMPLEMENTATION -- the refinement has a cycle 0 and a |b|^2 bookkeeping of its own: section 16.
 * Preconditioner (section 7): supported.  R needs the caller's A: the buffer's while it has not been scaled -- R is formed first, then
 *   the set-up scales A --, the kept copy (section 9) once it has, patches of setBlocks('A') that no set-up has seen yet included, as in
 *   section 10.  The correction solve runs on A M^-1; its result is back-transformed into D before X0 is added.  Scaled and no copy kept:
 *   TFQMRGPU_NO_IMPLEMENTATION, as residual.
 * A user-defined operator (section 5): TFQMRGPU_NO_IMPLEMENTATION.  Several ranks (section 4): TFQMRGPU_NO_IMPLEMENTATION on every rank,
 *   through the collective in front of a solve, so that all ranks leave together.
 * Deterministic: one work group per chunk and per block column of the plan's own tables, every sum in a fixed order, no atomics.  Two
 *   calls from the same X0 give the same bits.
 * Memory: X0 and R, two X-shaped vectors in the plan's precision, are device memory that the library owns, allocated by the first call,
 *   released by destroyPlan, bufferSize and setBuffer.  A X0 lives in work vector v9, which the driver writes before it reads.  bufferSize
 *   and the buffer layout do not change; a plan that never makes the call allocates nothing and runs the launches it ran before.
 * Stream: asynchronous on the handle's stream; it synchronises where solve does.  Do not call it during a solve.
 * All checks come before the first device call, in the order of section 10: plan / handle pointers: TFQMRGPU_POINTER_INVALID; no
 *   bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; no buffer: TFQMRGPU_POINTER_INVALID; a user-defined operator: TFQMRGPU_NO_IMPLEMENTATION;
 *   an 'm' plan: TFQMRGPU_NO_IMPLEMENTATION; A never set whole on this buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; A
 *   scaled and no copy kept: TFQMRGPU_NO_IMPLEMENTATION.  After any error nothing has been written: not X, not the results of the last solve. */
tfqmrgpuStatus_t tfqmrgpuExt_solveFrom(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double threshold, int maxIterations);

/* ---- (15) carry A, B and X from one plan to another on the device ------------------------------------------------------------------- */
/* Every turn of the loop of sections 10 to 14 -- residual, truncationLeak, leakMap and growPattern, dropCost and shrinkPattern,
 * createPlan, solveFrom -- ends in a NEW plan, while the operands sit in the old plan's buffer.  carry copies one operand of `src` into
 * `dst` device to device, through a block map, and zero-fills the blocks that are new: no host transfer of values, no scratch memory of
 * the caller's, every byte moved once.
 *
 * The map: block n of operand `var` of dst becomes block oldBlock[n] of the same operand of src; oldBlock[n] == -1 makes it a zero
 *   block.  n counts in dst's caller block order (the order of the bsrColInd array given to createPlan), oldBlock[n] in src's; both are
 *   0-based whatever indexOffset: exactly what tfqmrgpuGrownPattern_t::oldBlock of growPattern and shrinkPattern holds.  nBlocks must be
 *   dst's nnzb of that operand.  oldBlock == NULL is the identity and needs equal nnzb in both plans (A and B: their patterns do not
 *   change in the loop).  A source block may be named more than once.  The map is the caller's claim: block rows and block columns are
 *   not compared.
 * Source values.  'X': what getMatrix('X') of src would return at that moment -- the back-transformed solution after a preconditioned
 *   solve, or the caller's X after setMatrix('X') / setBlocks('X').  'B': what the last setMatrix('B') / setBlocks('B') left.  'A': the
 *   caller's A, chosen as in section 10: the buffer's A, or the kept copy of section 9 while the buffer holds A M^-1; patches of
 *   setBlocks('A') that no set-up has seen yet are included.
 * Effects on dst: exactly those of a whole setMatrix(var).  For 'A': A counts as set, the preconditioner is stale (the next solve sets it
 *   up again), the float floor of an 'm' plan and pending patches are forgotten, and an 'm' plan gets both its copies of A, the double
 *   one and the float one.  src is only read.
 * Precisions: 'z', 'c' and 'm' on either side, in every combination.  The operand is read and written in each plan's storage precision
 *   (an 'm' plan stores X, B and A in double): float -> double is exact, double -> float rounds to nearest, once.  So a cheap 'c' solve on
 *   a coarse pattern can seed a 'z' plan for solveFrom.  Each plan keeps its own element order inside a block; the call translates.
 * LM and LN must be the same in both plans.
 * Stream: asynchronous on the handle's stream; work of src that is pending on another stream is the caller's to wait for.  Uploading the
 *   list synchronises that stream once (A and B without a list upload nothing).  Do not call it during a solve of either plan.
 * Memory: the device copy of the list is library-owned memory of dst, grown on demand and released by destroyPlan.  bufferSize and the
 *   buffer layout do not change; a plan that never makes the call allocates nothing and runs the launches it ran before.
 * Deterministic: a copy.  Two calls give the same bits.
 * All checks come before the first device call, in this order: handle, dst or src NULL, or dst == src: TFQMRGPU_POINTER_INVALID; either
 *   plan without bufferSize: TFQMRGPU_UNDOCUMENTED_ERROR; an unknown var: the status of setMatrix (TFQMRGPU_VARIABLENAME_UNKNOWN with the
 *   key character var); LM or LN differ: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'L'; nBlocks is not dst's nnzb, the list is
 *   NULL and the two nnzb differ, an entry is below -1, or an entry is at or above src's nnzb: TFQMRGPU_UNDOCUMENTED_ERROR with the key
 *   character var; (nBlocks == 0 with nnzb 0 returns success HERE and touches nothing;) either plan without a buffer:
 *   TFQMRGPU_POINTER_INVALID; for 'A' the source checks of section 10 on src: a user-defined operator: TFQMRGPU_NO_IMPLEMENTATION; A never
 *   set whole: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; A scaled and no copy kept: TFQMRGPU_NO_IMPLEMENTATION.  After any
 *   error nothing has been written, not in either buffer and not in the plan state.
 * Several ranks (section 4): local to the rank's own two plans, no collective. */
tfqmrgpuStatus_t tfqmrgpuExt_carry(tfqmrgpuHandle_t handle,
    tfqmrgpuBsrsvPlan_t dst, tfqmrgpuBsrsvPlan_t src, char var /* 'A', 'B', 'X' */,
    int32_t nBlocks, int32_t const *oldBlock /* HOST [nBlocks], or NULL */);

/* ---- (16) mixed-precision warm start: refine from the X in the plan ------------------------------------------------------------------ */
/* The loop of sections 8 to 15 ends every turn in a solve that has a good X at hand, and the fastest solver, the mixed-precision plan
 * ('m': float tfQMR inside a refinement in double), was the one that could not take part: solveFrom refuses it (section 14), and solve
 * starts the refinement from zero and throws away the digits X already has.  refineFrom runs the refinement from X0, the X in the plan.
 *
 * 'z' and 'c' plans: the call IS tfqmrgpuExt_solveFrom (section 14), call for call -- the same statuses, the same bits --, so that one
 *   call serves a loop in any precision.  What follows describes 'm' plans.
 * X0 is what getMatrix('X') would return at that moment: the last solution (back-transformed on a preconditioned plan, section 7), or
 *   what setMatrix('X') / setBlocks('X') / carry (section 15) brought.  It is read from the plan's double copy.
 * It runs as a correction refinement: R = B - A X0, truncated to the pattern of X as every product is, formed ONCE, in double, from the
 *   caller's A in its double copy; then the refinement of solve on A D = R from D = 0 -- per cycle r = R - A D in double (cycle 0: r = R),
 *   A d = r by the float tfQMR driver and its kernels, unchanged, D += d in double --; then X = X0 + D in double.
 * threshold and getInfo keep the meaning they have after solve on an 'm' plan: max over the right-hand sides of |B - A X| / |B| in
 *   double.  |B|^2 per right-hand side comes from B, not from the first cycle's |r|^2.  A right-hand side with b = 0 has nothing to be
 *   relative to and is graded against its own |r0|, as in section 14.  getInfo: iterations is the sum of the float iterations,
 *   residuum_reached the final residual; flops_performed additionally counts the product A X0, the residual pass and the update.
 * getRefinementHistory: residual[0] is |B - A X0| / |B| in front of the first float solve -- no longer 1 --, the last entry is the
 *   final residual, iterations[i] are as after solve.  getBoundHistory holds the bounds of the float solves, as after solve.
 * X0 already converged -- the first residual is at or below threshold --: TFQMRGPU_STATUS_SUCCESS with 0 iterations, and X keeps X0
 *   bit for bit: no float solve, no back transform, no update.
 * maxIterations <= 0: X = X0 is left untouched bit for bit; the status is TFQMRGPU_STATUS_MAX_ITERATIONS and getInfo is as solveFrom
 *   leaves it in that case.
 * A right-hand side whose R is exactly zero keeps its X0 bit for bit through every cycle: a right-hand side only ever sees itself, so
 *   its D stays exactly zero, and the update keeps X0's bits where D is 0.  It is neither a breakdown nor a NaN and takes no part in
 *   the status.
 * Stagnation and breakdown are reported as solve reports them on an 'm' plan: two cycles without a factor 2 end the refinement with
 *   TFQMRGPU_STATUS_MAX_ITERATIONS (TFQMRGPU_STATUS_BREAKDOWN if the last float solve broke down).  X is then X0 + the D reached.
 * tfqmrgpu_bsrsv_solve on the same plan, before or after, is bit for bit the solve it was: the same launches, the same buffer layout,
 *   the same bufferSize.  refineFrom reads the float floor that solve remembers per plan for its first cycle and does NOT write it: a
 *   later solve does not depend on whether a refineFrom ran in between.
 * Preconditioner (section 7): supported, in the order of section 14.  R is formed first and needs the caller's A: the buffer's double A
 *   while it has not been scaled, the double part of the kept copy (section 9) once it has, patches of setBlocks('A') that no set-up
 *   has seen yet included, as in section 10.  Then the set-up; the cycles run on A M^-1; D is back-transformed before X0 is added.
 *   Scaled and no copy kept: TFQMRGPU_NO_IMPLEMENTATION, as residual.
 * A user-defined operator (section 5): TFQMRGPU_NO_IMPLEMENTATION.  Several ranks (section 4): TFQMRGPU_NO_IMPLEMENTATION on every
 *   rank, through the mixed solve's own first collective -- the max-reduction of three doubles with the third value set; exactly one
 *   collective, so that all ranks leave together.  ('z' and 'c' plans: the vote of section 14, by forwarding.)
 * Deterministic: one work group per chunk and per block column of the plan's own tables, every sum in a fixed order, no atomics.  Two
 *   calls from the same X0 give the same bits.
 * Memory: X0 and R, two X-shaped vectors of doubles, are device memory that the library owns -- the allocation of section 14, sized
 *   for doubles --, allocated by the first call, released by destroyPlan, bufferSize and setBuffer.  A X0 lives in the work vectors
 *   that the refinement uses for A x (v4 ... v7).  A plan that never makes the call allocates nothing and runs the launches it ran before.
 * Stream: asynchronous on the handle's stream; it synchronises where solve does on an 'm' plan.  Do not call it during a solve.
 * All checks come before the first device call, in the order of section 14: plan / handle pointers: TFQMRGPU_POINTER_INVALID; no
 *   bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; no buffer: TFQMRGPU_POINTER_INVALID; a user-defined operator:
 *   TFQMRGPU_NO_IMPLEMENTATION; A never set whole on this buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; A scaled and no
 *   copy kept: TFQMRGPU_NO_IMPLEMENTATION.  After any error nothing has been written: not X, not the results of the last solve, not
 *   the float floor. */
tfqmrgpuStatus_t tfqmrgpuExt_refineFrom(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double threshold, int maxIterations);

/* ---- (17) start projection: blend the kept solutions per right-hand side ------------------------------------------------------------- */
/* Every turn of the loop of sections 8 to 16 ends in solveFrom / refineFrom from "the X in the plan", and that X is ONE vector: the solution
 * of the previous energy.  A caller who has solved at E1, E2, E3 holds three good vectors when E4 arrives.  These calls keep up to four
 * solutions in the plan and, in front of the solve, put into X the combination of them that minimises the residual of the NEW system
 * (Fischer's projection for successive right-hand sides).  Every right-hand side of every block column is a system of its own here, so
 * the projection is a k x k least-squares problem per (compressed block column c, right-hand side j), k <= 4; nothing couples columns or
 * ranks.  The loop: setBlocks('A'), projectStart, solveFrom, pushStart.  Nothing that exists changes; solveFrom starts from a better X0.
 *
 * keepStarts(plan, depth): the plan keeps the `depth` newest starts, depth = 0 (the default: off) ... 4.  Call it after bufferSize; it
 *   survives bufferSize and setBuffer as the preconditioner kind does (the starts themselves do not: they hold values of one buffer).  A depth
 *   outside 0 ... 4: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X' (status = 14 + 1000 * line + 10^7 * 'X').  A smaller depth drops
 *   the oldest starts, 0 releases everything; changing the depth while starts are held waits for the device (the call has no stream).  A
 *   plan that never calls it, or calls it with 0, is bit for bit the plan it was: same launches, same buffer, same results.
 * pushStart: copies what getMatrix('X') would return at that moment -- after a solve the solution (back-transformed on a preconditioned
 *   plan, section 7), after setMatrix('X') / setBlocks('X') / carry the caller's X -- into slot 0; the older starts move up one slot, and
 *   with `depth` starts held the oldest leaves.  The copy is device to device on the handle's stream, in the plan's storage precision and
 *   internal order; an 'm' plan copies its double X.  Checks, in this order: plan / handle pointers: TFQMRGPU_POINTER_INVALID; no
 *   bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; depth 0: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'; no buffer:
 *   TFQMRGPU_POINTER_INVALID.
 * startCount: the number of starts held, 0 ... depth (0 for a plan pointer that is none).  startDepth: the depth that keepStarts set, which
 *   sizes `coefficients` of projectStart (0 for a plan pointer that is none).
 *
 * projectStart works with the k = startCount starts S_0 (the newest) ... S_{k-1}:
 *   W_i = A S_i by the plan's own multiply, truncated to the pattern of X as every product is, in the plan's storage
 *     precision.  A is the caller's A, chosen as in section 14: the buffer's A while it has not been scaled, the kept copy (section 9)
 *     once it has, patches of setBlocks('A') that no set-up has seen yet included.  'm' plans use the double side, as refineFrom does.
 *   Per (c, j), with <u, v> = sum conj(u) v over the blocks of block column c and column j of each block, all summed in double:
 *     G_il = <W_i, W_l>,  g_i = <W_i, B>,  |B|^2;  B is zero under X blocks that carry no B block, as in sections 10 and 14.
 *   gamma minimises |B - sum_i gamma_i W_i|: G gamma = g by a Cholesky factorisation G = L L^H in double, the starts taken in the order
 *     newest first.  Start i is DROPPED for that right-hand side (gamma_i = 0, it takes no part in the rows behind it) when its pivot
 *     d_i = G_ii - sum_{l < i} |L_il|^2 is not greater than G_ii * TFQMRGPU_PROJECT_PIVOT_DOUBLE (2^-26, double storage: 'z' and 'm') or
 *     G_ii * TFQMRGPU_PROJECT_PIVOT_FLOAT (2^-12, 'c') -- the square root of the rounding unit of the storage type.  Normal equations can
 *     be trusted only while 1 / cond^2 stays above the rounding of the Gram entries; a start below the threshold adds less than that
 *     fraction of a new direction.  A start with G_ii = 0 is dropped.  A right-hand side with b = 0 gets gamma = 0 and nUsed = 0.
 *   x := sum_i gamma_i[c, j] S_i is written into the plan's X: accumulated in double by fused multiply-adds in slot order, rounded once
 *     to the storage precision.  The ring is not changed.
 *   coefficients[((c*LN + j)*depth + i)*2 + {0, 1}] = Re, Im of gamma_i, a HOST array [nCols][LN][depth][2] of double, zeros for dropped
 *     and absent slots, may be NULL;  nUsed[c*LN + j] = the number of kept starts, a HOST array [nCols][LN], may be NULL.  With both
 *     NULL the call still projects.
 *   No residual is returned: tfqmrgpuExt_residual (section 10) grades the result on the same A, B and X.  By construction, up to
 *     rounding, the projected residual of every right-hand side is at most that of X = S_0 and at most |B|.
 * All checks of projectStart come before the first device call, in the order of section 14: plan / handle pointers:
 *   TFQMRGPU_POINTER_INVALID; no bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; no buffer: TFQMRGPU_POINTER_INVALID; a user-defined operator
 *   (section 5): TFQMRGPU_NO_IMPLEMENTATION; A never set whole on this buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; A
 *   scaled and no copy kept: TFQMRGPU_NO_IMPLEMENTATION; no start held: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'.  After any
 *   error nothing has been written: not X, not the host arrays.
 * Precisions: 'z', 'c' and 'm'.  Several ranks (section 4): local to the rank's own block columns, no collective, like section 10.
 * Deterministic: one record of k^2 + 2k + 1 doubles per right-hand side and chunk (the diagonal of G, Re / Im of its upper triangle,
 *   Re / Im of g, |B|^2), written by one work group; the chunks of a column are added in chunk order by one work group per column; no
 *   atomics.  Two calls give the same bits.
 * Non-destructive: the three calls write nothing into the caller's buffer but X (projectStart) -- not the work vectors v4 ... v9, not the
 *   results of the last solve, not its control block, not the float floor of an 'm' plan; getWorkVector, getBoundHistory and getInfo
 *   behind them return what they returned in front of them.
 * Memory: library-owned device memory -- `depth` starts, allocated by the first pushStart; `depth` images W, the records and gamma,
 *   allocated by the first projectStart.  Released by destroyPlan, bufferSize, setBuffer and keepStarts(plan, 0).  bufferSize and the
 *   buffer layout do not change.
 * Stream: asynchronous on the handle's stream; projectStart synchronises it once if a host array is asked for.  Do not call any of them
 *   during a solve. */
#define TFQMRGPU_PROJECT_PIVOT_DOUBLE 1.4901161193847656e-08   /* 2^-26 */
#define TFQMRGPU_PROJECT_PIVOT_FLOAT  2.44140625e-04           /* 2^-12 */
tfqmrgpuStatus_t tfqmrgpuExt_keepStarts(tfqmrgpuBsrsvPlan_t plan, int depth);                 /* 0 (default, off) ... 4 */
tfqmrgpuStatus_t tfqmrgpuExt_pushStart(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan);    /* X of the plan -> slot 0, older ones move up */
int32_t          tfqmrgpuExt_startCount(tfqmrgpuBsrsvPlan_t plan);                            /* starts held, 0 ... depth */
int32_t          tfqmrgpuExt_startDepth(tfqmrgpuBsrsvPlan_t plan);                            /* the depth kept, 0 ... 4 */
tfqmrgpuStatus_t tfqmrgpuExt_projectStart(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double *coefficients /* HOST [nCols][LN][depth][2] (Re, Im), may be NULL */,
    int32_t *nUsed       /* HOST [nCols][LN], may be NULL */);

/* ---- (18) padded plans: any block shape up to 64 x 64 on the listed kernels ---------------------------------------------------------- */
/* The solver has kernels for the fifteen block shapes of tfqmrgpu_bsrsv_allowedBlockSizes; every other shape ends at bufferSize with
 * TFQMRGPU_BLOCKSIZE_MISSING.  Callers come with (lmax+1)^2 = 9, 25, 36, with 18 or 50 when spin is included, or with one right-hand side
 * per block column.  With padding allowed, bufferSize picks the smallest listed shape that holds the caller's, and the operand calls move
 * the caller's COMPACT blocks into and out of it on the device.  The caller's shape is lm x ln, the plan's LM x LN.
 *
 * Why it is exact.  In every block of A, B and X the rows lm ... LM-1 are zero, in A their columns too; the columns ln ... LN-1 of B and X
 *   are zero; the diagonal blocks of A carry 1 on the padded part of their diagonal.  Then A_pad = A (+) 1 is as regular as A; every Krylov
 *   vector stays exactly 0 in the padding, because 0 * finite sums to 0 in every multiply; the padded right-hand sides are zero columns of
 *   B, which the solve and sections 10 to 17 already treat as such; and the inverse in the block-Jacobi set-up (section 7) is A_ii^-1 (+) 1
 *   -- without the ones every padded diagonal block would be singular and fall back to M_ii = 1.  No iteration kernel, no window of the
 *   buffer and no reduction knows of the padding: a padded plan IS the plan of shape LM x LN fed with the padded operands, bit for bit.
 *
 * allowPadding(plan, on): call it after createPlan and before bufferSize; default 0.  It survives bufferSize and setBuffer, as the
 *   preconditioner kind does.  A plan pointer that is none: TFQMRGPU_POINTER_INVALID.  A plan that never calls it, or calls it with 0, is
 *   bit for bit the plan it was: the same statuses (TFQMRGPU_BLOCKSIZE_MISSING included), the same launches, the same buffer.
 * bufferSize(ldA = blockDim = lm, ldB = RhsBlockDim = ln, ...) on a plan with padding on: the checks ldA == blockDim, ldB == RhsBlockDim and
 *   the pointer checks stay, in their order; the check lm > ln is dropped -- a caller may bring fewer right-hand sides than rows, down to
 *   ln = 1; lm < 1 or ln < 1: TFQMRGPU_UNDOCUMENTED_ERROR.  The plan's shape is the listed (LM, LN) with LM >= lm and LN >= ln that has the
 *   smallest LM for which such an LN exists, then the smallest such LN (LM first: the products cost LM^2 LN).  A listed (lm, ln) picks
 *   itself; the plan is then not padded and runs the path of a plan without the switch.  lm > 64 or ln > 64: TFQMRGPU_BLOCKSIZE_MISSING
 *   with lm and ln, as without padding.  The buffer size returned is that of the plan's shape.
 * paddedShape(plan, &lm, &ln, &LM, &LN): the caller's shape as given to bufferSize, and the plan's; any pointer may be NULL.  Before
 *   bufferSize: TFQMRGPU_UNDOCUMENTED_ERROR.  On a plan that is not padded the two pairs are equal.
 *
 * WHICH CALL SPEAKS WHICH SHAPE.
 *   The caller's shape: bufferSize and the four operand calls -- setMatrix, getMatrix, setBlocks, getBlocks (section 8), with host or
 *     device `values`, every layout, every `trans`, 'm' plans with 'c' or 'z' data.  The arrays hold compact blocks: A [nnzbA] blocks of
 *     lm x lm, B and X blocks of lm x ln (ln x lm where `trans` says so) -- exactly what a plan of that shape without padding would take.
 *     Setting writes EVERY element of each block of the buffer it touches: the caller's values inside, +0.0 in the padding, 1.0 in the
 *     real plane of the padded diagonal of the blocks of A whose block row equals their block column; nothing stale survives a set.
 *     Getting reads the inside only.  All checks and their order are those of a plan without padding: these calls gain no status.
 *   The plan's shape (paddedShape tells it): the per-right-hand-side arrays of sections 10 to 17, sized [nCols][LN]; getPreconditioner,
 *     sized [mb][2][LM][LM]; getWorkVector, get / setShadowVector and planView (LM, LN); the flop counts of getInfo, which count the
 *     padded products.  The padded right-hand sides are zero columns of B: residual2 = bnorm2 = 0 there, which *worst ignores, and
 *     nUsed = 0.
 *   carry (section 15) requires equal caller's shapes on both plans as well as equal plan shapes; otherwise its status with the key 'L'.
 *   tfqmrgpu_bsrsv_z / _c, the Fortran wrappers and allowedBlockSizes are unchanged and keep refusing unlisted shapes.
 *   A user-defined operator (section 5) on a padded plan: solve returns TFQMRGPU_NO_IMPLEMENTATION, on several ranks through the vote, as
 *     the preconditioner's refusal travels -- the callback contract names one shape.
 *
 * WHAT PADDING COSTS: the buffer, the memory traffic and the products of the PLAN's shape.  25 x 25 on 32 x 32 is 1.64 x the elements of X
 *   and 2.1 x the products; 9 x 9 on 16 x 16 is 3.2 x and 5.6 x.  What is saved is the host pass over every operand on either side of
 *   every solve, and setBlocks / getBlocks with device arrays keep their point.
 * Memory: one byte per block of A in library-owned device memory (which blocks are diagonal blocks), built from A's pattern at the first
 *   padded transfer of A, uploaded once, released by destroyPlan.  No scratch beyond the staging that the operand calls have.
 * Several ranks (section 4): local to the rank's plan; every rank pads alike. */
tfqmrgpuStatus_t tfqmrgpuExt_allowPadding(tfqmrgpuBsrsvPlan_t plan, int on);      /* default 0 */
tfqmrgpuStatus_t tfqmrgpuExt_paddedShape(tfqmrgpuBsrsvPlan_t plan,
    int32_t *lm, int32_t *ln,      /* the caller's block shape, as given to bufferSize */
    int32_t *LM, int32_t *LN);     /* the plan's shape: one of the fifteen; any pointer may be NULL */

/* ---- (19) energy mesh: shift A's diagonal, sum X, one call -------------------------------------------------------------------------- */
/* Sections 8 to 18 serve one loop: solve at energy E1, change the diagonal blocks of A, solve at E2 from what is known.  Where the change
 * is a multiple of the unit matrix, A(E) = A_base + sigma(E) 1, two steps of that loop still crossed the host at every energy: the caller
 * added sigma on the host and sent all mb diagonal blocks through setBlocks('A'), and fetched X with getBlocks to add it into a weighted
 * sum -- a contour integral wants sum_E w_E X(E) on the on-site blocks, not X(E).  shiftDiagonal and the sum do both on the device, and
 * solveMesh runs the whole loop.  The energies run one after the other through the iteration kernels as they are: nothing that exists changes.
 *
 * (19a) shiftDiagonal(handle, plan, sigmaRe, sigmaIm): A := A_base + sigma 1.  Only the diagonal elements of the diagonal blocks of A are
 *   written -- mb * lm complex numbers, which the device already holds.
 * A_base is the diagonal of the caller's A as the last setMatrix('A'), setBlocks('A') or carry(.., 'A') (section 15) left it: mb * LM
 *   complex numbers in the plan's storage precision ('m': double) in library-owned device memory.  The first shift behind such a write
 *   captures it: from the buffer's A, or from the kept copy (section 9) while the buffer holds A M^-1.  Those three writes call it stale,
 *   and only where they have written: a setMatrix('A') or carry that has written a whole A all of it, a setBlocks('A') that has succeeded
 *   the block rows whose diagonal block it names -- their part of the base becomes the diagonal of the blocks it wrote, the other rows
 *   keep theirs (the A around them may carry a shift), so that a patch between two energies patches A_base, however often it is made.  A
 *   call that is refused (the wrong precision, no values, ...) has written nothing and leaves the base as it is.
 *   Shifts do not accumulate: shift(sigma) followed by shift(0) gives back A_base (its bits, but for a -0.0 on the diagonal, which
 *   -0.0 + 0.0 turns into +0.0 -- on the host as well).
 * Arithmetic, per component (Re, Im), one rounding each: 'z' and the double A of an 'm' plan: base + sigma in double; 'c': sigma is
 *   rounded to float once, then added in float; the float A of an 'm' plan gets the shifted DOUBLE value rounded to float (to nearest),
 *   which is what setBlocks('A') with 'z' data writes there.
 * Contract: the call is bit for bit setBlocks('A', all diagonal blocks, 'n') with A_base_ii + sigma 1 formed on the host as above --
 *   in the A window(s) of the buffer, or in the kept copy on a plan whose A is scaled and kept; and in the plan's state: the float floor
 *   of an 'm' plan is forgotten; on a kept plan every block row and block column that holds a diagonal block is marked, so that the next
 *   set-up redoes them (section 9); "a whole A has been set" stays as it was.
 * Padded plans (section 18): only the first lm diagonal elements of a block move; the ones on the padded diagonal stay:
 *   A_pad = (A + sigma 1) (+) 1.
 * All checks come before the first device call, in the order of section 8: plan / handle pointers: TFQMRGPU_POINTER_INVALID; no
 *   bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; a user-defined operator (section 5): TFQMRGPU_NO_IMPLEMENTATION; no buffer:
 *   TFQMRGPU_POINTER_INVALID; A never set whole on this buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'A'; a block row of A
 *   without a diagonal block in the pattern -- A + sigma 1 cannot be represented --: TFQMRGPU_UNDOCUMENTED_ERROR with the key character
 *   'D'; A scaled and no copy kept: TFQMRGPU_NO_IMPLEMENTATION, as setBlocks('A').  After any error nothing has been written.
 * Memory: the base (mb * LM complex numbers) and, unless the block-Jacobi set-up has uploaded it already (section 7), the list of the
 *   diagonal blocks (mb indices) are device memory that the library owns, allocated by the first call, released by destroyPlan,
 *   bufferSize and setBuffer.  A plan that never makes the call allocates nothing.
 * Stream: one launch ('m': two, the double and the float A) of one thread per diagonal element on the handle's stream, no
 *   synchronisation; the first call behind a write of A adds one launch that captures, and behind a setBlocks('A') the upload of the
 *   list of its rows, which synchronises once.  Do not call it during a solve.  Several ranks (section 4): every rank holds all of A and shifts its own.
 *
 * (19b) the weighted sum S = sum w X on the nnzbB blocks of X that carry a block of B (tfqmrgpuPlanView_t::subset).
 * keepSum(plan, on): default off.  Call it after bufferSize; it survives bufferSize and setBuffer as the depth of keepStarts does (the
 *   sum itself does not: it holds values of one buffer).  Every call, on or off, ends the sum that is held (it waits for the device: the
 *   call has no stream); behind keepSum(plan, 1) S is zero.  A plan that never calls it is bit for bit the plan it was and allocates nothing.
 * addToSum(handle, plan, wRe, wIm): S += w X.  X is what getMatrix('X') would return at that moment -- the back-transformed solution on
 *   a preconditioned plan, the double X of an 'm' plan.  S is complex double in every precision; 'c' data is converted on load (exactly).
 *   Per element, in exactly this order, every operation rounded once to double, nothing contracted:
 *     t1 = wRe * xRe;  t2 = wIm * xIm;  S.re += (t1 - t2);      t3 = wRe * xIm;  t4 = wIm * xRe;  S.im += (t3 + t4);
 *   so that a host restatement in real double arithmetic gives the same bits.  One thread per complex element, no atomics; nothing is
 *   written into the caller's buffer.
 * getSum(handle, plan, values, nTerms): values is a HOST array [nnzbB][lm][ln][2] of double -- B's block order, blocks row-major,
 *   (Re, Im); on a padded plan (section 18) the caller's compact shape, as getBlocks speaks it --; *nTerms the number of addToSum calls
 *   since the sum was last zero.  Either pointer may be NULL.  It synchronises the stream once where `values` is given.
 * clearSum(handle, plan): S := 0, *nTerms := 0.
 * Checks of addToSum, getSum and clearSum, in the order of pushStart (section 17): plan / handle pointers: TFQMRGPU_POINTER_INVALID; no
 *   bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; keepSum off: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'; no buffer:
 *   TFQMRGPU_POINTER_INVALID.  A user-defined operator (section 5) is accepted: the sum only reads X.
 * Memory: S, nnzbB * LM * LN complex doubles of library-owned device memory, allocated and cleared by the first addToSum, released by
 *   destroyPlan, bufferSize, setBuffer and keepSum.  Stream: asynchronous on the handle's stream.  Several ranks (section 4): the sum
 *   is local to the rank's own block columns; no collective.
 *
 * (19c) solveMesh: for e = 0 ... nE - 1 exactly these public calls, in this order:
 *     1. shiftDiagonal(sigma[e]);
 *     2. e == 0 and fromX == 0: tfqmrgpu_bsrsv_solve(threshold, maxIterations); otherwise projectStart(NULL, NULL) if startCount > 0,
 *        then refineFrom(threshold, maxIterations) (section 16; on 'z' and 'c' plans that is solveFrom);
 *     3. getInfo into iterations[e] and residual[e]; the status of the solve into status[e];
 *     4. pushStart if startDepth > 0;
 *     5. addToSum(weight[e]) if weight is given and the sum is kept.
 *   The mesh is bit for bit the same loop written by the caller.  It stops behind the first energy whose solve returns neither
 *   TFQMRGPU_STATUS_SUCCESS nor TFQMRGPU_STATUS_MAX_ITERATIONS (steps 4 and 5 of that energy do not run) and returns that status; a
 *   status other than success of any other step ends it as well and is returned.  Otherwise it returns
 *   TFQMRGPU_STATUS_MAX_ITERATIONS if the solve of any energy returned it, else TFQMRGPU_STATUS_SUCCESS.  *nDone is the number of
 *   energies whose solve ran; the host arrays are written for those energies only.  A stays at the last sigma applied, X is the last solution.
 * Checks in front of the loop, in this order: plan / handle pointers: TFQMRGPU_POINTER_INVALID (*nDone, if given, is 0 from here on);
 *   sigma == NULL: TFQMRGPU_POINTER_INVALID; nE <= 0: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'E'; several ranks (section 4):
 *   TFQMRGPU_NO_IMPLEMENTATION, decided from the handle's own rank count -- the same on every rank, no collective, nothing written --; a
 *   user-defined operator (section 5): TFQMRGPU_NO_IMPLEMENTATION.  Then those of shiftDiagonal, by the call itself.
 * iterations, residual, status and nDone may be NULL.  The call synchronises where its solves do. */
tfqmrgpuStatus_t tfqmrgpuExt_shiftDiagonal(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double sigmaRe, double sigmaIm);
tfqmrgpuStatus_t tfqmrgpuExt_keepSum(tfqmrgpuBsrsvPlan_t plan, int on);                        /* default 0 */
tfqmrgpuStatus_t tfqmrgpuExt_addToSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, double wRe, double wIm);
tfqmrgpuStatus_t tfqmrgpuExt_getSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double *values   /* HOST [nnzbB][lm][ln][2] (Re, Im), may be NULL */,
    int32_t *nTerms  /* may be NULL */);
tfqmrgpuStatus_t tfqmrgpuExt_clearSum(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan);
tfqmrgpuStatus_t tfqmrgpuExt_solveMesh(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan, int32_t nE,
    double const *sigma  /* HOST [nE][2] (Re, Im) */,
    double const *weight /* HOST [nE][2] (Re, Im), may be NULL */,
    double threshold, int maxIterations, int fromX,
    int32_t *iterations, double *residual, tfqmrgpuStatus_t *status /* HOST [nE] each, may be NULL */,
    int32_t *nDone       /* may be NULL */);

/* ---- (20) selection on the device: the blocks to drop and the leak positions to take ------------------------------------------------ */
/* The loop of sections 10 to 15 -- residual, truncationLeak, leakMap, growPattern, dropCost, shrinkPattern, createPlan, carry,
 * solveFrom -- moves whole record arrays to the host in two places, for a rule of one line that the caller then applies: cost2
 * [nnzbX][LN] of section 13 to find the blocks to drop, pos2 [nLeakBlocks][LN] of section 12 to find the positions to take.  The operands
 * of both rules are on the device already.  selectDrop and selectLeak apply them there, and only the chosen indices (and one [LN] sum per
 * block column) cross to the host.
 *
 * selectDrop.  Block n of X, at block row k and compressed block column c, is selected when
 *   (1) it carries no block of B (tfqmrgpuPlanView_t::subset) -- shrinkPattern refuses such a block --, and
 *   (2) cost2[n*LN + j] <= (eta*eta) * bnorm2[c*LN + j]  for EVERY j < LN.
 * blocks[0 .. *nSelected) = the selected blocks in the caller's block order of X, ascending, a HOST array [capacity], may be NULL: the
 *                           `drop` argument of shrinkPattern as it stands;
 * spent[c*LN + j]         = the sum over the selected blocks n of block column c of sqrt(cost2[n*LN + j]), a HOST array [nCols][LN] of
 *                           double, may be NULL: the triangle-inequality bound of section 13 on what dropping the whole set adds to
 *                           the residual norm of that right-hand side.  A caller checks a budget with it and bisects eta.
 *
 * selectLeak.  Position p of the leak map (section 12: ascending compressed block column, then block row), in block column c, is
 * selected when there is a j < LN with  bnorm2[c*LN + j] > 0  and  pos2[p*LN + j] > (eta*eta) * bnorm2[c*LN + j].
 * take[0 .. *nSelected) = the selected positions, ascending, a HOST array [capacity], may be NULL: the `take` argument of growPattern as
 *                         it stands;
 * left[c*LN + j]        = the sum of pos2[p*LN + j] over the positions of block column c that were NOT selected, a HOST array
 *                         [nCols][LN] of double, may be NULL: the leak that stays.
 *
 * Both.  *nSelected = the number selected, may be NULL.  All three outputs NULL: TFQMRGPU_STATUS_NO_INFO_PASSED.
 * The rules are part of the interface: applied in numpy to what dropCost, leakMap and residual return at that moment, they give the
 *   same index lists, entry for entry.  cost2 is bit for bit dropCost's, pos2 leakMap's, bnorm2 residual's -- the same kernels write
 *   them into the same library-owned memory; eta*eta is rounded once in double (on the host), its product with bnorm2 once (on the
 *   device); nothing is contracted into a fused multiply-add.  A comparison that involves a NaN is false: a block with a NaN in its
 *   record is not dropped, a NaN never makes a position taken.
 * Padded right-hand sides (section 18) have bnorm2 = 0 and cost2 = pos2 = 0: they pass the <= of selectDrop and never meet the > of
 *   selectLeak.  No special case.
 * Operands and arithmetic are those of sections 10, 12 and 13: the caller's A -- the buffer's, or the kept copy (section 9) while the
 *   buffer holds A M^-1 --; X what getMatrix('X') would return at that moment; every product and sum in double on 'z', 'c' and 'm'.
 * Deterministic.  The list ascends by construction: one flag per block (position), then an ordered compaction in three plain passes --
 *   the flags set per tile of 256 items, one work group that turns the tile counts into prefix sums, one work group per tile that writes
 *   its indices behind its prefix.  No work group waits for another.  spent and left: one work group per block column; lane t has
 *   right-hand side t % LN and is number r = t / LN of the R = floor(256 / LN) lanes of that right-hand side; it adds the column's
 *   entries r, r + R, r + 2 R, ... in that order -- the column's blocks in the plan's internal order, sorted by block row, for spent;
 *   its leak positions, sorted by block row, for left --, and the R partial sums are added in ascending r.  No atomics: two calls on
 *   the same data give the same bits.  The values are those of that order, not of a host sum; compare them within
 *   (entries of the column) * 2^-52 * (the sum of the magnitudes).
 * Non-destructive: nothing in the caller's buffer is written.  Work vectors, bound history, and a solve, residual, dropCost or leakMap
 *   that follows are bit for bit what they would have been.  bufferSize and the buffer layout do not change.
 * Memory: the records are those of sections 10, 12 and 13, in their memory.  The flags, the tile counts, the index list, the per-column
 *   sums and three index lists of the plan (selectDrop: the block column of every block, the blocks of every column; selectLeak: the
 *   block column of every position, the first position of every column) are device memory that the library owns, allocated and
 *   uploaded by the first call of each kind, released by destroyPlan and by bufferSize.  A plan that never makes the call allocates
 *   nothing and launches nothing new.
 * Stream: asynchronous on the handle's stream up to ONE synchronise for the copy-out (one more in a first call that uploads a listing).
 *   What is copied: the count, min(capacity, items) 32-bit indices if the index array is given, [nCols][LN] doubles if the sums are.
 *   With only nSelected given the call counts and copies out eight bytes or fewer.  Do not call it during a solve.
 * All checks but one come before the first device call, in the order of sections 12 and 13: plan / handle pointers:
 *   TFQMRGPU_POINTER_INVALID; no bufferSize yet: TFQMRGPU_UNDOCUMENTED_ERROR; all three outputs NULL: TFQMRGPU_STATUS_NO_INFO_PASSED;
 *   eta < 0 or a NaN: TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'E'; no buffer: TFQMRGPU_POINTER_INVALID; a plan with a
 *   user-defined operator: TFQMRGPU_NO_IMPLEMENTATION; A never set whole on this buffer: TFQMRGPU_UNDOCUMENTED_ERROR with the key
 *   character 'A'; the A in the buffer has been scaled by the preconditioner and the plan keeps no copy: TFQMRGPU_NO_IMPLEMENTATION.
 *   The exception needs the count, so it comes behind the kernels: the index array given and capacity < the number selected:
 *   TFQMRGPU_UNDOCUMENTED_ERROR with the key character 'X'; *nSelected (if given) HAS been filled in -- the room to come back with --
 *   and nothing else.  After any other error nothing has been written, neither the host arrays nor *nSelected.
 * Several ranks (section 4): local to the rank's plan, no collective. */
tfqmrgpuStatus_t tfqmrgpuExt_selectDrop(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double eta, uint64_t capacity,
    int32_t  *blocks,             /* HOST [capacity], may be NULL: the selected X blocks, caller's order, ascending */
    uint64_t *nSelected,          /* may be NULL */
    double   *spent);             /* HOST [nCols][LN], may be NULL */
tfqmrgpuStatus_t tfqmrgpuExt_selectLeak(tfqmrgpuHandle_t handle, tfqmrgpuBsrsvPlan_t plan,
    double eta, uint64_t capacity,
    uint64_t *take,               /* HOST [capacity], may be NULL: the selected leak-map positions, ascending */
    uint64_t *nSelected,          /* may be NULL */
    double   *left);              /* HOST [nCols][LN], may be NULL */

#ifdef __cplusplus
}
#endif
#endif /* TFQMRGPU_EXT_H */
