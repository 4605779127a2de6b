/* Host-side walk of a plan's life for a sanitizer build (scripts/host_sanitize.sh): the paths that need no device.
 * createPlan -> bufferSize -> bufferSize with another shape -> destroyPlan, and the argument checks of setBlocks / getBlocks /
 * setMatrix / getMatrix that return before the first device call -- what tests/test_blocks_cpu.py walks through Python.
 * Prints "host_walk: OK" and returns 0 when every status is the expected one; the sanitizers speak for themselves. */
#include <stdio.h>
#include <stdint.h>
#include <stddef.h>
#include "tfqmrgpu.h"
#include "tfqmrgpu_ext.h"

static int failures = 0;
#define CODE(st) ((int)((st) % 1000))
#define EXPECT(call, code) do { tfqmrgpuStatus_t const st_ = (call); if (CODE(st_) != (code)) { ++failures; \
    printf("line %d: %s returned %d, expected code %d\n", __LINE__, #call, (int)st_, (code)); } } while (0)

int main(void) {
    /* a 3 x 3 block tridiagonal A, X dense in one block column, B its first block */
    int32_t const rowPtrA[4] = {0, 2, 5, 7}, colIndA[7] = {0, 1, 0, 1, 2, 1, 2};
    int32_t const rowPtrX[4] = {0, 1, 2, 3}, colIndX[3] = {0, 0, 0};
    int32_t const rowPtrB[4] = {0, 1, 1, 1}, colIndB[1] = {0};
    static double values[7 * 2 * 8 * 8];
    tfqmrgpuHandle_t handle = NULL;
    tfqmrgpuBsrsvPlan_t plan = NULL;
    size_t bytes = 0;
    int32_t list[4] = {0, 2, 1, 0};
    int const OK = TFQMRGPU_STATUS_SUCCESS, PTR = TFQMRGPU_POINTER_INVALID, UND = TFQMRGPU_UNDOCUMENTED_ERROR;
    tfqmrgpuDataLayout_t const L = TFQMRGPU_LAYOUT_RIRIRIRI;

    EXPECT(tfqmrgpuCreateHandle(&handle), OK);
    EXPECT(tfqmrgpu_bsrsv_createPlan(handle, &plan, 3, rowPtrA, 7, colIndA, rowPtrX, 3, colIndX, rowPtrB, 1, colIndB, 0, 0), OK);
    /* before bufferSize */
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 1, list, values, 'z', 'n', L), UND);
    EXPECT(tfqmrgpuExt_getBlocks(handle, plan, 'X', 1, NULL, values, 'z', 'n', L), UND);
    EXPECT(tfqmrgpu_bsrsv_setMatrix(handle, plan, 'A', values, 'z', 4, 4, 'n', L), UND);

    EXPECT(tfqmrgpu_bsrsv_bufferSize(handle, plan, 4, 4, 4, 4, 'z', &bytes), OK);
    EXPECT(tfqmrgpuExt_setPreconditioner(plan, TFQMRGPU_PRECOND_BLOCK_JACOBI), OK);
    EXPECT(tfqmrgpuExt_keepOperator(plan, 1), OK);
    EXPECT(tfqmrgpu_bsrsv_bufferSize(handle, plan, 4, 4, 8, 8, 'm', &bytes), OK);      /* another shape, another precision */
    EXPECT(tfqmrgpu_bsrsv_bufferSize(handle, plan, 8, 8, 4, 4, 'z', &bytes), UND);     /* LM > LN: refused, the plan stays */
    EXPECT(tfqmrgpu_bsrsv_bufferSize(handle, plan, 4, 4, 7, 7, 'z', &bytes), TFQMRGPU_BLOCKSIZE_MISSING);
    EXPECT(tfqmrgpu_bsrsv_bufferSize(handle, plan, 8, 8, 8, 8, 'z', &bytes), OK);
    EXPECT(tfqmrgpuExt_keepOperator(plan, 0), OK);
    EXPECT(tfqmrgpuExt_keepOperator(plan, 1), OK);

    /* the list checks, in the order the entry points have them; a valid list reaches the buffer check */
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 0, NULL, NULL, 'z', 'n', L), OK);
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', -1, list, values, 'z', 'n', L), UND);
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 2, NULL, values, 'z', 'n', L), PTR);
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 4, list, values, 'z', 'n', L), UND);      /* block 0 twice */
    EXPECT(tfqmrgpuExt_getBlocks(handle, plan, 'X', 4, list, values, 'z', 'n', L), PTR);      /* reading twice is harmless: no buffer */
    list[3] = 7;
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 4, list, values, 'z', 'n', L), UND);      /* 7 is past the end of A */
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'B', 1, list + 1, values, 'z', 'n', L), UND);  /* 2 is past the end of B */
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'X', 3, list, values, 'z', 'n', L), PTR);
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 3, list, values, 'z', 'n', L), PTR);
    EXPECT(tfqmrgpuExt_getBlocks(handle, plan, 'X', 1, NULL, values, 'z', 'n', L), PTR);      /* B's pattern: no buffer */
    EXPECT(tfqmrgpuExt_getBlocks(handle, plan, 'X', 2, NULL, values, 'z', 'n', L), PTR);      /* B's pattern has one block */
    EXPECT(tfqmrgpuExt_getBlocks(handle, plan, 'A', 1, list, values, 'z', 'n', L), UND);      /* only X: getMatrix's status */
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'Q', 1, list, values, 'z', 'n', L), TFQMRGPU_VARIABLENAME_UNKNOWN);
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 1, list, values, 'z', 'q', L), TFQMRGPU_TANSPOSITION_UNKNOWN);
    EXPECT(tfqmrgpuExt_setBlocks(handle, plan, 'A', 1, list, values, 'z', 'n', (tfqmrgpuDataLayout_t)0x77), TFQMRGPU_DATALAYOUT_UNKNOWN);
    EXPECT(tfqmrgpu_bsrsv_setMatrix(handle, plan, 'A', values, 'z', 8, 8, 'n', L), PTR);
    EXPECT(tfqmrgpu_bsrsv_getMatrix(handle, plan, 'X', values, 'z', 8, 8, 'n', L), PTR);
    EXPECT(tfqmrgpu_bsrsv_getMatrix(handle, plan, 'B', values, 'z', 8, 8, 'n', L), UND);
    EXPECT(tfqmrgpuExt_multiplyRelease(NULL), OK);

    EXPECT(tfqmrgpu_bsrsv_destroyPlan(handle, plan), OK);
    EXPECT(tfqmrgpu_bsrsv_destroyPlan(handle, NULL), PTR);
    /* a plan that never saw bufferSize */
    plan = NULL;
    EXPECT(tfqmrgpu_bsrsv_createPlan(handle, &plan, 3, rowPtrA, 7, colIndA, rowPtrX, 3, colIndX, rowPtrB, 1, colIndB, 0, 0), OK);
    EXPECT(tfqmrgpu_bsrsv_destroyPlan(handle, plan), OK);
    EXPECT(tfqmrgpuDestroyHandle(handle), OK);
    if (failures) { printf("host_walk: %d unexpected statuses\n", failures); return 1; }
    printf("host_walk: OK\n");
    return 0;
}
