/* Host-side check of the argument validation of libprd_sasa.so (include/prd_sasa.h), meant to run under AddressSanitizer on a machine
 * WITHOUT a GPU: every call below must be refused (a negative PRD_SASA_ERR_* code) before any HIP API is touched, with no out-of-bounds
 * access on the host side.
 * Build + run: protein_redesign_amd.build.build_side_check("sasa")   (tests/test_sasa_cpu.py) */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/prd_sasa.h"

static int failures = 0;
#define EXPECT(call, code)                                                                 \
    do {                                                                                   \
        const int got_ = (call);                                                           \
        if (got_ != (code)) { printf("FAIL %s -> %d (want %d)\n", #call, got_, (code)); ++failures; } \
    } while (0)

/* the arguments of a call that would be accepted; a test changes one of them */
struct args {
    int* count; const float* pos; long long stride_s, stride_a; const float* reach; const int *present, *group; const float* sphere;
    int mode, S, A, P;
};

static int count(const struct args* a) {
    return prd_sasa_count(a->count, a->pos, a->stride_s, a->stride_a, a->reach, a->present, a->group, a->sphere, a->mode, a->S, a->A, a->P, 0);
}

int main(void) {
    float* fbuf = (float*)malloc(16 * sizeof(float));    /* host memory standing in for device pointers: never followed by the checks */
    int* ibuf = (int*)malloc(16 * sizeof(int));
    const struct args ok = {ibuf, fbuf, 15, 3, fbuf, ibuf, ibuf, fbuf, PRD_SASA_SAME_GROUP, 2, 5, 256};
    struct args a;
    EXPECT(prd_sasa_version(), PRD_SASA_VERSION);
#define CALL(change, code) do { a = ok; change; EXPECT(count(&a), code); } while (0)
    CALL(a.count = 0, PRD_SASA_ERR_ARG);
    CALL(a.pos = 0, PRD_SASA_ERR_ARG);
    CALL(a.reach = 0, PRD_SASA_ERR_ARG);
    CALL(a.present = 0, PRD_SASA_ERR_ARG);
    CALL(a.sphere = 0, PRD_SASA_ERR_ARG);
    CALL(a.group = 0, PRD_SASA_ERR_ARG);                 /* SAME_GROUP without group */
    CALL(a.S = 0, PRD_SASA_ERR_ARG);
    CALL(a.A = 0, PRD_SASA_ERR_ARG);
    CALL(a.P = 0, PRD_SASA_ERR_ARG);
    CALL(a.S = -1, PRD_SASA_ERR_ARG);
    CALL(a.A = -7, PRD_SASA_ERR_ARG);
    CALL(a.P = -64, PRD_SASA_ERR_ARG);
    CALL(a.mode = 2, PRD_SASA_ERR_ARG);
    CALL(a.mode = -1, PRD_SASA_ERR_ARG);
    CALL(a.stride_a = 2, PRD_SASA_ERR_ARG);              /* rows that overlap */
    CALL(a.stride_a = 0, PRD_SASA_ERR_ARG);
    CALL(a.stride_a = -3, PRD_SASA_ERR_ARG);
    CALL(a.stride_s = 14, PRD_SASA_ERR_ARG);             /* structures that overlap: (A - 1) stride_a + 3 = 15 */
    CALL(a.stride_s = 0, PRD_SASA_ERR_ARG);
    CALL(a.stride_s = -15, PRD_SASA_ERR_ARG);
    CALL((a.stride_a = 4, a.stride_s = 18), PRD_SASA_ERR_ARG);
    CALL((a.stride_a = LLONG_MAX, a.stride_s = LLONG_MAX), PRD_SASA_ERR_ARG);      /* the product is formed without overflow */
    CALL(a.P = 100, PRD_SASA_ERR_UNSUPPORTED);
    CALL(a.P = 63, PRD_SASA_ERR_UNSUPPORTED);
    CALL(a.P = PRD_SASA_MAX_P + 64, PRD_SASA_ERR_UNSUPPORTED);
    CALL((a.A = PRD_SASA_MAX_A + 1, a.stride_s = 3LL * (PRD_SASA_MAX_A + 1)), PRD_SASA_ERR_UNSUPPORTED);
    CALL(a.S = PRD_SASA_MAX_S + 1, PRD_SASA_ERR_UNSUPPORTED);
    CALL((a.P = 100, a.reach = 0), PRD_SASA_ERR_ARG);    /* a bad argument is named before a limit */
    CALL((a.mode = PRD_SASA_ALL, a.group = 0, a.P = 100), PRD_SASA_ERR_UNSUPPORTED);       /* ALL takes no group: only the limit is left */
    free(fbuf);
    free(ibuf);
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("sasa_abi_check OK\n");
    return 0;
}
