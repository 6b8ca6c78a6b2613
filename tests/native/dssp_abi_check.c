/* Host-side check of the argument validation of libprd_dssp.so (include/prd_dssp.h), meant to run under AddressSanitizer on a machine
 * WITHOUT a GPU: every call below must be refused (a negative PRD_DSSP_ERR_* code) before any HIP API is touched, with no out-of-bounds
 * access on the host side.
 * Build + run: protein_redesign_amd.build.build_side_check("dssp")   (tests/test_dssp_cpu.py) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/prd_dssp.h"

static int failures = 0;
#define EXPECT(call, code)                                                                 \
    do {                                                                                   \
        const int got_ = (call);                                                           \
        if (got_ != (code)) { printf("FAIL %s -> %d (want %d)\n", #call, got_, (code)); ++failures; } \
    } while (0)

/* the arguments of two calls that would be accepted; a test changes one of them */
struct args {
    int* partner; float* energy; uint8_t* classes; int *flags, *bridge;
    const float* atoms; const int* built; const float *link, *donor;
    float q, e_min, cutoff, cos_bend; int S, N;
};

static int hbonds(const struct args* a) {
    return prd_dssp_hbonds(a->partner, a->energy, a->atoms, a->built, a->link, a->donor, a->q, a->e_min, a->S, a->N, 0);
}

static int assign(const struct args* a) {
    return prd_dssp_assign(a->classes, a->flags, a->bridge, a->partner, a->energy, a->atoms, a->built, a->link, a->cutoff, a->cos_bend, a->S, a->N, 0);
}

int main(void) {
    float* fbuf = (float*)malloc(16 * sizeof(float));    /* host memory standing in for device pointers: never followed by the checks */
    int* ibuf = (int*)malloc(16 * sizeof(int));
    const struct args ok = {ibuf, fbuf, (uint8_t*)ibuf, ibuf, ibuf, fbuf, ibuf, fbuf, fbuf, 27.888f, -9.9f, -0.5f, 0.342020143f, 2, 5};
    struct args a;
    EXPECT(prd_dssp_version(), PRD_DSSP_VERSION);
#define BOTH(change, code) do { a = ok; change; EXPECT(hbonds(&a), code); EXPECT(assign(&a), code); } while (0)
#define HB(change, code) do { a = ok; change; EXPECT(hbonds(&a), code); } while (0)
#define AS(change, code) do { a = ok; change; EXPECT(assign(&a), code); } while (0)
    BOTH(a.partner = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.energy = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.atoms = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.built = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.link = 0, PRD_DSSP_ERR_ARG);
    AS(a.classes = 0, PRD_DSSP_ERR_ARG);
    AS(a.flags = 0, PRD_DSSP_ERR_ARG);
    AS(a.bridge = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.S = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.N = 0, PRD_DSSP_ERR_ARG);
    BOTH(a.S = -1, PRD_DSSP_ERR_ARG);
    BOTH(a.N = -7, PRD_DSSP_ERR_ARG);
    const float bad[3] = {NAN, INFINITY, -INFINITY};
    for (int k = 0; k < 3; ++k) {                        /* every scalar: not finite */
        HB(a.q = bad[k], PRD_DSSP_ERR_ARG);
        HB(a.e_min = bad[k], PRD_DSSP_ERR_ARG);
        AS(a.cutoff = bad[k], PRD_DSSP_ERR_ARG);
        AS(a.cos_bend = bad[k], PRD_DSSP_ERR_ARG);
    }
    HB(a.q = 0.f, PRD_DSSP_ERR_ARG);
    HB(a.q = -27.888f, PRD_DSSP_ERR_ARG);
    HB(a.e_min = 0.f, PRD_DSSP_ERR_ARG);
    HB(a.e_min = 9.9f, PRD_DSSP_ERR_ARG);
    AS(a.cutoff = 0.f, PRD_DSSP_ERR_ARG);
    AS(a.cutoff = 0.5f, PRD_DSSP_ERR_ARG);
    AS(a.cos_bend = 1.f, PRD_DSSP_ERR_ARG);
    AS(a.cos_bend = -1.f, PRD_DSSP_ERR_ARG);
    AS(a.cos_bend = 1.5f, PRD_DSSP_ERR_ARG);
    BOTH(a.N = PRD_DSSP_MAX_N + 1, PRD_DSSP_ERR_UNSUPPORTED);
    BOTH(a.S = PRD_DSSP_MAX_S + 1, PRD_DSSP_ERR_UNSUPPORTED);
    BOTH((a.N = PRD_DSSP_MAX_N + 1, a.link = 0), PRD_DSSP_ERR_ARG);       /* a bad argument is named before a limit */
    free(fbuf);
    free(ibuf);
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("dssp_abi_check OK\n");
    return 0;
}
