/* Host-side check of the argument validation of libprd_backbone.so (include/prd_backbone.h), meant to run under AddressSanitizer on a
 * machine WITHOUT a GPU: every call below must be refused (a negative PRD_BACKBONE_ERR_* code) before any HIP API is touched, with no
 * out-of-bounds access on the host side.
 * Build + run: protein_redesign_amd.build.build_side_check("backbone")   (tests/test_backbone_cpu.py) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/prd_backbone.h"

static int failures = 0;
#define EXPECT(call, code)                                                                 \
    do {                                                                                   \
        const int got_ = (call);                                                           \
        if (got_ != (code)) { printf("FAIL %s -> %d (want %d)\n", #call, got_, (code)); ++failures; } \
    } while (0)

/* the arguments of a call that would be accepted; a test changes one of them */
struct args {
    float* atoms; int* built;
    const float* x; long long xs; int xr; const float *mask, *link, *table;
    float g[13]; int S, N;       /* l0, ac, rc, ao, ro, an, rn, ka, kb, kc, bond_lo2, bond_hi2, sin2_min */
};

static int build(const struct args* a) {
    return prd_backbone_build(a->atoms, a->built, a->x, a->xs, a->xr, a->mask, a->link, a->table, a->g[0], a->g[1], a->g[2], a->g[3], a->g[4], a->g[5],
                              a->g[6], a->g[7], a->g[8], a->g[9], a->g[10], a->g[11], a->g[12], a->S, a->N, 0);
}

int main(void) {
    float* fbuf = (float*)malloc(16 * sizeof(float));    /* host memory standing in for device pointers: never followed by the checks */
    int* ibuf = (int*)malloc(16 * sizeof(int));
    const struct args ok = {fbuf, ibuf, fbuf, 30, 3, fbuf, fbuf, fbuf,
                            {3.80395484f, 1.42842114f, 0.534076810f, 1.64217305f, 1.74637675f, -1.40831709f, -0.377368599f,
                             -0.58273431f, 0.56802827f, -0.54067466f, 10.89f, 18.49f, 0.0301536899f},
                            2, 5};
    struct args a;
    EXPECT(prd_backbone_version(), PRD_BACKBONE_VERSION);
#define WITH(change, code) do { a = ok; change; EXPECT(build(&a), code); } while (0)
    WITH(a.atoms = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.built = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.x = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.mask = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.link = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.table = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.S = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.N = 0, PRD_BACKBONE_ERR_ARG);
    WITH(a.S = -1, PRD_BACKBONE_ERR_ARG);
    WITH(a.N = -7, PRD_BACKBONE_ERR_ARG);
    WITH(a.xr = 2, PRD_BACKBONE_ERR_ARG);
    WITH(a.xs = -1, PRD_BACKBONE_ERR_ARG);
    for (int k = 0; k < 13; ++k) {                   /* every scalar: not finite */
        WITH(a.g[k] = NAN, PRD_BACKBONE_ERR_ARG);
        WITH(a.g[k] = INFINITY, PRD_BACKBONE_ERR_ARG);
        WITH(a.g[k] = -INFINITY, PRD_BACKBONE_ERR_ARG);
    }
    WITH(a.g[0] = 0.f, PRD_BACKBONE_ERR_ARG);        /* l0 */
    WITH(a.g[0] = -3.8f, PRD_BACKBONE_ERR_ARG);
    WITH(a.g[7] = 0.f, PRD_BACKBONE_ERR_ARG);        /* ka: D-residues are not on offer */
    WITH(a.g[7] = 0.58f, PRD_BACKBONE_ERR_ARG);
    WITH((a.g[10] = 18.49f, a.g[11] = 10.89f), PRD_BACKBONE_ERR_ARG);     /* a bad window */
    WITH(a.g[10] = a.g[11], PRD_BACKBONE_ERR_ARG);
    WITH(a.g[10] = 0.f, PRD_BACKBONE_ERR_ARG);
    WITH(a.g[10] = -1.f, PRD_BACKBONE_ERR_ARG);
    WITH(a.g[12] = -0.01f, PRD_BACKBONE_ERR_ARG);    /* sin^2 outside [0, 1) */
    WITH(a.g[12] = 1.f, PRD_BACKBONE_ERR_ARG);
    WITH(a.N = PRD_BACKBONE_MAX_N + 1, PRD_BACKBONE_ERR_UNSUPPORTED);
    WITH(a.S = PRD_BACKBONE_MAX_S + 1, PRD_BACKBONE_ERR_UNSUPPORTED);
    WITH((a.N = PRD_BACKBONE_MAX_N + 1, a.xr = 2), PRD_BACKBONE_ERR_ARG);   /* a bad argument is named before a limit */
    free(fbuf);
    free(ibuf);
    if (failures) {
        printf("%d FAILED\n", failures);
        return 1;
    }
    printf("backbone_abi_check OK\n");
    return 0;
}
