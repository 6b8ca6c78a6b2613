/* Launch trace of SINGLE calls of the GEMM family (prd_gemm, prd_ln_rows, prd_softmax_rows, prd_single_fc1_folded and the two host
 * queries prd_gemm_slab_ok / prd_single_fc1_folded_ok), for a machine WITHOUT a GPU.  Linked against the trace build of the library
 * (csrc/prd_launch.h under -DPRD_LAUNCH_TRACE: a launch prints "L kernel grid block lds args" and returns 0).  One case per line of
 * stdin:
 *     <id> <entry> key=value key=value ...
 * Integer keys are the fields of PrdGemm (or the arguments of the entry) by name; a POINTER key (colscale, bias, addmat, colmask,
 * rowmask, mulmat, resid, ln_out, C2, rscale, ws, wsum, out_ln, a_amax; x, y, gamma for ln_rows) is 0 = NULL, 1 = a dummy non-null
 * 16-byte aligned address, 2 = the same address + 4 bytes (misaligned).  A, B and C are always given.  Per case the driver prints
 *     # <id>
 *     the library's own L lines
 *     C <entry> = <return code>        (Q <entry> = <value> for the queries)
 * tests/test_gemm_dispatch_cpu.py feeds it the table of tests/gemm_cases.py.  No device is touched.
 * Build: protein_redesign_amd.build.build_gemm_dispatch() */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/prd_hip.h"

/* dummy device pointers: distinct, 16-byte aligned, never dereferenced */
#define DP(k) ((float*)(uintptr_t)(0x100000000ull + (unsigned long long)(k) * 0x10000000ull))
#define BIG ((size_t)1 << 44)

#define MAXKV 64
static char* keys[MAXKV];
static long long vals[MAXKV];
static int nkv;

static long long get(const char* key, long long dflt) {
    for (int i = 0; i < nkv; ++i)
        if (!strcmp(keys[i], key)) return vals[i];
    return dflt;
}

/* 0 -> NULL, 1 -> DP(k), 2 -> DP(k) + 4 bytes */
static float* ptr(const char* key, int k, long long dflt) {
    const long long v = get(key, dflt);
    if (!v) return NULL;
    return (float*)((char*)DP(k) + (v == 2 ? 4 : 0));
}

int main(void) {
    static char line[4096];
    hipStream_t s = 0;
    while (fgets(line, sizeof line, stdin)) {
        char* id = strtok(line, " \t\r\n");
        if (!id || id[0] == '#') continue;
        char* entry = strtok(NULL, " \t\r\n");
        if (!entry) { fprintf(stderr, "case %s: no entry\n", id); return 2; }
        nkv = 0;
        for (char* t = strtok(NULL, " \t\r\n"); t; t = strtok(NULL, " \t\r\n")) {
            char* eq = strchr(t, '=');
            if (!eq || nkv == MAXKV) { fprintf(stderr, "case %s: bad token %s\n", id, t); return 2; }
            *eq = 0;
            keys[nkv] = t;
            vals[nkv++] = atoll(eq + 1);
        }
        printf("# %s\n", id);
        const int arith = (int)(get("arith", 0) | PRD_TUNE(get("tune", 0)));
        if (!strcmp(entry, "gemm")) {
            PrdGemm g;
            memset(&g, 0, sizeof g);
            g.A = ptr("A", 1, 1); g.B = ptr("B", 2, 1); g.C = ptr("C", 3, 1);
            g.M = (int)get("M", 0); g.N = (int)get("N", 0); g.K = (int)get("K", 0);
            g.lda = (int)get("lda", g.K); g.ldb = (int)get("ldb", get("b_kn", 0) ? g.N : g.K); g.ldc = (int)get("ldc", g.N);
            g.G1 = (int)get("G1", 1); g.G2 = (int)get("G2", 1);
            g.b_kn = (int)get("b_kn", 0); g.alpha = 1.0f;
            g.colscale = ptr("colscale", 4, 0); g.bias = ptr("bias", 5, 0);
            g.act = (int)get("act", 0); g.act_from = (int)get("act_from", 0);
            g.addmat = ptr("addmat", 6, 0); g.ldadd = (int)get("ldadd", g.N);
            g.colmask = ptr("colmask", 7, 0);
            g.rowmask = ptr("rowmask", 8, 0); g.rowmask_cols = (int)get("rowmask_cols", 0);
            g.mulmat = ptr("mulmat", 9, 0); g.ldmul = (int)get("ldmul", g.N); g.mul_pos = (int)get("mul_pos", 0);
            g.resid = ptr("resid", 10, 0); g.ldr = (int)get("ldr", g.N); g.rscale = ptr("rscale", 11, 0);
            g.tile_hint = (int)get("tile_hint", 0); g.a_ln = (int)get("a_ln", 0);
            g.ln_out = ptr("ln_out", 12, 0); g.ldlo = (int)get("ldlo", g.K);
            g.arith = arith;
            g.C2 = ptr("C2", 13, 0); g.ldc2 = (int)get("ldc2", g.N); g.n_split = (int)get("n_split", 0);
            g.ws = ptr("ws", 14, 0); g.ws_bytes = (size_t)get("ws_bytes", (long long)BIG);
            g.wsum = ptr("wsum", 15, 0);
            g.out_ln = ptr("out_ln", 16, 0); g.ldol = (int)get("ldol", g.N);
            g.a_amax = (const unsigned*)ptr("a_amax", 17, 0);
            printf("C gemm = %d\n", prd_gemm(&g, s));
        } else if (!strcmp(entry, "ln_rows")) {
            const int C = (int)get("C", 0);
            const int r = prd_ln_rows(ptr("x", 1, 1), ptr("y", 2, 1), ptr("gamma", 3, 0), ptr("gamma", 4, 0), (int)get("rows", 0), C,
                                      (int)get("ldx", C), (int)get("ldy", C), s);
            printf("C ln_rows = %d\n", r);
        } else if (!strcmp(entry, "softmax_rows")) {
            const int n = (int)get("n", 0);
            printf("C softmax_rows = %d\n", prd_softmax_rows(DP(1), (int)get("rows", 0), n, (int)get("ld", n), s));
        } else if (!strcmp(entry, "fc1_folded")) {
            const int r = prd_single_fc1_folded(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), (int)get("M", 0), (int)get("S", 0),
                                                (int)get("HC", 0), (int)get("Hd", 0), DP(11), BIG, arith, s);
            printf("C fc1_folded = %d\n", r);
        } else if (!strcmp(entry, "slab_ok")) {
            printf("Q slab_ok = %d\n", prd_gemm_slab_ok((int)get("M", 0), (int)get("N", 0), (int)get("K", 0), arith));
        } else if (!strcmp(entry, "fc1_folded_ok")) {
            printf("Q fc1_folded_ok = %d\n", prd_single_fc1_folded_ok((int)get("M", 0), (int)get("S", 0), (int)get("HC", 0), (int)get("Hd", 0), arith));
        } else {
            fprintf(stderr, "case %s: unknown entry %s\n", id, entry);
            return 2;
        }
    }
    return 0;
}
