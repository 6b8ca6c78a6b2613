/* Launch trace of libprd_hip (include/prd_hip.h), for a machine WITHOUT a GPU: linked against the trace build of the library
 * (csrc/prd_launch.h under -DPRD_LAUNCH_TRACE: a launch prints "L kernel grid block lds args" and returns 0), this driver walks the
 * entry points over a sweep of shapes, arithmetics, switches and head layouts with distinct dummy device pointers and prints
 *   C entry(arguments) = return value      after the L lines of that call
 *   Q query(arguments) = value             for the host-only queries
 * so every host decision above a launch -- which kernel, its grid, its LDS bytes, its arguments -- is text that two trees can be
 * compared by (tests/test_launch_trace_cpu.py holds this tree to the recorded trace).  Only entry points whose sole HIP use is the
 * launch helper are called: not prd_tri_attn_pair (device query, memset) and not the prd_debug_* reads.  No device is touched.
 * Build + run: python -m protein_redesign_amd.build --trace */
#include <stdio.h>
#include <string.h>

#include "../../include/prd_hip.h"

/* dummy device pointers: distinct, 16-byte aligned, never dereferenced */
#define DP(k) ((float*)(uintptr_t)(0x100000000ull + (unsigned long long)(k) * 0x10000000ull))
#define IP(k) ((int64_t*)DP(k))
#define BIG ((size_t)1 << 44)
#define LEN(a) ((int)(sizeof(a) / sizeof((a)[0])))
#define CALL(fmt, call, ...)                          \
    do {                                              \
        const int r_ = (call);                        \
        printf("C " fmt, __VA_ARGS__);                \
        printf(" = %d\n", r_);                        \
    } while (0)
#define QI(fmt, call, ...)                            \
    do {                                              \
        printf("Q " fmt, __VA_ARGS__);                \
        printf(" = %lld\n", (long long)(call));       \
    } while (0)

static const int NS[] = {1, 31, 32, 33, 63, 64, 65, 319, 320, 321, 352, 383, 384, 385, 400, 416, 417, 448, 449, 769, 960, 961, 1024, 1025, 1961, 4096};
static const int NS_FEW[] = {33, 320, 384, 385, 449, 769, 1025};        /* one row length per kernel of the attention dispatch */
static const int BS[] = {1, 2, 8};
static const int PS[] = {32, 64, 48};                                   /* 48: refused */
static const int SS[] = {128, 256, 384, 512, 2528, 36};                 /* 36: refused */
static const int DD[] = {8, 72, 128, 136, 256, 384, 512, 624, 632, 640};   /* dist_dim / C: at and off multiples of 128, at the LDS limits */
static const int HEADS[][2] = {{4, 16}, {8, 8}, {2, 32}, {1, 64}, {3, 20}, {16, 4}};
static int TUNES[32];
static int NTUNE = 0;
static hipStream_t s = 0;

static void tunes(void) {
    const int t[] = {0, 10, 1, 2, 3, PRD_TUNE_TA2_NO_V3, PRD_TUNE_TA2_NO_LONG, PRD_TUNE_TA2_FLAGS(0), PRD_TUNE_TA2_FLAGS(1), PRD_TUNE_TA2_FLAGS(2),
                     PRD_TUNE_TA2_FLAGS(4), PRD_TUNE_TA2_FLAGS(8), PRD_TUNE_TA2_FLAGS(31), PRD_TUNE_OL_GEN2, PRD_TUNE_TMS_NW12, PRD_TUNE_TMS_NW16,
                     PRD_TUNE_TMS_DEPTH3, PRD_TUNE_TA2_NO_XCD8, PRD_TUNE_TA2_NO_GV, PRD_TUNE_TMP_NW16, PRD_TUNE_TA2_NO_TAIL_SPLIT,
                     PRD_TUNE_GEMM_XCD_COLS, PRD_TUNE_GEMM_NO_BATCHED_RING, PRD_TUNE_GEMM_NO_SLAB, PRD_TUNE_GEMM_NO_KG};
    for (int k = 0; k < LEN(t); ++k) TUNES[NTUNE++] = t[k];
}

/* ---- the pair track and the triangle operators at one (b, N, P, arith word) ---- */
static void pair_track(int b, int N, int P, int a) {
    const float* w8[8] = {DP(20), DP(21), DP(22), DP(23), DP(24), DP(25), DP(26), DP(27)};
    const float* v8[8] = {DP(30), DP(31), DP(32), DP(33), DP(34), DP(35), DP(36), DP(37)};
    printf("# pair track b %d N %d P %d arith %d\n", b, N, P, a);
    CALL("pair_bias", prd_pair_bias(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), b, N, P, 4, s), 0);
    CALL("pair_bias2", prd_pair_bias2(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), 8, DP(7), 0, 0, DP(8), DP(9), 4, b, N, P, s), 0);
    CALL("tri_mul in %d res %d", prd_tri_mul(DP(1), DP(2), DP(3), w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7], N & 1, b & 1, b, N, P, DP(9), BIG,
                                             (int*)DP(10), a, s), N & 1, b & 1);
    CALL("tri_mul_contract", prd_tri_mul_contract(DP(1), DP(2), b, N, P, a, s), 0);
    CALL("tri_mul_contract_scaled", prd_tri_mul_contract_scaled(DP(1), DP(2), (const unsigned*)DP(3), b, N, P, a, s), 0);
    CALL("tri_mul_chain", prd_tri_mul_chain(DP(1), DP(2), w8, v8, b, N, P, DP(9), BIG, a, s), 0);
    CALL("tri_attn", prd_tri_attn(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), N & 1, 1, b, N, P, 4, 16, DP(11), BIG, (int*)DP(12), a, s), 0);
    CALL("tri_attn_core", prd_tri_attn_core(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 1, b, N, P, 4, 16, a, s), 0);
    CALL("tri_attn_out", prd_tri_attn_out(DP(1), DP(2), DP(3), DP(4), DP(5), 0, b, N, P, (int*)DP(6), a, s), 0);
    CALL("pair_transition", prd_pair_transition(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), 1, b, N, P, (int*)DP(7), a, s), 0);
    CALL("block_tail", prd_block_tail(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), b, N, P, 4, (int*)DP(12), a, s), 0);
    CALL("block_tail no bias", prd_block_tail(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, 0, 0, b, N, P, 0, 0, a, s), 0);
    CALL("coord_head", prd_coord_head(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), b, N, P, a, s), 0);
    CALL("tri_mul_proj_bwd", prd_tri_mul_proj_bwd(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), 0, 1, b, N, P, a, s), 0);
    for (int k = 0; k < LEN(SS); ++k)
        CALL("outer_linear S %d", prd_outer_linear(DP(1), DP(2), DP(3), DP(4), P + 64, DP(5), DP(6), k & 1, b, N, P, SS[k], (int*)DP(7), a, s), SS[k]);
}

/* entry points without an arithmetic argument (or whose kernels ignore it) */
static void no_arith(int b, int N, int P) {
    printf("# no arith b %d N %d P %d\n", b, N, P);
    CALL("static_pair", prd_static_pair(DP(1), DP(2), DP(3), DP(4), IP(5), IP(6), IP(7), IP(8), DP(9), DP(10), DP(11), DP(12), DP(13), 7, 32, b, N, P, s), 0);
    CALL("tri_attn_core_chunked", prd_tri_attn_core_chunked(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, b, N, P, 4, 16, DP(9), BIG, s), 0);
    CALL("tri_attn_core_fused", prd_tri_attn_core_fused(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), 0, b, N, P, 4, 16, s), 0);
    CALL("tri_attn_bwd_core", prd_tri_attn_bwd_core(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), 1, b, N, P, 4, 16, s), 0);
    CALL("tri_attn_bwd_core_v2", prd_tri_attn_bwd_core_v2(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), 0, b, N, P, 4, 16, s), 0);
    CALL("tri_attn_bwd_core_v2 no lse", prd_tri_attn_bwd_core_v2(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), 0, 0, 1, b, N, P, 4, 16, s), 0);
    CALL("tri_mul_out_bwd", prd_tri_mul_out_bwd(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), 0, 0, DP(12), DP(13), 0, b, N, P, s), 0);
    CALL("tri_mul_out_bwd_amax", prd_tri_mul_out_bwd_amax(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), DP(13), 0, 0, 4 * P, b,
                                                          N, P, (unsigned*)DP(14), s), 0);
    CALL("tri_mul_bwd_operands", prd_tri_mul_bwd_operands(DP(1), DP(2), b, N, P, s), 0);
    CALL("sym_rows", prd_sym_rows(DP(1), DP(2), 0.5f, b, N, P, s), 0);
    CALL("sym_transpose", prd_sym_transpose(DP(1), DP(2), b, N, P, s), 0);
    CALL("sym_transpose_amax", prd_sym_transpose_amax(DP(1), DP(2), b, N, P, (unsigned*)DP(3), s), 0);
    CALL("pair_bias_bwd", prd_pair_bias_bwd(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), b, (long long)N * N, b == 2 ? 8 : 4, P, s), 0);
    CALL("rbf_rows", prd_rbf_rows(DP(1), DP(2), DP(3), DP(4), b, N, 256, s), 0);
    CALL("single_attn_core", prd_single_attn_core(DP(1), DP(2), 256 + 64 * (b & 1), DP(3), b == 8 ? 0 : DP(4), b, N, 4, 16, s), 0);
    CALL("remove_mean", prd_remove_mean(DP(1), DP(2), DP(3), b, N, 3, s), 0);
    CALL("reverse_update", prd_reverse_update(DP(1), DP(2), IP(3), DP(4), DP(5), DP(6), DP(7), DP(8), b, N, 21, 1000, s), 0);
    CALL("step_boundary", prd_step_boundary(DP(1), DP(2), IP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), DP(13), DP(14), DP(15), (int*)DP(16), b,
                                            N, 21, 1000, 512, P, 256, 0, 0, 0, 0, s), 0);
    CALL("step_boundary seq_h", prd_step_boundary(DP(1), DP(2), IP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), DP(13), DP(14), DP(15),
                                                  (int*)DP(16), b, N, 21, 1000, 128, P, 64, DP(17), 512, DP(18), 512, s), 0);
    CALL("atom_embed", prd_atom_embed(DP(1), IP(2), DP(3), DP(4), (const int*)DP(5), 9, b, N, 512, s), 0);
    CALL("single_init", prd_single_init(DP(1), DP(2), DP(3), DP(4), DP(5), b * N, 512, 21, s), 0);
    CALL("time_embed", prd_time_embed(DP(1), IP(2), DP(3), DP(4), 1000, b, P, 256, s), 0);
    for (int m = 0; m < 5; ++m)
        CALL("mask_lowest_k mode %d", prd_mask_lowest_k(DP(1), DP(2), m & 1 ? IP(3) : 0, DP(4), DP(5), DP(6), DP(7), DP(8), 111, DP(9), m, b * 40, N * 5, s), m);
}

/* the attention cores over the head layouts */
static void heads(int b, int N, int P, int a) {
    for (int k = 0; k < LEN(HEADS); ++k) {
        const int H = HEADS[k][0], c = HEADS[k][1];
        printf("# heads b %d N %d P %d arith %d H %d c %d\n", b, N, P, a, H, c);
        QI("tri_attn_heads_supported", prd_tri_attn_heads_supported(N, P, H, c, a), 0);
        QI("tri_attn_heads_workspace_bytes", prd_tri_attn_heads_workspace_bytes(b, N, P, H, c), 0);
        QI("tri_attn_bwd_heads_supported", prd_tri_attn_bwd_heads_supported(N, P, H, c, a), 0);
        QI("tri_attn_bwd_heads_workspace_bytes", prd_tri_attn_bwd_heads_workspace_bytes(b, N, P, H, c), 0);
        CALL("tri_attn_core_heads", prd_tri_attn_core_heads(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, b, N, P, H, c, DP(9), BIG, a, s), 0);
        CALL("tri_attn_core_heads_lse", prd_tri_attn_core_heads_lse(DP(1), DP(10), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 1, b, N, P, H, c, DP(9), BIG, a, s), 0);
        CALL("tri_attn_bwd_core_heads", prd_tri_attn_bwd_core_heads(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), k & 1 ? DP(11) : 0,
                                                                     k & 2 ? DP(12) : 0, 1, b, N, P, H, c, DP(13), BIG, a, s), 0);
        CALL("tri_attn_core", prd_tri_attn_core(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, b, N, P, H, c, a, s), 0);
        CALL("tri_attn_core_v2", prd_tri_attn_core_v2(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, b, N, P, H, c, 0, s), 0);
        CALL("tri_attn_core_chunked", prd_tri_attn_core_chunked(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, b, N, P, H, c, DP(9), BIG, s), 0);
        CALL("tri_attn_core_fused", prd_tri_attn_core_fused(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), DP(11), DP(12), 0, b, N, P, H, c, s), 0);
        CALL("tri_attn_bwd_core", prd_tri_attn_bwd_core(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), 1, b, N, P, H, c, s), 0);
        CALL("tri_attn_bwd_core_v2", prd_tri_attn_bwd_core_v2(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), 0, 0, 0, b, N, P, H, c, s), 0);
        CALL("single_attn_core", prd_single_attn_core(DP(1), DP(2), 4 * H * c, DP(3), DP(4), b, N, H, c, s), 0);
    }
}

/* what depends on the switch word: the dispatch queries and the launches that read a switch */
static void switches(int b, int N, int P, int tune) {
    const int a = PRD_ARITH_SPLIT16 | PRD_TUNE(tune);
    const float* w8[8] = {DP(20), DP(21), DP(22), DP(23), DP(24), DP(25), DP(26), DP(27)};
    printf("# switches b %d N %d P %d tune %d\n", b, N, P, tune);
    QI("tri_attn_variant split", prd_tri_attn_variant(N, P, a), 0);
    QI("tri_attn_variant fp32", prd_tri_attn_variant(N, P, PRD_ARITH_FP32 | PRD_TUNE(tune)), 0);
    QI("tri_attn_v2_supported", prd_tri_attn_v2_supported(N, P, tune), 0);
    QI("tri_attn_v2_form", prd_tri_attn_v2_form(N, P, tune), 0);
    QI("tri_attn_pair_supported", prd_tri_attn_pair_supported(N, P, a), 0);
    QI("tri_attn_stats_bytes", prd_tri_attn_stats_bytes(b, N, P, 4, a), 0);
    QI("tri_attn_core_fused_supported", prd_tri_attn_core_fused_supported(N, P, a), 0);
    QI("tri_mul_chain_supported", prd_tri_mul_chain_supported(N, P, a), 0);
    CALL("tri_attn_core", prd_tri_attn_core(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 1, b, N, P, 4, 16, a, s), 0);
    CALL("tri_attn_core_v2", prd_tri_attn_core_v2(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 0, b, N, P, 4, 16, tune, s), 0);
    CALL("tri_attn_core_v2_lse", prd_tri_attn_core_v2_lse(DP(1), DP(9), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), 1, b, N, P, 4, 16, tune, s), 0);
    CALL("tri_attn", prd_tri_attn(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), 0, 0, b, N, P, 4, 16, DP(11), BIG, 0, a, s), 0);
    if (tune) {         /* (tune 0: pair_track has them) */
        CALL("tri_mul", prd_tri_mul(DP(1), DP(2), DP(3), w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7], 1, 1, b, N, P, DP(9), BIG, 0, a, s), 0);
        CALL("tri_mul_contract", prd_tri_mul_contract(DP(1), DP(2), b, N, 2 * P, a, s), 0);
        CALL("tri_mul_contract_scaled", prd_tri_mul_contract_scaled(DP(1), DP(2), (const unsigned*)DP(3), b, N, 2 * P, a, s), 0);
        CALL("tri_mul_chain", prd_tri_mul_chain(DP(1), DP(2), w8, w8, b, N, P, DP(9), BIG, a, s), 0);
        CALL("outer_linear", prd_outer_linear(DP(1), DP(2), DP(3), DP(4), P, DP(5), DP(6), 1, b, N, P, 512, (int*)DP(7), a, s), 0);
    }
}

/* the head of the pair track over dist_dim and C */
static void pair_head(int b, int N, int P, int a) {
    for (int i = 0; i < LEN(DD); ++i) {
        printf("# pair head b %d N %d P %d arith %d dd %d\n", b, N, P, a, DD[i]);
        CALL("pair_init", prd_pair_init(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), b, N, P, DD[i], a, s), 0);
        CALL("opm_pair", prd_opm_pair(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), 3, b, N, P, DD[i], a, s), 0);
        for (int j = 0; j < LEN(DD); ++j) {
            QI("pair_head_supported C %d", prd_pair_head_supported(P, DD[i], DD[j], a), DD[j]);
            if ((DD[i] % 128) == 0 && (DD[j] % 128) == 0)
                CALL("pair_head C %d", prd_pair_head(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DD[i], DP(8), DP(9), DP(10), DD[j], j & 1, DP(11), DP(12), DP(13),
                                                     DP(14), DP(15), 8, DP(16), 0, 0, DP(17), DP(18), 4, b, N, P, a, s), DD[j]);
        }
    }
}

/* ---- the single track: prd_gemm over the shapes of its dispatch ---- */
static void gemm_one(const char* what, PrdGemm* g) {
    CALL("gemm %s M %d N %d K %d G %d %d b_kn %d a_ln %d hint %d arith %d", prd_gemm(g, s), what, g->M, g->N, g->K, g->G1, g->G2, g->b_kn, g->a_ln, g->tile_hint, g->arith);
}

static void gemms(void) {
    static const int MS[] = {40, 96, 320, 640, 769, 2560}, NN[] = {21, 64, 256, 512, 2048}, KS[] = {36, 64, 128, 256, 512, 1024, 2048, 4096};
    PrdGemm g;
    for (int t = 0; t < NTUNE; ++t) {
        if (t && TUNES[t] < PRD_TUNE_GEMM_NO_KG) continue;           /* the switches of the GEMM dispatch */
        for (int ar = t ? 1 : 0; ar < 2; ++ar)                         /* (they act in the split-16 arithmetic only) */
            for (int i = 0; i < LEN(MS); ++i)
                for (int j = 0; j < LEN(NN); ++j)
                    for (int k = 0; k < LEN(KS); ++k) {
                        const int M = MS[i], N = NN[j], K = KS[k], a = ar | PRD_TUNE(TUNES[t]);
                        memset(&g, 0, sizeof g);
                        g.A = DP(1); g.B = DP(2); g.C = DP(3); g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.G1 = g.G2 = 1; g.arith = a;
                        g.alpha = 1.f; g.bias = DP(4);
                        gemm_one("plain", &g);
                        g.a_ln = 1;
                        gemm_one("ln", &g);
                        g.ln_out = DP(5); g.ldlo = K;
                        if (!t) gemm_one("ln ln_out", &g);
                        g.ln_out = 0; g.a_ln = 0;
                        if ((N % 4) == 0) {
                            g.ws = DP(6); g.ws_bytes = BIG;
                            gemm_one("ws", &g);
                            g.a_ln = 1; g.wsum = DP(7); g.out_ln = DP(8); g.ldol = N;
                            if (!t) gemm_one("ws ln out_ln", &g);
                            g.a_ln = 0; g.wsum = 0; g.out_ln = 0; g.ws = 0; g.ws_bytes = 0;
                        }
                        if (t == 0 && j == 2)
                            for (int h = 32; h <= 128; h *= 2) { g.tile_hint = h; gemm_one("hint", &g); }
                        g.tile_hint = 0;
                        /* batched: the per-head logits (A B^T) and P V (b_kn) of the single-track attention */
                        g.G1 = 2; g.G2 = 4; g.sa1 = 4L * M * K; g.sa2 = (long long)M * K; g.sb1 = 4L * N * K; g.sb2 = (long long)N * K; g.sc1 = 4L * M * N; g.sc2 = (long long)M * N;
                        gemm_one("batched", &g);
                        g.b_kn = 1; g.ldb = N;
                        gemm_one("batched b_kn", &g);
                        g.a_ln = 2; g.a_scale = 16.f;
                        if (!t) gemm_one("batched b_kn softmax", &g);
                        if (t == 0) {
                            QI("gemm_slab_ok M %d N %d K %d arith %d", prd_gemm_slab_ok(M, N, K, a), M, N, K, a);
                            QI("gemm_slab_workspace M %d N %d K %d", prd_gemm_slab_workspace(M, N, K), M, N, K);
                        }
                    }
    }
    for (int ar = 0; ar < 2; ++ar)
        for (int i = 0; i < LEN(MS); ++i) {
            static const int SH[][3] = {{512, 64, 2048}, {512, 64, 4096}, {512, 64, 8192}, {512, 128, 2048}, {256, 64, 1024}, {1024, 64, 2048}, {384, 64, 1536}};
            for (int k = 0; k < LEN(SH); ++k) {
                QI("single_fc1_folded_ok M %d S %d HC %d Hd %d arith %d", prd_single_fc1_folded_ok(MS[i], SH[k][0], SH[k][1], SH[k][2], ar), MS[i], SH[k][0], SH[k][1],
                   SH[k][2], ar);
                CALL("single_fc1_folded M %d S %d HC %d Hd %d arith %d", prd_single_fc1_folded(DP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), DP(10), MS[i],
                                                                                            SH[k][0], SH[k][1], SH[k][2], DP(11), BIG, ar, s),
                     MS[i], SH[k][0], SH[k][1], SH[k][2], ar);
            }
        }
    for (int i = 0; i < LEN(MS); ++i) {
        const int rows = MS[i] * MS[i];
        CALL("ln_rows rows %d C 64", prd_ln_rows(DP(1), DP(2), DP(3), DP(4), rows, 64, 64, 64, s), rows);
        CALL("ln_rows rows %d C 64 unaligned", prd_ln_rows(DP(1) + 1, DP(2), 0, 0, rows, 64, 64, 64, s), rows);
        CALL("ln_rows rows %d C 512", prd_ln_rows(DP(1), DP(2), 0, 0, MS[i], 512, 512, 512, s), MS[i]);
        CALL("softmax_rows rows %d", prd_softmax_rows(DP(1), rows, MS[i], MS[i] + 3, s), rows);
        CALL("ln_rows_bwd rows %d C 64", prd_ln_rows_bwd(DP(1), DP(2), DP(3), DP(4), rows, 64, s), rows);
        CALL("ln_rows_bwd rows %d C 64 unaligned", prd_ln_rows_bwd(DP(1), DP(2) + 1, DP(3), 0, rows, 64, s), rows);
        CALL("ln_rows_bwd rows %d C 512", prd_ln_rows_bwd(DP(1), DP(2), DP(3), 0, MS[i], 512, s), MS[i]);
    }
}

/* the single-track attention with wide heads, and the row / weight-gradient kernels of the training backward */
static void rows_and_wgrads(void) {
    static const int CS[] = {64, 128, 256, 512, 576, 32, 96};
    static const long long RW[] = {1, 100, 511, 512, 513, 102400, 131072, 1048576, 16777216};
    static const int KO[][2] = {{64, 64}, {64, 256}, {256, 64}, {256, 256}, {64, 128}};
    static const int OI[][2] = {{1, 64}, {4, 64}, {8, 128}, {16, 256}, {64, 64}, {128, 64}, {192, 64}, {256, 256}, {64, 192}, {96, 64}, {320, 64}};
    for (int ar = 0; ar < 2; ++ar)
        for (int i = 0; i < LEN(NS); ++i)
            for (int j = 0; j < LEN(BS); ++j)
                for (int k = 0; k < LEN(CS); ++k) {
                    const int b = BS[j], N = NS[i], H = 4, c = CS[k];
                    if (j && k > 1) continue;
                    QI("spa_attn_core_supported N %d c %d arith %d", prd_spa_attn_core_supported(N, c, ar), N, c, ar);
                    QI("spa_attn_core_workspace b %d N %d H %d c %d", prd_spa_attn_core_workspace(b, N, H, c), b, N, H, c);
                    CALL("spa_attn_core b %d N %d c %d arith %d", prd_spa_attn_core(DP(1), DP(2), 4 * H * c, DP(3), j ? DP(4) : 0, b, N, H, c, DP(5), BIG, ar, s), b, N, c, ar);
                }
    for (int r = 0; r < LEN(RW); ++r) {
        const long long rows = RW[r];
        for (int ar = 0; ar < 2; ++ar) {
            for (int k = 0; k < LEN(KO); ++k) {
                if (!r) QI("pair_linear_supported K %d OUT %d arith %d", prd_pair_linear_supported(KO[k][0], KO[k][1], ar), KO[k][0], KO[k][1], ar);
                CALL("pair_linear rows %lld K %d OUT %d arith %d", prd_pair_linear(DP(1), DP(2), DP(3), DP(4), rows, KO[k][0], KO[k][1], KO[k][0] == 64, KO[k][0] == 64 ? DP(5) : 0,
                                                                                   k & 1, DP(6), k & 1, ar, s), rows, KO[k][0], KO[k][1], ar);
            }
            for (int k = 0; k < LEN(OI); ++k) {
                const int O = OI[k][0], I = OI[k][1];
                if (!ar) QI("linear_wgrad_workspace rows %lld O %d I %d", prd_linear_wgrad_workspace(rows, O, I), rows, O, I);
                CALL("linear_wgrad rows %lld O %d I %d arith %d", prd_linear_wgrad(DP(1), k & 1 ? DP(2) : 0, DP(3), DP(4), rows, O, I, O + 2, I, DP(5), BIG, ar, s), rows, O, I, ar);
            }
        }
        {
            const long long* ids[3] = {(const long long*)DP(20), (const long long*)DP(21), (const long long*)DP(22)};
            const float* sc[3] = {DP(23), 0, DP(24)};
            const int cards[3] = {8, 34, 65}, big[3] = {64, 64, 8};
            QI("embed_wgrad_workspace rows %lld", prd_embed_wgrad_workspace(rows, 65, 64), rows);
            CALL("embed_wgrad rows %lld", prd_embed_wgrad(DP(1), (const long long*)DP(2), DP(3), DP(4), rows, 65, 64, 64, DP(5), BIG, s), rows);
            CALL("embed_wgrad rows %lld card 128 C 32", prd_embed_wgrad(DP(1), (const long long*)DP(2), DP(3), 0, rows, 128, 32, 64, DP(5), BIG, s), rows);
            CALL("embed_wgrad rows %lld card 129", prd_embed_wgrad(DP(1), (const long long*)DP(2), DP(3), 0, rows, 129, 32, 64, DP(5), BIG, s), rows);
            CALL("embed_wgrad_multi rows %lld", prd_embed_wgrad_multi(DP(1), ids, sc, cards, 3, DP(2), rows, 64, 64, DP(3), BIG, s), rows);
            CALL("embed_wgrad_multi rows %lld no scale", prd_embed_wgrad_multi(DP(1), ids, 0, cards, 2, DP(2), rows, 48, 64, DP(3), BIG, s), rows);
            CALL("embed_wgrad_multi rows %lld 136 entries", prd_embed_wgrad_multi(DP(1), ids, 0, big, 3, DP(2), rows, 64, 64, DP(3), BIG, s), rows);
            CALL("outer_linear_bwd_reduce R %lld", prd_outer_linear_bwd_reduce(DP(1), DP(2), 4, DP(3), DP(4), DP(5), rows > 4096 ? 4096 : rows, 64, 512, s), rows);
        }
    }
}

int main(void) {
    static const char* const OPS[] = {"tri_mul", "tri_attn", "nonsense", "pair", "x"};
    tunes();
    QI("version", prd_version(), 0);
    for (int i = 0; i < LEN(NS); ++i)
        for (int j = 0; j < LEN(BS); ++j)
            for (int k = 0; k < LEN(PS); ++k) {
                for (int a = 0; a < 2; ++a) pair_track(BS[j], NS[i], PS[k], a);
                no_arith(BS[j], NS[i], PS[k]);
                QI("tri_attn_bwd_core_v2_supported N %d P %d", prd_tri_attn_bwd_core_v2_supported(NS[i], PS[k]), NS[i], PS[k]);
                for (int o = 0; o < LEN(OPS); ++o)
                    QI("workspace_bytes %s b %d N %d P %d", prd_workspace_bytes(OPS[o], BS[j], NS[i], 512, PS[k]), OPS[o], BS[j], NS[i], PS[k]);
                for (int a = 0; a < 2; ++a) QI("tri_attn_stats_bytes H 8 arith %d", prd_tri_attn_stats_bytes(BS[j], NS[i], PS[k], 8, a), a);
            }
    for (int i = 0; i < LEN(NS); ++i)
        for (int k = 0; k < 2; ++k)
            for (int t = 0; t < NTUNE; ++t) switches(k + 1, NS[i], PS[k], TUNES[t]);
    for (int i = 0; i < LEN(NS_FEW); ++i)
        for (int j = 0; j < LEN(BS); ++j)
            for (int k = 0; k < LEN(PS); ++k)
                for (int a = 0; a < 2; ++a) {
                    heads(BS[j], NS_FEW[i], PS[k], a);
                    if (i < 3) pair_head(BS[j], NS_FEW[i], PS[k], a);
                }
    gemms();
    rows_and_wgrads();
    /* bad arithmetic words and null arguments are refused the same way */
    QI("tri_attn_variant arith 2", prd_tri_attn_variant(320, 64, 2), 0);
    QI("tri_attn_variant arith -1", prd_tri_attn_variant(320, 64, -1), 0);
    QI("tri_attn_variant N 0", prd_tri_attn_variant(0, 64, 1), 0);
    QI("workspace_bytes null", prd_workspace_bytes(0, 1, 320, 512, 64), 0);
    QI("workspace_bytes b 0", prd_workspace_bytes("tri_mul", 0, 320, 512, 64), 0);
    return 0;
}
