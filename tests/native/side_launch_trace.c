/* Launch trace of the five side libraries (include/prd_align.h, prd_tmalign.h, prd_quality.h, prd_condition.h, prd_sequence.h), for a
 * machine WITHOUT a GPU: the companion of launch_trace.c.  Linked against their trace builds (csrc/prd_launch.h under
 * -DPRD_LAUNCH_TRACE: a launch prints "L kernel grid block lds args", the memset ahead of a launch "M address value bytes", and both
 * return 0), this driver walks every entry point of the five headers with distinct dummy device pointers and prints
 *   C entry(arguments) = return value      after the L / M lines of that call
 *   Q query(arguments) = value             for the workspace-size queries
 * The sweep holds the shapes at which a host decision changes, and only those: the edges of every grid, the 4 -> 8 waves of the
 * align search, each 48 KiB threshold of dynamic LDS, every limit and one above it, every optional pointer given and absent, and the
 * argument checks in the order the entry points make them.  tests/test_launch_trace_cpu.py holds this tree to the recorded output.
 * No device is touched.  Build + run: python -m protein_redesign_amd.build --trace-side */
#include <math.h>
#include <stdio.h>

#include "../../include/prd_align.h"
#include "../../include/prd_condition.h"
#include "../../include/prd_quality.h"
#include "../../include/prd_sequence.h"
#include "../../include/prd_tmalign.h"

/* dummy device pointers: distinct, 16-byte aligned, never dereferenced */
#define VP(k) ((void*)(uintptr_t)(0x100000000ull + (unsigned long long)(k) * 0x10000000ull))
#define DP(k) ((float*)VP(k))
#define IP(k) ((int*)VP(k))
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

static hipStream_t s = 0;

/* ---- align: N at the wave count's step, at the LDS threshold and at the limit ---- */
static int superimpose(const float* y, int S, int R, int N, int pairs, int mode, int mirror, void* ws, size_t ws_bytes) {
    return prd_align_superimpose(DP(1), DP(2), DP(3), DP(4), IP(5), DP(6), 3LL * N, 3, y, 37LL * N, 37, DP(8), S, R, N, pairs, mode, mirror, ws, ws_bytes, s);
}

static void align(void) {
    static const int NS[] = {1, 3, 1024, 1025, 2048, 2049, PRD_ALIGN_MAX_N, PRD_ALIGN_MAX_N + 1};
    static const int SR[][3] = {{1, 1, PRD_ALIGN_PAIRS_CROSS}, {8, 1, PRD_ALIGN_PAIRS_CROSS}, {1, 1, PRD_ALIGN_PAIRS_SELF}, {8, 8, PRD_ALIGN_PAIRS_SELF}};
    QI("align_version", prd_align_version(), 0);
    for (int i = 0; i < LEN(NS); ++i)
        for (int k = 0; k < LEN(SR); ++k)
            for (int mode = 0; mode < 2; ++mode)
                for (int mirror = 0; mirror < 2; ++mirror) {
                    const int N = NS[i], S = SR[k][0], R = SR[k][1], pairs = SR[k][2];
                    printf("# align N %d S %d R %d pairs %d mode %d mirror %d\n", N, S, R, pairs, mode, mirror);
                    QI("align_workspace_bytes", prd_align_workspace_bytes(S, R, N, pairs, mode, mirror), 0);
                    CALL("align_superimpose", superimpose(pairs ? 0 : DP(7), S, R, N, pairs, mode, mirror, VP(9), BIG), 0);
                }
    {
        const size_t need = prd_align_workspace_bytes(8, 1, 1025, 0, 0, 1);
        printf("# align workspace\n");
        CALL("align_superimpose ws exact", superimpose(DP(7), 8, 1, 1025, 0, 0, 1, VP(9), need), 0);
        CALL("align_superimpose ws one byte short", superimpose(DP(7), 8, 1, 1025, 0, 0, 1, VP(9), need - 1), 0);
        CALL("align_superimpose ws misaligned", superimpose(DP(7), 8, 1, 1025, 0, 0, 1, (char*)VP(9) + 8, BIG), 0);
        CALL("align_superimpose self, y == x", prd_align_superimpose(DP(1), DP(2), DP(3), DP(4), IP(5), DP(6), 9, 3, DP(6), 0, 0, DP(8), 8, 8, 3, 1, 0, 0, VP(9), BIG, s), 0);
    }
    printf("# align refusals\n");
    CALL("align_superimpose tm null", prd_align_superimpose(0, DP(2), DP(3), DP(4), IP(5), DP(6), 9, 3, DP(7), 9, 3, DP(8), 1, 1, 3, 0, 0, 0, VP(9), BIG, s), 0);
    CALL("align_superimpose ws null", superimpose(DP(7), 1, 1, 3, 0, 0, 0, 0, BIG), 0);
    CALL("align_superimpose S 0", superimpose(DP(7), 0, 1, 3, 0, 0, 0, VP(9), BIG), 0);
    CALL("align_superimpose N 0 and pairs 2", superimpose(DP(7), 1, 1, 0, 2, 0, 0, VP(9), BIG), 0);
    CALL("align_superimpose pairs 2", superimpose(DP(7), 1, 1, 3, 2, 0, 0, VP(9), BIG), 0);
    CALL("align_superimpose mode 2", superimpose(DP(7), 1, 1, 3, 0, 2, 0, VP(9), BIG), 0);
    CALL("align_superimpose x row stride 2", prd_align_superimpose(DP(1), DP(2), DP(3), DP(4), IP(5), DP(6), 9, 2, DP(7), 9, 3, DP(8), 1, 1, 3, 0, 0, 0, VP(9), BIG, s), 0);
    CALL("align_superimpose x struct stride -1", prd_align_superimpose(DP(1), DP(2), DP(3), DP(4), IP(5), DP(6), -1, 3, DP(7), 9, 3, DP(8), 1, 1, 3, 0, 0, 0, VP(9), BIG, s), 0);
    CALL("align_superimpose self R != S", superimpose(0, 8, 1, 3, 1, 0, 0, VP(9), BIG), 0);
    CALL("align_superimpose self y other", superimpose(DP(7), 8, 8, 3, 1, 0, 0, VP(9), BIG), 0);
    CALL("align_superimpose cross y null", superimpose(0, 8, 1, 3, 0, 0, 0, VP(9), BIG), 0);
    CALL("align_superimpose cross y row stride 2", prd_align_superimpose(DP(1), DP(2), DP(3), DP(4), IP(5), DP(6), 9, 3, DP(7), 9, 2, DP(8), 1, 1, 3, 0, 0, 0, VP(9), BIG, s), 0);
    CALL("align_superimpose N above the limit, ws short", superimpose(DP(7), 1, 1, PRD_ALIGN_MAX_N + 1, 0, 0, 0, VP(9), 0), 0);
    QI("align_workspace_bytes 2^31 pairs", prd_align_workspace_bytes(65536, 32768, 3, 0, 0, 0), 0);
    CALL("align_superimpose 2^31 pairs", superimpose(DP(7), 65536, 32768, 3, 0, 0, 0, VP(9), BIG), 0);
    QI("align_workspace_bytes 2^30 pairs mirrored", prd_align_workspace_bytes(32768, 32768, 3, 0, 0, 1), 0);
    QI("align_workspace_bytes pairs 2", prd_align_workspace_bytes(1, 1, 3, 2, 0, 0), 0);
    QI("align_workspace_bytes mode 2", prd_align_workspace_bytes(1, 1, 3, 0, 2, 0), 0);
    QI("align_workspace_bytes self R != S", prd_align_workspace_bytes(8, 1, 3, 1, 0, 0), 0);
    {
        static const int AN[] = {1, 256, 257}, AS[] = {1, 65535, 65536};
        for (int i = 0; i < LEN(AN); ++i)
            for (int k = 0; k < LEN(AS); ++k) CALL("align_apply S %d N %d", prd_align_apply(DP(1), DP(2), DP(3), DP(4), AS[k], AN[i], s), AS[k], AN[i]);
        CALL("align_apply out null", prd_align_apply(0, DP(2), DP(3), DP(4), 1, 1, s), 0);
        CALL("align_apply trans null", prd_align_apply(DP(1), DP(2), DP(3), 0, 1, 1, s), 0);
        CALL("align_apply N 0", prd_align_apply(DP(1), DP(2), DP(3), DP(4), 65536, 0, s), 0);
    }
}

/* ---- tmalign: lengths on either side of the 48 KiB of each kernel (refine 711 | 712, search 1536 | 1537), the limits ---- */
static int tm_align(const float* y, int S, int R, int Nx, int Ny, int mirror, void* ws, size_t ws_bytes) {
    return prd_tmalign_align(DP(1), DP(2), DP(3), DP(4), IP(5), IP(6), IP(7), DP(8), 3LL * Nx, 3, DP(9), y, 37LL * Ny, 37, DP(11), S, R, Nx, Ny, mirror, ws, ws_bytes, s);
}

static void tmalign(void) {
    static const int NN[][2] = {{1, 1}, {2, 1}, {1, 2}, {711, 711}, {712, 712}, {712, 711}, {711, 712}, {1536, 1536}, {1537, 1537}, {1537, 1536}, {1536, 1537},
                                {PRD_TMALIGN_MAX_N, 1}, {1, PRD_TMALIGN_MAX_N}, {PRD_TMALIGN_MAX_N, PRD_TMALIGN_MAX_N}, {PRD_TMALIGN_MAX_N + 1, 1}, {1, PRD_TMALIGN_MAX_N + 1}};
    /* S * R * (mirror ? 2 : 1) * 3 at the largest value within PRD_TMALIGN_MAX_PROBLEMS and one pair above it */
    static const int SRM[][3] = {{349525, 1, 0}, {349526, 1, 0}, {1, 349525, 0}, {5 * 11, 5 * 31 * 41, 0}, {174762, 1, 1}, {174763, 1, 1}, {2, 87381, 1}, {1048576, 1, 0}};
    QI("tmalign_version", prd_tmalign_version(), 0);
    for (int i = 0; i < LEN(NN); ++i)
        for (int k = 0; k < 2; ++k)
            for (int mirror = 0; mirror < 2; ++mirror) {
                const int Nx = NN[i][0], Ny = NN[i][1], S = k ? 3 : 1, R = k ? 2 : 1;
                printf("# tmalign Nx %d Ny %d S %d R %d mirror %d\n", Nx, Ny, S, R, mirror);
                QI("tmalign_workspace_bytes", prd_tmalign_workspace_bytes(S, R, Nx, Ny, mirror), 0);
                CALL("tmalign_align", tm_align(DP(10), S, R, Nx, Ny, mirror, VP(12), BIG), 0);
            }
    for (int k = 0; k < LEN(SRM); ++k) {
        printf("# tmalign problems S %d R %d mirror %d\n", SRM[k][0], SRM[k][1], SRM[k][2]);
        QI("tmalign_workspace_bytes", prd_tmalign_workspace_bytes(SRM[k][0], SRM[k][1], 7, 5, SRM[k][2]), 0);
        CALL("tmalign_align", tm_align(DP(10), SRM[k][0], SRM[k][1], 7, 5, SRM[k][2], VP(12), BIG), 0);
    }
    {
        const size_t need = prd_tmalign_workspace_bytes(3, 2, 33, 17, 1);
        printf("# tmalign workspace\n");
        CALL("tmalign_align ws exact", tm_align(DP(10), 3, 2, 33, 17, 1, VP(12), need), 0);
        CALL("tmalign_align ws one byte short", tm_align(DP(10), 3, 2, 33, 17, 1, VP(12), need - 1), 0);
        CALL("tmalign_align ws misaligned", tm_align(DP(10), 3, 2, 33, 17, 1, (char*)VP(12) + 4, BIG), 0);
    }
    printf("# tmalign refusals\n");
    CALL("tmalign_align y null", tm_align(0, 1, 1, 7, 5, 0, VP(12), BIG), 0);
    CALL("tmalign_align ws null", tm_align(DP(10), 1, 1, 7, 5, 0, 0, BIG), 0);
    CALL("tmalign_align S 0", tm_align(DP(10), 0, 1, 7, 5, 0, VP(12), BIG), 0);
    CALL("tmalign_align Ny 0", tm_align(DP(10), 1, 1, 7, 0, 0, VP(12), BIG), 0);
    CALL("tmalign_align x row stride 2", prd_tmalign_align(DP(1), DP(2), DP(3), DP(4), IP(5), IP(6), IP(7), DP(8), 21, 2, DP(9), DP(10), 15, 3, DP(11), 1, 1, 7, 5, 0, VP(12), BIG, s), 0);
    CALL("tmalign_align y struct stride -1", prd_tmalign_align(DP(1), DP(2), DP(3), DP(4), IP(5), IP(6), IP(7), DP(8), 21, 3, DP(9), DP(10), -1, 3, DP(11), 1, 1, 7, 5, 0, VP(12), BIG, s), 0);
    CALL("tmalign_align Nx above the limit, ws short", tm_align(DP(10), 1, 1, PRD_TMALIGN_MAX_N + 1, 5, 0, VP(12), 0), 0);
    CALL("tmalign_align too many problems, ws short", tm_align(DP(10), 349526, 1, 7, 5, 0, VP(12), 0), 0);
}

/* ---- quality: the row tiles of 64, the limits of N and S, exclude given and absent ---- */
static void quality(void) {
    static const int NS[] = {1, 64, 65, PRD_QUALITY_MAX_N, PRD_QUALITY_MAX_N + 1}, SS[] = {1, PRD_QUALITY_MAX_S, PRD_QUALITY_MAX_S + 1};
    QI("quality_version", prd_quality_version(), 0);
    for (int i = 0; i < LEN(NS); ++i)
        for (int k = 0; k < LEN(SS); ++k) {
            const int N = NS[i], S = SS[k];
            printf("# quality N %d S %d\n", N, S);
            CALL("quality_lddt", prd_quality_lddt(IP(1), IP(2), DP(3), 3LL * N, 3, DP(4), 37, DP(5), DP(6), 15.0f, S, N, s), 0);
            CALL("quality_contacts exclude", prd_quality_contacts(IP(1), DP(2), DP(3), 3LL * N, 3, DP(4), DP(5), (const uint8_t*)VP(6), 4.0f, S, N, s), 0);
            CALL("quality_contacts no exclude", prd_quality_contacts(IP(1), DP(2), DP(3), 3LL * N, 3, DP(4), DP(5), 0, 4.0f, S, N, s), 0);
        }
    printf("# quality refusals\n");
    CALL("quality_lddt total null", prd_quality_lddt(IP(1), 0, DP(3), 9, 3, DP(4), 3, DP(5), DP(6), 15.0f, 1, 3, s), 0);
    CALL("quality_lddt y row stride 2", prd_quality_lddt(IP(1), IP(2), DP(3), 9, 3, DP(4), 2, DP(5), DP(6), 15.0f, 1, 3, s), 0);
    CALL("quality_lddt x null", prd_quality_lddt(IP(1), IP(2), 0, 9, 3, DP(4), 3, DP(5), DP(6), 15.0f, 1, 3, s), 0);
    CALL("quality_lddt x row stride 2", prd_quality_lddt(IP(1), IP(2), DP(3), 9, 2, DP(4), 3, DP(5), DP(6), 15.0f, 1, 3, s), 0);
    CALL("quality_lddt x struct stride -1", prd_quality_lddt(IP(1), IP(2), DP(3), -1, 3, DP(4), 3, DP(5), DP(6), 15.0f, 1, 3, s), 0);
    CALL("quality_lddt radius 0", prd_quality_lddt(IP(1), IP(2), DP(3), 9, 3, DP(4), 3, DP(5), DP(6), 0.0f, 1, 3, s), 0);
    CALL("quality_lddt radius nan, N above the limit", prd_quality_lddt(IP(1), IP(2), DP(3), 9, 3, DP(4), 3, DP(5), DP(6), NAN, 1, PRD_QUALITY_MAX_N + 1, s), 0);
    CALL("quality_lddt S 0", prd_quality_lddt(IP(1), IP(2), DP(3), 9, 3, DP(4), 3, DP(5), DP(6), 15.0f, 0, 3, s), 0);
    CALL("quality_contacts count null", prd_quality_contacts(0, DP(2), DP(3), 9, 3, DP(4), DP(5), 0, 4.0f, 1, 3, s), 0);
    CALL("quality_contacts b_mask null", prd_quality_contacts(IP(1), DP(2), DP(3), 9, 3, DP(4), 0, 0, 4.0f, 1, 3, s), 0);
    CALL("quality_contacts cutoff inf", prd_quality_contacts(IP(1), DP(2), DP(3), 9, 3, DP(4), DP(5), 0, INFINITY, 1, 3, s), 0);
    CALL("quality_contacts cutoff -1", prd_quality_contacts(IP(1), DP(2), DP(3), 9, 3, DP(4), DP(5), 0, -1.0f, 1, 3, s), 0);
}

/* ---- condition: elements per sample on either side of a multiple of 256 (3 N without the sequence clamp, 24 N with it) ---- */
static void condition(void) {
    static const int NS[] = {1, 31, 32, 33, 85, 86, 255, 256, 257, PRD_CONDITION_MAX_N, PRD_CONDITION_MAX_N + 1}, BS[] = {1, 8, PRD_CONDITION_MAX_B, PRD_CONDITION_MAX_B + 1};
    QI("condition_version", prd_condition_version(), 0);
    for (int i = 0; i < LEN(NS); ++i)
        for (int k = 0; k < LEN(BS); ++k)
            for (int keep = 0; keep < 4; ++keep) {
                const int N = NS[i], b = BS[k];
                if (k >= 2 && i != 2 && i < 9) continue;          /* the limits of b at one N and at the limits of N */
                CALL("condition_rows N %d b %d keep_z %d keep_seq %d", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), keep & 1 ? DP(5) : 0, DP(6), DP(7), DP(8),
                                                                                       keep & 2 ? DP(9) : 0, b, N, 21, 1000, s), N, b, keep & 1, keep >> 1);
            }
    printf("# condition refusals\n");
    CALL("condition_rows b 0", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), 0, 32, 21, 1000, s), 0);
    CALL("condition_rows levels 0", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), 1, 32, 21, 0, s), 0);
    CALL("condition_rows t null", prd_condition_rows(DP(1), DP(2), 0, DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), 1, 32, 21, 1000, s), 0);
    CALL("condition_rows keep_z, noise null", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), DP(5), 0, DP(7), DP(8), DP(9), 1, 32, 21, 1000, s), 0);
    CALL("condition_rows no keep_z, z null", prd_condition_rows(0, DP(2), (const int64_t*)VP(3), 0, 0, 0, 0, DP(8), DP(9), 1, 32, 21, 1000, s), 0);
    CALL("condition_rows keep_seq, seq0 null", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), DP(5), DP(6), DP(7), 0, DP(9), 1, 32, 21, 1000, s), 0);
    CALL("condition_rows no keep_seq, seq_t null, n_cls 20", prd_condition_rows(DP(1), 0, (const int64_t*)VP(3), DP(4), DP(5), DP(6), DP(7), 0, 0, 1, 32, 20, 1000, s), 0);
    CALL("condition_rows keep_seq, n_cls 20", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), DP(5), DP(6), DP(7), DP(8), DP(9), 1, 32, 20, 1000, s), 0);
    CALL("condition_rows nothing kept, N above the limit", prd_condition_rows(DP(1), DP(2), (const int64_t*)VP(3), DP(4), 0, DP(6), DP(7), DP(8), 0, 1, PRD_CONDITION_MAX_N + 1, 21, 1000, s), 0);
}

/* ---- sequence: the row tiles of 8, the census blocks at N n_cls on either side of a multiple of 64, the limits ---- */
static void sequence(void) {
    static const int NS[] = {1, 8, 9, 64, 65, PRD_SEQUENCE_MAX_N, PRD_SEQUENCE_MAX_N + 1};
    static const int BS[] = {1, PRD_SEQUENCE_MAX_B, PRD_SEQUENCE_MAX_B + 1}, SS[] = {1, 2, PRD_SEQUENCE_MAX_S, PRD_SEQUENCE_MAX_S + 1};
    QI("sequence_version", prd_sequence_version(), 0);
    for (int i = 0; i < LEN(NS); ++i) {
        const int N = NS[i];
        for (int k = 0; k < LEN(BS); ++k) {
            const int b = BS[k];
            printf("# sequence constrain N %d b %d\n", N, b);
            CALL("sequence_constrain no bias", prd_sequence_constrain(DP(1), DP(2), 0, DP(4), b, N, 21, 0, s), 0);
            CALL("sequence_constrain bias_b 1", prd_sequence_constrain(DP(1), DP(2), DP(3), DP(4), b, N, 21, 1, s), 0);
            CALL("sequence_constrain bias_b b", prd_sequence_constrain(DP(1), DP(2), DP(3), DP(4), b, N, 21, b, s), 0);
            CALL("sequence_constrain no rows", prd_sequence_constrain(DP(1), DP(2), DP(3), 0, b, N, 21, 1, s), 0);
        }
        for (int k = 0; k < LEN(SS); ++k) {
            const int S = SS[k];
            printf("# sequence decode, census N %d S %d\n", N, S);
            CALL("sequence_decode no bias, no gumbel", prd_sequence_decode((int32_t*)IP(1), DP(2), DP(3), DP(4), 0, DP(6), 0, 1.0f, S, N, 21, 0, s), 0);
            CALL("sequence_decode bias_b 1, gumbel", prd_sequence_decode((int32_t*)IP(1), DP(2), DP(3), DP(4), DP(5), DP(6), DP(7), 2.0f, S, N, 21, 1, s), 0);
            CALL("sequence_decode bias_b S, no gumbel", prd_sequence_decode((int32_t*)IP(1), DP(2), DP(3), DP(4), DP(5), DP(6), 0, 0.5f, S, N, 21, S, s), 0);
            CALL("sequence_census reference", prd_sequence_census((int32_t*)IP(1), (int32_t*)IP(2), (int32_t*)IP(3), (const int32_t*)IP(4), (const int32_t*)IP(5), DP(6), S, N, 21, s), 0);
            CALL("sequence_census no reference", prd_sequence_census((int32_t*)IP(1), 0, (int32_t*)IP(3), (const int32_t*)IP(4), 0, DP(6), S, N, 21, s), 0);
        }
    }
    printf("# sequence refusals\n");
    CALL("sequence_constrain b 0", prd_sequence_constrain(DP(1), DP(2), DP(3), DP(4), 0, 8, 21, 1, s), 0);
    CALL("sequence_constrain N 0, n_cls 20", prd_sequence_constrain(DP(1), DP(2), DP(3), DP(4), 1, 0, 20, 1, s), 0);
    CALL("sequence_constrain n_cls 20", prd_sequence_constrain(DP(1), DP(2), DP(3), DP(4), 1, 8, 20, 1, s), 0);
    CALL("sequence_constrain bias_b 2 of 8", prd_sequence_constrain(DP(1), DP(2), DP(3), DP(4), 8, 8, 21, 2, s), 0);
    CALL("sequence_constrain bias_b 2 of 8, no rows", prd_sequence_constrain(DP(1), DP(2), DP(3), 0, 8, 8, 21, 2, s), 0);
    CALL("sequence_constrain seq_t null", prd_sequence_constrain(0, DP(2), DP(3), DP(4), 8, 8, 21, 1, s), 0);
    CALL("sequence_constrain seq_t null, no rows", prd_sequence_constrain(0, DP(2), DP(3), 0, 8, 8, 21, 1, s), 0);
    CALL("sequence_decode bias_b 2 of 8", prd_sequence_decode((int32_t*)IP(1), DP(2), DP(3), DP(4), DP(5), DP(6), 0, 1.0f, 8, 8, 21, 2, s), 0);
    CALL("sequence_decode rows null", prd_sequence_decode((int32_t*)IP(1), DP(2), DP(3), DP(4), DP(5), 0, 0, 1.0f, 8, 8, 21, 1, s), 0);
    CALL("sequence_decode entropy null", prd_sequence_decode((int32_t*)IP(1), DP(2), 0, DP(4), DP(5), DP(6), 0, 1.0f, 8, 8, 21, 1, s), 0);
    CALL("sequence_census mask null", prd_sequence_census((int32_t*)IP(1), (int32_t*)IP(2), (int32_t*)IP(3), (const int32_t*)IP(4), (const int32_t*)IP(5), 0, 8, 8, 21, s), 0);
    CALL("sequence_census recovery without reference", prd_sequence_census((int32_t*)IP(1), (int32_t*)IP(2), (int32_t*)IP(3), (const int32_t*)IP(4), 0, DP(6), 8, 8, 21, s), 0);
    CALL("sequence_census reference without recovery", prd_sequence_census((int32_t*)IP(1), 0, (int32_t*)IP(3), (const int32_t*)IP(4), (const int32_t*)IP(5), DP(6), 8, 8, 21, s), 0);
    CALL("sequence_census n_cls 20", prd_sequence_census((int32_t*)IP(1), 0, (int32_t*)IP(3), (const int32_t*)IP(4), 0, DP(6), 8, 8, 20, s), 0);
}

int main(void) {
    align();
    tmalign();
    quality();
    condition();
    sequence();
    return 0;
}
