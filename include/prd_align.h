/* libprd_align.so -- C ABI of the post-processing of generated samples: superposition and TM-score on the device.
 *
 * The reference's generate.py:163-195 superimposes every sample on a reference structure with the TM-align program, once as it is
 * and once mirrored, keeps the better of the two and writes the scores.  The residue correspondence is known here (same chain,
 * same length, position i <-> position i), so what is left of TM-align is the TM-score superposition search: Kabsch fits on seeded
 * subsets, iterated.  That search is what this library does, for many pairs of structures in one call.
 *
 * It is a library of its own: post-processing of samples is not part of the denoiser ABI (include/prd_hip.h), and nothing here
 * depends on libprd_hip.so.  The rules of the boundary are those of prd_hip.h:
 *   - extern "C", plain pointers / ints only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory: scratch is passed in as `ws` with its size in bytes (query with
 *     prd_align_workspace_bytes; 16-byte aligned).  No process-wide state, no environment variable.
 *   - Every call only enqueues kernels on `stream`, never synchronises, and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from a launch, or a negative PRD_ALIGN_ERR_*.
 *
 * The problem.  Structures X[S][N][3] and Y[R][N][3] (fp32, Angstrom; element (s, i, c) at x[s * x_struct_stride + i * x_row_stride + c],
 * strides in floats, so Y may be the C-alpha column of a residue_atom_pos tensor) and ONE 0/1 mask m[N] shared by all structures
 * (m[i] > 0.5: position i takes part; ligand atoms, padding, residues without a C-alpha are 0).  L = number of masked positions,
 * counted on the device.  For every requested pair (s, r):
 *   rot[s][r][3][3], trans[s][r][3]   the transform in the reference's row-vector convention  y ~ trans + x @ rot  (generate.py:180)
 *   tm[s][r]                          TM = (1/L) sum_i 1 / (1 + d_i^2 / d0^2),  d_i = |trans + x_i @ rot - y_i| over the masked positions,
 *                                     d0 = 1.24 (L - 15)^(1/3) - 1.8 for L > 21 and 0.5 otherwise (TM-score's convention)
 *   rmsd[s][r]                        sqrt((1/L) sum_i d_i^2) under that transform
 *   mirrored[s][r]                    int32: 1 when the mirror image of x fitted better (then det(rot) = -1), else 0
 * tm and rmsd are evaluated in double precision from the fp32 transform that is returned.
 *
 * PRD_ALIGN_PAIRS_CROSS: all S x R pairs.  PRD_ALIGN_PAIRS_SELF: Y is X (pass y = NULL or y = x, R = S): only s < r is searched, the
 * result is written to (s, r) and, inverted, to (r, s); the diagonal is tm 1, rmsd 0, identity, not mirrored.
 *
 * PRD_ALIGN_MODE_RMSD: one Kabsch fit over all masked positions (proper rotation).
 * PRD_ALIGN_MODE_TM: maximise TM.  With d0_search = clamp(d0, 4.5, 8):
 *   1. fragment lengths Lf = L, L/2, L/4, ... (integer halving) while they exceed 4, then 4 itself, and for 4 <= L <= 21 also 3
 *      (d0 is 0.5 there and d_cut at least 3.5: the rounds cannot shed an outlier of so small a chain); L itself when L < 4;
 *   2. fragment starts every max(1, Lf/2) positions plus the last possible start, positions counted in the compacted, masked order;
 *   3. per seed up to 20 rounds of: Kabsch on the current subset; score all L positions and keep the best TM seen; the next subset
 *      is {i : d_i < d_cut}, d_cut = d0_search - 1 after the first fit and d0_search + 1 afterwards, raised by 0.5 until at least 3
 *      positions qualify; stop when the subset does not change;
 *   4. best over seeds, ties to the lowest seed index.
 * `mirror` != 0: the same is done for x * diag(1, 1, -1) and the better result is kept (TM mode: the higher TM; RMSD mode: the lower
 * RMSD; a tie goes to the unmirrored one).  The matrix returned for a mirrored result is diag(1, 1, -1) @ rot', so that
 * y ~ trans + x @ rot holds for the caller's own x.
 * L < 3: every requested entry, the diagonal included, is tm 0, rmsd 0, identity, not mirrored.
 *
 * Limits: N <= PRD_ALIGN_MAX_N (else PRD_ALIGN_ERR_UNSUPPORTED); S * R is limited by the workspace alone.  Coordinates are expected
 * within ~100 Angstrom of the origin: distances are formed in fp32 from uncentred coordinates (~1e-5 Angstrom there). */
#ifndef PRD_ALIGN_H
#define PRD_ALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_ALIGN_VERSION 100
#define PRD_ALIGN_ERR_ARG (-1)          /* null pointer / non-positive dimension / row stride below 3 / unknown mode */
#define PRD_ALIGN_ERR_UNSUPPORTED (-3)  /* N above PRD_ALIGN_MAX_N; more pairs than a launch takes (2^31 - 1 with the mirror images) */
#define PRD_ALIGN_ERR_WORKSPACE (-4)    /* workspace too small or not 16-byte aligned */
#define PRD_ALIGN_MAX_N 4096
#define PRD_ALIGN_MODE_TM 0
#define PRD_ALIGN_MODE_RMSD 1
#define PRD_ALIGN_PAIRS_CROSS 0
#define PRD_ALIGN_PAIRS_SELF 1

int prd_align_version(void);

/* bytes of `ws` that prd_align_superimpose needs for these arguments (0 for arguments it would refuse) */
size_t prd_align_workspace_bytes(int S, int R, int N, int pairs, int mode, int mirror);

/* outputs [S][R] (rot [S][R][3][3], trans [S][R][3]), row-major; see the head of this file */
int prd_align_superimpose(float* tm, float* rmsd, float* rot, float* trans, int* mirrored,
                          const float* x, long long x_struct_stride, int x_row_stride,
                          const float* y, long long y_struct_stride, int y_row_stride,
                          const float* mask, int S, int R, int N, int pairs, int mode, int mirror,
                          void* ws, size_t ws_bytes, hipStream_t stream);

/* out[s][i][:] = trans[s] + pos[s][i][:] @ rot[s] for contiguous pos / out [S][N][3] (whole rows: ligand atoms included); out may
 * be pos.  No limit on N; S <= 65535 (else PRD_ALIGN_ERR_UNSUPPORTED). */
int prd_align_apply(float* out, const float* pos, const float* rot, const float* trans, int S, int N, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
