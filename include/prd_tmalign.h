/* libprd_tmalign.so -- C ABI of the structural alignment of generated samples to a reference of ANOTHER length, on the device.
 *
 * include/prd_align.h is the half of TM-align that assumes the correspondence is known (position i <-> position i).  This library is
 * the other half: it finds the correspondence by structure -- a dynamic-programming alignment (Needleman-Wunsch over a TM-score
 * matrix) iterated with Kabsch fits -- for many pairs of structures in one call.  It is a cut of TM-align, stated in full below and
 * restated in float64 numpy by tests/tmalign_ref.py.
 *
 * A library of its own, with the boundary rules of prd_align.h:
 *   - extern "C", plain pointers / ints only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory: scratch is passed in as `ws` with its size in bytes (query with
 *     prd_tmalign_workspace_bytes; 16-byte aligned).  No environment variable, and no process-wide state of the library's own; the one
 *     thing a call changes outside its arguments is an attribute of its own kernels: where a workgroup needs more than 48 KiB of
 *     dynamic LDS (rows beyond ~700), hipFuncSetAttribute raises that kernel's limit to what PRD_TMALIGN_MAX_N needs -- the same
 *     value every time, before anything is enqueued, also under stream capture (it is no stream operation).
 *   - Every call only enqueues kernels on `stream`, never synchronises (all lengths stay on the device), and is capturable into a
 *     hipGraph.  No atomics, one owner per output element: two calls on the same inputs are bit-equal.
 *   - Return value: 0 on success, a positive hipError_t from a launch, or a negative PRD_TMALIGN_ERR_*.
 *
 * The problem.  Samples X[S][Nx][3] with ONE 0/1 mask mx[Nx] shared by the samples, references Y[R][Ny][3] with one mask my[Ny]
 * (fp32, Angstrom; element (s, i, c) at x[s * x_struct_stride + i * x_row_stride + c], strides in floats, as in
 * prd_align_superimpose; m[i] > 0.5: row i takes part).  Lx and Ly are the masked counts, counted on the device.  All S x R pairs are
 * processed.  Per pair (s, r):
 *   rot[s][r][3][3], trans[s][r][3]   row-vector convention  y ~ trans + x @ rot
 *   tm[s][r]                          (1/Ly) sum over the aligned pairs of 1 / (1 + d^2 / d0^2), d0 = d0(Ly) as defined in prd_align.h:
 *                                     the TM-score normalised by the reference (TM-align's TM2)
 *   rmsd[s][r]                        over the aligned pairs
 *   n_aligned[s][r]                   int32: number of aligned pairs
 *   mirrored[s][r]                    int32: 1 when the mirror image of x aligned better (then det(rot) = -1)
 *   map[s][r][Nx]                     int32: the ROW of Y (caller's layout, not compacted) aligned to row i of X, or -1; strictly
 *                                     increasing over the aligned rows
 * tm and rmsd are evaluated in double precision from the fp32 transform and the mapping that are returned.
 *
 * The algorithm.  Positions are counted in the compacted, masked order.  All scores use d0 = d0(Ly); a "score" of an alignment under
 * a transform T is sum over its pairs of 1 / (1 + |T x_i - y_j|^2 / d0^2).
 *   1. Secondary structure of both chains.  For an interior position i with the five C-alphas 1 .. 5 = i-2 .. i+2 and their
 *      distances d13, d14, d15, d24, d25, d35:  helix when |d15 - 6.37| < 2.1, |d14 - 5.18| < 1.42, |d25 - 5.18| < 1.42 and
 *      |d13 - 5.45|, |d24 - 5.45|, |d35 - 5.45| < 0.81;  else strand when |d15 - 13.0|, |d14 - 10.4|, |d25 - 10.4|, |d13 - 6.1|,
 *      |d24 - 6.1|, |d35 - 6.1| < 1.42;  else turn when d15 < 8;  else coil.  The two positions at each end are coil.
 *   2. Three initial alignments:
 *      A  gapless threading: every offset k (x_i <-> y_{i+k}, k ascending) whose overlap has at least max(min(Lx, Ly) / 2, 5)
 *         positions (integer division); one Kabsch fit on the overlap; the offset of the best score, ties to the lowest k;
 *      B  the DP of step 3 with s_ij = 1 where the classes are equal, 0 otherwise, and gap = -1;
 *      C  the DP with s_ij = 0.5 [classes equal] + 1 / (1 + |T_A x_i - y_j|^2 / d0^2) under the fit T_A of A's best offset, gap = -1.
 *      An alignment of fewer than 3 pairs is dropped.
 *   3. The DP.  val[0][.] = val[.][0] = 0 and diag = false on the borders (end gaps are free);
 *         D = val[i-1][j-1] + s_ij,  H = val[i-1][j] + (diag[i-1][j] ? gap : 0),  V = val[i][j-1] + (diag[i][j-1] ? gap : 0),
 *         val[i][j] = max(D, H, V),  diag[i][j] = (D >= H and D >= V);
 *      the direction of a cell is recorded when it is filled: D when diag, else H when H >= V, else V.  The traceback runs from
 *      (Lx, Ly) along the recorded directions (D aligns x_i with y_j); a cell on a border ends it.  s_ij is an fp32 number, the
 *      recurrence runs in fp64.
 *   4. Refinement of each initial alignment.  T, score <- fast search on its pairs.  Then for gap in (-0.6, 0), up to 30 rounds of:
 *      the DP with s_ij = 1 / (1 + |T x_i - y_j|^2 / d0^2); this gap value ends when the alignment equals the previous round's (before
 *      the first round: the current one) or has fewer than 3 pairs; otherwise T, score <- fast search on the new pairs, and the best
 *      (alignment, T, score) seen is kept (the earlier one among equals).  T is always that of the LATEST search.
 *      The fast search is the search of prd_align.h, TM mode, steps 1-4, over the n aligned pairs (x_i, y_j) in order, scored with
 *      d0(Ly), with step 1 cut to the first two fragment lengths (n, and the next one of that list for n).
 *   5. The best of the three refinements, ties to A, then B, then C.  Pairs farther apart than d8 = 1.5 Ly^0.3 + 3.5 under its
 *      transform are dropped unless fewer than 3 would remain.  The full search of prd_align.h (all fragment lengths) runs on what
 *      remains and gives the transform; the mapping is what remains.
 *   `mirror` != 0: the same for x * diag(1, 1, -1); the higher score is kept, a tie goes to the unmirrored result, and the matrix
 *   returned for a mirrored result is diag(1, 1, -1) @ rot', so that y ~ trans + x @ rot holds for the caller's own x.
 *   Lx < 5 or Ly < 5: tm 0, rmsd 0, 0 aligned pairs, identity, not mirrored, a mapping of all -1.
 * Still outside the cut: TM-align's fragment-pair seeds (get_initial5), its second normalisation (TM1), circular permutation,
 * multi-chain references.
 *
 * Limits: Nx, Ny <= PRD_TMALIGN_MAX_N (else PRD_TMALIGN_ERR_UNSUPPORTED); S * R * (mirror ? 2 : 1) * 3
 * <= PRD_TMALIGN_MAX_PROBLEMS, the workgroups of the refinement launch, and S + R likewise (the direction bits
 * of the DP are 2 bits per cell per (pair, mirror, initial alignment): 1 MiB each at 2048 x 2048).  Coordinates are expected within
 * ~100 Angstrom of the origin.  Every loop whose bound comes from device data is clamped by a constant (30 rounds, 20 search rounds,
 * Nx + Ny traceback steps): non-finite input ends, with a result that means nothing. */
#ifndef PRD_TMALIGN_H
#define PRD_TMALIGN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_TMALIGN_VERSION 100
#define PRD_TMALIGN_ERR_ARG (-1)          /* null pointer / non-positive dimension / row stride below 3 / negative struct stride */
#define PRD_TMALIGN_ERR_UNSUPPORTED (-3)  /* Nx or Ny above PRD_TMALIGN_MAX_N; more than PRD_TMALIGN_MAX_PROBLEMS */
#define PRD_TMALIGN_ERR_WORKSPACE (-4)    /* workspace too small or not 16-byte aligned */
#define PRD_TMALIGN_MAX_N 2048
#define PRD_TMALIGN_MAX_PROBLEMS 1048576  /* (pair, mirror, initial alignment) triples of one call */

int prd_tmalign_version(void);

/* bytes of `ws` that prd_tmalign_align needs for these arguments (0 for arguments it would refuse) */
size_t prd_tmalign_workspace_bytes(int S, int R, int Nx, int Ny, int mirror);

/* outputs [S][R] (rot [S][R][3][3], trans [S][R][3], map [S][R][Nx]), row-major; see the head of this file */
int prd_tmalign_align(float* tm, float* rmsd, float* rot, float* trans, int* n_aligned, int* mirrored, int* map,
                      const float* x, long long x_struct_stride, int x_row_stride, const float* mask_x,
                      const float* y, long long y_struct_stride, int y_row_stride, const float* mask_y,
                      int S, int R, int Nx, int Ny, int mirror,
                      void* ws, size_t ws_bytes, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
