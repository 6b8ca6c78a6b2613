/* libprd_quality.so -- C ABI of the superposition-free scores of generated samples: lDDT and pair censuses on the device.
 *
 * libprd_align.so and libprd_tmalign.so score a sample after a global fit.  The questions asked first about a protein-ligand complex are
 * local and need no fit: is the neighbourhood of every position preserved (lDDT, and its protein-ligand form), do atoms sit on top of
 * each other, are bonded atoms at bond length, which residues line the pocket.  All of them are counts over the N x N distances of a
 * structure; this library makes them in one sweep that reads 24 bytes per position and never holds an N x N matrix.
 *
 * It is a library of its own: nothing here is part of the denoiser ABI (include/prd_hip.h), and nothing here depends on libprd_hip.so,
 * libprd_align.so or libprd_tmalign.so.  The rules of the boundary are those of prd_align.h:
 *   - extern "C", plain pointers / ints only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch at all (there is no `ws`, hence no workspace query).  No
 *     process-wide state, no environment variable.
 *   - Every call only enqueues work on `stream` (kernels, and for prd_quality_contacts one memset node of S ints), never synchronises,
 *     and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from a launch, or a negative PRD_QUALITY_ERR_*.  A refusal launches nothing
 *     and leaves the outputs untouched.
 *
 * Structures X[S][N][3] (fp32, Angstrom; element (s, i, c) at x[s * x_struct_stride + i * x_row_stride + c], strides in floats) and, for
 * lDDT, ONE reference Y[N][3] with a row stride of its own, so Y may be the C-alpha column of a residue_atom_pos tensor.  Masks are fp32
 * 0 / 1 as in prd_align.h (m[i] > 0.5: set).
 *
 * Distances.  d_ij = |x_i - x_j| and D_ij = |y_i - y_j| are formed in fp32 from the caller's uncentred coordinates: three differences,
 * their squares summed in the order x, y, z without fused multiply-adds, so d_ij == d_ji bit for bit, and a structure and its mirror
 * image (one coordinate negated) have bit-identical distances.  Coordinates are expected within ~100 Angstrom of each other (a
 * difference of two fp32 coordinates that lie within a factor of two of each other is exact, so a structure translated far from the
 * origin loses nothing that its fp32 coordinates had not lost already): a distance is then good to ~2e-5 Angstrom.
 * The inclusion radius and the contact cutoff are compared SQUARED: D_ij^2 < radius * radius and d_ij^2 < cutoff * cutoff, the
 * right-hand sides rounded once to fp32.  The lDDT thresholds are compared on the distances themselves, |d_ij - D_ij| < t, with one
 * hardware square root (1 ulp) for each of the two.  All comparisons are strict.
 *
 * prd_quality_lddt.  A pair (i, j) is INCLUDED when row_mask[i] > 0.5, col_mask[j] > 0.5, i != j and D_ij^2 < radius^2.
 *   total[i]          int32: the number of included pairs of row i (a property of the reference alone; written once per call)
 *   preserved[s][i]   int32: sum over the included pairs of row i and over t in {0.5, 1, 2, 4} Angstrom of [ |d_ij - D_ij| < t ], d of sample s
 * Rows with row_mask[i] <= 0.5 get 0 in both.  Every element of both outputs is written.  The scores are quotients of these
 * integers (per position preserved / (4 total); pooled over a structure sum preserved / (4 sum total)), formed by the caller.
 *
 * prd_quality_contacts.  A pair (i, j) QUALIFIES when a_mask[i] > 0.5, b_mask[j] > 0.5, i != j and (exclude == NULL or
 * exclude[i * N + j] == 0; uint8, [N][N] row-major).
 *   count[s]          int32: the number of qualifying pairs with d_ij^2 < cutoff^2.  A pair whose reverse (j, i) qualifies as well (both
 *                     ends in A and in B, neither order excluded) is counted once, not twice.
 *   nearest[s][i]     fp32: the minimum d_ij over the qualifying pairs of row i, +inf when there is none; rows outside A get +inf
 * Every element of both outputs is written.  count is accumulated with INTEGER atomic adds, one per workgroup, onto a memset of the
 * same call: there is no floating-point atomic anywhere, and both operators give bit-identical results from one launch to the next.
 *
 * Limits: N <= PRD_QUALITY_MAX_N = 32768 -- the columns are swept in tiles of 256 through the LDS, so N is bounded by int32 counts
 * (N^2 pairs <= 2^30), not by memory; S <= 65535, the second grid dimension (else PRD_QUALITY_ERR_UNSUPPORTED). */
#ifndef PRD_QUALITY_H
#define PRD_QUALITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_QUALITY_VERSION 100
#define PRD_QUALITY_ERR_ARG (-1)          /* null required pointer / non-positive dimension / row stride below 3 / negative structure stride /
                                             radius or cutoff not finite or not positive */
#define PRD_QUALITY_ERR_UNSUPPORTED (-3)  /* N above PRD_QUALITY_MAX_N; S above PRD_QUALITY_MAX_S */
#define PRD_QUALITY_MAX_N 32768
#define PRD_QUALITY_MAX_S 65535

int prd_quality_version(void);

/* preserved [S][N], total [N], both int32 and contiguous; see the head of this file */
int prd_quality_lddt(int* preserved, int* total,
                     const float* x, long long x_struct_stride, int x_row_stride,
                     const float* y, int y_row_stride,
                     const float* row_mask, const float* col_mask, float radius, int S, int N, hipStream_t stream);

/* count [S] int32, nearest [S][N] fp32, both contiguous; exclude [N][N] uint8 or NULL; see the head of this file */
int prd_quality_contacts(int* count, float* nearest,
                         const float* x, long long x_struct_stride, int x_row_stride,
                         const float* a_mask, const float* b_mask, const uint8_t* exclude, float cutoff, int S, int N,
                         hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
