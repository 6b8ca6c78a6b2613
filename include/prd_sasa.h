/* libprd_sasa.so -- C ABI of the solvent-accessibility count: Shrake and Rupley's point test on the atoms of every sample.
 *
 * Every atom carries a REACH, its van der Waals radius plus the probe radius.  P points lie on the sphere of that radius about the atom;
 * the count of an atom is the number of its points that lie inside no other atom's sphere.  4 pi reach^2 count / P is its
 * solvent-accessible area; the caller forms that quotient (protein_redesign_amd/sasa.py: area), the library returns integers.
 *
 * A library of its own under the rules of prd_backbone.h:
 *   - extern "C", plain pointers / ints / floats only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch.  No process-wide state, no environment variable.
 *   - A call only enqueues ONE kernel on `stream`, never synchronises, and is capturable.
 *   - Return value: 0 on success, a positive hipError_t from the launch, or a negative PRD_SASA_ERR_*.  Every refusal happens on the host
 *     before any HIP call, launches nothing and leaves the output untouched.
 *   - No read-modify-write of memory of any kind.  Every output element has one owner and is written; two calls on the same input give
 *     equal bits.
 *
 * ---- prd_sasa_count ---------------------------------------------------------------------------------------------------------------
 * Inputs.  pos: element (s, a, c) at pos[s * stride_s + a * stride_a + c], strides in floats, the last stride 1 -- so the samples may be a
 * strided view.  reach[A]: shared by the samples.  present[S][A] int32: 0, the atom does not exist in this sample.  group[A] int32 or
 * NULL.  sphere[P][3]: unit vectors, the same P directions for every atom.
 *
 * DEFINITION.  Atom i of sample s, at c_i, has the points  p_k = reach_i * sphere_k  (k = 0 .. P-1), in the frame centred on atom i.
 * With d_j = c_j - c_i, point k is BURIED when
 *       |p_k - d_j|^2 < reach_j^2          (strictly)
 * for some atom j != i that is present and counts under `mode`.  count[s][i] is the number of points that are not buried; it is 0 for
 * an atom that is not present.
 *   mode = PRD_SASA_ALL         every present j counts; `group` is not read.
 *   mode = PRD_SASA_SAME_GROUP  only j with group[j] == group[i] count: every partner's own surface, the others taken away.
 *                               `group` is required.
 *
 * ARITHMETIC, part of the definition.  fp32 without fused multiply-adds (the build keeps -ffp-contract=off):
 *       d = c_j - c_i per coordinate;  p_k = reach_i * sphere_k per coordinate;  e = p_k - d per coordinate;
 *       |e|^2 = (ex * ex + ey * ey) + ez * ez;   compared against  reach_j * reach_j.
 * No reciprocal, no square root.  Everything happens in the RELATIVE frame c_j - c_i, so a common offset of all coordinates costs the
 * accuracy of one subtraction and no more.  The kernel skips an atom j whose centre lies so far away that no point can be buried by it,
 * |d_j|^2 >= (reach_i + reach_j)^2 (1 + 1e-4); the factor is two orders of magnitude above what the fp32 rounding of either test can make
 * of a tangent pair, so the skip changes no count.  There is no cap on the number of neighbours.
 *
 * The caller's duties.  reach is finite and >= 0 for every atom, and the coordinates of every PRESENT atom are finite (the Python layer
 * checks reach, which it builds).  The coordinates of an atom that is not present may be anything, NaN included: they enter no
 * comparison and influence no count.
 *
 * Refusals.  PRD_SASA_ERR_ARG: a null pointer (group under PRD_SASA_ALL excepted); S, A or P not positive; a mode that is neither of
 * the two; PRD_SASA_SAME_GROUP without group; strides that overlap -- stride_a < 3, or, for S > 1, stride_s < (A - 1) stride_a + 3.
 * PRD_SASA_ERR_UNSUPPORTED: P no multiple of 64 (a lane of the wave owns the points l, l + 64, ...); P > PRD_SASA_MAX_P;
 * A > PRD_SASA_MAX_A; S > PRD_SASA_MAX_S (a grid dimension).  A bad argument is named before a limit.
 *
 * The point set is the caller's.  With the Fibonacci lattice of sasa.py the directions are not mirror-symmetric: the mirror image of a
 * structure gets nearly the same counts, not the same bits. */
#ifndef PRD_SASA_H
#define PRD_SASA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_SASA_VERSION 100
#define PRD_SASA_ERR_ARG (-1)          /* null required pointer / non-positive S, A or P / unknown mode / SAME_GROUP without group /
                                          overlapping strides */
#define PRD_SASA_ERR_UNSUPPORTED (-3)  /* P no multiple of 64 or above PRD_SASA_MAX_P; A above PRD_SASA_MAX_A; S above PRD_SASA_MAX_S */
#define PRD_SASA_MAX_P 1024
#define PRD_SASA_MAX_A 65536
#define PRD_SASA_MAX_S 65535
#define PRD_SASA_ALL 0
#define PRD_SASA_SAME_GROUP 1

int prd_sasa_version(void);

/* count [S][A] int32; pos [S][A][3] fp32 by strides; reach [A] fp32; present [S][A] int32; group [A] int32 or NULL; sphere [P][3] fp32 */
int prd_sasa_count(int* count, const float* pos, long long stride_s, long long stride_a, const float* reach, const int* present,
                   const int* group, const float* sphere, int mode, int S, int A, int P, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
