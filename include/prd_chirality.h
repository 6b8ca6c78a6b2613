/* libprd_chirality.so -- C ABI of the handedness census of generated samples: which hand a sample has, read off the sample itself.
 *
 * The denoiser is equivariant under reflections, so a sample is as likely to come out as the mirror image of a protein as the right way
 * round, and every score of libprd_quality.so is blind to it (distances only).  The information is local: the virtual dihedral of four
 * consecutive C-alphas is about +50 degrees in a right-handed alpha-helix and about -50 degrees in its mirror image, and the signed volume
 * at a tetrahedral centre of the ligand changes sign under reflection.  This library counts both on the device, decides per sample, and
 * reflects the samples judged mirrored in place.
 *
 * It is a library of its own: nothing here is part of the denoiser ABI (include/prd_hip.h), and nothing here depends on another library
 * of the project.  The rules of the boundary are those of prd_quality.h:
 *   - extern "C", plain pointers / ints / floats only.  All pointers are DEVICE pointers owned by the caller, with ONE exception that
 *     is named as such: centres_host, the caller's host copy of the centre list, which is read on the host during the call and never
 *     handed to a kernel (see "Ligand centres").
 *   - The library never allocates device memory and needs no scratch (there is no `ws`).  No process-wide state, no environment variable.
 *   - Every call only enqueues ONE kernel on `stream`, never synchronises, and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from the launch, or a negative PRD_CHIRALITY_ERR_*.  A refusal launches nothing
 *     and leaves the outputs untouched.
 *   - No atomics of any kind: one workgroup owns a sample and sums its counts in a fixed order.  Two launches on the same input give
 *     equal bits.
 *
 * Structures X[S][N][3] (fp32, Angstrom; element (s, i, c) at x[s * x_struct_stride + i * x_row_stride + c], strides in floats, the row
 * stride at least 3, the structure stride not negative).  Masks are fp32 0 / 1 (m[i] > 0.5: set).
 *
 * Arithmetic.  Everything is fp32 without fused multiply-adds (the build keeps -ffp-contract=off).  A difference is d = p_b - p_a per
 * coordinate; a dot product is (u0 v0 + u1 v1) + u2 v2; a cross product is (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).  Negating
 * one coordinate of a structure therefore leaves every bond length, every b.b' and n1.n2 bit-identical and negates b1.n2 and every
 * signed volume exactly: the census of a mirror image is the census of the original with the hands swapped, bit for bit.
 *
 * Trace quads.  Row i STARTS A QUAD (i, i+1, i+2, i+3) when i + 3 < N, mask[i..i+3] > 0.5, link[i], link[i+1], link[i+2] > 0.5
 * (link[i]: rows i and i+1 are consecutive residues of one chain -- the caller's statement; link[N-1] is never read as a bond) and each
 * of the three virtual bonds b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2 has bond_lo^2 < |b|^2 < bond_hi^2 (the squares of the two
 * arguments are formed once in fp32 on the host; strict).  With n1 = b1 x b2 and n2 = b2 x b3:
 *   tau      = atan2(|b2| (b1.n2), n1.n2), the sign of the first argument copied onto the result: tau(-y, x) == -tau(y, x) bit for bit
 *   cos th1  = -(b1.b2) / (|b1| |b2|), cos th2 = -(b2.b3) / (|b2| |b3|): the cosines of the angles at p1 and p2
 * A quad's CLASS (all comparisons strict):
 *   1 right helical           helix_cos_lo < cos th1, cos th2 < helix_cos_hi     and  helix_tau_lo < tau < helix_tau_hi
 *   2 left helical            the same cosines                                      and  helix_tau_lo < -tau < helix_tau_hi
 *   3 extended, native twist  ext_cos_lo < cos th1, cos th2 < ext_cos_hi           and  ext_tau_lo < -tau < ext_tau_hi
 *   4 extended, mirror twist  the same cosines                                      and  ext_tau_lo < tau < ext_tau_hi
 *   0 none                    anything else; the helical window is looked at first
 * The cosine edges are the cosines of the angle window's edges (an angle window (75, 110) degrees is the cosine window (cos 110, cos 75)),
 * the tau edges are radians in [0, pi]; the caller rounds each once to fp32.  The mirror classes use the mirrored tau window, so classes
 * 1 <-> 2 and 3 <-> 4 swap under reflection by construction.
 *
 * Ligand centres.  centres[C][4] int32 holds rows (c, n1, n2, n3) of the structure.
 *   V = (x_n1 - x_c) . ((x_n2 - x_c) x (x_n3 - x_c))      (an ideal sp3 centre with 1.5 Angstrom bonds: |V| = 2.60 Angstrom^3)
 * centre_ref[C] fp32 is the same volume in the caller's reference structure, or NULL.  A centre is FLAT when |V| < vmin; otherwise, with
 * a reference, KEPT when (V > 0) == (centre_ref[c] > 0) and INVERTED when not.  Without a reference only the flat ones are counted.
 * WHO VALIDATES THE ROWS: the library, on the host.  With C > 0 the caller passes the same list twice: `centres` on the device, which
 * the kernel reads, and `centres_host`, the copy the device list was uploaded from, which this call walks before it launches: a row
 * outside [0, N) is PRD_CHIRALITY_ERR_ARG and nothing is launched.  The library cannot look at device memory without synchronising;
 * that the two copies are equal is the caller's statement (protein_redesign_amd/chirality.py uploads the one from the other).
 * With C == 0 all three pointers are ignored and may be NULL.
 *
 * Outputs (every element written; tau, cls and volume may be NULL, volume is ignored when C == 0):
 *   counts[S][8]  int32: helix_right, helix_left, extended_native, extended_mirror, quads (rows that start a quad), centres_kept,
 *                 centres_inverted, centres_flat
 *   verdict[S]    int32: +1 natural hand, -1 mirror image, 0 undecided;  basis[S] int32: the rule that decided (below)
 *   tau[S][N]     fp32 radians, NaN where row i starts no quad;  cls[S][N] int32, 0 there
 *   volume[S][C]  fp32
 * Verdict, evaluated after the sums, in this order:
 *   1  h = helix_right - helix_left; |h| >= min_helix and h != 0: verdict = sign(h), basis PRD_CHIRALITY_BASIS_HELIX
 *   2  else, with a centre reference, kept + inverted >= 1 and one of the two 0: +1 for all kept, -1 for all inverted,
 *      basis PRD_CHIRALITY_BASIS_CENTRES
 *   3  else e = extended_native - extended_mirror; |e| >= min_extended and e != 0: verdict = sign(e), basis PRD_CHIRALITY_BASIS_EXTENDED
 *   4  else 0, basis PRD_CHIRALITY_BASIS_NONE
 *
 * prd_chirality_reflect negates coordinate 0 of every row of every structure s with flip[s] != 0 (flip: int32 on the device, so nothing
 * goes to the host between a census and the reflection) and touches nothing else.  The negation is a change of the sign bit: applying it
 * twice restores the bits, and every distance of prd_quality.h is bit-identical to the original's.
 *
 * Limits (else PRD_CHIRALITY_ERR_UNSUPPORTED): N <= PRD_CHIRALITY_MAX_N, S <= PRD_CHIRALITY_MAX_S (a grid dimension), C <= PRD_CHIRALITY_MAX_C. */
#ifndef PRD_CHIRALITY_H
#define PRD_CHIRALITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_CHIRALITY_VERSION 100
#define PRD_CHIRALITY_ERR_ARG (-1)          /* null required pointer / non-positive S or N / negative C / row stride below 3 / negative structure
                                               stride / a window edge not finite, a cosine edge outside [-1, 1], a tau edge outside [0, pi], lo >= hi /
                                               bond_lo not positive or not below bond_hi / vmin not positive and finite / a negative minimum /
                                               C > 0 without centres or centres_host / a centre row outside [0, N) */
#define PRD_CHIRALITY_ERR_UNSUPPORTED (-3)  /* N above PRD_CHIRALITY_MAX_N; S above PRD_CHIRALITY_MAX_S; C above PRD_CHIRALITY_MAX_C */
#define PRD_CHIRALITY_MAX_N 32768
#define PRD_CHIRALITY_MAX_S 65535
#define PRD_CHIRALITY_MAX_C 1024
#define PRD_CHIRALITY_BASIS_NONE 0
#define PRD_CHIRALITY_BASIS_HELIX 1
#define PRD_CHIRALITY_BASIS_CENTRES 2
#define PRD_CHIRALITY_BASIS_EXTENDED 3

int prd_chirality_version(void);

/* counts [S][8], verdict [S], basis [S], cls [S][N] int32; tau [S][N], volume [S][C] fp32; all contiguous; see the head of this file */
int prd_chirality_census(int* counts, int* verdict, int* basis, float* tau, int* cls, float* volume,
                         const float* x, long long x_struct_stride, int x_row_stride,
                         const float* mask, const float* link,
                         const int* centres, const int* centres_host, const float* centre_ref, int C,
                         float helix_cos_lo, float helix_cos_hi, float helix_tau_lo, float helix_tau_hi,
                         float ext_cos_lo, float ext_cos_hi, float ext_tau_lo, float ext_tau_hi,
                         float bond_lo, float bond_hi, float vmin, int min_helix, int min_extended,
                         int S, int N, hipStream_t stream);

/* x [S][N][3] with the strides above, flip [S] int32; see the head of this file */
int prd_chirality_reflect(float* x, long long x_struct_stride, int x_row_stride, const int* flip, int S, int N, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
