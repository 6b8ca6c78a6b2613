/* libprd_dssp.so -- C ABI of the secondary-structure assignment: the Kabsch-Sander hydrogen bonds of every sample and the eight DSSP
 * classes read off their pattern.
 *
 * It consumes what prd_backbone_build writes, as it is: atoms[S][N][5][3] fp32 (N, CA, C, CB, O of row i), built[S][N] int32 (bit k set
 * when atom k of that order is present) and the caller's link[N] (fp32 0 / 1, > 0.5: rows i and i+1 are consecutive residues of one
 * chain; link[N-1] is never read as a bond).  Any all-atom structure in this layout is a valid input, not only a built one.
 *
 * A library of its own under the rules of prd_backbone.h:
 *   - extern "C", plain pointers / ints / floats only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch.  No process-wide state, no environment variable.
 *   - A call only enqueues kernels on `stream` (prd_dssp_hbonds ONE, prd_dssp_assign TWO), never synchronises, and is capturable.
 *   - Return value: 0 on success, a positive hipError_t from a launch, or a negative PRD_DSSP_ERR_*.  Every refusal happens on the host
 *     before any HIP call, launches nothing and leaves the outputs untouched.
 *   - No atomics of any kind.  Every output element has one owner and is written; two calls on the same input give equal bits.
 *
 * Arithmetic.  fp32 without fused multiply-adds (the build keeps -ffp-contract=off), in the order prd_backbone.h states: a difference
 * is p_b - p_a per coordinate, a dot product is (u0 v0 + u1 v1) + u2 v2, |v| is sqrt(v.v) and v / |v| divides each coordinate by it.
 * Square roots and divisions are the correctly rounded IEEE ones (sqrtf and 1.0f / r), no v_rsq / v_rcp approximation.
 *
 * ---- prd_dssp_hbonds ----------------------------------------------------------------------------------------------------------------
 * Residue a is an ACCEPTOR when its C and O are present.  Residue d is a DONOR (has an amide hydrogen) when its N is present, d >= 1,
 * link[d-1] is set, residue d-1 has C and O present, and donor[d] > 0.5 (donor == NULL: every residue may donate; a caller clears it
 * for proline).  The hydrogen is  H_d = N_d + (C_d-1 - O_d-1) / |C_d-1 - O_d-1|.
 * A pair (a, d) is a candidate when a is an acceptor, d is a donor, a != d, and not (a == d - 1 and link[a] set).  Its energy is
 *   E = q (((1 / r_ON + 1 / r_CH) - 1 / r_OH) - 1 / r_CN)        r_XY = |Y_d - X_a|, X of the acceptor, Y of the donor
 * If any of the four distances is below 0.5 Angstrom, E = e_min; otherwise E = max(E, e_min).  q (27.888 = 0.084 x 332 kcal/mol) and
 * e_min (-9.9) are arguments, float64 on the host rounded once to fp32.  There is NO C-alpha distance prefilter: every candidate pair
 * is evaluated (DSSP skips pairs whose C-alphas lie 9 Angstrom apart; their energies are above -0.5 anyway, but not above 0).
 * Outputs partner[S][N][4] int32 and energy[S][N][4] fp32: slots 0 and 1 hold the two lowest-energy acceptors of residue i as donor,
 * slots 2 and 3 the two lowest-energy donors of residue i as acceptor, the lower energy first.  Only candidates with E < 0 are kept;
 * equal energies go by the lower partner index; an empty slot is -1 with energy 0.  E(a, d) is one function of the same twelve
 * coordinates wherever it is evaluated, so the energy in a donor's slot and in its acceptor's slot are the same bits.
 *
 * ---- prd_dssp_assign ----------------------------------------------------------------------------------------------------------------
 * Per-residue logic on the lists above; all comparisons strict.  lk(k): 0 <= k < N-1 and link[k] set.
 *   Bond(a, d)     a is in slot 0 or 1 of d with an energy below `cutoff` (-0.5), and d is in slot 2 or 3 of a: the MUTUAL two-best
 *                  rule.  False when a or d lies outside 0 .. N-1.
 *   cont(i, n)     lk(i), ..., lk(i+n-1)
 *   Turn_n(i)      n = 3, 4, 5: cont(i, n) and Bond(i, i+n)
 *   Bridge(i, j)   |i - j| >= 3, cont(i-1, 2), cont(j-1, 2), and
 *                    parallel:      [Bond(i-1, j) and Bond(j, i+1)] or [Bond(j-1, i) and Bond(i, j+1)]
 *                    antiparallel:  [Bond(i, j) and Bond(j, i)]     or [Bond(i-1, j+1) and Bond(j-1, i+1)]
 *   bridge[S][N][2]  the two LOWEST rows j with Bridge(i, j) of either type, -1 for none, the lower first
 *   Ladder(i)      for one of the (at most two) rows j of bridge[i] and a type t of that bridge: Bridge_t(i+1, j+1) or Bridge_t(i-1, j-1)
 *                  when t is parallel, Bridge_t(i+1, j-1) or Bridge_t(i-1, j+1) when t is antiparallel
 *   Bend(r)        cont(r-2, 4), rows r-2, r and r+2 have CA present, and with u = CA_r - CA_r-2, v = CA_r+2 - CA_r
 *                  (u . v) / (|u| |v|) < cos_bend   (cos 70 degrees)
 * flags[S][N] int32, written by the first launch:
 *   bit 0, 1, 2   Turn_3(i), Turn_4(i), Turn_5(i)            PRD_DSSP_FLAG_TURN3 << (n - 3)
 *   bit 3, 4      bridge[i][0] is parallel / antiparallel    PRD_DSSP_FLAG_PAR0, PRD_DSSP_FLAG_ANTI0
 *   bit 5, 6      bridge[i][1] is parallel / antiparallel    PRD_DSSP_FLAG_PAR1, PRD_DSSP_FLAG_ANTI1
 *   bit 7         Ladder(i)                                  PRD_DSSP_FLAG_LADDER
 *   bit 8         Bend(i)                                    PRD_DSSP_FLAG_BEND
 * classes[S][N] uint8, codes 0 .. 7 in the alphabet "-HBEGITS", written by the second launch, in priority order:
 *   H  some i in [r-3, r] has Turn_4(i-1) and Turn_4(i)                          (r lies in a minimal 4-helix i .. i+3)
 *   B  bridge[r][0] >= 0 and not Ladder(r);   E  bridge[r][0] >= 0 and Ladder(r)
 *   G  some i in [r-2, r] has Turn_3(i-1) and Turn_3(i), and none of i .. i+2 is H, B or E
 *   I  some i in [r-4, r] has Turn_5(i-1) and Turn_5(i), and none of i .. i+4 is H, B, E or G
 *   T  some i and n have Turn_n(i) and i < r < i + n
 *   S  Bend(r)
 *   -  otherwise, and every row whose CA is not present.
 * Tiling.  One thread owns one residue of one sample, in tiles of PRD_DSSP_TILE = 256 rows.  The first launch stages {CA, link} of its
 * tile with a halo of PRD_DSSP_HALO = 10 rows on either side through the LDS (it reaches rows r-2 .. r+5) and follows partner rows,
 * which lie anywhere, through memory.  The second stages the flags and the bridged state of the same rows: the class of row r is a
 * function of the flags of rows r-10 .. r+6.  Nothing passes between threads within a launch, so no result depends on the tiling.
 *
 * Deviations from DSSP proper: (1) the mutual two-best rule -- DSSP takes a bond from the donor's list alone; (2) ladders are not
 * merged across beta-bulges; (3) there are no sheet labels.  Every quantity is a function of distances: a mirror image is assigned
 * exactly like the original (telling the hands apart is prd_chirality.h's business).
 *
 * Limits (else PRD_DSSP_ERR_UNSUPPORTED): N <= PRD_DSSP_MAX_N, S <= PRD_DSSP_MAX_S (a grid dimension). */
#ifndef PRD_DSSP_H
#define PRD_DSSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_DSSP_VERSION 100
#define PRD_DSSP_ERR_ARG (-1)          /* null pointer (donor excepted) / non-positive S or N / a scalar not finite / q not positive /
                                          e_min not below 0 / cutoff not below 0 / cos_bend outside (-1, 1).  e_min and cutoff reach
                                          different calls: that e_min lies below cutoff is refused by the host spec, which holds both
                                          (protein_redesign_amd/dssp.py: Dssp) */
#define PRD_DSSP_ERR_UNSUPPORTED (-3)  /* N above PRD_DSSP_MAX_N; S above PRD_DSSP_MAX_S */
#define PRD_DSSP_MAX_N 32768
#define PRD_DSSP_MAX_S 65535
#define PRD_DSSP_TILE 256
#define PRD_DSSP_HALO 10
#define PRD_DSSP_FLAG_TURN3 1
#define PRD_DSSP_FLAG_PAR0 8
#define PRD_DSSP_FLAG_ANTI0 16
#define PRD_DSSP_FLAG_PAR1 32
#define PRD_DSSP_FLAG_ANTI1 64
#define PRD_DSSP_FLAG_LADDER 128
#define PRD_DSSP_FLAG_BEND 256

int prd_dssp_version(void);

/* partner [S][N][4] int32, energy [S][N][4] fp32; atoms [S][N][5][3] fp32, built [S][N] int32, link [N] fp32, donor [N] fp32 or NULL */
int prd_dssp_hbonds(int* partner, float* energy, const float* atoms, const int* built, const float* link, const float* donor,
                    float q, float e_min, int S, int N, hipStream_t stream);

/* classes [S][N] uint8, flags [S][N] int32, bridge [S][N][2] int32; partner and energy as prd_dssp_hbonds wrote them */
int prd_dssp_assign(uint8_t* classes, int* flags, int* bridge, const int* partner, const float* energy, const float* atoms,
                    const int* built, const float* link, float cutoff, float cos_bend, int S, int N, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
