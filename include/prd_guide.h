/* libprd_guide.so -- C ABI of guided sampling: distance restraints and clash repulsion evaluated on the clean-structure estimate of a
 * reverse-diffusion step, their gradient added to the predicted noise before the step's boundary (protein_redesign_amd/guidance.py).
 *
 * The step boundary (prd_step_boundary of include/prd_hip.h, prd_solver_boundary of include/prd_solver.h) evaluates
 * x0 = q (z - r eps) and moves the state along eps.  prd_guide_eps runs between the network and that boundary: it evaluates the same
 * x0, an energy E on it, and writes eps_out = eps_raw + lam dE/dx0 (capped per position) for the boundary to consume in place of
 * eps_raw.  E pushes pairs apart that are closer than a floor (a clash) and pulls pairs into a distance window (a restraint).
 *
 * It is a library of its own: nothing here is part of the denoiser ABI (include/prd_hip.h), and nothing here depends on libprd_hip.so
 * or on another library.  The rules are those of prd_solver.h / prd_condition.h:
 *   - extern "C", plain pointers / ints only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch.  No process-wide state, no environment variable.
 *   - The call only enqueues one kernel on `stream`, never synchronises, and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from the launch, or a negative PRD_GUIDE_ERR_*.  A refusal launches nothing
 *     and leaves the tensors untouched.
 *   - No floating-point atomics: every sum has a fixed order, two launches on equal inputs give equal bits.
 *
 * prd_guide_eps.  All tensors contiguous, masks 0 / 1, lengths in nanometres (the unit of the state).
 *   z        [b][N][3]  fp32   the state entering the boundary (read)
 *   eps_raw  [b][N][3]  fp32   the coordinate head's output before its masked mean is removed (read)
 *   eps_out  [b][N][3]  fp32   written; must not overlap eps_raw (other workgroups still read eps_raw)
 *   mask     [b][N]     fp32   residue_and_atom_mask
 *   counter  [b] int64         the loop's counter (the level t without a solver, the counter k with one); NULL: row 0 for every sample
 *   table    [rows][4]  fp32   per counter {q, r, lam, cap}; 16-byte aligned
 *   cls      [b][N]     int32  0 = part of no clash term, 1 = residue (C-alpha), 2 = ligand atom; any other value counts as 0
 *   floors   [3], wclash [3]  fp32   minimum distance and weight of the pair classes residue-residue, residue-ligand, ligand-ligand
 *   exclude  [b][N][N]  uint8 or NULL: non-zero = the pair takes no part in the clash term
 *   rs_ptr   [b][N+1]   int32, rs_j [R] int32, rs_par [R][4] fp32 {lo, hi, w, 0} (16-byte aligned), or all three NULL (R is then
 *                       ignored): the restraints in CSR form by owning row -- row i of sample s owns the entries
 *                       [rs_ptr[s][i], rs_ptr[s][i+1]) -- each restraint listed under BOTH of its ends.  Samples may share entries.
 *                       An entry outside [0, R) or a partner outside [0, N) is skipped, never followed.
 *   e_out    [b][N][2]  fp32 or NULL: the row's share of the clash and of the restraint energy
 * Per sample s with kk = counter[s], 0 <= kk < rows, and (q, r, lam, cap) = table[kk]:
 *   eps   = eps_raw - mask * (masked mean of eps_raw over the sample)     summed in the order the boundary sums it
 *   x     = q * (z - r * eps)                                              the boundary's own x0, centred
 *   d_ij  = |x_i - x_j|;  a pair with d_ij^2 < 1e-12 contributes nothing to any term
 *   E_clash     = sum over i < j, both classes non-zero, both masks 1, not excluded, c the pair class:
 *                 wclash[c] / 2 * max(0, floors[c] - d_ij)^2
 *   E_restraint = sum over restraints:  w / 2 * ( max(0, d_ij - hi)^2 + max(0, lo - d_ij)^2 )
 *   g_i   = dE / dx_i;   delta_i = lam * g_i;   if |delta_i| > cap: delta_i *= cap / |delta_i|
 *   eps_out_i = eps_raw_i + mask_i * delta_i      (the mean is NOT removed here: the boundary does that);  lam == 0: eps_raw_i itself
 *   e_out[i]  = half of every pair term row i takes part in, so that the sum over the rows is E
 * A sample with kk < 0 or kk >= rows is left alone: no table row is read, nothing of it is written.
 * With lam == 0 and e_out == NULL no pair is visited: the launch is a copy. */
#ifndef PRD_GUIDE_H
#define PRD_GUIDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_GUIDE_VERSION 100
#define PRD_GUIDE_ERR_ARG (-1)          /* a required pointer NULL; b, N or rows below 1; eps_out overlapping eps_raw; one or two of
                                           rs_ptr, rs_j, rs_par NULL; all three given and R below 1 */
#define PRD_GUIDE_ERR_ALIGN (-2)        /* table or rs_par not 16-byte aligned */
#define PRD_GUIDE_ERR_UNSUPPORTED (-3)  /* b, N, rows or R above their PRD_GUIDE_MAX_* */
#define PRD_GUIDE_MAX_B 4096
#define PRD_GUIDE_MAX_N 8192
#define PRD_GUIDE_MAX_R 1048576         /* entries of rs_j: twice the number of distinct restraints */
#define PRD_GUIDE_MAX_ROWS 1048576
#define PRD_GUIDE_TABLE_STRIDE 4

int prd_guide_version(void);

int prd_guide_eps(const float* z, const float* eps_raw, float* eps_out, const float* mask, const int64_t* counter, const float* table,
                  const int* cls, const float* floors, const float* wclash, const uint8_t* exclude, const int* rs_ptr, const int* rs_j,
                  const float* rs_par, float* e_out, int b, int N, int rows, int R, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
