/* libprd_multistep.so -- C ABI of multistep few-step sampling: the higher-order correction of a reverse-diffusion step and the history
 * of clean-structure estimates it needs (second and third order in the log-SNR variable, DPM-Solver++ 2M and its relatives;
 * protein_redesign_amd/solver.py).
 *
 * prd_solver_boundary (include/prd_solver.h) takes the first-order step z <- a (z - w eps) and writes the step's clean-structure
 * estimate x0.  prd_multistep_correct runs AFTER it, on the counter as the boundary left it: it adds to z the gains of the step times
 * the differences between x0 and the estimates of the previous one or two steps, then pushes x0 onto that history.  The boundary, its
 * header and its version stay what they are; a loop of order 1 never calls this library.
 *
 * It is a library of its own: nothing here is part of the denoiser ABI (include/prd_hip.h), and nothing here depends on libprd_hip.so
 * or on another library.  The rules are those of prd_solver.h / prd_guide.h:
 *   - extern "C", plain pointers / ints only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch.  No process-wide state, no environment variable.
 *   - The call only enqueues one kernel on `stream`, never synchronises, and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from the launch, or a negative PRD_MULTISTEP_ERR_*.  A refusal launches nothing
 *     and leaves the tensors untouched.
 *   - Every element is read and written by one thread: no dependence between workgroups, no arrival counter, no atomic; two launches
 *     on equal inputs give equal bits.
 *
 * prd_multistep_correct.  All tensors contiguous.
 *   z      [b][N][3]     fp32   the state the boundary has just written (first order), corrected in place
 *   x0     [b][N][3]     fp32   the boundary's x0_out: the clean-structure estimate of the step that has just run (read)
 *   hist   [2][b][N][3]  fp32   slot 0: the estimate of the previous step, slot 1: of the step before it; read and written
 *   k      [b] int64            per sample the counter as the boundary LEFT it (read)
 *   first  [b] int64            per sample the counter of the first step run since the history was last dropped (the loop's reset() /
 *                               restart()); written by the host, only read here
 *   gain   [K][4]        fp32   per counter {g | one history entry, g1 | two entries, g2 | two entries, 0}; 16-byte aligned
 * Per sample s with cur = k[s] + 1, the counter of the step that has just run, 1 <= cur <= K - 1, and n = min(first[s] - cur, 2) >= 0
 * the history entries that exist; elementwise, every product and sum rounded on its own, in this order:
 *   n == 1:  z += gain[cur][0] * (x0 - hist0)
 *   n == 2:  z += gain[cur][1] * (x0 - hist0) + gain[cur][2] * (x0 - hist1)
 *   always:  hist1 <- hist0;  hist0 <- x0
 * With n == 0 no row of gain is read.  A sample with cur < 1, cur > K - 1 or first[s] < cur is left alone: nothing of it is read from
 * gain, nothing of it is written.  That covers a finished sample (k = -1: its last step is first order by construction, and its
 * history is not needed again) and a counter outside the table. */
#ifndef PRD_MULTISTEP_H
#define PRD_MULTISTEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_MULTISTEP_VERSION 100
#define PRD_MULTISTEP_ERR_ARG (-1)          /* a pointer NULL; b, N or K below 1 */
#define PRD_MULTISTEP_ERR_ALIGN (-2)        /* gain not 16-byte aligned */
#define PRD_MULTISTEP_ERR_UNSUPPORTED (-3)  /* b, N or K above their PRD_MULTISTEP_MAX_* (the values of prd_solver.h) */
#define PRD_MULTISTEP_MAX_B 4096
#define PRD_MULTISTEP_MAX_N 262144
#define PRD_MULTISTEP_MAX_K 1048576
#define PRD_MULTISTEP_GAIN_STRIDE 4

int prd_multistep_version(void);

int prd_multistep_correct(float* z, const float* x0, float* hist, const int64_t* k, const int64_t* first, const float* gain,
                          int b, int N, int K, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
