/* libprd_condition.so -- C ABI of structure-conditioned sampling: the rows of the reverse-diffusion state that are held to an input
 * structure (replacement conditioning) and the rows of the sequence state that are held to the known sequence.
 *
 * The reverse-diffusion loop (include/prd_hip.h: prd_step_boundary / prd_reverse_update) advances every row of z [b][N][3] and
 * seq_t [b][N][n_cls].  A conditioned loop overwrites, after every boundary, the rows it keeps: a kept coordinate row is the input
 * structure noised to the level of the step that comes next (the forward process q of training, with noise of its own per level), and
 * the input structure itself once the counter has run out; a kept sequence row is the known one-hot row.  One kernel does both, for the
 * initial state and for every step; it reads the device-resident step counter, so it sits in the captured graph of a step.
 *
 * It is a library of its own: nothing here is part of the denoiser ABI (include/prd_hip.h), and nothing here depends on libprd_hip.so
 * or on another side library.  The rules of the boundary are those of prd_align.h:
 *   - extern "C", plain pointers / ints only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch.  No process-wide state, no environment variable.
 *   - The call only enqueues one kernel on `stream`, never synchronises, and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from the launch, or a negative PRD_CONDITION_ERR_*.  A refusal launches nothing
 *     and leaves the tensors untouched.
 *
 * prd_condition_rows.  All tensors fp32 and contiguous, masks 0 / 1 (m >= 0.5: set); t [b] int64.
 *   z        [b][N][3]            the coordinate state, updated in place
 *   seq_t    [b][N][n_cls]        the sequence state, updated in place
 *   t        [b]                  per sample the counter l of the step that comes NEXT (what prd_step_boundary leaves behind); samples
 *                                 of a batch may differ
 *   x0c      [b][N][3]            the centred input structure
 *   keep_z   [b][N]               rows of z that are kept, or NULL: z is not touched
 *   noise    [levels][b][N][3]    conditioning noise, indexed by level
 *   level    [>= levels][2]       (sqrt(abar_l), sqrt(1 - abar_l)) per level
 *   seq0     [b][N][n_cls]        the known sequence rows
 *   keep_seq [b][N]               rows of seq_t that are kept, or NULL: seq_t is not touched (seq_t and seq0 may then be NULL too)
 * Rows with keep_z[s][i] >= 0.5, with l = t[s]:
 *   l < 0             z[s][i][c] = x0c[s][i][c]
 *   0 <= l < levels   z[s][i][c] = level[2 l] * x0c[s][i][c] + level[2 l + 1] * noise[l][s][i][c]
 *                     -- two fp32 products, each rounded on its own, then one fp32 sum: no fused multiply-add
 *   l >= levels       nothing is written for sample s; the tables are never read out of range
 * Rows with keep_seq[s][i] >= 0.5: seq_t[s][i][:] = seq0[s][i][:], whatever l.
 * No other row, and nothing outside the tensors, is written.  With both masks NULL the call is a successful no-op. */
#ifndef PRD_CONDITION_H
#define PRD_CONDITION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_CONDITION_VERSION 100
#define PRD_CONDITION_ERR_ARG (-1)          /* b or N below 1; levels below 1; t NULL; a tensor NULL that the given masks need */
#define PRD_CONDITION_ERR_UNSUPPORTED (-3)  /* keep_seq given and n_cls != PRD_CONDITION_N_CLS; b above PRD_CONDITION_MAX_B; N above
                                               PRD_CONDITION_MAX_N */
#define PRD_CONDITION_N_CLS 21
#define PRD_CONDITION_MAX_B 65535
#define PRD_CONDITION_MAX_N 16777216

int prd_condition_version(void);

int prd_condition_rows(float* z, float* seq_t, const int64_t* t,
                       const float* x0c, const float* keep_z, const float* noise, const float* level,
                       const float* seq0, const float* keep_seq,
                       int b, int N, int n_cls, int levels, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
