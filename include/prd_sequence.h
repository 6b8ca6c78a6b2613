/* libprd_sequence.so -- C ABI of the sequence rules of sampling: which residue classes a row of the sequence state may take, an additive
 * bias on its logits, the decoding of the final logits on the device, and the census of the decoded sequences.
 *
 * The reverse-diffusion loop (include/prd_hip.h: prd_step_boundary / prd_reverse_update) feeds seq_t = 2 softmax(seq_pred) - 1 back
 * over all n_cls classes at every position.  A loop with sequence rules rewrites, after every boundary, the rows it rules: the softmax
 * is retaken over the ALLOWED classes of logits + bias, a banned class is told to the network as -1.  The same rule decodes the final
 * logits (argmax, or a Gumbel-max draw at a temperature), and one more call counts what the decoded samples share.
 *
 * It is a library of its own: nothing here is part of the denoiser ABI (include/prd_hip.h), and nothing here depends on libprd_hip.so
 * or on another side library.  The rules of the boundary are those of prd_condition.h:
 *   - extern "C", plain pointers / ints / floats only.  All pointers are DEVICE pointers owned by the caller.
 *   - The library never allocates device memory and needs no scratch.  No process-wide state, no environment variable.
 *   - A call only enqueues one kernel on `stream`, never synchronises, and is capturable into a hipGraph.
 *   - Return value: 0 on success, a positive hipError_t from the launch, or a negative PRD_SEQUENCE_ERR_*.  A refusal launches nothing
 *     and leaves the tensors untouched.
 *
 * THE BAN RULE.  All float tensors are fp32 and contiguous.  bias is [bias_b][N][n_cls] with bias_b == 1 (one table for every sample)
 * or bias_b == the number of samples; bias == NULL: no bias and no ban (bias_b is then not looked at).  In a ruled row an entry with
 * bias <= PRD_SEQUENCE_BANNED is BANNED: it is left out of every maximum and every sum, whatever its logit -- a test on the bias, not
 * arithmetic with a large negative number.  Every other entry has x = logits + bias, ONE fp32 addition, rounded.  Rows are marked
 * in a [samples][N] tensor of 0 / 1, tested as >= 0.5.
 *
 * prd_sequence_constrain.  seq_t [b][N][n_cls] updated in place; logits [b][N][n_cls] read only; rows [b][N].  For a marked row, with m
 *   the maximum of x over the allowed entries:  p = exp(x - m) / sum over the allowed entries of exp(x - m);  seq_t = 2 p - 1 (the
 *   product exact, one rounded subtraction); a banned entry has p = 0 and seq_t = -1.0f exactly.  A row with every class banned gives
 *   seq_t = -1 throughout, no NaN.  Unmarked rows, and everything outside seq_t, are not written.  rows == NULL: a successful no-op.
 *
 * prd_sequence_decode.  tokens [S][N] int32, logp [S][N], entropy [S][N] written for EVERY row; logits [S][N][n_cls], rows [S][N] (not
 *   NULL), gumbel [S][N][n_cls] or NULL.  For a marked row: token = the lowest index that maximises x (gumbel == NULL) or
 *   inv_temperature * x + gumbel (one rounded product, one rounded sum) over the allowed entries; logp = log_softmax(x)[token] over the
 *   allowed entries, at temperature 1; entropy = - sum p log p in nats over the allowed entries (0 log 0 = 0).  Unmarked rows, and a
 *   row with every class banned: token -1, logp 0, entropy 0.
 *
 * prd_sequence_census.  tokens [S][N] int32, ref_tokens [N] int32 or NULL, mask [N] (not NULL).  All outputs int32 counts, every
 *   element of them written by the call (the caller need not zero them), no atomics: deterministic.  A token < 0 never matches.
 *   identity [S][S]   the positions i with mask[i] >= 0.5 at which tokens[s][i] == tokens[r][i] >= 0
 *   recovery [S]      those at which tokens[s][i] == ref_tokens[i] >= 0; NULL together with ref_tokens (one without the other: ERR_ARG)
 *   profile [N][n_cls] the samples with tokens[s][i] == c, 0 where mask[i] < 0.5
 *   No [S][S][N] temporary: one wave per pair of samples walks the row. */
#ifndef PRD_SEQUENCE_H
#define PRD_SEQUENCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define PRD_SEQUENCE_VERSION 100
#define PRD_SEQUENCE_ERR_ARG (-1)          /* a count below 1; a required tensor NULL; bias given with bias_b neither 1 nor the number of
                                              samples; recovery without ref_tokens or the reverse */
#define PRD_SEQUENCE_ERR_UNSUPPORTED (-3)  /* n_cls != PRD_SEQUENCE_N_CLS; b above PRD_SEQUENCE_MAX_B; S above PRD_SEQUENCE_MAX_S; N above
                                              PRD_SEQUENCE_MAX_N */
#define PRD_SEQUENCE_N_CLS 21
#define PRD_SEQUENCE_BANNED (-32768.0f)    /* a bias at or below this bans the class: the reference's own mask fill */
#define PRD_SEQUENCE_MAX_B 65535
#define PRD_SEQUENCE_MAX_N 16777216
#define PRD_SEQUENCE_MAX_S 4096

int prd_sequence_version(void);

int prd_sequence_constrain(float* seq_t, const float* logits, const float* bias, const float* rows,
                           int b, int N, int n_cls, int bias_b, hipStream_t stream);

int prd_sequence_decode(int32_t* tokens, float* logp, float* entropy,
                        const float* logits, const float* bias, const float* rows, const float* gumbel, float inv_temperature,
                        int S, int N, int n_cls, int bias_b, hipStream_t stream);

int prd_sequence_census(int32_t* identity, int32_t* recovery, int32_t* profile,
                        const int32_t* tokens, const int32_t* ref_tokens, const float* mask,
                        int S, int N, int n_cls, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
