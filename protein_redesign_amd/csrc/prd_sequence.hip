// Sequence rules of sampling on the device (include/prd_sequence.h): the ruled rows of the sequence state retaken as a softmax over the
// allowed classes, the final logits decoded under the same rule, and the census of the decoded samples.
//   constrain_kernel / decode_kernel   grid (row tiles, samples), 256 threads = 8 lane groups of 32, one group per row of 21 classes: lane c
//                            of a group owns class c (lanes 21 .. 31 take part in the butterflies with neutral values).  The lanes of a
//                            group read consecutive floats and the next group's row starts where this one's ends, so every load and
//                            store coalesces.  Maximum, sum and argmax are xor butterflies inside the group (__shfl_xor, width 32): a
//                            fixed order, so two launches give the same bits.  A group leaves as a whole (row past N, row unmarked), so no
//                            butterfly reads a lane that is gone.
//   census_kernel            one wave per block.  The first S (S + 1) blocks: the pair (s, r) of samples, r == S being the reference
//                            sequence; the lanes stride over the row, one butterfly, lane 0 writes the count.  The blocks after them:
//                            the profile, one thread per (position, class), a loop over the samples.  Every output element has
//                            exactly one writer, so nothing is zeroed first.
// No LDS, no scratch, no atomics.  A row is 84 bytes: the launches are latency, not bandwidth.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/prd_sequence.h"
#include "prd_launch.h"

namespace {

constexpr int Q_THREADS = 256;
constexpr int Q_GROUP = 32;                                     // lanes per row; n_cls == 21 <= 32 is checked on the host
constexpr int Q_ROWS = Q_THREADS / Q_GROUP;
constexpr int Q_WAVE = 64;

__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int m = Q_GROUP / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, Q_GROUP));
    return v;
}

__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = Q_GROUP / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, Q_GROUP);
    return v;
}

// x = logits + bias of this lane's class and whether the class takes part (false: banned, or a lane past n_cls)
__device__ __forceinline__ bool ruled_entry(const float* __restrict__ logits, const float* __restrict__ bias, size_t at, size_t bias_at,
                                            int c, int n_cls, float& x) {
    x = 0.0f;
    if (c >= n_cls) return false;
    float bv = 0.0f;
    if (bias) {
        bv = bias[bias_at];
        if (bv <= PRD_SEQUENCE_BANNED) return false;
    }
    x = logits[at] + bv;
    return true;
}

__global__ __launch_bounds__(Q_THREADS) void constrain_kernel(float* __restrict__ seq_t, const float* __restrict__ logits,
                                                             const float* __restrict__ bias, const float* __restrict__ rows, int N,
                                                             int n_cls, int bias_b) {
    const int s = blockIdx.y;
    const int i = blockIdx.x * Q_ROWS + threadIdx.x / Q_GROUP;  // < 2^31: N <= PRD_SEQUENCE_MAX_N, checked on the host
    const int c = threadIdx.x % Q_GROUP;
    if (i >= N) return;                                         // the whole group
    if (!(rows[(size_t)s * N + i] >= 0.5f)) return;             // the whole group
    const size_t at = ((size_t)s * N + i) * n_cls + c;
    const size_t bias_at = ((size_t)(bias_b == 1 ? 0 : s) * N + i) * n_cls + c;
    float x;
    const bool on = ruled_entry(logits, bias, at, bias_at, c, n_cls, x);
    const float m = group_max(on ? x : -INFINITY);
    const float e = on ? expf(x - m) : 0.0f;
    const float sum = group_sum(e);
    if (c >= n_cls) return;
    float out = -1.0f;
    if (on) {
        const float p = e / sum;                                // an allowed entry exists, the one at the maximum has e == 1: sum >= 1
        out = 2.0f * p - 1.0f;
    }
    seq_t[at] = out;
}

__global__ __launch_bounds__(Q_THREADS) void decode_kernel(int32_t* __restrict__ tokens, float* __restrict__ logp, float* __restrict__ entropy,
                                                          const float* __restrict__ logits, const float* __restrict__ bias,
                                                          const float* __restrict__ rows, const float* __restrict__ gumbel,
                                                          float inv_temperature, int N, int n_cls, int bias_b) {
    const int s = blockIdx.y;
    const int i = blockIdx.x * Q_ROWS + threadIdx.x / Q_GROUP;
    const int c = threadIdx.x % Q_GROUP;
    if (i >= N) return;                                         // the whole group
    const size_t row = (size_t)s * N + i;
    if (!(rows[row] >= 0.5f)) {                                 // the whole group
        if (c == 0) {
            tokens[row] = -1;
            logp[row] = 0.0f;
            entropy[row] = 0.0f;
        }
        return;
    }
    const size_t at = row * n_cls + c;
    const size_t bias_at = ((size_t)(bias_b == 1 ? 0 : s) * N + i) * n_cls + c;
    float x;
    const bool on = ruled_entry(logits, bias, at, bias_at, c, n_cls, x);
    // the key that is maximised, the lowest index winning a tie; a lane that takes no part loses to every lane that does
    float key = -INFINITY;
    int idx = Q_GROUP + c;
    if (on) {
        key = x;
        if (gumbel) {
            const float scaled = inv_temperature * x;           // -ffp-contract=off: a rounded product, then a rounded sum
            key = scaled + gumbel[at];
        }
        idx = c;
    }
#pragma unroll
    for (int m = Q_GROUP / 2; m >= 1; m >>= 1) {
        const float ok = __shfl_xor(key, m, Q_GROUP);
        const int oi = __shfl_xor(idx, m, Q_GROUP);
        if (ok > key || (ok == key && oi < idx)) {
            key = ok;
            idx = oi;
        }
    }
    const float mx = group_max(on ? x : -INFINITY);
    const float d = x - mx;
    const float e = on ? expf(d) : 0.0f;
    const float sum = group_sum(e);
    const float wsum = group_sum(e > 0.0f ? e * d : 0.0f);      // sum of e (x - m): 0 log 0 = 0
    const bool any = idx < Q_GROUP;                             // false: every class banned
    const float x_tok = __shfl(x, any ? idx : 0, Q_GROUP);
    if (c == 0) {
        float lp = 0.0f, h = 0.0f;
        if (any) {
            const float ls = logf(sum);
            lp = (x_tok - mx) - ls;
            h = ls - wsum / sum;
        }
        tokens[row] = any ? idx : -1;
        logp[row] = lp;
        entropy[row] = h;
    }
}

__global__ __launch_bounds__(Q_WAVE) void census_kernel(int32_t* __restrict__ identity, int32_t* __restrict__ recovery,
                                                       int32_t* __restrict__ profile, const int32_t* __restrict__ tokens,
                                                       const int32_t* __restrict__ ref_tokens, const float* __restrict__ mask, int S, int N,
                                                       int n_cls, int pairs) {
    const int others = S + (ref_tokens ? 1 : 0);                // samples, then the reference sequence if there is one
    if ((int)blockIdx.x >= pairs) {                             // the profile: one thread per (position, class)
        const int e = (blockIdx.x - pairs) * Q_WAVE + threadIdx.x;      // < 2^31: N * 21 <= 21 * 2^24
        if (e >= N * n_cls) return;
        const int i = e / n_cls, c = e % n_cls;
        int n = 0;
        if (mask[i] >= 0.5f)
            for (int s = 0; s < S; ++s) n += tokens[(size_t)s * N + i] == c ? 1 : 0;
        profile[e] = n;
        return;
    }
    const int s = blockIdx.x / others, r = blockIdx.x % others;
    const int32_t* a = tokens + (size_t)s * N;
    const int32_t* o = r < S ? tokens + (size_t)r * N : ref_tokens;
    int n = 0;
    for (int i = threadIdx.x; i < N; i += Q_WAVE) {
        const int32_t t = a[i];
        n += (mask[i] >= 0.5f && t >= 0 && t == o[i]) ? 1 : 0;
    }
#pragma unroll
    for (int m = Q_WAVE / 2; m >= 1; m >>= 1) n += __shfl_xor(n, m, Q_WAVE);
    if (threadIdx.x == 0) {
        if (r < S) identity[(size_t)s * S + r] = n;
        else recovery[s] = n;
    }
}

int refuse(int samples, int max_samples, int N, int n_cls) {
    if (samples < 1 || N < 1) return PRD_SEQUENCE_ERR_ARG;
    if (n_cls != PRD_SEQUENCE_N_CLS) return PRD_SEQUENCE_ERR_UNSUPPORTED;
    if (samples > max_samples || N > PRD_SEQUENCE_MAX_N) return PRD_SEQUENCE_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int prd_sequence_version(void) { return PRD_SEQUENCE_VERSION; }

extern "C" int prd_sequence_constrain(float* seq_t, const float* logits, const float* bias, const float* rows, int b, int N, int n_cls,
                                      int bias_b, hipStream_t stream) {
    if (const int r = refuse(b, PRD_SEQUENCE_MAX_B, N, n_cls)) return r;
    if (bias && bias_b != 1 && bias_b != b) return PRD_SEQUENCE_ERR_ARG;
    if (!rows) return 0;
    if (!seq_t || !logits) return PRD_SEQUENCE_ERR_ARG;
    return prd_launch<constrain_kernel>(dim3((N + Q_ROWS - 1) / Q_ROWS, b), dim3(Q_THREADS), 0, stream, seq_t, logits, bias, rows, N, n_cls, bias_b);
}

extern "C" int prd_sequence_decode(int32_t* tokens, float* logp, float* entropy, const float* logits, const float* bias, const float* rows,
                                   const float* gumbel, float inv_temperature, int S, int N, int n_cls, int bias_b, hipStream_t stream) {
    if (const int r = refuse(S, PRD_SEQUENCE_MAX_S, N, n_cls)) return r;
    if (bias && bias_b != 1 && bias_b != S) return PRD_SEQUENCE_ERR_ARG;
    if (!tokens || !logp || !entropy || !logits || !rows) return PRD_SEQUENCE_ERR_ARG;
    return prd_launch<decode_kernel>(dim3((N + Q_ROWS - 1) / Q_ROWS, S), dim3(Q_THREADS), 0, stream, tokens, logp, entropy, logits, bias, rows,
                                     gumbel, inv_temperature, N, n_cls, bias_b);
}

extern "C" int prd_sequence_census(int32_t* identity, int32_t* recovery, int32_t* profile, const int32_t* tokens, const int32_t* ref_tokens,
                                   const float* mask, int S, int N, int n_cls, hipStream_t stream) {
    if (const int r = refuse(S, PRD_SEQUENCE_MAX_S, N, n_cls)) return r;
    if (!identity || !profile || !tokens || !mask) return PRD_SEQUENCE_ERR_ARG;
    if ((recovery == nullptr) != (ref_tokens == nullptr)) return PRD_SEQUENCE_ERR_ARG;
    const int pairs = S * (S + (ref_tokens ? 1 : 0));             // <= 4096 * 4097; with the profile's blocks below 2^31
    const int blocks = pairs + (N * n_cls + Q_WAVE - 1) / Q_WAVE;
    return prd_launch<census_kernel>(dim3(blocks), dim3(Q_WAVE), 0, stream, identity, recovery, profile, tokens, ref_tokens, mask, S, N, n_cls, pairs);
}
