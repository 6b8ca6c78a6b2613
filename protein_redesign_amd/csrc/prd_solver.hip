// Few-step sampling on the device (include/prd_solver.h): the step boundary of a loop that visits K chosen levels, in ONE
// multi-workgroup launch.  It is step_boundary_kernel of csrc/prd_pair.hip with three tables in place of its three fixed rules:
//   the counter k[s] indexes `levels` and `coef` (there: t itself indexes the schedule),
//   the next time embedding is taken at levels[k-1] / num_steps (there: (t - 1) / num_steps),
//   the noise row is K - 1 - k (there: T - 1 - t), and the table may be absent (a deterministic solver),
// and the clean-structure estimate q (z - r eps) may be written beside the new state.  Everything else -- the sequence head's last
// layer, seq_t <- 2 softmax - 1, its LayerNorm, the next single input -- is that kernel's code, and the update is written in that
// kernel's order, so that equal tables give equal bits.
//   solver_boundary_kernel   grid b * (ceil(N / 8) + ceil(P / 4)), 256 threads.  Workgroups [0, nblk) of a sample own 8 nodes each
//                            (the work has to be wide, not deep: a workgroup is one chain of dependent L2 round trips); the masked
//                            means over all nodes are recomputed by every one of them (N x 7 loads, N x 4 without noise).  Workgroups
//                            [nblk, nblk + neb) compute four time-embedding outputs each.  The LAST workgroup to arrive at sync[0]
//                            advances the counters and writes the levels that come next, and resets sync[0] for the next replay.
// A sample whose counter is outside [0, K) is left alone by every workgroup of it: no table row is read, nothing is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_solver.h"
#include "prd_launch.h"

namespace {

constexpr int SV_NODES = 8;
constexpr int SV_CS = PRD_SOLVER_COEF_STRIDE;

// ReLU that propagates NaN (csrc/prd_common.h: relu_nan): NaN < 0 is false, the NaN stays and trips the sticky flag
__device__ __forceinline__ float sv_relu_nan(float v) { return v < 0.f ? 0.f : v; }

template <int NCLS>
__global__ __launch_bounds__(256) void solver_boundary_kernel(
    float* __restrict__ z, float* __restrict__ seq_t, int64_t* __restrict__ kcnt, int64_t* __restrict__ t,
    const float* __restrict__ eps_raw, float* __restrict__ seq_pred, const float* __restrict__ noise, const float* __restrict__ mask,
    const int64_t* __restrict__ levels, const float* __restrict__ coef,
    float* __restrict__ single_next, const float* __restrict__ stat, const float* __restrict__ rm, const float* __restrict__ w_rt,
    float* __restrict__ ebeta_next, const float* __restrict__ freqs, const float* __restrict__ w_beta, int* __restrict__ sync,
    float* __restrict__ x0_out, int b, int N, int K, int num_steps, int S, int P, int TD, int nblk, int neb,
    const float* __restrict__ seq_h, int ldh, const float* __restrict__ w_seq, int Sh) {
    constexpr int ncls = NCLS, CPL = (NCLS + 7) / 8;      // classes per lane in the 8-lanes-per-node softmax
    __shared__ float red[4][8];
    __shared__ float lg[SV_NODES][NCLS + 3];      // seq_h given: the logits of the workgroup's nodes (computed here)
    __shared__ float mean[8];
    __shared__ float xs[SV_NODES][NCLS + 3];      // LayerNorm-ed new seq_t of the workgroup's nodes
    __shared__ float feat[PRD_SOLVER_MAX_TIME_DIM];
    __shared__ int last;
    const int per = nblk + neb;
    const int bb = blockIdx.x / per, blk = blockIdx.x - bb * per;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long kk = kcnt[bb];
    const bool live = kk >= 0 && kk < K;         // uniform over the workgroup
    if (live && blk >= nblk) {                   // ---- time embedding of the NEXT step (none after the last one) ----
        if (kk > 0) {
            const float tau = (float)levels[kk - 1] / (float)num_steps;
            const int half = TD / 2;
            for (int j = tid; j < half; j += 256) {
                const float wx = freqs[j] * tau;
                feat[j] = sinf(wx);
                feat[half + j] = cosf(wx);
            }
            __syncthreads();
            const int p = (blk - nblk) * 4 + wave;   // one wave per output: coalesced reads of W_beta's row, shuffle reduction
            if (p < P) {
                float acc = 0.f;
                for (int j = lane; j < TD; j += 64) acc += feat[j] * w_beta[p * TD + j];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                if (lane == 0) ebeta_next[bb * P + p] = acc;
            }
        }
    } else if (live) {                           // ---- 8 nodes: x0, z, seq_t, and the next step's single input ----
        const int i0 = blk * SV_NODES;
        const float wn = coef[kk * SV_CS + 0], isa = coef[kk * SV_CS + 1], sb = coef[kk * SV_CS + 2];
        const float rr = coef[kk * SV_CS + 3], qq = coef[kk * SV_CS + 4];
        const bool noisy = kk > 0 && noise != nullptr;
        const float* nz = noisy ? noise + ((long)(K - 1 - kk) * b + bb) * N * 3 : nullptr;
        const float* ep = eps_raw + (long)bb * N * 3;
        {   // masked sums over ALL nodes: predicted noise (3), drawn noise (3), node count
            float s7[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (noisy) {
                for (int i = tid; i < N; i += 256) {
                    const float m = mask[bb * N + i];
                    s7[0] += m * ep[i * 3]; s7[1] += m * ep[i * 3 + 1]; s7[2] += m * ep[i * 3 + 2];
                    s7[3] += m * nz[i * 3]; s7[4] += m * nz[i * 3 + 1]; s7[5] += m * nz[i * 3 + 2];
                    s7[6] += m;
                }
            } else {
                for (int i = tid; i < N; i += 256) {
                    const float m = mask[bb * N + i];
                    s7[0] += m * ep[i * 3]; s7[1] += m * ep[i * 3 + 1]; s7[2] += m * ep[i * 3 + 2];
                    s7[6] += m;
                }
            }
#pragma unroll
            for (int d = 0; d < 7; ++d) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s7[d] += __shfl_xor(s7[d], o);
                if (lane == 0) red[wave][d] = s7[d];
            }
        }
        if (seq_h) {
            // the sequence head's LAST layer (Linear(S, 21, bias=False) on the ReLU hidden units seq_h) for the workgroup's 8 nodes:
            // 32 threads per node, 16 hidden units each per 512, shuffle reduction.  The logits are also written to seq_pred.
            const int n = tid >> 5, part = tid & 31, i = i0 + n;
            const bool ok = i < N;
            const float* hr = seq_h + ((long)bb * N + (ok ? i : 0)) * ldh;
            float acc[NCLS];
#pragma unroll
            for (int c = 0; c < NCLS; ++c) acc[c] = 0.f;
            for (int j = 4 * part; j < Sh; j += 128) {
                const float4 hv = *reinterpret_cast<const float4*>(hr + j);
#pragma unroll
                for (int c = 0; c < NCLS; ++c) {
                    const float4 wv = *reinterpret_cast<const float4*>(w_seq + (long)c * Sh + j);
                    acc[c] += (hv.x * wv.x + hv.y * wv.y) + (hv.z * wv.z + hv.w * wv.w);
                }
            }
#pragma unroll
            for (int c = 0; c < NCLS; ++c) {
#pragma unroll
                for (int o = 1; o < 32; o <<= 1) acc[c] += __shfl_xor(acc[c], o);
            }
            if (part == 0) {
#pragma unroll
                for (int c = 0; c < NCLS; ++c) {
                    lg[n][c] = acc[c];
                    if (ok) seq_pred[((long)bb * N + i) * ncls + c] = acc[c];
                }
            }
            __syncthreads();
        }
        if (tid < 8 * SV_NODES) {   // seq_t: 2 softmax - 1 and its LayerNorm; 8 lanes per node, classes l, l+8, ...
            const int n = tid >> 3, l = tid & 7, i = i0 + n;
            const bool ok = i < N;
            const float* lp = seq_h ? &lg[n][0] : seq_pred + ((long)bb * N + (ok ? i : 0)) * ncls;
            float v[CPL];
#pragma unroll
            for (int q = 0; q < CPL; ++q) v[q] = (l + 8 * q < ncls) ? lp[l + 8 * q] : -INFINITY;
            float mx = v[0];
#pragma unroll
            for (int q = 1; q < CPL; ++q) mx = fmaxf(mx, v[q]);
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
            float sum = 0.f;
#pragma unroll
            for (int q = 0; q < CPL; ++q) { v[q] = (l + 8 * q < ncls) ? expf(v[q] - mx) : 0.f; sum += v[q]; }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) sum += __shfl_xor(sum, o);
            float mu = 0.f;
#pragma unroll
            for (int q = 0; q < CPL; ++q) { v[q] = (l + 8 * q < ncls) ? v[q] / sum * 2.f - 1.f : 0.f; mu += v[q]; }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) mu += __shfl_xor(mu, o);
            mu /= ncls;
            float var = 0.f;
#pragma unroll
            for (int q = 0; q < CPL; ++q) { const float dlt = (l + 8 * q < ncls) ? v[q] - mu : 0.f; var += dlt * dlt; }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) var += __shfl_xor(var, o);
            const float rstd = 1.0f / sqrtf(var / ncls + 1e-5f);
            float* sp = seq_t + ((long)bb * N + (ok ? i : 0)) * ncls;
            bool bad = false;
#pragma unroll
            for (int q = 0; q < CPL; ++q)
                if (l + 8 * q < ncls) {
                    if (ok) sp[l + 8 * q] = v[q];
                    bad |= ok && !(fabsf(v[q]) <= 1.5f);        // 2 softmax - 1 lies in [-1, 1]: anything else is inf / NaN logits
                    xs[n][l + 8 * q] = ok ? (v[q] - mu) * rstd : 0.f;
                }
            if (bad) sync[1] = 1;
        }
        __syncthreads();
        if (tid < 7) mean[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        __syncthreads();
        if (tid >= 64 && tid < 64 + 3 * SV_NODES) {      // x0 and z of the workgroup's nodes
            const int q = tid - 64, i = i0 + q / 3, d = q - (q / 3) * 3;
            if (i < N) {
                const long g = ((long)bb * N + i) * 3 + d;
                const float m = mask[bb * N + i];
                const float npred = eps_raw[g] - m * mean[d] / mean[6];
                const float zin = z[g];
                if (x0_out) x0_out[g] = qq * (zin - rr * npred);
                float out = isa * (zin - wn * npred);
                if (noisy) out = out + sb * (nz[i * 3 + d] - m * mean[3 + d] / mean[6]);
                z[g] = out;
                if (!(fabsf(out) <= 3.0e38f)) sync[1] = 1;      // sticky: inf / NaN coordinates
            }
        }
        // single input of the next step: thread -> channels c, c + 256, ...; W_rt row in registers; the static-single / mask loads
        // of the 8 nodes are issued together
        for (int c = tid; c < S; c += 256) {
            float w[NCLS], st8[SV_NODES], rm8[SV_NODES];
#pragma unroll
            for (int u = 0; u < SV_NODES; ++u) {
                const int i = i0 + u;
                const long row = (long)bb * N + (i < N ? i : N - 1);
                st8[u] = stat[row * S + c];
                rm8[u] = rm[row];
            }
#pragma unroll
            for (int j = 0; j < NCLS; ++j) w[j] = w_rt[c * NCLS + j];
#pragma unroll
            for (int u = 0; u < SV_NODES; ++u) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < NCLS; ++j) acc += xs[u][j] * w[j];
                if (i0 + u < N) single_next[((long)bb * N + i0 + u) * S + c] = st8[u] + rm8[u] * sv_relu_nan(acc);
            }
        }
    }
    // advance the counters once every workgroup has read them
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const int arrived = atomicAdd(sync, 1);
        last = (arrived == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (last) {
        for (int s = tid; s < b; s += 256) {
            const long ks = kcnt[s];
            if (ks >= 0 && ks < K) {
                kcnt[s] = ks - 1;
                t[s] = ks > 0 ? levels[ks - 1] : -1;
            }
        }
        if (tid == 0) atomicExch(sync, 0);
    }
}

}  // namespace

extern "C" int prd_solver_version(void) { return PRD_SOLVER_VERSION; }

extern "C" int prd_solver_boundary(float* z, float* seq_t, int64_t* k, int64_t* t, const float* eps_raw, float* seq_pred,
                                   const float* noise, const float* mask, const int64_t* levels, const float* coef,
                                   float* single_next, const float* static_single, const float* residue_mask, const float* w_rt,
                                   float* ebeta_next, const float* freqs, const float* w_beta, int* sync, float* x0_out,
                                   int b, int N, int n_cls, int K, int num_steps, int S, int P, int time_dim,
                                   const float* seq_h, int ldh, const float* w_seq, int S_h, hipStream_t stream) {
    if (!z || !seq_t || !k || !t || !eps_raw || !seq_pred || !mask || !levels || !coef || !single_next || !static_single ||
        !residue_mask || !w_rt || !ebeta_next || !freqs || !w_beta || !sync || b < 1 || N < 1 || K < 1 || S < 1 || P < 1 || num_steps < 1)
        return PRD_SOLVER_ERR_ARG;
    if (n_cls != PRD_SOLVER_N_CLS || time_dim < 2 || time_dim > PRD_SOLVER_MAX_TIME_DIM || (time_dim & 1)) return PRD_SOLVER_ERR_UNSUPPORTED;
    if (b > PRD_SOLVER_MAX_B || N > PRD_SOLVER_MAX_N || K > PRD_SOLVER_MAX_K || S > PRD_SOLVER_MAX_S || P > PRD_SOLVER_MAX_P)
        return PRD_SOLVER_ERR_UNSUPPORTED;
    if (seq_h && (!w_seq || S_h < 1)) return PRD_SOLVER_ERR_ARG;
    if (seq_h && ((S_h & 3) || (ldh & 3) || ldh < S_h)) return PRD_SOLVER_ERR_ALIGN;
    // grid <= MAX_B * (MAX_N / 8 + MAX_P / 4) = 4096 * 33792 < 2^31; b * N <= 2^30 fits the kernel's int row index
    const int nblk = (N + SV_NODES - 1) / SV_NODES, neb = (P + 3) / 4;
    return prd_launch<solver_boundary_kernel<PRD_SOLVER_N_CLS>>(dim3(b * (nblk + neb)), dim3(256), 0, stream, z, seq_t, k, t, eps_raw, seq_pred,
                                                               noise, mask, levels, coef, single_next, static_single, residue_mask, w_rt,
                                                               ebeta_next, freqs, w_beta, sync, x0_out, b, N, K, num_steps, S, P, time_dim,
                                                               nblk, neb, seq_h, ldh, w_seq, S_h);
}
