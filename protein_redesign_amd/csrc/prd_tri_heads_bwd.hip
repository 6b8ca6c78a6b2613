// Backward core of the gated triangle attention for ANY head layout of 1 <= H <= 8 heads of width c (a multiple of 4, c <= 64),
// pair_dim P in {32, 64}, rows of any length: the gradient counterpart of prd_tri_heads.hip, with the contract of
// prd_tri_attn_bwd_core (prd_bwd.hip).  Given dog = d(gated head outputs) and og of the forward it writes
//     dqkvg[b, N, N, 4, H c] = d(W_q x) | d(W_k x) | d(W_v x) | d(gate pre-activation)          by pair position, channels head-major,
// with x = LN(pair) (also left in x_out for the weight gradients).  Per (row, head), with gate = sigmoid(W_g x + b_g):
//     do = dog * gate,   delta_q = sum_c dog * og,   d(gate pre) = dog * og * (1 - gate)        (og = gate * o: no division by the gate)
//     p = 2^((s - m) - log2 l),   dP = do V^T,   dS = p (dP - delta)  (0 at a replaced logit: masked_fill passes no gradient),
//     dq = dS K / sqrt(c),   dk = dS^T q,   dv = p^T do.
// The masked-logit convention is the forward's: a masked key's logit is REPLACED by -2^15 log2(e) (so a fully masked row averages V
// over all N keys and v still receives p * do), keys beyond the row are -inf.  A replaced logit is evaluated as (fill - m) - log2 l
// with the two terms apart (m + log2 l is not exact in fp32 on exactly those rows).
//
// Layout.  Persistent workgroups of 8 waves over (row, head) tasks, head h = blockIdx.x % H with the head's four weight blocks
// staged once, as in the forward.  Per row:
//   projection  every wave LayerNorms 16-position tiles of the row and projects q (scaled by log2(e) / sqrt(c)) | k | v | gate; it
//               writes q | k | v | do [Npad][CP] and delta [Npad] into the workgroup's OWN slab of the workspace (re-read at once: it stays
//               in the L2 / Infinity Cache), d(gate pre) into dqkvg and, for head 0, LN(pair) into x_out.  Positions N..Npad-1 are zeros.
//   statistics  (lse == NULL only) queries owned, keys streamed: one logits-only sweep with the online (m, l) of the forward; written
//               to the slab.  With lse given, (m, log2 l) of the forward are read instead.
//   pass A      queries owned (16 per wave, q and do in registers), keys streamed through the LDS in chunks of 64: dq.
//   pass B      keys owned (k and v in registers), queries streamed with their (m, log2 l, delta): dk, dv.
// Each output element has ONE owner that accumulates it in registers in a fixed order: no atomics, bit-reproducible from run to run.
// Nothing of size N lives in the LDS (weights + two 64-position chunks), so there is no row limit; the workspace is
// (workgroups) x Npad x (4 CP + 4) floats and nothing grows as N^3.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 throughout, in BOTH arithmetic modes (the `arith` word is validated, its split bit ignored).
// Both passes are one code path: with "owned" positions on the lanes and "streamed" positions in the registers,
//     Z1[s][o] = Y1[s] . X1[o] (the logits, Y1 = k or q),  Z2[s][o] = Y2[s] . X2[o] (dP, Y2 = v or do),
//     acc1^T[d][o] += Y1[s][d] dS[s][o] (dq or dk),  acc2^T[d][o] += Y2[s][d] p[s][o] (dv, pass B only):
// the A operands of Z are float4 row reads of the chunk [64][CP + 4], those of the accumulations column reads of the same image (both
// conflict-free at pitch CP + 4), the B operands are the owned registers / the dS, p tiles as they come out of the MFMA.
#include "prd_common.h"
#include "../../include/prd_hip.h"
#include "prd_launch.h"

namespace {

constexpr float TB_LOG2E = 1.4426950408889634f;
constexpr float TB_MASKED = -32768.0f * TB_LOG2E;       // the replaced logit in the exp2 domain
constexpr int TB_NW = 8;                                // waves per workgroup; an owned group = 128 positions (16 per wave)
constexpr int TB_SC = 64;                               // streamed positions per LDS chunk (4 tiles of 16)

template <int P, int CP>
struct TbLds {
    static constexpr int WP = P + 1;                    // weight row pitch
    static constexpr int RP = CP + 4;                   // chunk row pitch
    static constexpr int W = 0, Y1 = 4 * CP * WP, Y2 = Y1 + TB_SC * RP, SM = Y2 + TB_SC * RP, SL = SM + TB_SC, SD = SL + TB_SC,
                         KF = SD + TB_SC, FLOATS = KF + TB_SC;
};

PRD_DEV int tb_npad(int N) { return (N + TB_SC - 1) / TB_SC * TB_SC; }

// x[s] = LN(row)[g P/4 + s] (no affine, eps 1e-5) of the position this lane's 16-lane column holds; invalid positions give zeros
template <int P>
PRD_DEV void tb_load_ln(const float* __restrict__ src, bool valid, int g, float (&x)[P / 4]) {
    if (valid) {
        const float4* s4 = reinterpret_cast<const float4*>(src + g * (P / 4));
#pragma unroll
        for (int e = 0; e < P / 16; ++e) {
            const float4 v = s4[e];
            x[4 * e] = v.x; x[4 * e + 1] = v.y; x[4 * e + 2] = v.z; x[4 * e + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int s = 0; s < P / 4; ++s) x[s] = 0.f;
    }
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < P / 4; ++s) sum += x[s];
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / P);
    float v2 = 0.f;
#pragma unroll
    for (int s = 0; s < P / 4; ++s) { x[s] -= mean; v2 += x[s] * x[s]; }
    v2 += __shfl_xor(v2, 16);
    v2 += __shfl_xor(v2, 32);
    const float rstd = 1.0f / sqrtf(v2 * (1.0f / P) + 1e-5f);
#pragma unroll
    for (int s = 0; s < P / 4; ++s) x[s] *= rstd;
}

// Y^T [CP][16 positions] = W [CP][P] . LN(X)^T: tile t of the output holds channels 16 t + 4 g + r (reg r) of position i
template <int P, int CP>
PRD_DEV void tb_project(const float* Wl, const float (&x)[P / 4], f32x4 (&y)[CP / 16], int i, int g) {
#pragma unroll
    for (int t = 0; t < CP / 16; ++t) y[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < P / 4; ++s) {
#pragma unroll
        for (int t = 0; t < CP / 16; ++t) y[t] = mfma16(Wl[(16 * t + i) * TbLds<P, CP>::WP + g * (P / 4) + s], x[s], y[t]);
    }
}

// 64 positions [s0, s0 + 64) of a slab array [Npad][CP] into the LDS image [64][CP + 4]
template <int CP>
PRD_DEV void tb_stage(float* dst, const float* src, int s0, int tid) {
    constexpr int NT = TB_NW * 64, RP = CP + 4, Q = CP / 4;
    const float4* s4 = reinterpret_cast<const float4*>(src + (long)s0 * CP);
#pragma unroll
    for (int idx = tid; idx < TB_SC * Q; idx += NT) {
        const int p = idx / Q, d0 = 4 * (idx - p * Q);
        *reinterpret_cast<float4*>(dst + p * RP + d0) = s4[idx];
    }
}

// the owned registers of position `pos` of a slab array: tile t holds channels 16 t + 4 g .. + 3
template <int CP>
PRD_DEV void tb_load_owned(const float* src, int pos, int g, f32x4 (&x)[CP / 16]) {
#pragma unroll
    for (int t = 0; t < CP / 16; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(src + (long)pos * CP + 16 * t + 4 * g);
        x[t] = f32x4{v.x, v.y, v.z, v.w};
    }
}

// Z[st][r] = Y[16 st + 4 g + r] . X[lane position i], summed over the channels in the order (t, r) of the forward's logits
template <int CP>
PRD_DEV void tb_dots(const float* Yl, const f32x4 (&x)[CP / 16], f32x4 (&z)[4], int i, int g) {
    constexpr int RP = CP + 4;
#pragma unroll
    for (int st = 0; st < 4; ++st) z[st] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < CP / 16; ++t) {
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const float4 a = *reinterpret_cast<const float4*>(Yl + (16 * st + i) * RP + 16 * t + 4 * g);
            z[st] = mfma16(a.x, x[t][0], z[st]);
            z[st] = mfma16(a.y, x[t][1], z[st]);
            z[st] = mfma16(a.z, x[t][2], z[st]);
            z[st] = mfma16(a.w, x[t][3], z[st]);
        }
    }
}

// acc^T[d = 16 t + 4 g' + r'][i] += sum over the 64 streamed positions s of Y[s][d] w[s][i]
template <int CP>
PRD_DEV void tb_accumulate(const float* Yl, const f32x4 (&w)[4], f32x4 (&acc)[CP / 16], int i, int g) {
    constexpr int RP = CP + 4;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* yrow = Yl + (16 * st + 4 * g + r) * RP + i;
#pragma unroll
            for (int t = 0; t < CP / 16; ++t) acc[t] = mfma16(yrow[16 * t], w[st][r], acc[t]);
        }
    }
}

template <int P, int CP>
__global__ __launch_bounds__(TB_NW * 64) void tri_attn_heads_bwd_kernel(
    float* __restrict__ dqkvg, const float* __restrict__ dog, const float* __restrict__ og, const float* __restrict__ pair,
    const float* __restrict__ mask, const float* __restrict__ wq, const float* __restrict__ wk, const float* __restrict__ wv,
    const float* __restrict__ wg, const float* __restrict__ bg, const float* __restrict__ lse, float* __restrict__ x_out,
    float* ws, int b, int N, int H, int c, int ending) {
    using L = TbLds<P, CP>;
    constexpr int NT = TB_NW * 64, NCT = CP / 16, OG = TB_NW * 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Wk = smem + L::W;
    float* Wv = Wk + CP * L::WP;
    float* Wq = Wv + CP * L::WP;
    float* Wg = Wq + CP * L::WP;
    float* Y1 = smem + L::Y1;                  // [64][CP + 4]: k (pass A) or q (pass B) of the streamed chunk
    float* Y2 = smem + L::Y2;                  // v or do
    float* sm = smem + L::SM;                  // pass B: m, log2 l, delta of the streamed queries
    float* sl = smem + L::SL;
    float* sd = smem + L::SD;
    float* kf = smem + L::KF;                  // pass A: 1 key kept, 0 masked (logit replaced), -1 beyond the row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int h = blockIdx.x % H;
    const int rstride = gridDim.x / H;
    const int HC = H * c;
    const int npad = tb_npad(N);
    // the workgroup's slab: q | k | v | do [npad][CP], statistics [npad][2], delta [npad] (+ npad floats that keep the slabs 16-byte aligned)
    float* slab = ws + (long)blockIdx.x * npad * (4 * CP + 4);
    float* Qs = slab;
    float* Ks = Qs + (long)npad * CP;
    float* Vs = Ks + (long)npad * CP;
    float* Ds = Vs + (long)npad * CP;
    float* St = Ds + (long)npad * CP;
    float* De = St + 2 * (long)npad;

    for (int idx = tid; idx < 4 * CP * P; idx += NT) {
        const int m = idx / (CP * P), rem = idx - m * (CP * P), d = rem / P, p = rem - d * P;
        const float* W = m == 0 ? wk : m == 1 ? wv : m == 2 ? wq : wg;
        smem[m * CP * L::WP + d * L::WP + p] = d < c ? W[((long)h * c + d) * P + p] : 0.f;
    }
    const float qscale = TB_LOG2E / sqrtf((float)c);
    const float dq_scale = 1.0f / sqrtf((float)c);        // q = W_q x / sqrt(c)
    const float dk_scale = 1.0f / TB_LOG2E;               // the q of the slab carries log2(e)

    for (long bu = blockIdx.x / H; bu < (long)b * N; bu += rstride) {
        const long bb = bu / N, u = bu - bb * N;
        const float mu = mask[bu];
        const long rowbase = ending ? bb * N * N + u : bu * N;      // position of element v of the row: rowbase + v * vstep
        const long vstep = ending ? N : 1;
        const float* stats = lse ? lse + (bu * H + h) * (long)N * 2 : St;      // (m, log2 l) of query q at stats[2 q]
        __syncthreads();                       // the previous row's slab and chunks are consumed (and the weights are staged)

        // ---- projection: 16-position tiles of the row, tile = wave, wave + 8, ... ----
        for (int v0 = wave * 16; v0 < npad; v0 += OG) {
            const int v = v0 + i;
            const bool valid = v < N;
            const long pos = rowbase + (valid ? v : 0) * vstep;
            float x[P / 4];
            tb_load_ln<P>(pair + pos * P, valid, g, x);
            if (x_out != nullptr && h == 0 && valid) {
                float4* xo = reinterpret_cast<float4*>(x_out + pos * P + g * (P / 4));
#pragma unroll
                for (int e = 0; e < P / 16; ++e) xo[e] = make_float4(x[4 * e], x[4 * e + 1], x[4 * e + 2], x[4 * e + 3]);
            }
            f32x4 y[NCT];
            tb_project<P, CP>(Wq, x, y, i, g);
#pragma unroll
            for (int t = 0; t < NCT; ++t)
                *reinterpret_cast<float4*>(Qs + (long)v * CP + 16 * t + 4 * g) =
                    make_float4(y[t][0] * qscale, y[t][1] * qscale, y[t][2] * qscale, y[t][3] * qscale);
            __builtin_amdgcn_sched_barrier(0);
            tb_project<P, CP>(Wk, x, y, i, g);
#pragma unroll
            for (int t = 0; t < NCT; ++t)
                *reinterpret_cast<float4*>(Ks + (long)v * CP + 16 * t + 4 * g) = make_float4(y[t][0], y[t][1], y[t][2], y[t][3]);
            __builtin_amdgcn_sched_barrier(0);
            tb_project<P, CP>(Wv, x, y, i, g);
#pragma unroll
            for (int t = 0; t < NCT; ++t)
                *reinterpret_cast<float4*>(Vs + (long)v * CP + 16 * t + 4 * g) = make_float4(y[t][0], y[t][1], y[t][2], y[t][3]);
            __builtin_amdgcn_sched_barrier(0);
            tb_project<P, CP>(Wg, x, y, i, g);
            float dsum = 0.f;
#pragma unroll
            for (int t = 0; t < NCT; ++t) {
                const int d0 = 16 * t + 4 * g;
                float4 dov = make_float4(0.f, 0.f, 0.f, 0.f);
                if (valid && d0 < c) {
                    const float4 dg = *reinterpret_cast<const float4*>(dog + pos * HC + h * c + d0);
                    const float4 o4 = *reinterpret_cast<const float4*>(og + pos * HC + h * c + d0);
                    const float* bh = bg + h * c + d0;
                    const float g0 = sigmoidf_(y[t][0] + bh[0]), g1 = sigmoidf_(y[t][1] + bh[1]), g2 = sigmoidf_(y[t][2] + bh[2]),
                                g3 = sigmoidf_(y[t][3] + bh[3]);
                    dov = make_float4(dg.x * g0, dg.y * g1, dg.z * g2, dg.w * g3);
                    const float e0 = dg.x * o4.x, e1 = dg.y * o4.y, e2 = dg.z * o4.z, e3 = dg.w * o4.w;
                    dsum += (e0 + e1) + (e2 + e3);
                    *reinterpret_cast<float4*>(dqkvg + pos * (4 * HC) + 3 * HC + h * c + d0) =
                        make_float4(e0 * (1.0f - g0), e1 * (1.0f - g1), e2 * (1.0f - g2), e3 * (1.0f - g3));
                }
                *reinterpret_cast<float4*>(Ds + (long)v * CP + d0) = dov;
            }
            dsum += __shfl_xor(dsum, 16);
            dsum += __shfl_xor(dsum, 32);
            if (g == 0) De[v] = dsum;
        }
        __syncthreads();                       // the slab of the row is complete

        // ---- statistics (lse == NULL) and pass A: queries owned, keys streamed ----
        for (int q0 = 0; q0 < N; q0 += OG) {
            const bool active = q0 + wave * 16 < N;                  // wave-uniform: the wave owns queries of this group
            const int qi = q0 + wave * 16 + i;                       // < npad when active
            const bool qok = qi < N;
            f32x4 qv[NCT], dov[NCT], dq[NCT];
            float mq = 0.f, lq = 0.f, delta = 0.f;
            if (active) {
                tb_load_owned<CP>(Qs, qi, g, qv);
                tb_load_owned<CP>(Ds, qi, g, dov);
                delta = De[qi];
#pragma unroll
                for (int t = 0; t < NCT; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (lse == nullptr) {
                float mrun = -INFINITY, lrun = 0.f;
                for (int k0 = 0; k0 < N; k0 += TB_SC) {
                    __syncthreads();                                 // the previous chunk is consumed
                    tb_stage<CP>(Y1, Ks, k0, tid);
                    if (tid < TB_SC) {
                        const int key = k0 + tid;
                        kf[tid] = key >= N ? -1.f : (mu * mask[bb * N + key] >= 0.5f ? 1.f : 0.f);
                    }
                    __syncthreads();
                    if (!active) continue;
                    f32x4 s[4];
                    tb_dots<CP>(Y1, qv, s, i, g);
                    float mx = -INFINITY;
#pragma unroll
                    for (int st = 0; st < 4; ++st)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float f = kf[16 * st + 4 * g + r];
                            const float v = f > 0.f ? s[st][r] : (f == 0.f ? TB_MASKED : -INFINITY);
                            s[st][r] = v;
                            mx = fmaxf(mx, v);
                        }
                    mx = fmaxf(mx, __shfl_xor(mx, 16));
                    mx = fmaxf(mx, __shfl_xor(mx, 32));
                    // key 0 of the row is in the first chunk and is never -inf, so m_new is finite from the first chunk on
                    const float mnew = fmaxf(mrun, mx);
                    const float alpha = exp2f(mrun - mnew);
                    mrun = mnew;
                    float ls = 0.f;
#pragma unroll
                    for (int st = 0; st < 4; ++st)
#pragma unroll
                        for (int r = 0; r < 4; ++r) ls += exp2f(s[st][r] - mnew);
                    lrun = lrun * alpha + ls;
                }
                if (active) {
                    lrun += __shfl_xor(lrun, 16);
                    lrun += __shfl_xor(lrun, 32);
                    mq = mrun;
                    lq = log2f(lrun);
                    if (g == 0) *reinterpret_cast<float2*>(St + 2 * qi) = make_float2(mq, lq);      // pass B reads them
                }
            } else if (active && qok) {
                const float2 st2 = *reinterpret_cast<const float2*>(stats + 2 * (long)qi);
                mq = st2.x;
                lq = st2.y;
            }
            for (int k0 = 0; k0 < N; k0 += TB_SC) {
                __syncthreads();                                     // the previous chunk is consumed
                tb_stage<CP>(Y1, Ks, k0, tid);
                tb_stage<CP>(Y2, Vs, k0, tid);
                if (tid < TB_SC) {
                    const int key = k0 + tid;
                    kf[tid] = key >= N ? -1.f : (mu * mask[bb * N + key] >= 0.5f ? 1.f : 0.f);
                }
                __syncthreads();
                if (!active) continue;
                f32x4 s[4], dp[4];
                tb_dots<CP>(Y1, qv, s, i, g);
                __builtin_amdgcn_sched_barrier(0);
                tb_dots<CP>(Y2, dov, dp, i, g);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int st = 0; st < 4; ++st)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float f = kf[16 * st + 4 * g + r];
                        const float v = f > 0.f ? s[st][r] : (f == 0.f ? TB_MASKED : -INFINITY);
                        const float p = exp2f((v - mq) - lq);
                        s[st][r] = f > 0.f ? p * (dp[st][r] - delta) : 0.f;
                    }
                __builtin_amdgcn_sched_barrier(0);
                tb_accumulate<CP>(Y1, s, dq, i, g);
            }
            if (active && qok) {
                float* dst = dqkvg + (rowbase + (long)qi * vstep) * (4 * HC) + h * c;
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    const int d0 = 16 * t + 4 * g;
                    if (d0 < c)
                        *reinterpret_cast<float4*>(dst + d0) =
                            make_float4(dq[t][0] * dq_scale, dq[t][1] * dq_scale, dq[t][2] * dq_scale, dq[t][3] * dq_scale);
                }
            }
        }

        // ---- pass B: keys owned, queries streamed ----
        for (int j0 = 0; j0 < N; j0 += OG) {
            const bool active = j0 + wave * 16 < N;
            const int ki = j0 + wave * 16 + i;
            const bool kok = ki < N;
            f32x4 kv[NCT], vv[NCT], dk[NCT], dv[NCT];
            float fo = -1.f;
            if (active) {
                tb_load_owned<CP>(Ks, ki, g, kv);
                tb_load_owned<CP>(Vs, ki, g, vv);
                if (kok) fo = mu * mask[bb * N + ki] >= 0.5f ? 1.f : 0.f;
#pragma unroll
                for (int t = 0; t < NCT; ++t) { dk[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
            for (int q0 = 0; q0 < N; q0 += TB_SC) {
                __syncthreads();               // the previous chunk is consumed (first chunk: pass A's statistics are in the slab)
                tb_stage<CP>(Y1, Qs, q0, tid);
                tb_stage<CP>(Y2, Ds, q0, tid);
                if (tid < TB_SC) {
                    const int q = q0 + tid;
                    // queries beyond the row: log2 l = +inf makes p = 0 (their q and do rows are zeros as well)
                    float2 st2 = make_float2(0.f, INFINITY);
                    if (q < N) st2 = *reinterpret_cast<const float2*>(stats + 2 * (long)q);
                    sm[tid] = st2.x;
                    sl[tid] = st2.y;
                    sd[tid] = q < N ? De[q] : 0.f;
                }
                __syncthreads();
                if (!active) continue;
                f32x4 s[4], dp[4];
                tb_dots<CP>(Y1, kv, s, i, g);
                __builtin_amdgcn_sched_barrier(0);
                tb_dots<CP>(Y2, vv, dp, i, g);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    const float4 m4 = *reinterpret_cast<const float4*>(sm + 16 * st + 4 * g);
                    const float4 l4 = *reinterpret_cast<const float4*>(sl + 16 * st + 4 * g);
                    const float4 e4 = *reinterpret_cast<const float4*>(sd + 16 * st + 4 * g);
                    const float mv[4] = {m4.x, m4.y, m4.z, m4.w}, lv[4] = {l4.x, l4.y, l4.z, l4.w}, ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = fo > 0.f ? s[st][r] : (fo == 0.f ? TB_MASKED : -INFINITY);
                        const float p = exp2f((v - mv[r]) - lv[r]);
                        s[st][r] = p;
                        dp[st][r] = fo > 0.f ? p * (dp[st][r] - ev[r]) : 0.f;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                tb_accumulate<CP>(Y1, dp, dk, i, g);
                __builtin_amdgcn_sched_barrier(0);
                tb_accumulate<CP>(Y2, s, dv, i, g);
            }
            if (active && kok) {
                float* dst = dqkvg + (rowbase + (long)ki * vstep) * (4 * HC) + h * c;
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
                    const int d0 = 16 * t + 4 * g;
                    if (d0 < c) {
                        *reinterpret_cast<float4*>(dst + HC + d0) =
                            make_float4(dk[t][0] * dk_scale, dk[t][1] * dk_scale, dk[t][2] * dk_scale, dk[t][3] * dk_scale);
                        *reinterpret_cast<float4*>(dst + 2 * HC + d0) = make_float4(dv[t][0], dv[t][1], dv[t][2], dv[t][3]);
                    }
                }
            }
        }
    }
}

// workgroups of a launch: per head the smallest count that reaches the minimum number of row rounds, one workgroup per CU (as the
// forward core); the workspace query and the launch must agree on it
long tb_grid(int b, int N, int H) {
    return prd_rows_per_head((long)b * N, 256 / H) * H;
}

int tb_cp(int c) { return c <= 16 ? 16 : c <= 32 ? 32 : 64; }

template <int P, int CP>
int tb_launch(float* dqkvg, const float* dog, const float* og, const float* pair, const float* mask, const float* wq, const float* wk,
               const float* wv, const float* wg, const float* bg, const float* lse, float* x_out, float* ws, int ending, int b, int N,
               int H, int c, hipStream_t stream) {
    const size_t lds = (size_t)TbLds<P, CP>::FLOATS * sizeof(float);
    return prd_launch<tri_attn_heads_bwd_kernel<P, CP>>(dim3((unsigned)tb_grid(b, N, H)), dim3(TB_NW * 64), lds, stream,
                                                        dqkvg, dog, og, pair, mask, wq, wk, wv, wg, bg, lse, x_out, ws, b, N, H, c, ending);
}

}  // namespace

extern "C" int prd_tri_attn_bwd_heads_supported(int N, int P, int H, int c, int arith) {
    PRD_SPLIT_ARITH(arith);
    if (N <= 0) return 0;
    return (P == 32 || P == 64) && H >= 1 && H <= 8 && c >= 4 && c <= 64 && c % 4 == 0 ? 1 : 0;
}

extern "C" size_t prd_tri_attn_bwd_heads_workspace_bytes(int b, int N, int P, int H, int c) {
    if (b <= 0 || prd_tri_attn_bwd_heads_supported(N, P, H, c, PRD_ARITH_FP32) != 1) return 0;
    const size_t npad = (size_t)((N + TB_SC - 1) / TB_SC) * TB_SC;
    return (size_t)tb_grid(b, N, H) * npad * (4 * tb_cp(c) + 4) * sizeof(float);      // one slab per workgroup
}

extern "C" int prd_tri_attn_bwd_core_heads(float* dqkvg, const float* dog, const float* og, const float* pair, const float* mask,
                                           const float* wq, const float* wk, const float* wv, const float* wg, const float* bg,
                                           const float* lse, float* x_out, int ending, int b, int N, int P, int H, int c,
                                           float* ws, size_t ws_bytes, int arith, hipStream_t stream) {
    PRD_SPLIT_ARITH(arith);                    // validated; the split bit is ignored (fp32 MFMA in both modes)
    if (!dqkvg || !dog || !og || !pair || !mask || !wq || !wk || !wv || !wg || !bg || !ws || b <= 0 || N <= 0) return PRD_ERR_ARG;
    if (prd_tri_attn_bwd_heads_supported(N, P, H, c, arith) != 1) return PRD_ERR_UNSUPPORTED;
    if (ws_bytes < prd_tri_attn_bwd_heads_workspace_bytes(b, N, P, H, c)) return PRD_ERR_WORKSPACE;
    if (((uintptr_t)dqkvg | (uintptr_t)dog | (uintptr_t)og | (uintptr_t)pair | (uintptr_t)x_out | (uintptr_t)ws) & 15)
        return PRD_ERR_ALIGN;
    if ((uintptr_t)lse & 7) return PRD_ERR_ALIGN;
    const int cp = tb_cp(c);
    return PRD_FOR_P(P, PP, PRD_FOR_3(cp, CC, 16, 32, 64,
        tb_launch<PP, CC>(dqkvg, dog, og, pair, mask, wq, wk, wv, wg, bg, lse, x_out, ws, ending, b, N, H, c, stream)));
}
