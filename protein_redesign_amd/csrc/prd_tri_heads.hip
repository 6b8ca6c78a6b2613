// Gated triangle-attention core for ANY head layout of 1 <= H <= 8 heads of width c (a multiple of 4, c <= 64), pair_dim P in
// {32, 64}, rows of any length, in ONE launch (modules.py:185-225 via 236-243):
//     og[b, i, j, h c + d] = sigmoid(LN(x_j) Wg_h^T + bg_h)_d * sum_k softmax_k(s_jk) (LN(x_k) Wv_h^T)_d,
//     s_jk = (LN(x_j) Wq_h^T / sqrt(c)) . (LN(x_k) Wk_h^T), replaced by -2^15 where mask[b, i] mask[b, k] < 0.5 (masked_fill),
// with x = pair[b, i, :, :] ("starting") or pair[b, :, i, :] ("ending"); og is written in the pair's own (i, j) layout in both
// orientations, [b, N, N, H c], so the output projection is a plain row GEMM.  The tuned 4 x 16 kernels (prd_tri.hip,
// prd_tri2.hip) stay the model's path for that layout; this one serves every other layout.
//
// Layout.  Persistent workgroups of 8 waves over (row, head) tasks: head h = blockIdx.x % H, so a workgroup stages Wk | Wv | Wq | Wg of
// ONE head (4 c P floats, rows c..CP-1 zero) once and walks its rows.  The head width is padded to a compile-time CP in {16, 32, 64}
// (c = 20 runs on the 32-wide instance; the zero rows make the padded channels of Q, K and V exactly 0).  Per row the queries are
// taken in groups of 256 (8 waves x 2 blocks of 16); per group the keys stream through the LDS in chunks of 64: the workgroup
// LayerNorms and projects K^T and V of the chunk, then every wave runs its two query blocks over it with a running (m, l, acc) in
// registers -- the online softmax, so no row limit and no statistics outside the registers.  Rows longer than one query group
// re-project the chunks per group (the projection is P / 128 of the attention's MFMA work).
//
// Arithmetic: fp32-input MFMA (v_mfma_f32_16x16x4_f32) for the projections, S^T = K Q^T and O^T = V^T P^T, fp32 softmax with
// log2(e) / sqrt(c) folded into Q and exp2.  Exact fp32 products in BOTH arithmetic modes: the entry takes the `arith` word for the
// uniform ABI and ignores its split bit (no fp16 operands, so no operand-range guard either).
//
// Register layouts (16x16x4: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[4 (lane >> 4) + r][lane & 15]):
//   positions  lane (i, g) holds x[position i][g P/4 .. g P/4 + P/4) (one float4 row segment per load); k-step s of a projection pairs
//              it with W[d][g P/4 + s], so the projections come out TRANSPOSED: Y^T[d = 16 t + 4 g + r][position i] in reg r of tile t.
//   logits     S^T[key = 16 kt + 4 g + r][query i]: k-step (t, r) reads K^T[16 t + 4 g + r][key] against Q^T's register (t, r).
//   P V        the exp'ed logits are, unchanged, the B operand of O^T = V^T P^T (k-step (kt, r) = keys 16 kt + 4 g + r); O^T and the gate
//              share the layout Y^T, so the epilogue is elementwise and stores float4s of 4 channels.
#include "prd_common.h"
#include "../../include/prd_hip.h"
#include "prd_launch.h"

namespace {

constexpr float TH_LOG2E = 1.4426950408889634f;
constexpr int TH_NW = 8;                       // waves per workgroup
constexpr int TH_QB = 2;                       // query blocks of 16 per wave: a query group = 256 queries
constexpr int TH_KC = 64;                      // keys per LDS chunk (4 tiles of 16)
constexpr int TH_KTP = TH_KC + 4;              // pitch of K^T [CP][keys]: conflict-free reads (16 g + i banks)

template <int P, int CP>
struct ThLds {
    static constexpr int WP = P + 1;           // weight row pitch
    static constexpr int VP = CP + 4;          // pitch of V [keys][CP]: conflict-free reads
    static constexpr int W = 0, KT = 4 * CP * WP, V = KT + CP * TH_KTP, KF = V + TH_KC * VP, FLOATS = KF + TH_KC;
};

template <int P, int CP>
size_t th_lds_bytes() { return (size_t)ThLds<P, CP>::FLOATS * sizeof(float); }

// x[s] = LN(row)[g P/4 + s] (no affine, eps 1e-5) of the position this lane's 16-lane column holds; invalid positions give zeros
template <int P>
PRD_DEV void th_load_ln(const float* __restrict__ src, bool valid, int g, float (&x)[P / 4]) {
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
PRD_DEV void th_project(const float* Wl, const float (&x)[P / 4], f32x4 (&y)[CP / 16], int i, int g) {
#pragma unroll
    for (int t = 0; t < CP / 16; ++t) y[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < P / 4; ++s) {
#pragma unroll
        for (int t = 0; t < CP / 16; ++t) y[t] = mfma16(Wl[(16 * t + i) * ThLds<P, CP>::WP + g * (P / 4) + s], x[s], y[t]);
    }
}

// LSE: the running (m, log2 l) of every query, which sit in registers at the end of a query group, are also stored to
// lse [b*N rows][H][N][2] for the backward core (prd_tri_heads_bwd.hip); a compile-time flag, so the plain instance is unchanged
template <int P, int CP, bool LSE>
__global__ __launch_bounds__(TH_NW * 64) void tri_attn_heads_kernel(
    float* __restrict__ og, float* __restrict__ lse, const float* __restrict__ pair, const float* __restrict__ mask,
    const float* __restrict__ wq, const float* __restrict__ wk, const float* __restrict__ wv,
    const float* __restrict__ wg, const float* __restrict__ bg, int b, int N, int H, int c, int ending) {
    using L = ThLds<P, CP>;
    constexpr int NT = TH_NW * 64, NCT = CP / 16;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Wk = smem + L::W;
    float* Wv = Wk + CP * L::WP;
    float* Wq = Wv + CP * L::WP;
    float* Wg = Wq + CP * L::WP;
    float* Kt = smem + L::KT;                  // [CP][TH_KTP]: K^T of the chunk
    float* Vl = smem + L::V;                   // [TH_KC][VP]
    float* kf = smem + L::KF;                  // [TH_KC]: 1 key kept, 0 masked (logit replaced by -2^15), -1 beyond the row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int h = blockIdx.x % H;
    const int rstride = gridDim.x / H;
    const int HC = H * c;

    for (int idx = tid; idx < 4 * CP * P; idx += NT) {
        const int m = idx / (CP * P), rem = idx - m * (CP * P), d = rem / P, p = rem - d * P;
        const float* W = m == 0 ? wk : m == 1 ? wv : m == 2 ? wq : wg;
        smem[m * CP * L::WP + d * L::WP + p] = d < c ? W[((long)h * c + d) * P + p] : 0.f;
    }
    __syncthreads();                           // the query projections read Wq / Wg before the first chunk's barrier
    const float qscale = TH_LOG2E / sqrtf((float)c);
    constexpr float MASKED = -32768.0f * TH_LOG2E;

    for (long bu = blockIdx.x / H; bu < (long)b * N; bu += rstride) {
        const long bb = bu / N, u = bu - bb * N;
        const float mu = mask[bu];
        const long rowbase = ending ? bb * N * N + u : bu * N;      // position of element v of the row: rowbase + v * vstep
        const long vstep = ending ? N : 1;
        for (int q0 = 0; q0 < N; q0 += TH_NW * TH_QB * 16) {
            const bool active = q0 + wave * TH_QB * 16 < N;          // wave-uniform: the wave has queries in this group
            f32x4 qv[TH_QB][NCT], gv[TH_QB][NCT], acc[TH_QB][NCT];
            float mrun[TH_QB], lrun[TH_QB];
            if (active) {
#pragma unroll
                for (int qb = 0; qb < TH_QB; ++qb) {
                    const int qi = q0 + (wave * TH_QB + qb) * 16 + i;
                    const bool valid = qi < N;
                    float x[P / 4];
                    th_load_ln<P>(pair + (rowbase + (valid ? qi : 0) * vstep) * P, valid, g, x);
                    th_project<P, CP>(Wq, x, qv[qb], i, g);
                    th_project<P, CP>(Wg, x, gv[qb], i, g);
#pragma unroll
                    for (int t = 0; t < NCT; ++t) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int d = 16 * t + 4 * g + r;
                            qv[qb][t][r] *= qscale;
                            gv[qb][t][r] = sigmoidf_(gv[qb][t][r] + (d < c ? bg[h * c + d] : 0.f));
                        }
                        acc[qb][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    mrun[qb] = -INFINITY;
                    lrun[qb] = 0.f;
                }
            }
            for (int k0 = 0; k0 < N; k0 += TH_KC) {
                __syncthreads();                                      // the previous chunk (and the weight staging) is consumed
                {
                    // K^T / V of the chunk: wave w projects key tile w >> 1, K (even w) or V (odd w)
                    const int kt = wave >> 1;
                    const int key = k0 + 16 * kt + i;
                    const bool valid = key < N;
                    float x[P / 4];
                    th_load_ln<P>(pair + (rowbase + (valid ? key : 0) * vstep) * P, valid, g, x);
                    f32x4 y[NCT];
                    th_project<P, CP>((wave & 1) ? Wv : Wk, x, y, i, g);
                    if (wave & 1) {
#pragma unroll
                        for (int t = 0; t < NCT; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) Vl[(16 * kt + i) * L::VP + 16 * t + 4 * g + r] = y[t][r];
                    } else {
#pragma unroll
                        for (int t = 0; t < NCT; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) Kt[(16 * t + 4 * g + r) * TH_KTP + 16 * kt + i] = y[t][r];
                    }
                }
                if (tid < TH_KC) {
                    const int key = k0 + tid;
                    kf[tid] = key >= N ? -1.f : (mu * mask[bb * N + key] >= 0.5f ? 1.f : 0.f);
                }
                __syncthreads();
                if (!active) continue;
                f32x4 s[TH_QB][4];
#pragma unroll
                for (int qb = 0; qb < TH_QB; ++qb)
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt) s[qb][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < NCT; ++t) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* krow = Kt + (16 * t + 4 * g + r) * TH_KTP + i;
#pragma unroll
                        for (int kt = 0; kt < 4; ++kt) {
                            const float a = krow[16 * kt];
#pragma unroll
                            for (int qb = 0; qb < TH_QB; ++qb) s[qb][kt] = mfma16(a, qv[qb][t][r], s[qb][kt]);
                        }
                    }
                }
#pragma unroll
                for (int qb = 0; qb < TH_QB; ++qb) {
                    float mx = -INFINITY;
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float f = kf[16 * kt + 4 * g + r];
                            const float v = f > 0.f ? s[qb][kt][r] : (f == 0.f ? MASKED : -INFINITY);
                            s[qb][kt][r] = v;
                            mx = fmaxf(mx, v);
                        }
                    mx = fmaxf(mx, __shfl_xor(mx, 16));
                    mx = fmaxf(mx, __shfl_xor(mx, 32));
                    // key 0 of the row is in the first chunk and is never -inf, so m_new is finite from the first chunk on
                    const float mnew = fmaxf(mrun[qb], mx);
                    const float alpha = exp2f(mrun[qb] - mnew);
                    mrun[qb] = mnew;
                    float ls = 0.f;
#pragma unroll
                    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float p = exp2f(s[qb][kt][r] - mnew);
                            s[qb][kt][r] = p;
                            ls += p;
                        }
                    lrun[qb] = lrun[qb] * alpha + ls;
#pragma unroll
                    for (int t = 0; t < NCT; ++t) acc[qb][t] *= alpha;
                }
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* vrow = Vl + (16 * kt + 4 * g + r) * L::VP + i;
#pragma unroll
                        for (int t = 0; t < NCT; ++t) {
                            const float a = vrow[16 * t];
#pragma unroll
                            for (int qb = 0; qb < TH_QB; ++qb) acc[qb][t] = mfma16(a, s[qb][kt][r], acc[qb][t]);
                        }
                    }
                }
            }
            if (active) {
#pragma unroll
                for (int qb = 0; qb < TH_QB; ++qb) {
                    float l = lrun[qb];
                    l += __shfl_xor(l, 16);
                    l += __shfl_xor(l, 32);
                    const float il = 1.0f / l;
                    const int qi = q0 + (wave * TH_QB + qb) * 16 + i;
                    if constexpr (LSE) {
                        if (qi < N && g == 0)
                            *reinterpret_cast<float2*>(lse + ((bu * H + h) * N + qi) * 2) = make_float2(mrun[qb], log2f(l));
                    }
                    if (qi < N) {
                        float* dst = og + (rowbase + (long)qi * vstep) * HC + h * c;
#pragma unroll
                        for (int t = 0; t < NCT; ++t) {
                            const int d0 = 16 * t + 4 * g;
                            if (d0 < c)
                                *reinterpret_cast<float4*>(dst + d0) =
                                    make_float4(gv[qb][t][0] * (acc[qb][t][0] * il), gv[qb][t][1] * (acc[qb][t][1] * il),
                                                gv[qb][t][2] * (acc[qb][t][2] * il), gv[qb][t][3] * (acc[qb][t][3] * il));
                        }
                    }
                }
            }
        }
    }
}

template <int P, int CP, bool LSE>
int th_launch(float* og, float* lse, const float* pair, const float* mask, const float* wq, const float* wk, const float* wv,
               const float* wg, const float* bg, int ending, int b, int N, int H, int c, hipStream_t stream) {
    const size_t lds = th_lds_bytes<P, CP>();
    // persistent, one workgroup of 8 waves per CU (the registers allow no second one): per head the smallest workgroup count that
    // reaches the minimum number of row rounds, as prd_tri_attn_core
    const long per_head = prd_rows_per_head((long)b * N, 256 / H);
    return prd_launch<tri_attn_heads_kernel<P, CP, LSE>>(dim3((unsigned)(per_head * H)), dim3(TH_NW * 64), lds, stream,
                                                         og, lse, pair, mask, wq, wk, wv, wg, bg, b, N, H, c, ending);
}

}  // namespace

extern "C" int prd_tri_attn_heads_supported(int N, int P, int H, int c, int arith) {
    PRD_SPLIT_ARITH(arith);
    if (N <= 0) return 0;
    return (P == 32 || P == 64) && H >= 1 && H <= 8 && c >= 4 && c <= 64 && c % 4 == 0 ? 1 : 0;
}

extern "C" size_t prd_tri_attn_heads_workspace_bytes(int b, int N, int P, int H, int c) {
    if (b <= 0 || prd_tri_attn_heads_supported(N, P, H, c, PRD_ARITH_FP32) != 1) return 0;
    return (size_t)b * N * N * H * c * sizeof(float);       // og; the single-launch kernel keeps no softmax statistics outside registers
}

namespace {

int th_core(float* og, float* lse, const float* pair, const float* mask, const float* wq, const float* wk, const float* wv,
            const float* wg, const float* bg, int ending, int b, int N, int P, int H, int c, float* ws, size_t ws_bytes, int arith,
            hipStream_t stream) {
    PRD_SPLIT_ARITH(arith);                    // validated; the split bit is ignored (fp32 MFMA in both modes)
    if (!og || !pair || !mask || !wq || !wk || !wv || !wg || !bg || !ws || b <= 0 || N <= 0) return PRD_ERR_ARG;
    if (prd_tri_attn_heads_supported(N, P, H, c, arith) != 1) return PRD_ERR_UNSUPPORTED;
    if (ws_bytes < prd_tri_attn_heads_workspace_bytes(b, N, P, H, c)) return PRD_ERR_WORKSPACE;
    if (((uintptr_t)og | (uintptr_t)pair) & 15) return PRD_ERR_ALIGN;
    if ((uintptr_t)lse & 7) return PRD_ERR_ALIGN;
    const int cp = c <= 16 ? 16 : c <= 32 ? 32 : 64;
    return PRD_FOR_P(P, PP, PRD_FOR_3(cp, CC, 16, 32, 64, PRD_FOR_BOOL(lse != nullptr, LSE,
        th_launch<PP, CC, LSE>(og, lse, pair, mask, wq, wk, wv, wg, bg, ending, b, N, H, c, stream))));
}

}  // namespace

extern "C" int prd_tri_attn_core_heads(float* og, const float* pair, const float* mask, const float* wq, const float* wk,
                                       const float* wv, const float* wg, const float* bg, int ending, int b, int N, int P, int H,
                                       int c, float* ws, size_t ws_bytes, int arith, hipStream_t stream) {
    return th_core(og, nullptr, pair, mask, wq, wk, wv, wg, bg, ending, b, N, P, H, c, ws, ws_bytes, arith, stream);
}

extern "C" int prd_tri_attn_core_heads_lse(float* og, float* lse, const float* pair, const float* mask, const float* wq,
                                           const float* wk, const float* wv, const float* wg, const float* bg, int ending, int b,
                                           int N, int P, int H, int c, float* ws, size_t ws_bytes, int arith, hipStream_t stream) {
    return th_core(og, lse, pair, mask, wq, wk, wv, wg, bg, ending, b, N, P, H, c, ws, ws_bytes, arith, stream);
}
