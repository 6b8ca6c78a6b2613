// Superposition and TM-score of generated samples on the device (include/prd_align.h; the reference's generate.py:163-195 shells out
// to the TM-align program for this).  Three launches per call:
//   1. align_compact_kernel   one workgroup per structure: the masked rows of the structure, in order, as three coordinate planes
//                             in the workspace; L, the number of masked positions, is counted here and never travels to the host.
//   2. align_search_kernel    the unit of parallel work is (pair, mirror, seed): a workgroup holds the two coordinate sets of one
//                             (pair, mirror) in the LDS, each of its WAVES walks seeds of its own.  A fit is 15 sums over the
//                             subset -- accumulated in fp64 from the fp32 coordinates (the products are exact), so uncentred
//                             coordinates lose nothing in sum(x y) - sum(x) sum(y) / n -- and one wave reduction; the 4 x 4
//                             eigenproblem of the rotation is solved redundantly in every lane in fp64.  Distances and TM terms of
//                             the search are fp32.  Every workgroup writes ONE record (its best seed) to the workspace.
//   3. align_finalize_kernel  one wave per pair picks the best record (ties: unmirrored, then the lowest seed), evaluates tm and
//                             rmsd in fp64 from the fp32 transform it returns, and writes the outputs.
// The seeds, d0 and the fit itself are in prd_superpose.h, which prd_tmalign.hip includes as well.
// One owner per output element, plain vector stores, no atomics; every loop over rounds or cut-offs is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_align.h"
#include "prd_launch.h"
#include "prd_superpose.h"

namespace {

#define AL_DEV __device__ __forceinline__

constexpr int AL_COMPACT_WG = SP_COMPACT_WG;    // threads of a compaction workgroup; each owns AL_OWN consecutive positions
constexpr int AL_OWN = PRD_ALIGN_MAX_N / AL_COMPACT_WG;
constexpr int AL_REC = SP_REC;          // floats of a record; its key is the seed
constexpr int AL_ROUNDS = 20;
constexpr int AL_HDR = 16;              // ints at the head of the workspace; [0] = L
constexpr int AL_MAX_WAVES = 8;         // waves of a search workgroup: 4 (N <= 1024) or 8
constexpr int AL_SEEDS_PER_WAVE = 4;    // seeds a wave is meant to walk (sizes the second grid dimension)
constexpr int AL_MAX_G = 1024;          // records per (pair, mirror) at most
constexpr int AL_CUT_RAISES = 4096;     // d_cut is raised at most this often (2048 Angstrom: beyond any finite input in range)

// pair index -> (s, r): row-major S x R, or the pairs s < r of the self mode in row order
AL_DEV void al_pair_decode(long pair, int S, int R, int self, int& s, int& r) {
    if (!self) {
        s = (int)(pair / R);
        r = (int)(pair - (long)s * R);
        return;
    }
    s = 0;
    while (s < S - 1 && pair >= S - 1 - s) {
        pair -= S - 1 - s;
        ++s;
    }
    r = s + 1 + (int)pair;
}

// ---- 1. compaction ---------------------------------------------------------------------------------------------------------------
// planes[st][c][j] = coordinate c of the j-th masked position of structure st (st < nx: X, else Y); hdr[0] = L
__global__ __launch_bounds__(AL_COMPACT_WG) void align_compact_kernel(float* __restrict__ planes, int* __restrict__ hdr,
                                                                     const float* __restrict__ x, long long x_ss, int x_rs,
                                                                     const float* __restrict__ y, long long y_ss, int y_rs,
                                                                     const float* __restrict__ mask, int nx, int N) {
    __shared__ int cnt[AL_COMPACT_WG];
    const int st = blockIdx.x, tid = threadIdx.x;
    const float* src = st < nx ? x + (long long)st * x_ss : y + (long long)(st - nx) * y_ss;
    const int rs = st < nx ? x_rs : y_rs;
    const int i0 = tid * AL_OWN;
    int total, pos = sp_compact_start(cnt, mask, AL_OWN, N, total);
    float* dst = planes + (size_t)st * 3 * N;
    for (int i = i0; i < i0 + AL_OWN && i < N; ++i)
        if (mask[i] > 0.5f) sp_put_row(dst, N, pos++, src + (long long)i * rs);     // pos < total <= N
    if (st == 0 && tid == 0) hdr[0] = total;
}

// ---- 2. the search ---------------------------------------------------------------------------------------------------------------
// grid (problems, G): problem = pair * nm + mirror; the waves of workgroup (p, g) walk seeds g * nw + wave, + G * nw, ...
// rec[(p * G + g) * AL_REC ...]: the workgroup's best (score = sum of TM terms, or -sum d^2 in RMSD mode; -inf when it had no seed)
__global__ __launch_bounds__(64 * AL_MAX_WAVES) void align_search_kernel(float* __restrict__ rec, const float* __restrict__ planes,
                                                                        const int* __restrict__ hdr, int S, int R, int N, int self,
                                                                        int mode, int nm, int G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];        // 6 planes of N floats
    __shared__ float wrec[AL_MAX_WAVES][AL_REC];
    const int L = hdr[0];
    if (L < 3) return;                                                  // uniform; the finalize pass writes the documented zeros
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const long p = blockIdx.x;
    const int mir = (int)(p % nm);
    int s, r;
    al_pair_decode(p / nm, S, R, self, s, r);
    const float* xs = planes + (size_t)s * 3 * N;
    const float* ys = planes + (size_t)(self ? r : S + r) * 3 * N;
    float *X0 = lds, *X1 = lds + N, *X2 = lds + 2 * N, *Y0 = lds + 3 * N, *Y1 = lds + 4 * N, *Y2 = lds + 5 * N;
    for (int i = tid; i < L; i += blockDim.x) {
        X0[i] = xs[i];
        X1[i] = xs[N + i];
        X2[i] = mir ? -xs[2 * N + i] : xs[2 * N + i];
        Y0[i] = ys[i];
        Y1[i] = ys[N + i];
        Y2[i] = ys[2 * N + i];
    }
    __syncthreads();
    const Coords c = {X0, X1, X2, Y0, Y1, Y2};

    const int K = mode == PRD_ALIGN_MODE_RMSD ? 1 : sp_seed_count(L);
    const float d0 = (float)sp_d0(L);
    const float inv_d02 = 1.f / (d0 * d0);
    const float d0s = fminf(fmaxf(d0, 4.5f), 8.f);
    const float inf = __builtin_inff();
    float best = -inf, brot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, btr[3] = {0.f, 0.f, 0.f};
    int bseed = 0;

    for (int seed = blockIdx.y * nw + wave; seed < K; seed += G * nw) {     // wave-uniform
        int start, len;
        sp_seed_decode(L, seed, start, len);
        unsigned long long mem = 0ull;                                       // bit k: position lane + 64 k is in the subset (L <= 4096)
        for (int i = lane, k = 0; i < L; i += 64, ++k) mem |= (i >= start && i < start + len) ? 1ull << k : 0ull;
        float rot[9], tr[3];
        for (int it = 0; it < AL_ROUNDS; ++it) {
            // ---- the 15 sums of the subset, fp64 (plain arrays, not the Sums of prd_tmalign.hip: that takes this kernel from 158 to 156
            // registers, and its figures stay what they are: DESIGN 7.2)
            double sx[3] = {0., 0., 0.}, sy[3] = {0., 0., 0.}, sxy[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
            float cnt = 0.f;
            for (int i = lane, k = 0; i < L; i += 64, ++k) {
                if ((mem >> k) & 1ull) {
                    const double x[3] = {(double)X0[i], (double)X1[i], (double)X2[i]}, y[3] = {(double)Y0[i], (double)Y1[i], (double)Y2[i]};
                    cnt += 1.f;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        sx[a] += x[a];
                        sy[a] += y[a];
#pragma unroll
                        for (int b = 0; b < 3; ++b) sxy[3 * a + b] += x[a] * y[b];
                    }
                }
            }
            cnt = wave_sum(cnt);
            if (cnt < 3.f) break;                                            // only after non-finite input
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                sx[a] = wave_sum(sx[a]);
                sy[a] = wave_sum(sy[a]);
            }
#pragma unroll
            for (int a = 0; a < 9; ++a) sxy[a] = wave_sum(sxy[a]);
            kabsch_from_sums<false>(sx, sy, sxy, (double)cnt, rot, tr);

            // ---- score all positions; the three smallest squared distances of the wave
            float sc = 0.f, m0 = inf, m1 = inf, m2 = inf;
            for (int i = lane; i < L; i += 64) {
                const float d2 = sp_d2(c, i, i, rot, tr);
                sc += mode == PRD_ALIGN_MODE_RMSD ? -d2 : __builtin_amdgcn_rcpf(1.f + d2 * inv_d02);
                keep3(m0, m1, m2, d2);
            }
            sc = wave_sum(sc);
            if (sc > best) {                                                 // the first of equal scores stays: lowest seed, earliest round
                best = sc;
                bseed = seed;
#pragma unroll
                for (int a = 0; a < 9; ++a) brot[a] = rot[a];
#pragma unroll
                for (int a = 0; a < 3; ++a) btr[a] = tr[a];
            }
            if (mode == PRD_ALIGN_MODE_RMSD) break;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float o0 = __shfl_xor(m0, o), o1 = __shfl_xor(m1, o), o2 = __shfl_xor(m2, o);
                keep3(m0, m1, m2, o0);
                keep3(m0, m1, m2, o1);
                keep3(m0, m1, m2, o2);
            }
            // ---- the next subset: d_i < d_cut, d_cut raised by 0.5 until the third smallest distance is inside
            float cut = it == 0 ? d0s - 1.f : d0s + 1.f;
            for (int u = 0; u < AL_CUT_RAISES && !(m2 < cut * cut); ++u) cut += 0.5f;
            const float cut2 = cut * cut;
            unsigned long long next = 0ull;
            for (int i = lane, k = 0; i < L; i += 64, ++k)
                next |= sp_d2(c, i, i, rot, tr) < cut2 ? 1ull << k : 0ull;
            if (!__any(next != mem)) break;
            mem = next;
        }
    }

    if (lane == 0) {
        sp_record_write(wrec[wave], best, bseed, brot, btr);
        wrec[wave][14] = wrec[wave][15] = 0.f;
    }
    __syncthreads();
    if (tid < AL_REC) {
        int w = 0;
        for (int j = 1; j < nw; ++j) {
            const float sj = wrec[j][0], sw = wrec[w][0];
            if (sj > sw || (sj == sw && __float_as_int(wrec[j][1]) < __float_as_int(wrec[w][1]))) w = j;
        }
        rec[((size_t)p * G + blockIdx.y) * AL_REC + tid] = wrec[w][tid];
    }
}

// ---- 3. the outputs --------------------------------------------------------------------------------------------------------------
AL_DEV void al_store(float* tm, float* rmsd, float* rot, float* trans, int* mirrored, size_t o, float vtm, float vrmsd,
                     const float (&m)[9], const float (&t)[3], int mir) {
    tm[o] = vtm;
    rmsd[o] = vrmsd;
#pragma unroll
    for (int a = 0; a < 9; ++a) rot[o * 9 + a] = m[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) trans[o * 3 + a] = t[a];
    mirrored[o] = mir;
}

// one wave per block: blocks [0, npairs) own a searched pair (and its transposed entry in the self mode), blocks npairs + s the
// diagonal entry (s, s) of the self mode
__global__ __launch_bounds__(64) void align_finalize_kernel(float* __restrict__ tm, float* __restrict__ rmsd, float* __restrict__ rot,
                                                           float* __restrict__ trans, int* __restrict__ mirrored,
                                                           const float* __restrict__ rec, const float* __restrict__ planes,
                                                           const int* __restrict__ hdr, int S, int R, int N, int self, int nm, int G,
                                                           long npairs) {
    const int lane = threadIdx.x, L = hdr[0];
    const long blk = blockIdx.x;
    const float eye[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, zero[3] = {0.f, 0.f, 0.f};
    if (blk >= npairs) {                                 // diagonal of the self mode
        const int s = (int)(blk - npairs);
        if (lane == 0) al_store(tm, rmsd, rot, trans, mirrored, (size_t)s * R + s, L < 3 ? 0.f : 1.f, 0.f, eye, zero, 0);
        return;
    }
    int s, r;
    al_pair_decode(blk, S, R, self, s, r);
    const size_t o = (size_t)s * R + r, ot = (size_t)r * R + s;
    if (L < 3) {
        if (lane == 0) {
            al_store(tm, rmsd, rot, trans, mirrored, o, 0.f, 0.f, eye, zero, 0);
            if (self) al_store(tm, rmsd, rot, trans, mirrored, ot, 0.f, 0.f, eye, zero, 0);
        }
        return;
    }
    // ---- the best record: highest score, then unmirrored, then the lowest seed (records are mirror-major: j / G = mirror)
    const float* recs = rec + (size_t)blk * nm * G * AL_REC;
    float bs = -__builtin_inff();
    int bj = -1, bseed = 0x7fffffff;
    for (int j = lane; j < nm * G; j += 64) {
        const float sc = recs[(size_t)j * AL_REC];
        const int sd = __float_as_int(recs[(size_t)j * AL_REC + 1]);
        const bool better = bj < 0 ? sc > bs : (sc > bs || (sc == bs && (j / G < bj / G || (j / G == bj / G && sd < bseed))));
        if (better) { bs = sc; bj = j; bseed = sd; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float os = __shfl_xor(bs, off);
        const int oj = __shfl_xor(bj, off), osd = __shfl_xor(bseed, off);
        const bool better = oj >= 0 && (bj < 0 || os > bs || (os == bs && (oj / G < bj / G || (oj / G == bj / G && osd < bseed))));
        if (better) { bs = os; bj = oj; bseed = osd; }
    }
    if (bj < 0) {                                        // no finite score at all (non-finite input): say so
        const float nan = __builtin_nanf("");
        if (lane == 0) {
            al_store(tm, rmsd, rot, trans, mirrored, o, nan, nan, eye, zero, 0);
            if (self) al_store(tm, rmsd, rot, trans, mirrored, ot, nan, nan, eye, zero, 0);
        }
        return;
    }
    const int mir = bj / G;
    float m[9], t[3];
    sp_record_transform(recs + (size_t)bj * AL_REC, m, t);
    if (mir) sp_unmirror(m);
    // ---- tm and rmsd under the fp32 transform that is returned, fp64
    const float* xs = planes + (size_t)s * 3 * N;
    const float* ys = planes + (size_t)(self ? r : S + r) * 3 * N;
    const double d0 = sp_d0(L), inv_d02 = 1.0 / (d0 * d0);
    double stm = 0.0, sd2 = 0.0;
    for (int i = lane; i < L; i += 64) {
        const double d2 = sp_d2_f64(xs, N, i, ys, N, i, m, t);
        sd2 += d2;
        stm += 1.0 / (1.0 + d2 * inv_d02);
    }
    stm = wave_sum(stm);
    sd2 = wave_sum(sd2);
    if (lane == 0) {
        const float vtm = (float)(stm / L), vrmsd = (float)sqrt(sd2 / L);
        al_store(tm, rmsd, rot, trans, mirrored, o, vtm, vrmsd, m, t, mir);
        if (self) {                                      // x ~ (y - t) @ rot^T: the inverse isometry has the same distances
            float mt[9], tt[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) mt[3 * a + b] = m[3 * b + a];
#pragma unroll
            for (int b = 0; b < 3; ++b) tt[b] = (float)-((double)t[0] * mt[b] + (double)t[1] * mt[3 + b] + (double)t[2] * mt[6 + b]);
            al_store(tm, rmsd, rot, trans, mirrored, ot, vtm, vrmsd, mt, tt, mir);
        }
    }
}

__global__ __launch_bounds__(256) void align_apply_kernel(float* __restrict__ out, const float* __restrict__ pos, const float* __restrict__ rot,
                                                         const float* __restrict__ trans, int N) {
    const int s = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float* m = rot + (size_t)s * 9;
    const float* t = trans + (size_t)s * 3;
    const size_t o = ((size_t)s * N + i) * 3;
    const float x0 = pos[o], x1 = pos[o + 1], x2 = pos[o + 2];
    out[o] = t[0] + (x0 * m[0] + x1 * m[3] + x2 * m[6]);
    out[o + 1] = t[1] + (x0 * m[1] + x1 * m[4] + x2 * m[7]);
    out[o + 2] = t[2] + (x0 * m[2] + x1 * m[5] + x2 * m[8]);
}

// ---- host side: the shape of a call ----------------------------------------------------------------------------------------------
// dynamic LDS of a search workgroup: the three planes of both structures
constexpr size_t al_lds_bytes(int N) { return (size_t)6 * N * sizeof(float); }
static_assert(al_lds_bytes(PRD_ALIGN_MAX_N) + 1024 <= PRD_LDS_MAX, "the search kernel's LDS at the longest row the plan accepts, and its static wrec");

struct AlignPlan {
    int ok, self, nm, nw, G, nstruct;
    long npairs;
    size_t off_planes, off_rec, bytes;
};

AlignPlan align_plan(int S, int R, int N, int pairs, int mode, int mirror) {
    AlignPlan P = {};
    if (S <= 0 || R <= 0 || N <= 0 || N > PRD_ALIGN_MAX_N) return P;
    if (pairs != PRD_ALIGN_PAIRS_CROSS && pairs != PRD_ALIGN_PAIRS_SELF) return P;
    if (mode != PRD_ALIGN_MODE_TM && mode != PRD_ALIGN_MODE_RMSD) return P;
    P.self = pairs == PRD_ALIGN_PAIRS_SELF;
    if (P.self && R != S) return P;
    P.nm = mirror ? 2 : 1;
    P.nw = N <= 1024 ? 4 : AL_MAX_WAVES;
    int kmax = 1;                                       // the seed count is not monotonic in L: the largest one up to N
    if (mode == PRD_ALIGN_MODE_TM)
        for (int L = 3; L <= N; ++L) {
            const int k = sp_seed_count(L);
            kmax = k > kmax ? k : kmax;
        }
    const int per = P.nw * AL_SEEDS_PER_WAVE;
    P.G = (kmax + per - 1) / per;
    P.G = P.G > AL_MAX_G ? AL_MAX_G : P.G;
    P.npairs = P.self ? (long)S * (S - 1) / 2 : (long)S * R;
    if (P.npairs * P.nm + S > 0x7fffffffL) return P;   // the first grid dimension of the search and of the finalize pass
    P.nstruct = P.self ? S : S + R;
    P.off_planes = AL_HDR * sizeof(int);
    P.off_rec = P.off_planes + (size_t)P.nstruct * 3 * N * sizeof(float);
    P.off_rec = (P.off_rec + 15) & ~(size_t)15;
    // room for the records of 4-wave workgroups at every N: G halves where the workgroups go from 4 to 8 waves (N = 1025), and a
    // workspace sized for the longest row of a run has to do for every shorter one
    const int per4 = 4 * AL_SEEDS_PER_WAVE;
    int Ga = (kmax + per4 - 1) / per4;
    Ga = Ga > AL_MAX_G ? AL_MAX_G : Ga;
    P.bytes = P.off_rec + (size_t)P.npairs * P.nm * Ga * AL_REC * sizeof(float);
    P.bytes = P.bytes ? P.bytes : 16;
    P.ok = 1;
    return P;
}

}  // namespace

extern "C" int prd_align_version(void) { return PRD_ALIGN_VERSION; }

extern "C" size_t prd_align_workspace_bytes(int S, int R, int N, int pairs, int mode, int mirror) {
    const AlignPlan P = align_plan(S, R, N, pairs, mode, mirror);
    return P.ok ? P.bytes : 0;
}

extern "C" int prd_align_superimpose(float* tm, float* rmsd, float* rot, float* trans, int* mirrored,
                                     const float* x, long long x_struct_stride, int x_row_stride,
                                     const float* y, long long y_struct_stride, int y_row_stride,
                                     const float* mask, int S, int R, int N, int pairs, int mode, int mirror,
                                     void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!tm || !rmsd || !rot || !trans || !mirrored || !x || !mask || !ws || S <= 0 || R <= 0 || N <= 0) return PRD_ALIGN_ERR_ARG;
    if (pairs != PRD_ALIGN_PAIRS_CROSS && pairs != PRD_ALIGN_PAIRS_SELF) return PRD_ALIGN_ERR_ARG;
    if (mode != PRD_ALIGN_MODE_TM && mode != PRD_ALIGN_MODE_RMSD) return PRD_ALIGN_ERR_ARG;
    if (x_row_stride < 3 || x_struct_stride < 0) return PRD_ALIGN_ERR_ARG;
    const bool self = pairs == PRD_ALIGN_PAIRS_SELF;
    if (self && (R != S || (y && y != x))) return PRD_ALIGN_ERR_ARG;
    if (!self && (!y || y_row_stride < 3 || y_struct_stride < 0)) return PRD_ALIGN_ERR_ARG;
    if (N > PRD_ALIGN_MAX_N) return PRD_ALIGN_ERR_UNSUPPORTED;
    const AlignPlan P = align_plan(S, R, N, pairs, mode, mirror);
    if (!P.ok) return PRD_ALIGN_ERR_UNSUPPORTED;
    if (ws_bytes < P.bytes || (reinterpret_cast<uintptr_t>(ws) & 15)) return PRD_ALIGN_ERR_WORKSPACE;
    int* hdr = reinterpret_cast<int*>(ws);
    float* planes = reinterpret_cast<float*>(static_cast<char*>(ws) + P.off_planes);
    float* rec = reinterpret_cast<float*>(static_cast<char*>(ws) + P.off_rec);

    const size_t lds = al_lds_bytes(N);
    if (P.npairs > 0) PRD_TRY(prd_lds_ready<align_search_kernel>(lds));     // before anything is enqueued: a refusal leaves nothing launched
    PRD_TRY(prd_launch<align_compact_kernel>(dim3(P.nstruct), dim3(AL_COMPACT_WG), 0, stream, planes, hdr, x, x_struct_stride, x_row_stride,
                                             self ? x : y, self ? x_struct_stride : y_struct_stride, self ? x_row_stride : y_row_stride, mask, S, N));
    if (P.npairs > 0)
        PRD_TRY(prd_launch<align_search_kernel>(dim3((unsigned)(P.npairs * P.nm), P.G), dim3(64 * P.nw), lds, stream, rec, planes, hdr, S, R, N,
                                                self ? 1 : 0, mode, P.nm, P.G));
    const long nblocks = P.npairs + (self ? S : 0);
    return prd_launch<align_finalize_kernel>(dim3((unsigned)nblocks), dim3(64), 0, stream, tm, rmsd, rot, trans, mirrored, rec, planes, hdr, S, R, N,
                                             self ? 1 : 0, P.nm, P.G, P.npairs);
}

extern "C" int prd_align_apply(float* out, const float* pos, const float* rot, const float* trans, int S, int N, hipStream_t stream) {
    if (!out || !pos || !rot || !trans || S <= 0 || N <= 0) return PRD_ALIGN_ERR_ARG;
    if (S > 65535) return PRD_ALIGN_ERR_UNSUPPORTED;
    return prd_launch<align_apply_kernel>(dim3((N + 255) / 256, S), dim3(256), 0, stream, out, pos, rot, trans, N);
}
