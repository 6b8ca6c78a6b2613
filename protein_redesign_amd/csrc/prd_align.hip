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
// One owner per output element, plain vector stores, no atomics; every loop over rounds or cut-offs is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_align.h"

namespace {

#define AL_DEV __device__ __forceinline__

constexpr int AL_COMPACT_WG = 256;      // threads of a compaction workgroup; each owns AL_MAX_N / 256 consecutive positions
constexpr int AL_OWN = PRD_ALIGN_MAX_N / AL_COMPACT_WG;
constexpr int AL_REC = 16;              // floats of a record: score, seed (bits), rot[9], trans[3], 2 unused
constexpr int AL_ROUNDS = 20;
constexpr int AL_HDR = 16;              // ints at the head of the workspace; [0] = L
constexpr int AL_MAX_WAVES = 8;         // waves of a search workgroup: 4 (N <= 1024) or 8
constexpr int AL_SEEDS_PER_WAVE = 4;    // seeds a wave is meant to walk (sizes the second grid dimension)
constexpr int AL_MAX_G = 1024;          // records per (pair, mirror) at most
constexpr int AL_CUT_RAISES = 4096;     // d_cut is raised at most this often (2048 Angstrom: beyond any finite input in range)

AL_DEV double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
AL_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- the seeds of the search (prd_align.h, TM mode, steps 1 and 2) --------------------------------------------------------------
// fragment lengths L, L/2, L/4, ... as long as they exceed 4, then 4 itself (TM-score's own convention: the shortest fragment is 4),
// and for L <= 21 fragments of 3 as well: there d0 is 0.5 while d_cut is never below 3.5, so the rounds cannot shed an outlier of a
// chain that small and the seed itself has to be able to be free of them
__host__ __device__ inline int al_next_level(int Lf, int L) { return Lf > 4 ? (Lf / 2 > 4 ? Lf / 2 : 4) : (Lf == 4 && L <= 21 ? 3 : 0); }
__host__ __device__ inline int al_level_count(int L, int Lf) {
    const int step = Lf / 2 > 1 ? Lf / 2 : 1, span = L - Lf;
    return span / step + 1 + (span % step ? 1 : 0);
}
__host__ __device__ inline int al_seed_count(int L) {
    if (L < 4) return 1;
    int K = 0;
    for (int Lf = L; Lf >= 3; Lf = al_next_level(Lf, L)) K += al_level_count(L, Lf);
    return K;
}
// seed -> (first position, length) of its fragment; seed < al_seed_count(L)
AL_DEV void al_seed_decode(int L, int seed, int& start, int& len) {
    start = 0;
    len = L;
    if (L < 4) return;
    for (int Lf = L; Lf >= 3; Lf = al_next_level(Lf, L)) {
        const int c = al_level_count(L, Lf);
        if (seed < c) {
            const int step = Lf / 2 > 1 ? Lf / 2 : 1;
            const int s = seed * step;
            start = s < L - Lf ? s : L - Lf;        // the last one is the last possible start
            len = Lf;
            return;
        }
        seed -= c;
    }
}

AL_DEV double al_d0(int L) { return L > 21 ? 1.24 * cbrt((double)L - 15.0) - 1.8 : 0.5; }

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
    int c = 0;
    for (int i = i0; i < i0 + AL_OWN && i < N; ++i) c += mask[i] > 0.5f ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    int pos = 0, total = 0;
    for (int j = 0; j < AL_COMPACT_WG; ++j) {
        const int v = cnt[j];
        pos += j < tid ? v : 0;
        total += v;
    }
    float* dst = planes + (size_t)st * 3 * N;
    for (int i = i0; i < i0 + AL_OWN && i < N; ++i) {
        if (mask[i] > 0.5f) {                       // pos < total <= N
            const float* p = src + (long long)i * rs;
            dst[pos] = p[0];
            dst[N + pos] = p[1];
            dst[2 * N + pos] = p[2];
            ++pos;
        }
    }
    if (st == 0 && tid == 0) hdr[0] = total;
}

// ---- the fit -----------------------------------------------------------------------------------------------------------------------
// One Jacobi rotation of the symmetric 4 x 4 matrix A in the (P, Q) plane, accumulated into V.  The ANGLE is computed in fp32 (hardware
// reciprocal and reciprocal square root), the pair (c, s) is then brought back to c^2 + s^2 = 1 in fp64 (first-order correction:
// the fp32 pair is within 1e-7 of the unit circle, what is left is 1e-14) and applied in fp64 with the exact update of A[P][Q] -- an
// orthogonal similarity that merely does not annihilate the element completely.  The eigenvector is normalised in fp64 at the end,
// so the orthogonality of the rotation matrix does not depend on any of this.
template <int P, int Q>
AL_DEV void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    const float f = (float)apq;
    if (f == 0.f) return;
    const float th = 0.5f * (float)(A[Q][Q] - A[P][P]) * __builtin_amdgcn_rcpf(f);
    const float t = __builtin_copysignf(1.f, th) * __builtin_amdgcn_rcpf(__builtin_fabsf(th) + __builtin_sqrtf(th * th + 1.f));
    const float cf = __builtin_amdgcn_rsqf(t * t + 1.f), sf = t * cf;
    if (!(cf == cf) || !(sf == sf)) return;         // a NaN angle (non-finite input) rotates nothing
    double c = (double)cf, s = (double)sf;
    const double k = 1.5 - 0.5 * (c * c + s * s);
    c *= k;
    s *= k;
    const double app = A[P][P], aqq = A[Q][Q];
    A[P][P] = c * c * app - 2.0 * c * s * apq + s * s * aqq;
    A[Q][Q] = s * s * app + 2.0 * c * s * apq + c * c * aqq;
    A[P][Q] = A[Q][P] = (c * c - s * s) * apq + c * s * (app - aqq);
#pragma unroll
    for (int k2 = 0; k2 < 4; ++k2) {
        if (k2 != P && k2 != Q) {
            const double akp = A[k2][P], akq = A[k2][Q];
            A[k2][P] = A[P][k2] = c * akp - s * akq;
            A[k2][Q] = A[Q][k2] = s * akp + c * akq;
        }
        const double vkp = V[k2][P], vkq = V[k2][Q];
        V[k2][P] = c * vkp - s * vkq;
        V[k2][Q] = s * vkp + c * vkq;
    }
}

// sums over a subset of n >= 3 positions: sx[a] = sum x_a, sy[b] = sum y_b, sxy[3 a + b] = sum x_a y_b  ->  the proper rotation and
// translation of least squares, row-vector convention y ~ tr + x @ rot (Horn's quaternion form: the eigenvector of the largest
// eigenvalue of a symmetric 4 x 4 matrix; rank-deficient subsets -- three points are always coplanar -- are no special case)
AL_DEV void kabsch_from_sums(const double (&sx)[3], const double (&sy)[3], const double (&sxy)[9], double n, float (&rot)[9], float (&tr)[3]) {
    const double inv = 1.0 / n;
    double mx[3], my[3], M[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        mx[a] = sx[a] * inv;
        my[a] = sy[a] * inv;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) M[a][b] = sxy[3 * a + b] - sx[a] * my[b];
    double A[4][4], V[4][4];
    A[0][0] = M[0][0] + M[1][1] + M[2][2];
    A[1][1] = M[0][0] - M[1][1] - M[2][2];
    A[2][2] = -M[0][0] + M[1][1] - M[2][2];
    A[3][3] = -M[0][0] - M[1][1] + M[2][2];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 6; ++sweep) {
        jacobi_rotate<0, 1>(A, V);
        jacobi_rotate<0, 2>(A, V);
        jacobi_rotate<0, 3>(A, V);
        jacobi_rotate<1, 2>(A, V);
        jacobi_rotate<1, 3>(A, V);
        jacobi_rotate<2, 3>(A, V);
    }
    // the column of the largest diagonal element (selects: no dynamic register index)
    double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const bool up = A[j][j] > best;
        best = up ? A[j][j] : best;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i] = up ? V[i][j] : q[i];
    }
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * qn, a = q[1] * qn, b = q[2] * qn, c = q[3] * qn;
    // column convention y = Qm x; rot = Qm^T
    double Qm[3][3];
    Qm[0][0] = 1.0 - 2.0 * (b * b + c * c); Qm[0][1] = 2.0 * (a * b - w * c);       Qm[0][2] = 2.0 * (a * c + w * b);
    Qm[1][0] = 2.0 * (a * b + w * c);       Qm[1][1] = 1.0 - 2.0 * (a * a + c * c); Qm[1][2] = 2.0 * (b * c - w * a);
    Qm[2][0] = 2.0 * (a * c - w * b);       Qm[2][1] = 2.0 * (b * c + w * a);       Qm[2][2] = 1.0 - 2.0 * (a * a + b * b);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) rot[3 * i + j] = (float)Qm[j][i];
#pragma unroll
    for (int j = 0; j < 3; ++j) tr[j] = (float)(my[j] - (mx[0] * Qm[j][0] + mx[1] * Qm[j][1] + mx[2] * Qm[j][2]));
}

// squared distance of position i under (rot, tr), fp32
AL_DEV float al_d2(const float* X0, const float* X1, const float* X2, const float* Y0, const float* Y1, const float* Y2, int i,
                   const float (&rot)[9], const float (&tr)[3]) {
    const float x0 = X0[i], x1 = X1[i], x2 = X2[i];
    const float e0 = (tr[0] + (x0 * rot[0] + x1 * rot[3] + x2 * rot[6])) - Y0[i];
    const float e1 = (tr[1] + (x0 * rot[1] + x1 * rot[4] + x2 * rot[7])) - Y1[i];
    const float e2 = (tr[2] + (x0 * rot[2] + x1 * rot[5] + x2 * rot[8])) - Y2[i];
    return e0 * e0 + e1 * e1 + e2 * e2;
}

// keep the three smallest of (a <= b <= c) and v
AL_DEV void keep3(float& a, float& b, float& c, float v) {
    if (v < c) {
        c = v;
        if (c < b) { const float t = b; b = c; c = t; }
        if (b < a) { const float t = a; a = b; b = t; }
    }
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

    const int K = mode == PRD_ALIGN_MODE_RMSD ? 1 : al_seed_count(L);
    const float d0 = (float)al_d0(L);
    const float inv_d02 = 1.f / (d0 * d0);
    const float d0s = fminf(fmaxf(d0, 4.5f), 8.f);
    const float inf = __builtin_inff();
    float best = -inf, brot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, btr[3] = {0.f, 0.f, 0.f};
    int bseed = 0;

    for (int seed = blockIdx.y * nw + wave; seed < K; seed += G * nw) {     // wave-uniform
        int start, len;
        al_seed_decode(L, seed, start, len);
        unsigned long long mem = 0ull;                                       // bit k: position lane + 64 k is in the subset (L <= 4096)
        for (int i = lane, k = 0; i < L; i += 64, ++k) mem |= (i >= start && i < start + len) ? 1ull << k : 0ull;
        float rot[9], tr[3];
        for (int it = 0; it < AL_ROUNDS; ++it) {
            // ---- the 15 sums of the subset, fp64
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
            kabsch_from_sums(sx, sy, sxy, (double)cnt, rot, tr);

            // ---- score all positions; the three smallest squared distances of the wave
            float sc = 0.f, m0 = inf, m1 = inf, m2 = inf;
            for (int i = lane; i < L; i += 64) {
                const float d2 = al_d2(X0, X1, X2, Y0, Y1, Y2, i, rot, tr);
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
                next |= al_d2(X0, X1, X2, Y0, Y1, Y2, i, rot, tr) < cut2 ? 1ull << k : 0ull;
            if (!__any(next != mem)) break;
            mem = next;
        }
    }

    if (lane == 0) {
        wrec[wave][0] = best;
        wrec[wave][1] = __int_as_float(bseed);
#pragma unroll
        for (int a = 0; a < 9; ++a) wrec[wave][2 + a] = brot[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) wrec[wave][11 + a] = btr[a];
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
#pragma unroll
    for (int a = 0; a < 9; ++a) m[a] = recs[(size_t)bj * AL_REC + 2 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = recs[(size_t)bj * AL_REC + 11 + a];
    if (mir) { m[6] = -m[6]; m[7] = -m[7]; m[8] = -m[8]; }      // diag(1, 1, -1) @ rot: the fit saw x with its third coordinate negated
    // ---- tm and rmsd under the fp32 transform that is returned, fp64
    const float* xs = planes + (size_t)s * 3 * N;
    const float* ys = planes + (size_t)(self ? r : S + r) * 3 * N;
    const double d0 = al_d0(L), inv_d02 = 1.0 / (d0 * d0);
    double stm = 0.0, sd2 = 0.0;
    for (int i = lane; i < L; i += 64) {
        const double x0 = xs[i], x1 = xs[N + i], x2 = xs[2 * N + i];
        const double e0 = ((double)t[0] + (x0 * m[0] + x1 * m[3] + x2 * m[6])) - (double)ys[i];
        const double e1 = ((double)t[1] + (x0 * m[1] + x1 * m[4] + x2 * m[7])) - (double)ys[N + i];
        const double e2 = ((double)t[2] + (x0 * m[2] + x1 * m[5] + x2 * m[8])) - (double)ys[2 * N + i];
        const double d2 = e0 * e0 + e1 * e1 + e2 * e2;
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
            const int k = al_seed_count(L);
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

    const size_t lds = (size_t)6 * N * sizeof(float);
    if (P.npairs > 0 && lds > 48 * 1024) {              // before anything is enqueued: a refusal leaves nothing launched
        const hipError_t ea = hipFuncSetAttribute((const void*)align_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  6 * PRD_ALIGN_MAX_N * (int)sizeof(float));
        if (ea != hipSuccess) return (int)ea;
    }
    hipLaunchKernelGGL(align_compact_kernel, dim3(P.nstruct), dim3(AL_COMPACT_WG), 0, stream, planes, hdr, x, x_struct_stride, x_row_stride,
                       self ? x : y, self ? x_struct_stride : y_struct_stride, self ? x_row_stride : y_row_stride, mask, S, N);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (P.npairs > 0) {
        hipLaunchKernelGGL(align_search_kernel, dim3((unsigned)(P.npairs * P.nm), P.G), dim3(64 * P.nw), lds, stream, rec, planes, hdr, S, R, N,
                           self ? 1 : 0, mode, P.nm, P.G);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    const long nblocks = P.npairs + (self ? S : 0);
    hipLaunchKernelGGL(align_finalize_kernel, dim3((unsigned)nblocks), dim3(64), 0, stream, tm, rmsd, rot, trans, mirrored, rec, planes, hdr, S, R, N,
                       self ? 1 : 0, P.nm, P.G, P.npairs);
    return (int)hipGetLastError();
}

extern "C" int prd_align_apply(float* out, const float* pos, const float* rot, const float* trans, int S, int N, hipStream_t stream) {
    if (!out || !pos || !rot || !trans || S <= 0 || N <= 0) return PRD_ALIGN_ERR_ARG;
    if (S > 65535) return PRD_ALIGN_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(align_apply_kernel, dim3((N + 255) / 256, S), dim3(256), 0, stream, out, pos, rot, trans, N);
    return (int)hipGetLastError();
}
