// The superposition fit, once, for prd_align.hip and prd_tmalign.hip: the seeds of the TM-score search, d0, the least-squares fit from
// 15 sums (Horn's quaternion form by Jacobi sweeps), and what surrounds a fit in both sources -- distances under a transform, the
// 16-float record, the prefix of the compaction.  Device functions only, no kernel and no entry point; each source includes it once,
// and everything here has internal linkage in that source's library.  The two searches themselves (subset word, pairs through an
// index list or not, scalar or vector transforms) are NOT here: they differ for measured reasons.
#ifndef PRD_SUPERPOSE_H
#define PRD_SUPERPOSE_H
#include <hip/hip_runtime.h>

namespace {

#define SP_DEV __device__ __forceinline__

SP_DEV double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
SP_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a value that is the same in every lane of the wave, moved to a scalar register
SP_DEV float sp_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// ---- the seeds of the search (prd_align.h, TM mode, steps 1 and 2) --------------------------------------------------------------
// fragment lengths L, L/2, L/4, ... as long as they exceed 4, then 4 itself (TM-score's own convention: the shortest fragment is 4),
// and for L <= 21 fragments of 3 as well: there d0 is 0.5 while d_cut is never below 3.5, so the rounds cannot shed an outlier of a
// chain that small and the seed itself has to be able to be free of them
__host__ __device__ inline int sp_next_level(int Lf, int L) { return Lf > 4 ? (Lf / 2 > 4 ? Lf / 2 : 4) : (Lf == 4 && L <= 21 ? 3 : 0); }
__host__ __device__ inline int sp_level_count(int L, int Lf) {
    const int step = Lf / 2 > 1 ? Lf / 2 : 1, span = L - Lf;
    return span / step + 1 + (span % step ? 1 : 0);
}
__host__ __device__ inline int sp_seed_count(int L) {
    if (L < 4) return 1;
    int K = 0;
    for (int Lf = L; Lf >= 3; Lf = sp_next_level(Lf, L)) K += sp_level_count(L, Lf);
    return K;
}
// the seeds of the first `maxlev` fragment lengths alone.  An overload of its own, not a defaulted parameter of the one above: the
// level counter would stay live in align_search_kernel and change its code.
__host__ __device__ inline int sp_seed_count(int L, int maxlev) {
    if (L < 4) return 1;
    int K = 0, lev = 0;
    for (int Lf = L; Lf >= 3 && lev < maxlev; Lf = sp_next_level(Lf, L), ++lev) K += sp_level_count(L, Lf);
    return K;
}
// seed -> (first position, length) of its fragment; seed < sp_seed_count(L)
SP_DEV void sp_seed_decode(int L, int seed, int& start, int& len) {
    start = 0;
    len = L;
    if (L < 4) return;
    for (int Lf = L; Lf >= 3; Lf = sp_next_level(Lf, L)) {
        const int c = sp_level_count(L, Lf);
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

SP_DEV double sp_d0(int L) { return L > 21 ? 1.24 * cbrt((double)L - 15.0) - 1.8 : 0.5; }

// ---- the fit -----------------------------------------------------------------------------------------------------------------------
// One Jacobi rotation of the symmetric 4 x 4 matrix A in the (P, Q) plane, accumulated into V.  The ANGLE is computed in fp32 (hardware
// reciprocal and reciprocal square root), the pair (c, s) is then brought back to c^2 + s^2 = 1 in fp64 (first-order correction:
// the fp32 pair is within 1e-7 of the unit circle, what is left is 1e-14) and applied in fp64 with the exact update of A[P][Q] -- an
// orthogonal similarity that merely does not annihilate the element completely.  The eigenvector is normalised in fp64 at the end,
// so the orthogonality of the rotation matrix does not depend on any of this.
template <int P, int Q>
SP_DEV void jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
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
// eigenvalue of a symmetric 4 x 4 matrix; rank-deficient subsets -- three points are always coplanar -- are no special case).
// UNIFORM: every lane computed the same fit, and the 12 outputs go through sp_uniform into scalar registers.  prd_tmalign.hip asks
// for it (its refine kernel needs 40 B of scratch per lane without), prd_align.hip does not (its kernels are tuned as they are).
template <bool UNIFORM>
SP_DEV void kabsch_from_sums(const double (&sx)[3], const double (&sy)[3], const double (&sxy)[9], double n, float (&rot)[9], float (&tr)[3]) {
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
        for (int j = 0; j < 3; ++j) {
            const float v = (float)Qm[j][i];
            if constexpr (UNIFORM) rot[3 * i + j] = sp_uniform(v);
            else rot[3 * i + j] = v;
        }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float v = (float)(my[j] - (mx[0] * Qm[j][0] + mx[1] * Qm[j][1] + mx[2] * Qm[j][2]));
        if constexpr (UNIFORM) tr[j] = sp_uniform(v);
        else tr[j] = v;
    }
}

// keep the three smallest of (a <= b <= c) and v
SP_DEV void keep3(float& a, float& b, float& c, float v) {
    if (v < c) {
        c = v;
        if (c < b) { const float t = b; b = c; c = t; }
        if (b < a) { const float t = a; a = b; b = t; }
    }
}

// ---- what a fit reads and what it leaves ---------------------------------------------------------------------------------------------
// the two coordinate sets of a workgroup in the LDS, as planes
struct Coords {
    const float *X0, *X1, *X2, *Y0, *Y1, *Y2;
};

// squared distance of x_i and y_j under (rot, tr), fp32
SP_DEV float sp_d2(const Coords& c, int i, int j, const float (&rot)[9], const float (&tr)[3]) {
    const float x0 = c.X0[i], x1 = c.X1[i], x2 = c.X2[i];
    const float e0 = (tr[0] + (x0 * rot[0] + x1 * rot[3] + x2 * rot[6])) - c.Y0[j];
    const float e1 = (tr[1] + (x0 * rot[1] + x1 * rot[4] + x2 * rot[7])) - c.Y1[j];
    const float e2 = (tr[2] + (x0 * rot[2] + x1 * rot[5] + x2 * rot[8])) - c.Y2[j];
    return e0 * e0 + e1 * e1 + e2 * e2;
}

// the same distance in fp64 from planes in global memory (structures of nx and ny positions per plane): what the finalize passes report
SP_DEV double sp_d2_f64(const float* xs, int nx, int i, const float* ys, int ny, int j, const float (&m)[9], const float (&t)[3]) {
    const double x0 = xs[i], x1 = xs[nx + i], x2 = xs[2 * nx + i];
    const double e0 = ((double)t[0] + (x0 * m[0] + x1 * m[3] + x2 * m[6])) - (double)ys[j];
    const double e1 = ((double)t[1] + (x0 * m[1] + x1 * m[4] + x2 * m[7])) - (double)ys[ny + j];
    const double e2 = ((double)t[2] + (x0 * m[2] + x1 * m[5] + x2 * m[8])) - (double)ys[2 * ny + j];
    return e0 * e0 + e1 * e1 + e2 * e2;
}

// a record, in the LDS or in the workspace: score, key (the bits of an int: seed, offset or pair count), rot[9], trans[3], 2 unused
constexpr int SP_REC = 16;
SP_DEV void sp_record_write(float* rec, float score, int key, const float (&rot)[9], const float (&tr)[3]) {
    rec[0] = score;
    rec[1] = __int_as_float(key);
#pragma unroll
    for (int a = 0; a < 9; ++a) rec[2 + a] = rot[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) rec[11 + a] = tr[a];
}
SP_DEV void sp_record_transform(const float* rec, float (&rot)[9], float (&tr)[3]) {
#pragma unroll
    for (int a = 0; a < 9; ++a) rot[a] = rec[2 + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) tr[a] = rec[11 + a];
}

// diag(1, 1, -1) @ rot: the fit saw x with its third coordinate negated
SP_DEV void sp_unmirror(float (&rot)[9]) {
    rot[6] = -rot[6];
    rot[7] = -rot[7];
    rot[8] = -rot[8];
}

// ---- compaction of the masked rows ---------------------------------------------------------------------------------------------------
// thread tid of a workgroup of SP_COMPACT_WG owns the rows [tid * own, (tid + 1) * own) of a mask of N rows: the number of masked rows
// before its own, which is the compacted position of its first one, and the number of them all.  One barrier; cnt is in the LDS.
constexpr int SP_COMPACT_WG = 256;
SP_DEV int sp_compact_start(int (&cnt)[SP_COMPACT_WG], const float* mask, int own, int N, int& total) {
    const int tid = threadIdx.x, i0 = tid * own;
    int c = 0;
    for (int i = i0; i < i0 + own && i < N; ++i) c += mask[i] > 0.5f ? 1 : 0;
    cnt[tid] = c;
    __syncthreads();
    int pos = 0;
    total = 0;
    for (int j = 0; j < SP_COMPACT_WG; ++j) {
        const int v = cnt[j];
        pos += j < tid ? v : 0;
        total += v;
    }
    return pos;
}
// row p of the source -> position pos of the three planes of N floats at dst
SP_DEV void sp_put_row(float* dst, int N, int pos, const float* p) {
    dst[pos] = p[0];
    dst[N + pos] = p[1];
    dst[2 * N + pos] = p[2];
}

}  // namespace
#endif
