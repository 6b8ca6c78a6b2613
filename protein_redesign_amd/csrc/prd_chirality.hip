// The handedness census of generated samples on the device (include/prd_chirality.h): local chirality read off the sample itself.
//   chirality_census_kernel   grid S, CH_THREADS = 256 threads: ONE workgroup owns a sample, so its eight counts are summed in a fixed
//                             order by itself and the verdict is taken in the same launch.  The rows pass through the LDS in
//                             tiles of CH_TILE = 256 with a halo of CH_HALO = 3: each thread stages {x, y, z, mask} of one row as one
//                             float4 and its link flag (the first three threads also stage the halo), then thread t classifies the quad
//                             that row tile + t starts from four consecutive float4 reads -- lane l reads slots l .. l + 3, no bank
//                             conflict.  A coordinate is read from memory once per tile it belongs to (a halo row twice).  After the
//                             rows the threads stride over the ligand's centres, twelve coordinates each, straight from memory.  The
//                             counts meet through wave shuffles and CH_WAVES x 8 ints of LDS; thread 0 adds the waves in order,
//                             writes counts and takes the verdict.  Static LDS only: CH_LDS_BYTES.
//   chirality_reflect_kernel  grid (row tiles, S): the sign bit of coordinate 0 of the structures whose flag is set.  No LDS.
// A sample is N * 28 bytes read and N * 8 written: at S = 64, N = 384 the census is 64 workgroups of two tiles.  It is sized for the
// post-processing of a few hundred samples, not for throughput: S = 1 runs on one compute unit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/prd_chirality.h"
#include "prd_launch.h"

namespace {

constexpr int CH_THREADS = 256;                 // threads of a workgroup
constexpr int CH_WAVES = CH_THREADS / 64;
constexpr int CH_TILE = CH_THREADS;             // rows of a tile: one quad start per thread
constexpr int CH_HALO = 3;                      // the rows after a tile that its last quads reach
constexpr int CH_COUNTS = 8;                    // columns of counts (prd_chirality.h)
constexpr int CH_LDS_BYTES = 5312;              // the census kernel's static LDS: the struct below

struct ChShared {
    float4 p[CH_TILE + CH_HALO];                // {x, y, z, mask} of the tile's rows and the halo
    float link[CH_TILE + CH_HALO + 1];          // link of the same rows (one spare element keeps the struct a multiple of 16 bytes)
    int red[CH_WAVES][CH_COUNTS];               // the waves' partial counts
};
static_assert(sizeof(ChShared) == CH_LDS_BYTES, "CH_LDS_BYTES states the census kernel's LDS");

struct ChWindows {                              // prd_chirality.h: the class windows, the squared bond window, the flat volume
    float hc_lo, hc_hi, ht_lo, ht_hi, ec_lo, ec_hi, et_lo, et_hi, b2_lo, b2_hi, vmin;
};

__device__ __forceinline__ float ch_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;       // -ffp-contract=off: no fused multiply-add
}

__global__ __launch_bounds__(CH_THREADS) void chirality_census_kernel(
    int* __restrict__ counts, int* __restrict__ verdict, int* __restrict__ basis, float* __restrict__ tau, int* __restrict__ cls,
    float* __restrict__ volume, const float* __restrict__ x, long long x_ss, int x_rs, const float* __restrict__ mask,
    const float* __restrict__ link, const int* __restrict__ centres, const float* __restrict__ centre_ref, int C, ChWindows w,
    int min_helix, int min_extended, int N) {
    __shared__ ChShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.x;
    const float* xs = x + (long long)s * x_ss;
    int cnt[CH_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r0 = 0; r0 < N; r0 += CH_TILE) {
        if (r0 > 0) __syncthreads();            // the tile before has been read by everyone
        for (int k = tid; k < CH_TILE + CH_HALO; k += CH_THREADS) {
            const int j = r0 + k;
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f);         // past the end: unmasked, unlinked
            float l = 0.f;
            if (j < N) {
                const float* px = xs + (long long)j * x_rs;
                p = make_float4(px[0], px[1], px[2], mask[j]);
                l = link[j];
            }
            sh.p[k] = p;
            sh.link[k] = l;
        }
        __syncthreads();
        const int i = r0 + tid;
        if (i < N) {
            const float4 p0 = sh.p[tid], p1 = sh.p[tid + 1], p2 = sh.p[tid + 2], p3 = sh.p[tid + 3];
            bool valid = p0.w > 0.5f && p1.w > 0.5f && p2.w > 0.5f && p3.w > 0.5f && sh.link[tid] > 0.5f && sh.link[tid + 1] > 0.5f &&
                         sh.link[tid + 2] > 0.5f;               // a row past the end is staged unmasked: i + 3 < N is implied
            const float b1x = p1.x - p0.x, b1y = p1.y - p0.y, b1z = p1.z - p0.z;
            const float b2x = p2.x - p1.x, b2y = p2.y - p1.y, b2z = p2.z - p1.z;
            const float b3x = p3.x - p2.x, b3y = p3.y - p2.y, b3z = p3.z - p2.z;
            const float l1 = ch_dot(b1x, b1y, b1z, b1x, b1y, b1z), l2 = ch_dot(b2x, b2y, b2z, b2x, b2y, b2z), l3 = ch_dot(b3x, b3y, b3z, b3x, b3y, b3z);
            valid = valid && l1 > w.b2_lo && l1 < w.b2_hi && l2 > w.b2_lo && l2 < w.b2_hi && l3 > w.b2_lo && l3 < w.b2_hi;
            float t = __builtin_nanf("");
            int c = 0;
            if (valid) {
                const float n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
                const float n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
                const float d1 = sqrtf(l1), d2 = sqrtf(l2), d3 = sqrtf(l3);
                const float yy = d2 * ch_dot(b1x, b1y, b1z, n2x, n2y, n2z), xx = ch_dot(n1x, n1y, n1z, n2x, n2y, n2z);
                const float at = atan2f(fabsf(yy), xx);         // in [0, pi]; the sign goes on afterwards: odd in yy to the bit
                t = copysignf(at, yy);
                const float c1 = -ch_dot(b1x, b1y, b1z, b2x, b2y, b2z) / (d1 * d2), c2 = -ch_dot(b2x, b2y, b2z, b3x, b3y, b3z) / (d2 * d3);
                const bool plus = t > 0.f, minus = t < 0.f;     // +-0 is neither
                if (c1 > w.hc_lo && c1 < w.hc_hi && c2 > w.hc_lo && c2 < w.hc_hi && at > w.ht_lo && at < w.ht_hi) c = plus ? 1 : minus ? 2 : 0;
                else if (c1 > w.ec_lo && c1 < w.ec_hi && c2 > w.ec_lo && c2 < w.ec_hi && at > w.et_lo && at < w.et_hi) c = minus ? 3 : plus ? 4 : 0;
                cnt[4] += 1;
                cnt[0] += c == 1; cnt[1] += c == 2; cnt[2] += c == 3; cnt[3] += c == 4;
            }
            if (tau) tau[(size_t)s * N + i] = t;
            if (cls) cls[(size_t)s * N + i] = c;
        }
    }
    for (int k = tid; k < C; k += CH_THREADS) {                 // the centres: rows validated on the host (prd_chirality.h)
        const float* pc = xs + (long long)centres[4 * k] * x_rs;
        const float* pa = xs + (long long)centres[4 * k + 1] * x_rs;
        const float* pb = xs + (long long)centres[4 * k + 2] * x_rs;
        const float* pd = xs + (long long)centres[4 * k + 3] * x_rs;
        const float cx = pc[0], cy = pc[1], cz = pc[2];
        const float ax = pa[0] - cx, ay = pa[1] - cy, az = pa[2] - cz;
        const float bx = pb[0] - cx, by = pb[1] - cy, bz = pb[2] - cz;
        const float dx = pd[0] - cx, dy = pd[1] - cy, dz = pd[2] - cz;
        const float v = ch_dot(ax, ay, az, by * dz - bz * dy, bz * dx - bx * dz, bx * dy - by * dx);
        if (volume) volume[(size_t)s * C + k] = v;
        if (!(fabsf(v) >= w.vmin)) cnt[7] += 1;                 // a NaN volume is flat
        else if (centre_ref) {
            const bool same = (v > 0.f) == (centre_ref[k] > 0.f);
            cnt[5] += same;
            cnt[6] += !same;
        }
    }
#pragma unroll
    for (int k = 0; k < CH_COUNTS; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < CH_COUNTS; ++k) sh.red[wave][k] = cnt[k];
    }
    __syncthreads();
    if (tid == 0) {
        int tot[CH_COUNTS];
#pragma unroll
        for (int k = 0; k < CH_COUNTS; ++k) {
            tot[k] = (sh.red[0][k] + sh.red[1][k]) + (sh.red[2][k] + sh.red[3][k]);
            counts[(size_t)s * CH_COUNTS + k] = tot[k];
        }
        const int h = tot[0] - tot[1], e = tot[2] - tot[3];
        int v = 0, b = PRD_CHIRALITY_BASIS_NONE;
        if (h != 0 && (h < 0 ? -h : h) >= min_helix) v = h > 0 ? 1 : -1, b = PRD_CHIRALITY_BASIS_HELIX;
        else if (centre_ref && tot[5] + tot[6] >= 1 && (tot[5] == 0 || tot[6] == 0)) v = tot[6] == 0 ? 1 : -1, b = PRD_CHIRALITY_BASIS_CENTRES;
        else if (e != 0 && (e < 0 ? -e : e) >= min_extended) v = e > 0 ? 1 : -1, b = PRD_CHIRALITY_BASIS_EXTENDED;
        verdict[s] = v;
        basis[s] = b;
    }
}

__global__ __launch_bounds__(CH_THREADS) void chirality_reflect_kernel(float* __restrict__ x, long long x_ss, int x_rs, const int* __restrict__ flip, int N) {
    const int i = blockIdx.x * CH_THREADS + threadIdx.x, s = blockIdx.y;
    if (i < N && flip[s] != 0) {
        float* p = x + (long long)s * x_ss + (long long)i * x_rs;
        *p = -*p;                                               // the sign bit alone, NaN payloads included
    }
}

bool ch_finite(float v) { return v > -__builtin_inff() && v < __builtin_inff(); }     // NaN fails both comparisons

// 0, or the refusal the two entry points share
int chirality_refuse(const float* x, long long x_ss, int x_rs, int S, int N) {
    if (!x || S <= 0 || N <= 0 || x_rs < 3 || x_ss < 0) return PRD_CHIRALITY_ERR_ARG;
    if (N > PRD_CHIRALITY_MAX_N || S > PRD_CHIRALITY_MAX_S) return PRD_CHIRALITY_ERR_UNSUPPORTED;
    return 0;
}

bool ch_window(float lo, float hi, float least, float most) { return ch_finite(lo) && ch_finite(hi) && lo >= least && hi <= most && lo < hi; }

}  // namespace

extern "C" int prd_chirality_version(void) { return PRD_CHIRALITY_VERSION; }

extern "C" int prd_chirality_census(int* counts, int* verdict, int* basis, float* tau, int* cls, float* volume, const float* x,
                                    long long x_struct_stride, int x_row_stride, const float* mask, const float* link, const int* centres,
                                    const int* centres_host, const float* centre_ref, int C, float helix_cos_lo, float helix_cos_hi,
                                    float helix_tau_lo, float helix_tau_hi, float ext_cos_lo, float ext_cos_hi, float ext_tau_lo,
                                    float ext_tau_hi, float bond_lo, float bond_hi, float vmin, int min_helix, int min_extended, int S, int N,
                                    hipStream_t stream) {
    if (!counts || !verdict || !basis || !mask || !link || C < 0 || min_helix < 0 || min_extended < 0) return PRD_CHIRALITY_ERR_ARG;
    const int refused = chirality_refuse(x, x_struct_stride, x_row_stride, S, N);
    if (refused == PRD_CHIRALITY_ERR_ARG) return refused;
    const float pi = 3.14159274f;                               // fp32 pi, the largest value the arc tangent returns
    if (!ch_window(helix_cos_lo, helix_cos_hi, -1.f, 1.f) || !ch_window(ext_cos_lo, ext_cos_hi, -1.f, 1.f) ||
        !ch_window(helix_tau_lo, helix_tau_hi, 0.f, pi) || !ch_window(ext_tau_lo, ext_tau_hi, 0.f, pi))
        return PRD_CHIRALITY_ERR_ARG;
    if (!ch_finite(bond_lo) || !ch_finite(bond_hi) || !(bond_lo > 0.f) || !(bond_lo < bond_hi)) return PRD_CHIRALITY_ERR_ARG;
    if (!ch_finite(vmin) || !(vmin > 0.f)) return PRD_CHIRALITY_ERR_ARG;
    if (C > 0 && (!centres || !centres_host)) return PRD_CHIRALITY_ERR_ARG;
    if (refused) return refused;
    if (C > PRD_CHIRALITY_MAX_C) return PRD_CHIRALITY_ERR_UNSUPPORTED;
    for (int k = 0; k < 4 * C; ++k)                             // the host copy: no row outside [0, N) reaches the kernel
        if (centres_host[k] < 0 || centres_host[k] >= N) return PRD_CHIRALITY_ERR_ARG;
    const ChWindows w = {helix_cos_lo, helix_cos_hi, helix_tau_lo, helix_tau_hi, ext_cos_lo, ext_cos_hi, ext_tau_lo, ext_tau_hi,
                         bond_lo * bond_lo, bond_hi * bond_hi, vmin};
    return prd_launch<chirality_census_kernel>(dim3(S), dim3(CH_THREADS), 0, stream, counts, verdict, basis, tau, cls, C > 0 ? volume : nullptr, x,
                                               x_struct_stride, x_row_stride, mask, link, centres, C > 0 ? centre_ref : nullptr, C, w,
                                               min_helix, min_extended, N);
}

extern "C" int prd_chirality_reflect(float* x, long long x_struct_stride, int x_row_stride, const int* flip, int S, int N, hipStream_t stream) {
    if (!flip) return PRD_CHIRALITY_ERR_ARG;
    const int refused = chirality_refuse(x, x_struct_stride, x_row_stride, S, N);
    if (refused) return refused;
    return prd_launch<chirality_reflect_kernel>(dim3((N + CH_THREADS - 1) / CH_THREADS, S), dim3(CH_THREADS), 0, stream, x, x_struct_stride,
                                                x_row_stride, flip, N);
}
