// Superposition-free scores of generated samples on the device (include/prd_quality.h): lDDT counts and pair censuses, each one
// launch that sweeps the N x N distances of every structure and keeps its counts in registers.
//   quality_lddt_kernel      grid (row tiles, S).  A workgroup owns Q_ROWS = 64 rows of one sample: lane l of EVERY wave holds row
//                            tile * 64 + l of the sample and of the reference in registers.  The columns pass through the LDS in tiles of
//                            Q_COLS = 256 (one float4 of the sample and one of the reference per column, staged by the 256 threads, one
//                            column each); wave w sweeps the w-th quarter of the tile, every lane reading the SAME column in the same
//                            iteration (a broadcast read, no bank conflict).  The four partial counts of a row meet in the LDS and wave 0
//                            writes them: one owner per output element.
//   quality_contacts_kernel  the same sweep over the sample alone; a column outside B is staged at infinity, so the inner loop tests one
//                            distance and looks at the exclusion matrix only for a pair that would change the minimum or the count.
// No floating-point atomics: the only atomic is one integer add per workgroup onto count[s], which the call zeroed on the same stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/prd_quality.h"
#include "prd_launch.h"

namespace {

constexpr int Q_ROWS = 64;                  // rows of a workgroup: one per lane
constexpr int Q_WAVES = 4;                  // waves of a workgroup: each sweeps a quarter of a column tile
constexpr int Q_COLS = Q_ROWS * Q_WAVES;    // columns of a tile: one per thread when it is staged

__device__ __forceinline__ float q_d2(float ax, float ay, float az, const float4& b) {
    const float dx = ax - b.x, dy = ay - b.y, dz = az - b.z;
    return dx * dx + dy * dy + dz * dz;     // -ffp-contract=off: no fused multiply-add, so d2(i, j) == d2(j, i) bit for bit
}

__global__ __launch_bounds__(Q_COLS) void quality_lddt_kernel(int* __restrict__ preserved, int* __restrict__ total,
                                                             const float* __restrict__ x, long long x_ss, int x_rs,
                                                             const float* __restrict__ y, int y_rs, const float* __restrict__ row_mask,
                                                             const float* __restrict__ col_mask, float r2, int N) {
    __shared__ float4 cs[Q_COLS], cr[Q_COLS];                   // a column of the sample / of the reference; .w unused
    __shared__ int part[2][Q_WAVES][Q_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y;
    const int i = blockIdx.x * Q_ROWS + lane;
    const float* xs = x + (long long)s * x_ss;
    const float inf = __builtin_inff();
    const bool rm = i < N && row_mask[i] > 0.5f;
    float xi0 = 0.f, xi1 = 0.f, xi2 = 0.f, yi0 = 0.f, yi1 = 0.f, yi2 = 0.f;
    if (rm) {
        const float* px = xs + (long long)i * x_rs;
        const float* py = y + (long long)i * y_rs;
        xi0 = px[0], xi1 = px[1], xi2 = px[2];
        yi0 = py[0], yi1 = py[1], yi2 = py[2];
    }
    int pres = 0, tot = 0;
    if (__syncthreads_or(rm)) {                                 // the same for all four waves: they hold the same rows
        for (int c0 = 0; c0 < N; c0 += Q_COLS) {
            const int j = c0 + tid;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = make_float4(inf, inf, inf, 0.f);        // at infinity: never included
            if (j < N && col_mask[j] > 0.5f) {
                const float* px = xs + (long long)j * x_rs;
                const float* py = y + (long long)j * y_rs;
                a = make_float4(px[0], px[1], px[2], 0.f);
                b = make_float4(py[0], py[1], py[2], 0.f);
            }
            __syncthreads();                                    // the sweep of the tile before is over
            cs[tid] = a;
            cr[tid] = b;
            __syncthreads();
            const int base = wave * Q_ROWS, j0 = c0 + base;
            const int kn = N - j0 < Q_ROWS ? N - j0 : Q_ROWS;   // wave-uniform; <= 0: nothing of this quarter is a column
#pragma unroll 4
            for (int k = 0; k < kn; ++k) {
                const float4 p = cs[base + k], q = cr[base + k];
                const float D2 = q_d2(yi0, yi1, yi2, q), d2 = q_d2(xi0, xi1, xi2, p);
                const float diff = fabsf(__builtin_amdgcn_sqrtf(d2) - __builtin_amdgcn_sqrtf(D2));
                const int c = (diff < 0.5f) + (diff < 1.f) + (diff < 2.f) + (diff < 4.f);
                const bool inc = D2 < r2 && j0 + k != i;
                tot += inc ? 1 : 0;
                pres += inc ? c : 0;
            }
        }
    }
    part[0][wave][lane] = rm ? pres : 0;
    part[1][wave][lane] = rm ? tot : 0;
    __syncthreads();
    if (wave == 0 && i < N) {
        preserved[(size_t)s * N + i] = part[0][0][lane] + part[0][1][lane] + part[0][2][lane] + part[0][3][lane];
        if (s == 0) total[i] = part[1][0][lane] + part[1][1][lane] + part[1][2][lane] + part[1][3][lane];
    }
}

__global__ __launch_bounds__(Q_COLS) void quality_contacts_kernel(int* __restrict__ count, float* __restrict__ nearest,
                                                                 const float* __restrict__ x, long long x_ss, int x_rs,
                                                                 const float* __restrict__ a_mask, const float* __restrict__ b_mask,
                                                                 const uint8_t* __restrict__ exclude, float c2, int N) {
    __shared__ float4 cs[Q_COLS];                               // a column of the sample; .w: the bits of 1 when the column is in A
    __shared__ float pmin[Q_WAVES][Q_ROWS];
    __shared__ int pcnt[Q_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y;
    const int i = blockIdx.x * Q_ROWS + lane;
    const float* xs = x + (long long)s * x_ss;
    const float inf = __builtin_inff();
    const bool in_a = i < N && a_mask[i] > 0.5f, in_b = i < N && b_mask[i] > 0.5f;
    float xi0 = 0.f, xi1 = 0.f, xi2 = 0.f;
    if (in_a) {
        const float* px = xs + (long long)i * x_rs;
        xi0 = px[0], xi1 = px[1], xi2 = px[2];
    }
    float near2 = inf;
    int cnt = 0;
    if (__syncthreads_or(in_a)) {
        for (int c0 = 0; c0 < N; c0 += Q_COLS) {
            const int j = c0 + tid;
            float4 a = make_float4(inf, inf, inf, 0.f);         // at infinity: no contact, never the nearest
            if (j < N && b_mask[j] > 0.5f) {
                const float* px = xs + (long long)j * x_rs;
                a = make_float4(px[0], px[1], px[2], __int_as_float(a_mask[j] > 0.5f ? 1 : 0));
            }
            __syncthreads();
            cs[tid] = a;
            __syncthreads();
            const int base = wave * Q_ROWS, j0 = c0 + base;
            const int kn = N - j0 < Q_ROWS ? N - j0 : Q_ROWS;
#pragma unroll 4
            for (int k = 0; k < kn; ++k) {
                const float4 p = cs[base + k];
                const float d2 = q_d2(xi0, xi1, xi2, p);
                const int jj = j0 + k;
                if (in_a && jj != i && (d2 < c2 || d2 < near2)) {           // few pairs get here once a near one has been seen
                    if (!exclude || exclude[(size_t)i * N + jj] == 0) {
                        near2 = fminf(near2, d2);
                        if (d2 < c2) {
                            const bool reverse = in_b && __float_as_int(p.w) != 0 && (!exclude || exclude[(size_t)jj * N + i] == 0);
                            cnt += reverse && jj < i ? 0 : 1;               // a pair that qualifies in both orders: once, from its lower end
                        }
                    }
                }
            }
        }
    }
    pmin[wave][lane] = near2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (lane == 0) pcnt[wave] = cnt;
    __syncthreads();
    if (wave == 0 && i < N)
        nearest[(size_t)s * N + i] = in_a ? sqrtf(fminf(fminf(pmin[0][lane], pmin[1][lane]), fminf(pmin[2][lane], pmin[3][lane]))) : inf;
    if (tid == 0) {
        const int c = pcnt[0] + pcnt[1] + pcnt[2] + pcnt[3];
        if (c) atomicAdd(count + s, c);                         // integer: the order of the workgroups does not change the sum
    }
}

// 0, or the refusal shared by the two operators
int quality_refuse(const float* x, long long x_ss, int x_rs, float bound, int S, int N) {
    if (!x || S <= 0 || N <= 0 || x_rs < 3 || x_ss < 0) return PRD_QUALITY_ERR_ARG;
    if (!(bound > 0.f) || !(bound < __builtin_inff())) return PRD_QUALITY_ERR_ARG;          // NaN fails both comparisons
    if (N > PRD_QUALITY_MAX_N || S > PRD_QUALITY_MAX_S) return PRD_QUALITY_ERR_UNSUPPORTED;
    return 0;
}

}  // namespace

extern "C" int prd_quality_version(void) { return PRD_QUALITY_VERSION; }

extern "C" int prd_quality_lddt(int* preserved, int* total, const float* x, long long x_struct_stride, int x_row_stride,
                                const float* y, int y_row_stride, const float* row_mask, const float* col_mask, float radius,
                                int S, int N, hipStream_t stream) {
    if (!preserved || !total || !y || !row_mask || !col_mask || y_row_stride < 3) return PRD_QUALITY_ERR_ARG;
    const int refused = quality_refuse(x, x_struct_stride, x_row_stride, radius, S, N);
    if (refused) return refused;
    return prd_launch<quality_lddt_kernel>(dim3((N + Q_ROWS - 1) / Q_ROWS, S), dim3(Q_COLS), 0, stream, preserved, total, x, x_struct_stride,
                                           x_row_stride, y, y_row_stride, row_mask, col_mask, radius * radius, N);
}

extern "C" int prd_quality_contacts(int* count, float* nearest, const float* x, long long x_struct_stride, int x_row_stride,
                                    const float* a_mask, const float* b_mask, const uint8_t* exclude, float cutoff, int S, int N,
                                    hipStream_t stream) {
    if (!count || !nearest || !a_mask || !b_mask) return PRD_QUALITY_ERR_ARG;
    const int refused = quality_refuse(x, x_struct_stride, x_row_stride, cutoff, S, N);
    if (refused) return refused;
    PRD_TRY(prd_memset_async(count, 0, (size_t)S * sizeof(int), stream));
    return prd_launch<quality_contacts_kernel>(dim3((N + Q_ROWS - 1) / Q_ROWS, S), dim3(Q_COLS), 0, stream, count, nearest, x, x_struct_stride,
                                               x_row_stride, a_mask, b_mask, exclude, cutoff * cutoff, N);
}
