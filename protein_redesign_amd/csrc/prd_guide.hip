// Guided sampling on the device (include/prd_guide.h): the gradient of a clash and restraint energy, evaluated on the step's own
// clean-structure estimate x0 = q (z - r eps), added to the predicted noise in ONE launch between the network and the step boundary.
//   guide_eps_kernel   grid b * ceil(N / GD_ROWS), GD_ROWS * GD_LANES = 256 threads, static LDS only (the column tile: 4 KiB).
//                      A workgroup owns GD_ROWS = 64 rows of one sample, GD_LANES = 4 lanes per row.  Every workgroup recomputes the
//                      masked mean of its sample (four sums over N, in the order the boundary kernels sum them: cheaper than a second
//                      launch).  The columns are swept in tiles of GD_TILE = 256: each thread computes the estimate of one column and
//                      stages {x, y, z, class} as one float4, then lane l of a row visits the columns l, l + 4, ... of the tile in
//                      ascending order (a wave reads four distinct LDS addresses per step: broadcasts, no bank conflict).  After the
//                      tiles lane l visits the entries l, l + 4, ... of the row's own restraint list.  The four partial sums of a row
//                      are combined as (l0 + l1) + (l2 + l3): every sum has a fixed order, equal inputs give equal bits.
// The work is N * N / 4 distances per 64 rows: at N = 769 a thread visits 193 columns.  The kernel is one of 74 launches of a step and
// is sized for latency, not throughput: at b = 1, N = 320 it is five workgroups.
// A sample whose counter is outside [0, rows) is left alone by every workgroup of it: no table row is read, nothing is written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_guide.h"
#include "prd_launch.h"

namespace {

// the geometry, stated once: the kernel, its LDS and the host's grid all read these
constexpr int GD_LANES = 4;                          // lanes per row
constexpr int GD_ROWS = 64;                          // rows per workgroup
constexpr int GD_THREADS = GD_ROWS * GD_LANES;       // 256
constexpr int GD_TILE = GD_THREADS;                  // columns per tile: one per thread
constexpr float GD_COINCIDENT = 1e-12f;              // d^2 below this: the pair contributes nothing

// the boundary's own clean-structure estimate of row g (prd_solver.hip: npred = eps - m * mean / count; x0 = q * (z - r * npred))
__device__ __forceinline__ void gd_estimate(const float* __restrict__ z, const float* __restrict__ ep, long g, float m, const float* mean,
                                            float q, float r, float& x, float& y, float& w) {
    const float nx = ep[g * 3] - m * mean[0] / mean[3], ny = ep[g * 3 + 1] - m * mean[1] / mean[3], nz = ep[g * 3 + 2] - m * mean[2] / mean[3];
    x = q * (z[g * 3] - r * nx);
    y = q * (z[g * 3 + 1] - r * ny);
    w = q * (z[g * 3 + 2] - r * nz);
}

__device__ __forceinline__ int gd_class(int c, float m) { return (m > 0.5f && (c == 1 || c == 2)) ? c : 0; }

__global__ __launch_bounds__(GD_THREADS) void guide_eps_kernel(
    const float* __restrict__ z, const float* __restrict__ eps_raw, float* __restrict__ eps_out, const float* __restrict__ mask,
    const int64_t* __restrict__ counter, const float* __restrict__ table, const int* __restrict__ cls, const float* __restrict__ floors,
    const float* __restrict__ wclash, const uint8_t* __restrict__ exclude, const int* __restrict__ rs_ptr, const int* __restrict__ rs_j,
    const float* __restrict__ rs_par, float* __restrict__ e_out, int N, int rows, int R, int nblk) {
    __shared__ float4 tile[GD_TILE];              // {x, y, z, class as bits} of the tile's columns
    __shared__ float red[GD_THREADS / 64][4];
    __shared__ float mean[4];                     // masked sums of eps_raw (3) and the count
    const int bb = blockIdx.x / nblk, blk = blockIdx.x - bb * nblk;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long kk = counter ? (long)counter[bb] : 0;
    if (kk < 0 || kk >= rows) return;             // uniform over the workgroup
    const float4 co = reinterpret_cast<const float4*>(table)[kk];
    const float q = co.x, r = co.y, lam = co.z, cap = co.w;
    const long base = (long)bb * N;
    const float* ep = eps_raw + base * 3;
    const float* zp = z + base * 3;
    const float* mp = mask + base;
    {   // masked sums over ALL rows of the sample, in the boundary's order
        float s4[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < N; i += GD_THREADS) {
            const float m = mp[i];
            s4[0] += m * ep[i * 3]; s4[1] += m * ep[i * 3 + 1]; s4[2] += m * ep[i * 3 + 2];
            s4[3] += m;
        }
#pragma unroll
        for (int d = 0; d < 4; ++d) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s4[d] += __shfl_xor(s4[d], o);
            if (lane == 0) red[wave][d] = s4[d];
        }
        __syncthreads();
        if (tid < 4) mean[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        __syncthreads();
    }
    const int l = tid & (GD_LANES - 1), i = blk * GD_ROWS + tid / GD_LANES;
    const bool ok = i < N;
    float xi = 0.f, yi = 0.f, wi = 0.f, mi = 0.f;
    int ci = 0;
    if (ok) {
        mi = mp[i];
        gd_estimate(zp, ep, i, mi, mean, q, r, xi, yi, wi);
        ci = gd_class(cls[base + i], mi);
    }
    const float f0 = floors[0], f1 = floors[1], f2 = floors[2], w0 = wclash[0], w1 = wclash[1], w2 = wclash[2];
    float gx = 0.f, gy = 0.f, gz = 0.f, ec = 0.f, er = 0.f;
    const bool sweep = lam != 0.f || e_out != nullptr;         // uniform over the launch's sample
    if (sweep) {
        for (int j0 = 0; j0 < N; j0 += GD_TILE) {
            if (j0 > 0) __syncthreads();                       // the previous tile has been read by everyone
            {
                const int j = j0 + tid;
                float x = 0.f, y = 0.f, w = 0.f;
                int cj = 0;
                if (j < N) {
                    const float m = mp[j];
                    gd_estimate(zp, ep, j, m, mean, q, r, x, y, w);
                    cj = gd_class(cls[base + j], m);
                }
                tile[tid] = make_float4(x, y, w, __int_as_float(cj));
            }
            __syncthreads();
            if (ci != 0) {
                const int n = N - j0 < GD_TILE ? N - j0 : GD_TILE;
                for (int u = l; u < n; u += GD_LANES) {
                    const float4 tj = tile[u];
                    const int cj = __float_as_int(tj.w), j = j0 + u;
                    if (cj == 0 || j == i) continue;
                    const float dx = xi - tj.x, dy = yi - tj.y, dz = wi - tj.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const int c = ci + cj - 2;
                    const float f = c == 0 ? f0 : c == 1 ? f1 : f2;
                    if (d2 >= GD_COINCIDENT && d2 < f * f) {
                        if (exclude && exclude[(base + i) * N + j]) continue;
                        const float d = sqrtf(d2), h = f - d;
                        if (h > 0.f) {
                            const float w = c == 0 ? w0 : c == 1 ? w1 : w2;
                            const float s = -(w * h) / d;      // dE/dx_i = -w (f - d) (x_i - x_j) / d
                            gx += s * dx; gy += s * dy; gz += s * dz;
                            ec += 0.25f * w * (h * h);
                        }
                    }
                }
            }
        }
        if (rs_ptr && ok) {                                    // the row's own restraints, in list order
            int p0 = rs_ptr[bb * (N + 1) + i], p1 = rs_ptr[bb * (N + 1) + i + 1];
            if (p0 < 0) p0 = 0;
            if (p1 > R) p1 = R;
            for (int p = p0 + l; p < p1; p += GD_LANES) {
                const int j = rs_j[p];
                if (j < 0 || j >= N || j == i) continue;
                const float4 par = reinterpret_cast<const float4*>(rs_par)[p];      // {lo, hi, w, 0}
                float x, y, w;
                gd_estimate(zp, ep, j, mp[j], mean, q, r, x, y, w);
                const float dx = xi - x, dy = yi - y, dz = wi - w;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 < GD_COINCIDENT) continue;
                const float d = sqrtf(d2);
                const float over = fmaxf(0.f, d - par.y), under = fmaxf(0.f, par.x - d);
                const float s = par.z * (over - under) / d;    // dE/dx_i = w (over - under) (x_i - x_j) / d
                gx += s * dx; gy += s * dy; gz += s * dz;
                er += 0.25f * par.z * (over * over + under * under);
            }
        }
        // the four lanes of a row: (l0 + l1) + (l2 + l3), the same bits in every lane
#pragma unroll
        for (int o = 1; o < GD_LANES; o <<= 1) {
            gx += __shfl_xor(gx, o); gy += __shfl_xor(gy, o); gz += __shfl_xor(gz, o);
            ec += __shfl_xor(ec, o); er += __shfl_xor(er, o);
        }
    }
    if (ok && l == 0) {
        float ddx = lam * gx, ddy = lam * gy, ddz = lam * gz;
        const float nrm = sqrtf((ddx * ddx + ddy * ddy) + ddz * ddz);
        if (nrm > cap) {
            const float sc = cap / nrm;
            ddx *= sc; ddy *= sc; ddz *= sc;
        }
        const long g = (base + i) * 3;
        const float e0 = ep[i * 3], e1 = ep[i * 3 + 1], e2 = ep[i * 3 + 2];
        const bool copy = lam == 0.f;                          // to the bit, -0 included
        eps_out[g] = copy ? e0 : e0 + mi * ddx;
        eps_out[g + 1] = copy ? e1 : e1 + mi * ddy;
        eps_out[g + 2] = copy ? e2 : e2 + mi * ddz;
        if (e_out) {
            e_out[(base + i) * 2] = ec;
            e_out[(base + i) * 2 + 1] = er;
        }
    }
}

}  // namespace

extern "C" int prd_guide_version(void) { return PRD_GUIDE_VERSION; }

extern "C" int prd_guide_eps(const float* z, const float* eps_raw, float* eps_out, const float* mask, const int64_t* counter,
                             const float* table, const int* cls, const float* floors, const float* wclash, const uint8_t* exclude,
                             const int* rs_ptr, const int* rs_j, const float* rs_par, float* e_out, int b, int N, int rows, int R,
                             hipStream_t stream) {
    if (!z || !eps_raw || !eps_out || !mask || !table || !cls || !floors || !wclash || b < 1 || N < 1 || rows < 1) return PRD_GUIDE_ERR_ARG;
    const bool csr = rs_ptr || rs_j || rs_par;
    if (csr && (!rs_ptr || !rs_j || !rs_par || R < 1)) return PRD_GUIDE_ERR_ARG;
    if (b > PRD_GUIDE_MAX_B || N > PRD_GUIDE_MAX_N || rows > PRD_GUIDE_MAX_ROWS || (csr && R > PRD_GUIDE_MAX_R)) return PRD_GUIDE_ERR_UNSUPPORTED;
    {   // eps_out is written while other workgroups still read eps_raw: the two must not share a byte
        const uintptr_t a = (uintptr_t)eps_raw, o = (uintptr_t)eps_out, bytes = (uintptr_t)b * N * 3 * sizeof(float);
        if ((a <= o ? o - a : a - o) < bytes) return PRD_GUIDE_ERR_ARG;
    }
    if (((uintptr_t)table & 15) || (csr && ((uintptr_t)rs_par & 15))) return PRD_GUIDE_ERR_ALIGN;
    // grid <= MAX_B * MAX_N / GD_ROWS = 2^19; b * N * N <= 2^38 is indexed in long, b * (N + 1) fits an int
    const int nblk = (N + GD_ROWS - 1) / GD_ROWS;
    return prd_launch<guide_eps_kernel>(dim3(b * nblk), dim3(GD_THREADS), 0, stream, z, eps_raw, eps_out, mask, counter, table, cls, floors,
                                        wclash, exclude, rs_ptr, rs_j, rs_par, e_out, N, rows, csr ? R : 0, nblk);
}
