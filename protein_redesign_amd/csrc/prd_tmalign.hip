// Structural alignment of generated samples to references of another length on the device (include/prd_tmalign.h states the
// algorithm, a cut of TM-align; tests/tmalign_ref.py restates it in float64).  Four launches per call:
//   1. tmalign_compact_kernel   one workgroup per structure: the masked rows, in order, as three coordinate planes in the workspace;
//                               Lx, Ly, the compacted position of every row of X and the row of every compacted position of Y.
//   2. tmalign_refine_kernel    one workgroup per (pair, mirror, initial alignment): both coordinate sets stay in the LDS, the
//                               workgroup builds its initial alignment and runs the whole refinement loop.  The DP is an
//                               anti-diagonal wavefront: thread t owns rows t + 1, t + 1 + 512, ... and fills the cell of each on the
//                               current diagonal; three diagonals of val (fp64) / diag live in the LDS, indexed by row; scores are
//                               formed on the fly from the transformed coordinates; directions are packed 2 bits per cell into the
//                               workspace (a thread collects the 16 cells of a word of its row in a register and stores the word
//                               once); one lane walks the traceback.  The fits are the waves' seed walks of prd_align.h over the
//                               aligned pairs.  No workgroup waits on another.
//   3. tmalign_search_kernel    one workgroup per (pair, mirror): the best of the three refinements, the d8 filter, the full search.
//   4. tmalign_finalize_kernel  one wave per pair: the better mirror, tm / rmsd / n_aligned in fp64, the mapping in the caller's rows.
// The seeds, d0, the fit and the record are those of prd_align.hip: both include prd_superpose.h, and this source asks the fit for
// its outputs in scalar registers (kabsch_from_sums<true>).  The walk over the seeds is its own.
// One owner per output element, plain vector stores, no atomics; every loop over rounds, cut-offs or traceback steps is bounded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_tmalign.h"
#include "prd_launch.h"
#include "prd_superpose.h"

namespace {

#define TA_DEV __device__ __forceinline__

constexpr int TA_COMPACT_WG = SP_COMPACT_WG;    // threads of a compaction workgroup; each owns TA_OWN consecutive rows
constexpr int TA_OWN = PRD_TMALIGN_MAX_N / TA_COMPACT_WG;
constexpr int TA_WG = 512;              // threads of a refine / search workgroup
constexpr int TA_NW = TA_WG / 64;
constexpr int TA_ROWS = PRD_TMALIGN_MAX_N / TA_WG;      // DP rows a thread owns at most
constexpr int TA_REC = SP_REC;          // floats of a record; its key is a seed, a threading offset or a number of pairs
constexpr int TA_HDR = 16;              // ints at the head of the workspace; [0] = Lx, [1] = Ly
constexpr int TA_INITS = 3;
constexpr int TA_MIN_L = 5;
constexpr int TA_DP_ROUNDS = 30;
constexpr int TA_ROUNDS = 20;
constexpr int TA_CUT_RAISES = 4096;
constexpr int TA_ALL_LEVELS = 64;

// the 15 sums of a fit over the pairs (x_i, y_j) that the lanes of one wave add, fp64 (align_search_kernel of prd_align.hip keeps
// them as plain arrays: with this struct it takes 156 registers instead of its 158, and its figures are held where they are)
struct Sums {
    double sx[3], sy[3], sxy[9];
};
TA_DEV void sums_clear(Sums& s) {
#pragma unroll
    for (int a = 0; a < 3; ++a) s.sx[a] = s.sy[a] = 0.0;
#pragma unroll
    for (int a = 0; a < 9; ++a) s.sxy[a] = 0.0;
}
TA_DEV void sums_add(Sums& s, const Coords& c, int i, int j) {
    const double x[3] = {(double)c.X0[i], (double)c.X1[i], (double)c.X2[i]}, y[3] = {(double)c.Y0[j], (double)c.Y1[j], (double)c.Y2[j]};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s.sx[a] += x[a];
        s.sy[a] += y[a];
#pragma unroll
        for (int b = 0; b < 3; ++b) s.sxy[3 * a + b] += x[a] * y[b];
    }
}
TA_DEV void sums_reduce(Sums& s) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s.sx[a] = wave_sum(s.sx[a]);
        s.sy[a] = wave_sum(s.sy[a]);
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) s.sxy[a] = wave_sum(s.sxy[a]);
}

// the waves' records -> the best one in every thread: highest score, then the lowest key (seed or offset).  Two barriers.
TA_DEV float pick_wave_record(float (*wrec)[TA_REC], float best, int key, const float (&brot)[9], const float (&btr)[3], float (&rot)[9],
                              float (&tr)[3], int& okey) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sp_record_write(wrec[wave], best, key, brot, btr);
    __syncthreads();
    int w = 0;
    for (int j = 1; j < TA_NW; ++j) {
        const float sj = wrec[j][0], sw = wrec[w][0];
        if (sj > sw || (sj == sw && __float_as_int(wrec[j][1]) < __float_as_int(wrec[w][1]))) w = j;
    }
    const float sc = sp_uniform(wrec[w][0]);
    okey = __builtin_amdgcn_readfirstlane(__float_as_int(wrec[w][1]));
#pragma unroll
    for (int a = 0; a < 9; ++a) rot[a] = sp_uniform(wrec[w][2 + a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) tr[a] = sp_uniform(wrec[w][11 + a]);
    __syncthreads();
    return sc;
}

// ---- the search of prd_align.h over the n >= 3 pairs (pl[k], amap[pl[k]]), by the whole workgroup: wave w walks seeds w, w + 8, ...
// Returns the best sum of TM terms (-inf when there is none: non-finite input) and its transform, the same in every thread.
TA_DEV float wg_search(const Coords& c, const int* pl, const int* amap, int n, int maxlev, float inv_d02, float d0s, float (*wrec)[TA_REC],
                       float (&rot_out)[9], float (&tr_out)[3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = sp_seed_count(n, maxlev);
    const float inf = __builtin_inff();
    float best = -inf, brot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, btr[3] = {0.f, 0.f, 0.f};
    int bseed = 0x7fffffff;
    for (int seed = wave; seed < K; seed += TA_NW) {                        // wave-uniform
        int start, len;
        sp_seed_decode(n, seed, start, len);
        unsigned mem = 0u;                                                   // bit k: pair lane + 64 k is in the subset (n <= 2048)
        for (int i = lane, k = 0; i < n; i += 64, ++k) mem |= (i >= start && i < start + len) ? 1u << k : 0u;
        float rot[9], tr[3];
        for (int it = 0; it < TA_ROUNDS; ++it) {
            Sums s;
            sums_clear(s);
            float cnt = 0.f;
            for (int i = lane, k = 0; i < n; i += 64, ++k) {
                if ((mem >> k) & 1u) {
                    const int xi = pl[i];
                    sums_add(s, c, xi, amap[xi]);
                    cnt += 1.f;
                }
            }
            cnt = wave_sum(cnt);
            if (cnt < 3.f) break;                                            // only after non-finite input
            sums_reduce(s);
            kabsch_from_sums<true>(s.sx, s.sy, s.sxy, (double)cnt, rot, tr);
            float sc = 0.f, m0 = inf, m1 = inf, m2 = inf;
            for (int i = lane; i < n; i += 64) {
                const int xi = pl[i];
                const float d2 = sp_d2(c, xi, amap[xi], rot, tr);
                sc += __builtin_amdgcn_rcpf(1.f + d2 * inv_d02);
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
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float o0 = __shfl_xor(m0, o), o1 = __shfl_xor(m1, o), o2 = __shfl_xor(m2, o);
                keep3(m0, m1, m2, o0);
                keep3(m0, m1, m2, o1);
                keep3(m0, m1, m2, o2);
            }
            float cut = it == 0 ? d0s - 1.f : d0s + 1.f;
            for (int u = 0; u < TA_CUT_RAISES && !(m2 < cut * cut); ++u) cut += 0.5f;
            const float cut2 = cut * cut;
            unsigned next = 0u;
            for (int i = lane, k = 0; i < n; i += 64, ++k) {
                const int xi = pl[i];
                next |= sp_d2(c, xi, amap[xi], rot, tr) < cut2 ? 1u << k : 0u;
            }
            if (!__any(next != mem)) break;
            mem = next;
        }
    }
    int key;
    return pick_wave_record(wrec, best, bseed, brot, btr, rot_out, tr_out, key);
}

// ---- initial alignment A: gapless threading.  Wave w takes offsets o = w, w + 8, ... (k = o - (Lx - 1)).  Returns k and its fit.
TA_DEV int wg_threading(const Coords& c, int Lx, int Ly, float inv_d02, float (*wrec)[TA_REC], float (&rot_out)[9], float (&tr_out)[3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mn = Lx < Ly ? Lx : Ly, need = mn / 2 > 5 ? mn / 2 : 5;
    float best = -__builtin_inff(), brot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, btr[3] = {0.f, 0.f, 0.f};
    int bo = 0x7fffffff;
    for (int o = wave; o < Lx + Ly - 1; o += TA_NW) {
        const int k = o - (Lx - 1), i0 = k < 0 ? -k : 0, i1 = Lx < Ly - k ? Lx : Ly - k;
        if (i1 - i0 < need) continue;
        Sums s;
        sums_clear(s);
        for (int i = i0 + lane; i < i1; i += 64) sums_add(s, c, i, i + k);
        sums_reduce(s);
        float rot[9], tr[3];
        kabsch_from_sums<true>(s.sx, s.sy, s.sxy, (double)(i1 - i0), rot, tr);
        float sc = 0.f;
        for (int i = i0 + lane; i < i1; i += 64) sc += __builtin_amdgcn_rcpf(1.f + sp_d2(c, i, i + k, rot, tr) * inv_d02);
        sc = wave_sum(sc);
        if (sc > best) {
            best = sc;
            bo = o;
#pragma unroll
            for (int a = 0; a < 9; ++a) brot[a] = rot[a];
#pragma unroll
            for (int a = 0; a < 3; ++a) btr[a] = tr[a];
        }
    }
    int key;
    pick_wave_record(wrec, best, bo, brot, btr, rot_out, tr_out, key);
    if (key == 0x7fffffff) key = Lx - 1;                                    // no finite score (non-finite input): offset 0
    return key - (Lx - 1);
}

// the scratch of a workgroup's DP in the LDS
struct DpLds {
    double* V;              // [3][Nx + 1] val of three diagonals, by row
    unsigned char* F;       // [3][Nx + 1] diag
    int* amap;              // [Nx] the alignment: y position of x position i, or -1
    int* pl;                // [Nx] the aligned x positions, ascending, in pl[Nx - n .. Nx)
    const unsigned char *secx, *secy;
    int* n;                 // number of aligned pairs
};

// amap -> pl, n (one lane)
TA_DEV void wg_list_pairs(const DpLds& L, int Lx, int Nx) {
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        for (int i = Lx - 1; i >= 0; --i)
            if (L.amap[i] >= 0) L.pl[Nx - 1 - c++] = i;
        *L.n = c;
    }
    __syncthreads();
}

// ---- the DP (prd_tmalign.h, step 3) with s_ij = wss [classes equal] + wtm / (1 + |T x_i - y_j|^2 / d0^2) -> amap, pl, n
TA_DEV void wg_dp(const Coords& c, const DpLds& L, unsigned* dirs, int Lx, int Ly, int Nx, int Ny, const float (&rot)[9], const float (&tr)[3],
                  float wss, float wtm, double gap, float inv_d02) {
    const int tid = threadIdx.x, wpr = (Ny + 15) >> 4, ld = Nx + 1;
    float tx[TA_ROWS][3];
    int sx[TA_ROWS];
    unsigned acc[TA_ROWS];
#pragma unroll
    for (int k = 0; k < TA_ROWS; ++k) {
        const int i = tid + k * TA_WG;                                      // position (0-based) of the row tid + 1 + k * TA_WG
        acc[k] = 0u;
        sx[k] = 0;
        tx[k][0] = tx[k][1] = tx[k][2] = 0.f;
        if (i < Lx) {
            const float x0 = c.X0[i], x1 = c.X1[i], x2 = c.X2[i];
            tx[k][0] = tr[0] + (x0 * rot[0] + x1 * rot[3] + x2 * rot[6]);
            tx[k][1] = tr[1] + (x0 * rot[1] + x1 * rot[4] + x2 * rot[7]);
            tx[k][2] = tr[2] + (x0 * rot[2] + x1 * rot[5] + x2 * rot[8]);
            sx[k] = L.secx[i];
        }
    }
    for (int i = tid; i < Lx; i += TA_WG) L.amap[i] = -1;
    int cur = 2, p1 = 1, p2 = 0;                                            // d % 3, (d - 1) % 3, (d - 2) % 3 for d = 2
    for (int d = 2; d <= Lx + Ly; ++d) {
#pragma unroll
        for (int k = 0; k < TA_ROWS; ++k) {
            const int i = tid + 1 + k * TA_WG, j = d - i;
            if (i <= Lx && j >= 1 && j <= Ly) {
                const float e0 = tx[k][0] - c.Y0[j - 1], e1 = tx[k][1] - c.Y1[j - 1], e2 = tx[k][2] - c.Y2[j - 1];
                const float term = 1.f / (1.f + (e0 * e0 + e1 * e1 + e2 * e2) * inv_d02);
                const float s = wss * (sx[k] == (int)L.secy[j - 1] ? 1.f : 0.f) + wtm * term;
                const double D = ((i > 1 && j > 1) ? L.V[p2 * ld + i - 1] : 0.0) + (double)s;
                const double H = (i > 1 ? L.V[p1 * ld + i - 1] : 0.0) + ((i > 1 && L.F[p1 * ld + i - 1]) ? gap : 0.0);
                const double Vv = (j > 1 ? L.V[p1 * ld + i] : 0.0) + ((j > 1 && L.F[p1 * ld + i]) ? gap : 0.0);
                const bool isd = D >= H && D >= Vv;
                const double hv = H >= Vv ? H : Vv;
                L.V[cur * ld + i] = isd ? D : hv;
                L.F[cur * ld + i] = isd ? 1 : 0;
                const unsigned dir = isd ? 0u : (H >= Vv ? 1u : 2u);
                acc[k] |= dir << (2 * ((j - 1) & 15));
                if (((j - 1) & 15) == 15 || j == Ly) {                      // i - 1 < Nx, (j - 1) / 16 < wpr
                    dirs[(size_t)(i - 1) * wpr + ((j - 1) >> 4)] = acc[k];
                    acc[k] = 0u;
                }
            }
        }
        __syncthreads();
        const int t = p2;
        p2 = p1;
        p1 = cur;
        cur = t;
    }
    if (tid == 0) {                                                         // the traceback: at most Nx + Ny steps
        int i = Lx, j = Ly, cnt = 0;
        for (int step = 0; step < Nx + Ny && i > 0 && j > 0; ++step) {
            const unsigned w = dirs[(size_t)(i - 1) * wpr + ((j - 1) >> 4)];
            const unsigned dir = (w >> (2 * ((j - 1) & 15))) & 3u;
            if (dir == 0u) {
                L.amap[i - 1] = j - 1;
                L.pl[Nx - 1 - cnt++] = i - 1;
                --i;
                --j;
            } else if (dir == 1u) {
                --i;
            } else {
                --j;
            }
        }
        *L.n = cnt;
    }
    __syncthreads();
}

// class of position i of a chain of L positions (prd_tmalign.h, step 1): 0 coil, 1 helix, 2 strand, 3 turn
TA_DEV int ta_sec(const float* P0, const float* P1, const float* P2, int i, int L) {
    if (i < 2 || i >= L - 2) return 0;
    auto dist = [&](int a, int b) {
        const float e0 = P0[i + a] - P0[i + b], e1 = P1[i + a] - P1[i + b], e2 = P2[i + a] - P2[i + b];
        return __builtin_sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    };
    const float d13 = dist(-2, 0), d14 = dist(-2, 1), d15 = dist(-2, 2), d24 = dist(-1, 1), d25 = dist(-1, 2), d35 = dist(0, 2);
    auto near = [](float d, float m, float w) { return __builtin_fabsf(d - m) < w; };
    if (near(d15, 6.37f, 2.1f) && near(d14, 5.18f, 1.42f) && near(d25, 5.18f, 1.42f) && near(d13, 5.45f, 0.81f) && near(d24, 5.45f, 0.81f) &&
        near(d35, 5.45f, 0.81f))
        return 1;
    if (near(d15, 13.0f, 1.42f) && near(d14, 10.4f, 1.42f) && near(d25, 10.4f, 1.42f) && near(d13, 6.1f, 1.42f) && near(d24, 6.1f, 1.42f) &&
        near(d35, 6.1f, 1.42f))
        return 2;
    return d15 < 8.f ? 3 : 0;
}

// ---- 1. compaction ---------------------------------------------------------------------------------------------------------------
// planes of structure st: 3 planes of N floats (N = Nx for st < S, Ny otherwise); cposx[row of X] = compacted position or -1;
// idxy[compacted position of Y] = row
__global__ __launch_bounds__(TA_COMPACT_WG) void tmalign_compact_kernel(float* __restrict__ px, float* __restrict__ py, int* __restrict__ hdr,
                                                                       int* __restrict__ cposx, int* __restrict__ idxy,
                                                                       const float* __restrict__ x, long long x_ss, int x_rs,
                                                                       const float* __restrict__ mx, const float* __restrict__ y, long long y_ss,
                                                                       int y_rs, const float* __restrict__ my, int S, int Nx, int Ny) {
    __shared__ int cnt[TA_COMPACT_WG];
    const int st = blockIdx.x, tid = threadIdx.x;
    const bool isx = st < S;
    const float* src = isx ? x + (long long)st * x_ss : y + (long long)(st - S) * y_ss;
    const float* mask = isx ? mx : my;
    const int rs = isx ? x_rs : y_rs, N = isx ? Nx : Ny;
    float* dst = isx ? px + (size_t)st * 3 * Nx : py + (size_t)(st - S) * 3 * Ny;
    const int i0 = tid * TA_OWN;
    int total, pos = sp_compact_start(cnt, mask, TA_OWN, N, total);
    for (int i = i0; i < i0 + TA_OWN && i < N; ++i) {
        const bool in = mask[i] > 0.5f;
        if (in) {                                       // pos < total <= N
            sp_put_row(dst, N, pos, src + (long long)i * rs);
            if (st == S) idxy[pos] = i;
        }
        if (st == 0) cposx[i] = in ? pos : -1;
        pos += in ? 1 : 0;
    }
    if (tid == 0 && st == 0) hdr[0] = total;
    if (tid == 0 && st == S) hdr[1] = total;
}

// carve the dynamic LDS of a refine / search workgroup
struct Lds {
    float *X0, *X1, *X2, *Y0, *Y1, *Y2;
    DpLds dp;
    int *prev, *bestmap;
    unsigned char *secx, *secy;
};
__host__ __device__ constexpr size_t ta_lds_bytes(int Nx, int Ny, bool refine) {
    size_t b = refine ? (size_t)3 * (Nx + 1) * sizeof(double) : 0;
    b += (size_t)3 * (Nx + Ny) * sizeof(float) + (size_t)(refine ? 4 : 2) * Nx * sizeof(int);
    if (refine) b += (size_t)3 * (Nx + 1) + Nx + Ny;
    return (b + 15) & ~(size_t)15;
}
// (the size grows with both lengths and the refine workgroup's is the larger: the longest rows the plan accepts bound every launch;
// 1024: more than the static wrec and nslot of the two kernels, which share the 160 KiB)
static_assert(ta_lds_bytes(PRD_TMALIGN_MAX_N, PRD_TMALIGN_MAX_N, true) + 1024 <= PRD_LDS_MAX &&
                  ta_lds_bytes(PRD_TMALIGN_MAX_N, PRD_TMALIGN_MAX_N, false) + 1024 <= PRD_LDS_MAX,
              "the refine and search kernels' LDS at the longest rows the plan accepts");
TA_DEV Lds ta_carve(unsigned char* base, int Nx, int Ny, bool refine, int* nslot) {
    Lds l;
    unsigned char* p = base;
    l.dp.V = refine ? reinterpret_cast<double*>(p) : nullptr;
    p += refine ? (size_t)3 * (Nx + 1) * sizeof(double) : 0;
    float* f = reinterpret_cast<float*>(p);
    l.X0 = f; l.X1 = f + Nx; l.X2 = f + 2 * Nx;
    f += 3 * Nx;
    l.Y0 = f; l.Y1 = f + Ny; l.Y2 = f + 2 * Ny;
    f += 3 * Ny;
    int* q = reinterpret_cast<int*>(f);
    l.dp.amap = q;
    l.dp.pl = q + Nx;
    l.prev = refine ? q + 2 * Nx : nullptr;     // what the search kernel's smaller allocation does not hold is null there
    l.bestmap = refine ? q + 3 * Nx : nullptr;
    p = reinterpret_cast<unsigned char*>(q + (refine ? 4 : 2) * Nx);
    l.dp.F = refine ? p : nullptr;
    l.secx = refine ? p + 3 * (Nx + 1) : nullptr;
    l.secy = refine ? l.secx + Nx : nullptr;
    l.dp.secx = l.secx;
    l.dp.secy = l.secy;
    l.dp.n = nslot;
    return l;
}

TA_DEV void ta_load(const Lds& l, const float* xs, const float* ys, int Nx, int Ny, int Lx, int Ly, int mir) {
    for (int i = threadIdx.x; i < Lx; i += TA_WG) {
        l.X0[i] = xs[i];
        l.X1[i] = xs[Nx + i];
        l.X2[i] = mir ? -xs[2 * Nx + i] : xs[2 * Nx + i];
    }
    for (int i = threadIdx.x; i < Ly; i += TA_WG) {
        l.Y0[i] = ys[i];
        l.Y1[i] = ys[Ny + i];
        l.Y2[i] = ys[2 * Ny + i];
    }
}

TA_DEV void ta_write_record(float* rec, float score, int n, const float (&rot)[9], const float (&tr)[3]) {
    if (threadIdx.x == 0) {
        sp_record_write(rec, score, n, rot, tr);
        rec[14] = rec[15] = 0.f;
    }
}

// ---- 2. initial alignment and refinement -----------------------------------------------------------------------------------------
// problem = (pair * nm + mirror) * 3 + init;  rec1[problem], maps1[problem][Nx] (compacted positions), dirs[problem][Nx][wpr]
__global__ __launch_bounds__(TA_WG) void tmalign_refine_kernel(float* __restrict__ rec1, int* __restrict__ maps1, unsigned* dirs_all,
                                                              const float* __restrict__ px, const float* __restrict__ py,
                                                              const int* __restrict__ hdr, int R, int Nx, int Ny, int nm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float wrec[TA_NW][TA_REC];
    __shared__ int nslot;
    const int Lx = hdr[0], Ly = hdr[1];
    if (Lx < TA_MIN_L || Ly < TA_MIN_L || Lx > Nx || Ly > Ny) return;       // uniform; the finalize pass writes the documented zeros
    const int tid = threadIdx.x;
    const long prob = blockIdx.x;
    const int init = (int)(prob % TA_INITS), mir = (int)((prob / TA_INITS) % nm);
    const long pair = prob / TA_INITS / nm;
    const int s = (int)(pair / R), r = (int)(pair - (long)s * R);
    const Lds l = ta_carve(lds_raw, Nx, Ny, true, &nslot);
    ta_load(l, px + (size_t)s * 3 * Nx, py + (size_t)r * 3 * Ny, Nx, Ny, Lx, Ly, mir);
    __syncthreads();
    for (int i = tid; i < Lx; i += TA_WG) l.secx[i] = (unsigned char)ta_sec(l.X0, l.X1, l.X2, i, Lx);
    for (int i = tid; i < Ly; i += TA_WG) l.secy[i] = (unsigned char)ta_sec(l.Y0, l.Y1, l.Y2, i, Ly);
    __syncthreads();
    const Coords c = {l.X0, l.X1, l.X2, l.Y0, l.Y1, l.Y2};
    unsigned* dirs = dirs_all + (size_t)prob * Nx * ((Ny + 15) >> 4);
    float* rec = rec1 + (size_t)prob * TA_REC;
    int* mapout = maps1 + (size_t)prob * Nx;
    const float d0 = (float)sp_d0(Ly), inv_d02 = 1.f / (d0 * d0), d0s = fminf(fmaxf(d0, 4.5f), 8.f);
    const float inf = __builtin_inff();

    float rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tr[3] = {0.f, 0.f, 0.f};
    if (init != 1) {
        const int k = wg_threading(c, Lx, Ly, inv_d02, wrec, rot, tr);
        if (init == 0) {
            const int i0 = k < 0 ? -k : 0, i1 = Lx < Ly - k ? Lx : Ly - k;
            for (int i = tid; i < Lx; i += TA_WG) l.dp.amap[i] = (i >= i0 && i < i1) ? i + k : -1;
            wg_list_pairs(l.dp, Lx, Nx);
        }
    }
    // one loop holds the one call site of the DP and of the search: first the initial alignment (A: the threading's overlap, no DP;
    // B, C: a DP with their scores), then the rounds of the two gap values.  Every branch below is uniform over the workgroup.
    float best = -inf, brot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, btr[3] = {0.f, 0.f, 0.f};
    int bn = 0, g = 0, round = 0;
    bool have = false;                                                       // an alignment has been searched
    for (int iter = 0; iter < 2 * TA_DP_ROUNDS + 4; ++iter) {
        const bool initial = !have;
        if (!(initial && init == 0)) {
            const float wss = initial ? (init == 1 ? 1.f : 0.5f) : 0.f, wtm = initial && init == 1 ? 0.f : 1.f;
            const double gap = initial ? -1.0 : (g == 0 ? -0.6 : 0.0);
            for (int i = tid; i < Lx; i += TA_WG) l.prev[i] = initial ? -2 : l.dp.amap[i];
            __syncthreads();
            wg_dp(c, l.dp, dirs, Lx, Ly, Nx, Ny, rot, tr, wss, wtm, gap, inv_d02);
            int diff = 0;
            for (int i = tid; i < Lx; i += TA_WG) diff |= l.dp.amap[i] != l.prev[i];
            const int changed = __syncthreads_or(diff);
            if (!initial && (!changed || nslot < 3)) {                       // this gap value ends; the alignment stays the previous round's
                for (int i = tid; i < Lx; i += TA_WG) l.dp.amap[i] = l.prev[i];
                __syncthreads();
                round = 0;
                if (++g == 2) break;
                continue;
            }
        }
        const int n = nslot;
        if (n < 3) {                                                         // an initial alignment of fewer than 3 pairs is dropped
            ta_write_record(rec, -inf, 0, rot, tr);
            return;
        }
        const float sc = wg_search(c, l.dp.pl + (Nx - n), l.dp.amap, n, 2, inv_d02, d0s, wrec, rot, tr);
        if (initial || sc > best) {
            best = sc;
            bn = n;
#pragma unroll
            for (int a = 0; a < 9; ++a) brot[a] = rot[a];
#pragma unroll
            for (int a = 0; a < 3; ++a) btr[a] = tr[a];
            for (int i = tid; i < Lx; i += TA_WG) l.bestmap[i] = l.dp.amap[i];
        }
        have = true;
        if (!initial && ++round == TA_DP_ROUNDS) {
            round = 0;
            if (++g == 2) break;
        }
    }
    __syncthreads();
    for (int i = tid; i < Lx; i += TA_WG) mapout[i] = l.bestmap[i];
    ta_write_record(rec, best, bn, brot, btr);
}

// ---- 3. the best refinement, the d8 filter, the full search ----------------------------------------------------------------------
// grid: pair * nm + mirror;  rec2[pm], maps2[pm][Nx]
__global__ __launch_bounds__(TA_WG) void tmalign_search_kernel(float* __restrict__ rec2, int* __restrict__ maps2, const float* __restrict__ rec1,
                                                              const int* __restrict__ maps1, const float* __restrict__ px,
                                                              const float* __restrict__ py, const int* __restrict__ hdr, int R, int Nx, int Ny,
                                                              int nm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ float wrec[TA_NW][TA_REC];
    __shared__ int nslot;
    const int Lx = hdr[0], Ly = hdr[1];
    if (Lx < TA_MIN_L || Ly < TA_MIN_L || Lx > Nx || Ly > Ny) return;
    const int tid = threadIdx.x;
    const long pm = blockIdx.x;
    const int mir = (int)(pm % nm);
    const long pair = pm / nm;
    const int s = (int)(pair / R), r = (int)(pair - (long)s * R);
    const float inf = __builtin_inff();
    float rot[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tr[3] = {0.f, 0.f, 0.f};
    float* rec = rec2 + (size_t)pm * TA_REC;
    int bi = -1;
    float bs = -inf;
    for (int k = 0; k < TA_INITS; ++k) {                                     // ties to A, then B, then C
        const float v = rec1[((size_t)pm * TA_INITS + k) * TA_REC];
        if (v > bs) {
            bs = v;
            bi = k;
        }
    }
    if (bi < 0) {
        ta_write_record(rec, -inf, 0, rot, tr);
        return;
    }
    sp_record_transform(rec1 + ((size_t)pm * TA_INITS + bi) * TA_REC, rot, tr);
    const Lds l = ta_carve(lds_raw, Nx, Ny, false, &nslot);
    ta_load(l, px + (size_t)s * 3 * Nx, py + (size_t)r * 3 * Ny, Nx, Ny, Lx, Ly, mir);
    const int* bm = maps1 + ((size_t)pm * TA_INITS + bi) * Nx;
    for (int i = tid; i < Lx; i += TA_WG) {
        const int j = bm[i];
        l.dp.amap[i] = (j >= 0 && j < Ly) ? j : -1;
    }
    __syncthreads();
    const Coords c = {l.X0, l.X1, l.X2, l.Y0, l.Y1, l.Y2};
    const float d0 = (float)sp_d0(Ly), inv_d02 = 1.f / (d0 * d0), d0s = fminf(fmaxf(d0, 4.5f), 8.f);
    const float d8 = 1.5f * __builtin_powf((float)Ly, 0.3f) + 3.5f;
    int near = 0;
    for (int i = tid; i < Lx; i += TA_WG) {
        const int j = l.dp.amap[i];
        near += (j >= 0 && sp_d2(c, i, j, rot, tr) <= d8 * d8) ? 1 : 0;
    }
    // (a thread owns at most TA_ROWS positions: the count of a thread fits the predicate sum below)
    int total = 0;
    for (int k = 1; k <= TA_ROWS; ++k) total += __syncthreads_count(near >= k);
    if (total >= 3) {
        for (int i = tid; i < Lx; i += TA_WG) {
            const int j = l.dp.amap[i];
            if (j >= 0 && !(sp_d2(c, i, j, rot, tr) <= d8 * d8)) l.dp.amap[i] = -1;
        }
    }
    wg_list_pairs(l.dp, Lx, Nx);
    const int n = nslot;
    if (n < 3) {
        ta_write_record(rec, -inf, 0, rot, tr);
        return;
    }
    const float sc = wg_search(c, l.dp.pl + (Nx - n), l.dp.amap, n, TA_ALL_LEVELS, inv_d02, d0s, wrec, rot, tr);
    int* mapout = maps2 + (size_t)pm * Nx;
    for (int i = tid; i < Lx; i += TA_WG) mapout[i] = l.dp.amap[i];
    ta_write_record(rec, sc, n, rot, tr);
}

// ---- 4. the outputs ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void tmalign_finalize_kernel(float* __restrict__ tm, float* __restrict__ rmsd, float* __restrict__ rot,
                                                             float* __restrict__ trans, int* __restrict__ n_aligned, int* __restrict__ mirrored,
                                                             int* __restrict__ map, const float* __restrict__ rec2, const int* __restrict__ maps2,
                                                             const float* __restrict__ px, const float* __restrict__ py,
                                                             const int* __restrict__ hdr, const int* __restrict__ cposx,
                                                             const int* __restrict__ idxy, int R, int Nx, int Ny, int nm) {
    const int lane = threadIdx.x, Lx = hdr[0], Ly = hdr[1];
    const long pair = blockIdx.x;
    const int s = (int)(pair / R), r = (int)(pair - (long)s * R);
    const size_t o = (size_t)pair;
    int* mp = map + o * Nx;
    float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
    int bj = -1;
    if (Lx >= TA_MIN_L && Ly >= TA_MIN_L && Lx <= Nx && Ly <= Ny) {
        float bs = -__builtin_inff();
        for (int j = 0; j < nm; ++j) {                                       // a tie goes to the unmirrored result
            const float v = rec2[((size_t)pair * nm + j) * TA_REC];
            if (v > bs) {
                bs = v;
                bj = j;
            }
        }
    }
    if (bj < 0) {                                                            // a chain below 5 positions (or no finite score at all)
        for (int i = lane; i < Nx; i += 64) mp[i] = -1;
        if (lane == 0) {
            tm[o] = 0.f;
            rmsd[o] = 0.f;
            n_aligned[o] = 0;
            mirrored[o] = 0;
#pragma unroll
            for (int a = 0; a < 9; ++a) rot[o * 9 + a] = m[a];
#pragma unroll
            for (int a = 0; a < 3; ++a) trans[o * 3 + a] = t[a];
        }
        return;
    }
    sp_record_transform(rec2 + ((size_t)pair * nm + bj) * TA_REC, m, t);
    if (bj) sp_unmirror(m);
    const int* am = maps2 + ((size_t)pair * nm + bj) * Nx;
    const float* xs = px + (size_t)s * 3 * Nx;
    const float* ys = py + (size_t)r * 3 * Ny;
    const double d0 = sp_d0(Ly), inv_d02 = 1.0 / (d0 * d0);
    double stm = 0.0, sd2 = 0.0;
    float cnt = 0.f;
    for (int i = lane; i < Lx; i += 64) {
        const int j = am[i];
        if (j < 0 || j >= Ly) continue;
        const double d2 = sp_d2_f64(xs, Nx, i, ys, Ny, j, m, t);
        sd2 += d2;
        stm += 1.0 / (1.0 + d2 * inv_d02);
        cnt += 1.f;
    }
    stm = wave_sum(stm);
    sd2 = wave_sum(sd2);
    cnt = wave_sum(cnt);
    for (int i = lane; i < Nx; i += 64) {
        const int cp = cposx[i];
        const int j = (cp >= 0 && cp < Lx) ? am[cp] : -1;
        mp[i] = (j >= 0 && j < Ly) ? idxy[j] : -1;
    }
    if (lane == 0) {
        tm[o] = (float)(stm / Ly);
        rmsd[o] = cnt > 0.f ? (float)sqrt(sd2 / (double)cnt) : 0.f;
        n_aligned[o] = (int)cnt;
        mirrored[o] = bj;
#pragma unroll
        for (int a = 0; a < 9; ++a) rot[o * 9 + a] = m[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) trans[o * 3 + a] = t[a];
    }
}

// ---- host side: the shape of a call ----------------------------------------------------------------------------------------------
struct TmPlan {
    int ok, nm;
    long npairs, npm, nprob;
    size_t off_cposx, off_idxy, off_px, off_py, off_rec1, off_rec2, off_maps1, off_maps2, off_dirs, bytes;
};

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

TmPlan tm_plan(int S, int R, int Nx, int Ny, int mirror) {
    TmPlan P = {};
    if (S <= 0 || R <= 0 || Nx <= 0 || Ny <= 0 || Nx > PRD_TMALIGN_MAX_N || Ny > PRD_TMALIGN_MAX_N) return P;
    P.nm = mirror ? 2 : 1;
    P.npairs = (long)S * R;
    P.npm = P.npairs * P.nm;
    P.nprob = P.npm * TA_INITS;
    if (P.nprob > PRD_TMALIGN_MAX_PROBLEMS || (long)S + R > PRD_TMALIGN_MAX_PROBLEMS) return P;     // the grids of the launches
    const size_t wpr = (size_t)(Ny + 15) >> 4;
    P.off_cposx = TA_HDR * sizeof(int);
    P.off_idxy = up16(P.off_cposx + (size_t)Nx * sizeof(int));
    P.off_px = up16(P.off_idxy + (size_t)Ny * sizeof(int));
    P.off_py = up16(P.off_px + (size_t)S * 3 * Nx * sizeof(float));
    P.off_rec1 = up16(P.off_py + (size_t)R * 3 * Ny * sizeof(float));
    P.off_rec2 = P.off_rec1 + (size_t)P.nprob * TA_REC * sizeof(float);
    P.off_maps1 = P.off_rec2 + (size_t)P.npm * TA_REC * sizeof(float);
    P.off_maps2 = up16(P.off_maps1 + (size_t)P.nprob * Nx * sizeof(int));
    P.off_dirs = up16(P.off_maps2 + (size_t)P.npm * Nx * sizeof(int));
    P.bytes = up16(P.off_dirs + (size_t)P.nprob * Nx * wpr * sizeof(unsigned));
    P.ok = 1;
    return P;
}

}  // namespace

extern "C" int prd_tmalign_version(void) { return PRD_TMALIGN_VERSION; }

extern "C" size_t prd_tmalign_workspace_bytes(int S, int R, int Nx, int Ny, int mirror) {
    const TmPlan P = tm_plan(S, R, Nx, Ny, mirror);
    return P.ok ? P.bytes : 0;
}

extern "C" int prd_tmalign_align(float* tm, float* rmsd, float* rot, float* trans, int* n_aligned, int* mirrored, int* map,
                                 const float* x, long long x_struct_stride, int x_row_stride, const float* mask_x,
                                 const float* y, long long y_struct_stride, int y_row_stride, const float* mask_y,
                                 int S, int R, int Nx, int Ny, int mirror,
                                 void* ws, size_t ws_bytes, hipStream_t stream) {
    if (!tm || !rmsd || !rot || !trans || !n_aligned || !mirrored || !map || !x || !mask_x || !y || !mask_y || !ws) return PRD_TMALIGN_ERR_ARG;
    if (S <= 0 || R <= 0 || Nx <= 0 || Ny <= 0) return PRD_TMALIGN_ERR_ARG;
    if (x_row_stride < 3 || x_struct_stride < 0 || y_row_stride < 3 || y_struct_stride < 0) return PRD_TMALIGN_ERR_ARG;
    if (Nx > PRD_TMALIGN_MAX_N || Ny > PRD_TMALIGN_MAX_N) return PRD_TMALIGN_ERR_UNSUPPORTED;
    const TmPlan P = tm_plan(S, R, Nx, Ny, mirror);
    if (!P.ok) return PRD_TMALIGN_ERR_UNSUPPORTED;
    if (ws_bytes < P.bytes || (reinterpret_cast<uintptr_t>(ws) & 15)) return PRD_TMALIGN_ERR_WORKSPACE;
    char* w = static_cast<char*>(ws);
    int* hdr = reinterpret_cast<int*>(w);
    int* cposx = reinterpret_cast<int*>(w + P.off_cposx);
    int* idxy = reinterpret_cast<int*>(w + P.off_idxy);
    float* px = reinterpret_cast<float*>(w + P.off_px);
    float* py = reinterpret_cast<float*>(w + P.off_py);
    float* rec1 = reinterpret_cast<float*>(w + P.off_rec1);
    float* rec2 = reinterpret_cast<float*>(w + P.off_rec2);
    int* maps1 = reinterpret_cast<int*>(w + P.off_maps1);
    int* maps2 = reinterpret_cast<int*>(w + P.off_maps2);
    unsigned* dirs = reinterpret_cast<unsigned*>(w + P.off_dirs);

    const size_t lds_refine = ta_lds_bytes(Nx, Ny, true), lds_search = ta_lds_bytes(Nx, Ny, false);
    PRD_TRY(prd_lds_ready<tmalign_refine_kernel>(lds_refine));      // before anything is enqueued: a refusal leaves nothing launched
    PRD_TRY(prd_lds_ready<tmalign_search_kernel>(lds_search));
    PRD_TRY(prd_launch<tmalign_compact_kernel>(dim3(S + R), dim3(TA_COMPACT_WG), 0, stream, px, py, hdr, cposx, idxy, x, x_struct_stride,
                                               x_row_stride, mask_x, y, y_struct_stride, y_row_stride, mask_y, S, Nx, Ny));
    PRD_TRY(prd_launch<tmalign_refine_kernel>(dim3((unsigned)P.nprob), dim3(TA_WG), lds_refine, stream, rec1, maps1, dirs, px, py, hdr, R, Nx, Ny,
                                              P.nm));
    PRD_TRY(prd_launch<tmalign_search_kernel>(dim3((unsigned)P.npm), dim3(TA_WG), lds_search, stream, rec2, maps2, rec1, maps1, px, py, hdr, R, Nx,
                                              Ny, P.nm));
    return prd_launch<tmalign_finalize_kernel>(dim3((unsigned)P.npairs), dim3(64), 0, stream, tm, rmsd, rot, trans, n_aligned, mirrored, map, rec2,
                                               maps2, px, py, hdr, cposx, idxy, R, Nx, Ny, P.nm);
}
