// Solvent accessibility of samples on the device (include/prd_sasa.h): the Shrake-Rupley point count of every atom.
//   sasa_count_kernel   grid (ceil(A / 4), S), 256 threads.  ONE WAVE owns one atom i of one sample; a workgroup has SA_WAVES = 4 of them.
//                       Lane l owns the points l, l + 64, ... of the atom's sphere, SA_WORDS = 4 of them at a time in registers (a chunk
//                       of 256 points: P = 256 is one pass, P = 1024 four), bit w of its `alive` word saying that point (w0 + w) * 64 + l
//                       is buried by nobody so far.  The other atoms pass through the LDS in tiles of SA_TILE = 256 as
//                       float4 (x, y, z, reach), staged by the 256 threads, one atom each; an atom that is not present -- and the rest
//                       of a tile past A -- is staged as zeros: reach 0 buries nothing, and a NaN of its coordinates never leaves memory.
//                       Per 64 atoms of a tile every lane tests ONE atom j against the centre cutoff, j != i, presence and group, a
//                       ballot gathers the 64 answers, and the wave walks the set bits in a scalar loop: every lane reads neighbour j
//                       from the LDS at the same address (a broadcast read) and tests its own points against it.  No neighbour list, so
//                       no cap.  The walk ends, wave-uniformly, once a ballot over alive != 0 is empty; the wave then only helps staging.
//                       The count is the popcount of the ballot of each alive bit, summed over the words: integers, no order to fix.
// Every output element has one writer (lane 0 of the atom's wave).  Static LDS only, stated once below.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/prd_sasa.h"
#include "../prd_launch.h"

namespace {

constexpr int SA_WAVES = 4;                     // atoms of a workgroup: one per wave
constexpr int SA_TILE = 64 * SA_WAVES;          // atoms of a staged tile: one per thread
constexpr int SA_WORDS = 4;                     // points a lane holds in registers at a time
constexpr int SA_LDS_BYTES = 5120;              // the kernel's static LDS: the struct below
constexpr float SA_SLACK = 1.0001f;             // on the centre cutoff (prd_sasa.h): wider than any rounding of the point test

struct SaShared {
    float4 q[SA_TILE];                          // x, y, z and reach of a staged atom; reach 0: not present
    int g[SA_TILE];                             // its group (0 without a group array)
};
static_assert(sizeof(SaShared) == SA_LDS_BYTES, "SA_LDS_BYTES states the kernel's LDS");

__global__ __launch_bounds__(SA_TILE) void sasa_count_kernel(int* __restrict__ count, const float* __restrict__ pos, long long stride_s,
                                                             long long stride_a, const float* __restrict__ reach, const int* __restrict__ present,
                                                             const int* __restrict__ group, const float* __restrict__ sphere, int same_group, int A,
                                                             int P) {
    __shared__ SaShared sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = blockIdx.y, i = blockIdx.x * SA_WAVES + wave;                // wave-uniform
    const float* __restrict__ ps = pos + (size_t)s * (size_t)stride_s;
    const int* __restrict__ pr = present + (size_t)s * A;
    const bool owns = i < A && pr[i] != 0;                                      // a wave past A, or of an absent atom, only helps staging
    float cx = 0.f, cy = 0.f, cz = 0.f, ri = 0.f;
    int gi = 0;
    if (owns) {
        const float* c = ps + (size_t)i * (size_t)stride_a;
        cx = c[0], cy = c[1], cz = c[2];
        ri = reach[i];
        if (same_group) gi = group[i];
    }
    const int words = P >> 6;                                                   // P is a multiple of 64 (refused otherwise)
    int total = 0;
    for (int w0 = 0; w0 < words; w0 += SA_WORDS) {
        const int nw = words - w0 < SA_WORDS ? words - w0 : SA_WORDS;
        float px[SA_WORDS], py[SA_WORDS], pz[SA_WORDS];
        unsigned alive = 0;
#pragma unroll
        for (int w = 0; w < SA_WORDS; ++w) {
            px[w] = py[w] = pz[w] = 0.f;
            if (w < nw) {                                                       // (w0 + w) * 64 + lane < P
                const float* u = sphere + ((size_t)(w0 + w) * 64 + lane) * 3;
                px[w] = ri * u[0], py[w] = ri * u[1], pz[w] = ri * u[2];
                alive |= 1u << w;
            }
        }
        bool walking = owns;
        for (int t0 = 0; t0 < A; t0 += SA_TILE) {
            const int j = t0 + tid;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            int g = 0;
            if (j < A && pr[j] != 0) {
                const float* c = ps + (size_t)j * (size_t)stride_a;
                q = make_float4(c[0], c[1], c[2], reach[j]);
                if (same_group) g = group[j];
            }
            __syncthreads();                                                    // the walk of the tile before is over
            sh.q[tid] = q;
            sh.g[tid] = g;
            __syncthreads();
            if (!walking) continue;                                             // wave-uniform; the barriers above are met by every wave
            const int kn = A - t0 < SA_TILE ? A - t0 : SA_TILE;
            for (int k0 = 0; k0 < kn && walking; k0 += 64) {
                const float4 c = sh.q[k0 + lane];                               // past kn: zeros, reach 0
                const float dx = c.x - cx, dy = c.y - cy, dz = c.z - cz;
                const float d2 = (dx * dx + dy * dy) + dz * dz, cut = ri + c.w;
                const bool hit = c.w != 0.f && t0 + k0 + lane != i && d2 < (cut * cut) * SA_SLACK && (!same_group || sh.g[k0 + lane] == gi);
                unsigned long long m = __builtin_amdgcn_ballot_w64(hit);
                while (m) {
                    const int b = __builtin_ctzll(m);
                    m &= m - 1;
                    const float4 n = sh.q[k0 + b];                              // the same address in every lane
                    const float ex0 = n.x - cx, ey0 = n.y - cy, ez0 = n.z - cz, rr = n.w * n.w;
#pragma unroll
                    for (int w = 0; w < SA_WORDS; ++w)
                        if (w < nw) {
                            const float ex = px[w] - ex0, ey = py[w] - ey0, ez = pz[w] - ez0;
                            const float sq = (ex * ex + ey * ey) + ez * ez;
                            if (sq < rr) alive &= ~(1u << w);
                        }
                    if (__builtin_amdgcn_ballot_w64(alive != 0) == 0) {
                        walking = false;
                        break;
                    }
                }
            }
        }
#pragma unroll
        for (int w = 0; w < SA_WORDS; ++w) total += __builtin_popcountll(__builtin_amdgcn_ballot_w64((alive >> w) & 1u));
    }
    if (i < A && lane == 0) count[(size_t)s * A + i] = owns ? total : 0;
}

}  // namespace

extern "C" int prd_sasa_version(void) { return PRD_SASA_VERSION; }

extern "C" int prd_sasa_count(int* count, const float* pos, long long stride_s, long long stride_a, const float* reach, const int* present,
                              const int* group, const float* sphere, int mode, int S, int A, int P, hipStream_t stream) {
    if (!count || !pos || !reach || !present || !sphere || S <= 0 || A <= 0 || P <= 0) return PRD_SASA_ERR_ARG;
    if (mode != PRD_SASA_ALL && mode != PRD_SASA_SAME_GROUP) return PRD_SASA_ERR_ARG;
    if (mode == PRD_SASA_SAME_GROUP && !group) return PRD_SASA_ERR_ARG;
    if (stride_a < 3 || (S > 1 && (__int128)stride_s < (__int128)(A - 1) * stride_a + 3)) return PRD_SASA_ERR_ARG;
    if (P % 64 != 0 || P > PRD_SASA_MAX_P || A > PRD_SASA_MAX_A || S > PRD_SASA_MAX_S) return PRD_SASA_ERR_UNSUPPORTED;
    return prd_launch<sasa_count_kernel>(dim3((A + SA_WAVES - 1) / SA_WAVES, S), dim3(SA_TILE), 0, stream, count, pos, stride_s, stride_a, reach, present,
                                         group, sphere, mode == PRD_SASA_SAME_GROUP ? 1 : 0, A, P);
}
