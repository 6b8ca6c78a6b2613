// Multistep few-step sampling on the device (include/prd_multistep.h): the higher-order correction of a solver step and the push of
// the step's clean-structure estimate onto a history of two, in ONE launch after prd_solver_boundary.
//   multistep_correct_kernel   grid (ceil(3 N / MS_THREADS), b), MS_THREADS = 256 threads, no LDS.  Thread e of a sample owns the
//                              element e of its [N][3] rows in z, x0 and both history slots: it reads and writes nothing else, so no
//                              workgroup depends on another and equal inputs give equal bits.  The counter, `first` and the gain row
//                              are uniform over a workgroup (scalar loads); a sample that is left alone returns before any other read.
// It moves 60 bytes per position (z in and out, x0 in, two slots in, two out): at N = 769 that is 46 KB, four workgroups per sample.
// Launch latency, not bandwidth, is what it costs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_multistep.h"
#include "prd_launch.h"

namespace {

constexpr int MS_THREADS = 256;

__global__ __launch_bounds__(MS_THREADS) void multistep_correct_kernel(
    float* __restrict__ z, const float* __restrict__ x0, float* __restrict__ hist, const int64_t* __restrict__ k,
    const int64_t* __restrict__ first, const float* __restrict__ gain, int N, int K, long slot) {
    const int s = blockIdx.y;
    const long cur = (long)k[s] + 1;              // the counter of the step that has just run
    if (cur < 1 || cur > K - 1) return;           // uniform over the workgroup: finished, dead or outside the table
    const long have = (long)first[s] - cur;       // steps run since the history was dropped
    if (have < 0) return;
    const int n = have < 2 ? (int)have : 2;
    const int e = blockIdx.x * MS_THREADS + threadIdx.x;
    if (e >= 3 * N) return;
    const long at = (long)s * 3 * N + e;          // b * 3 N <= 2^32: long
    const float x = x0[at], h0 = hist[at];
    if (n == 1) {
        const float g = gain[cur * PRD_MULTISTEP_GAIN_STRIDE];
        z[at] = z[at] + g * (x - h0);
    } else if (n == 2) {
        const float4 g = reinterpret_cast<const float4*>(gain)[cur];
        const float h1 = hist[slot + at];
        z[at] = z[at] + (g.y * (x - h0) + g.z * (x - h1));
    }
    hist[slot + at] = h0;
    hist[at] = x;
}

}  // namespace

extern "C" int prd_multistep_version(void) { return PRD_MULTISTEP_VERSION; }

extern "C" int prd_multistep_correct(float* z, const float* x0, float* hist, const int64_t* k, const int64_t* first, const float* gain,
                                     int b, int N, int K, hipStream_t stream) {
    if (!z || !x0 || !hist || !k || !first || !gain || b < 1 || N < 1 || K < 1) return PRD_MULTISTEP_ERR_ARG;
    if (b > PRD_MULTISTEP_MAX_B || N > PRD_MULTISTEP_MAX_N || K > PRD_MULTISTEP_MAX_K) return PRD_MULTISTEP_ERR_UNSUPPORTED;
    if ((uintptr_t)gain & 15) return PRD_MULTISTEP_ERR_ALIGN;
    // grid.x <= 3 * MAX_N / 256 = 3072, grid.y <= MAX_B = 4096; 3 N < 2^20 fits an int, a slot of b * 3 N <= 2^32 elements is a long
    const int nblk = (3 * N + MS_THREADS - 1) / MS_THREADS;
    return prd_launch<multistep_correct_kernel>(dim3(nblk, b), dim3(MS_THREADS), 0, stream, z, x0, hist, k, first, gain, N, K,
                                                (long)b * 3 * N);
}
