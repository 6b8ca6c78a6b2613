// Structure-conditioned sampling on the device (include/prd_condition.h): one launch that puts the kept rows of the coordinate state
// back onto the noised input structure and the kept rows of the sequence state back onto the known sequence.
//   condition_rows_kernel    grid (element tiles, b), 256 threads, one thread per element of a sample: the first 3 N elements are z
//                            (row i = e / 3), the N n_cls after them seq_t (row i = e / n_cls; only present with keep_seq).  Consecutive
//                            threads touch consecutive floats of every tensor, so all loads and stores coalesce; the mask and the two
//                            level scalars are the same address for the threads of a row / of a sample and come from the cache.
// 24 floats per position in, at most as many out: the launch is latency, not bandwidth.  The step counter is read on the device, so
// the same launch serves every step of a captured graph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/prd_condition.h"
#include "prd_launch.h"

namespace {

constexpr int C_THREADS = 256;

__global__ __launch_bounds__(C_THREADS) void condition_rows_kernel(float* __restrict__ z, float* __restrict__ seq_t,
                                                                  const int64_t* __restrict__ t, const float* __restrict__ x0c,
                                                                  const float* __restrict__ keep_z, const float* __restrict__ noise,
                                                                  const float* __restrict__ level, const float* __restrict__ seq0,
                                                                  const float* __restrict__ keep_seq, int b, int N, int n_cls, int levels) {
    const int s = blockIdx.y;
    const int e = blockIdx.x * C_THREADS + threadIdx.x;         // < 2^31: N <= PRD_CONDITION_MAX_N, checked on the host
    const int nz = 3 * N;
    if (e < nz) {
        if (!keep_z) return;
        const long long l = t[s];
        if (l >= levels) return;                                // a level the tables do not hold: the sample is left alone
        const int i = e / 3;
        if (!(keep_z[(size_t)s * N + i] >= 0.5f)) return;
        const size_t at = (size_t)s * nz + e;
        const float x = x0c[at];
        if (l < 0) {
            z[at] = x;
        } else {
            const float a = level[2 * l] * x;
            const float n = level[2 * l + 1] * noise[((size_t)l * b + s) * nz + e];
            z[at] = a + n;                                      // -ffp-contract=off: two rounded products, one rounded sum
        }
        return;
    }
    if (!keep_seq) return;
    const int q = e - nz;
    if (q >= N * n_cls) return;
    const int i = q / n_cls;
    if (!(keep_seq[(size_t)s * N + i] >= 0.5f)) return;
    const size_t at = (size_t)s * N * n_cls + q;
    seq_t[at] = seq0[at];
}

}  // namespace

extern "C" int prd_condition_version(void) { return PRD_CONDITION_VERSION; }

extern "C" int prd_condition_rows(float* z, float* seq_t, const int64_t* t, const float* x0c, const float* keep_z, const float* noise,
                                  const float* level, const float* seq0, const float* keep_seq, int b, int N, int n_cls, int levels,
                                  hipStream_t stream) {
    if (b < 1 || N < 1 || levels < 1 || !t) return PRD_CONDITION_ERR_ARG;
    if (keep_z && (!z || !x0c || !noise || !level)) return PRD_CONDITION_ERR_ARG;
    if (keep_seq && (!seq_t || !seq0)) return PRD_CONDITION_ERR_ARG;
    if (keep_seq && n_cls != PRD_CONDITION_N_CLS) return PRD_CONDITION_ERR_UNSUPPORTED;
    if (b > PRD_CONDITION_MAX_B || N > PRD_CONDITION_MAX_N) return PRD_CONDITION_ERR_UNSUPPORTED;
    if (!keep_z && !keep_seq) return 0;
    const int per = N * (3 + (keep_seq ? n_cls : 0));           // <= 24 * 2^24 < 2^31
    return prd_launch<condition_rows_kernel>(dim3((per + C_THREADS - 1) / C_THREADS, b), dim3(C_THREADS), 0, stream, z, seq_t, t, x0c,
                                             keep_z, noise, level, seq0, keep_seq, b, N, n_cls, levels);
}
