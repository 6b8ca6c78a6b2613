// The one statement of the Kabsch-Sander energy on the device (include/prd_dssp.h): the amide hydrogen of a donor and E(acceptor, donor).
// Both roles of dssp_hbonds_kernel call the same two functions on the same coordinates, so a bond's energy is the same bits in the
// donor's list and in the acceptor's.  Device code only; -ffp-contract=off: no fused multiply-add anywhere below.
#pragma once
#include <hip/hip_runtime.h>

struct DsspV3 {
    float x, y, z;
};

// |b - a|: sqrt((d0 d0 + d1 d1) + d2 d2), the correctly rounded sqrtf
__device__ __forceinline__ float dssp_dist(DsspV3 a, DsspV3 b) {
    const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// H_d = N_d + (C_d-1 - O_d-1) / |C_d-1 - O_d-1|
__device__ __forceinline__ DsspV3 dssp_hydrogen(DsspV3 n, DsspV3 c_prev, DsspV3 o_prev) {
    const float dx = c_prev.x - o_prev.x, dy = c_prev.y - o_prev.y, dz = c_prev.z - o_prev.z;
    const float l = sqrtf((dx * dx + dy * dy) + dz * dz);
    return {n.x + dx / l, n.y + dy / l, n.z + dz / l};
}

// E = q (((1 / r_ON + 1 / r_CH) - 1 / r_OH) - 1 / r_CN), e_min when a distance is below 0.5 Angstrom, never below e_min.  IEEE
// divisions and square roots.  An acceptor or a donor staged at infinity gives four times 1 / inf = 0: E = 0, which no list keeps.
__device__ __forceinline__ float dssp_energy(DsspV3 c, DsspV3 o, DsspV3 n, DsspV3 h, float q, float e_min) {
    const float r_on = dssp_dist(o, n), r_ch = dssp_dist(c, h), r_oh = dssp_dist(o, h), r_cn = dssp_dist(c, n);
    const float e = q * (((1.0f / r_on + 1.0f / r_ch) - 1.0f / r_oh) - 1.0f / r_cn);
    const bool close = r_on < 0.5f || r_ch < 0.5f || r_oh < 0.5f || r_cn < 0.5f;
    return close ? e_min : fmaxf(e, e_min);
}
