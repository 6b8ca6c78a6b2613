// The backbone builder on the device (include/prd_backbone.h): N, CA, C, CB and O of every residue from the C-alpha trace.
//   backbone_build_kernel   grid (row tiles, S), BB_THREADS = 256 threads: ONE thread owns one residue of one sample.  The rows pass
//                           through the LDS in tiles of BB_TILE = 256 with a halo of BB_HALO = 3 on EITHER side: each thread stages
//                           {x, y, z, mask} of one row as one float4 and its link flag (the first six threads also stage the halo), then
//                           thread t reads the seven rows tile + t - 3 .. tile + t + 3 -- lane l reads slots l .. l + 6, no bank conflict
//                           -- finds where its row stands in its run, continues the run by the dyad rule where it ends within two
//                           rows, and evaluates peptide i - 1 (for N) and peptide i (for C and O) itself.  Nothing passes between
//                           threads after the staging, so the result does not depend on the tiling.  The orientation table (73 floats)
//                           is read from memory, two neighbouring entries per peptide.  A residue is stored as one 60-byte record of
//                           fifteen floats and one int.  Static LDS only: BB_LDS_BYTES.
// A sample is N * 20 bytes read and N * 64 written: at S = 64, N = 384 that is 2 MB, a few microseconds of memory traffic.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/prd_backbone.h"
#include "prd_launch.h"

namespace {

constexpr int BB_THREADS = 256;                 // threads of a workgroup
constexpr int BB_TILE = BB_THREADS;             // rows of a tile: one residue per thread
constexpr int BB_HALO = 3;                      // the rows before and after a tile that its outermost residues reach
constexpr int BB_SLOTS = BB_TILE + 2 * BB_HALO; // staged rows
constexpr int BB_LDS_BYTES = 5248;              // the kernel's static LDS: the struct below

struct BbShared {
    float4 p[BB_SLOTS];                         // {x, y, z, mask} of the tile's rows and both halos
    float link[BB_SLOTS + 2];                   // link of the same rows (two spare elements keep the struct a multiple of 16 bytes)
};
static_assert(sizeof(BbShared) == BB_LDS_BYTES, "BB_LDS_BYTES states the kernel's LDS");

struct BbParams {                               // prd_backbone.h: the peptide in its plane, the CB formula, the validity thresholds
    float l0, ac, rc, ao, ro, an, rn, ka, kb, kc, lo2, hi2, sin2;
};

struct V3 {
    float x, y, z;
};

// -ffp-contract=off: no fused multiply-add anywhere below
__device__ __forceinline__ V3 bb_sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 bb_add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 bb_mul(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float bb_dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 bb_cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 bb_unit(V3 a) {
    const float l = sqrtf(bb_dot(a, a));
    return {a.x / l, a.y / l, a.z / l};
}
__device__ __forceinline__ V3 bb_xyz(float4 p) { return {p.x, p.y, p.z}; }

// the vertex (a, c, b) is neither straight nor folded back
__device__ __forceinline__ bool bb_vertex(V3 a, V3 c, V3 b, float sin2) {
    const V3 u = bb_sub(a, c), v = bb_sub(b, c), w = bb_cross(u, v);
    return sin2 * bb_dot(u, u) * bb_dot(v, v) < bb_dot(w, w);
}

// x rotated by pi about the axis through c that bisects (a - c, b - c)
__device__ __forceinline__ V3 bb_dyad(V3 c, V3 a, V3 b, V3 x) {
    const V3 e = bb_unit(bb_add(bb_unit(bb_sub(a, c)), bb_unit(bb_sub(b, c)))), d = bb_sub(x, c);
    const float t = bb_dot(e, d);
    return bb_sub(bb_add(c, bb_mul(t, bb_mul(2.f, e))), d);
}

__device__ __forceinline__ bool bb_bond(V3 b, const BbParams& g) {
    const float l2 = bb_dot(b, b);
    return g.lo2 < l2 && l2 < g.hi2;
}

// the peptide between a and b, pm before a and pn after b: C and O from a, N from b; returns whether the four points make a valid one
__device__ __forceinline__ bool bb_peptide(V3 pm, V3 a, V3 b, V3 pn, const BbParams& g, const float* __restrict__ table, V3& c, V3& o, V3& n) {
    const V3 bm = bb_sub(a, pm), bb = bb_sub(b, a), bp = bb_sub(pn, b);
    const bool ok = bb_bond(bm, g) && bb_bond(bb, g) && bb_bond(bp, g) && bb_vertex(pm, a, b, g.sin2) && bb_vertex(a, b, pn, g.sin2);
    const float lb = sqrtf(bb_dot(bb, bb));
    const V3 u = {bb.x / lb, bb.y / lb, bb.z / lb};
    const V3 n1 = bb_cross(bm, bb), nn = bb_unit(n1), m = bb_cross(u, nn), w = bb_cross(bb, bp);
    float tau = atan2f(lb * bb_dot(bm, w), bb_dot(n1, w));
    if (tau < 0.f) tau = tau + 6.28318548f;                     // fp32 2 pi
    const float f = tau * 11.4591560f;                          // fp32 72 / (2 pi)
    int k = (int)f;
    k = k < 0 ? 0 : k > PRD_BACKBONE_TABLE - 2 ? PRD_BACKBONE_TABLE - 2 : k;   // a NaN of an invalid peptide reads inside the table too
    const float t0 = table[k], t1 = table[k + 1];
    const float xi = t0 + (f - (float)k) * (t1 - t0);
    const float sn = sinf(xi), cs = cosf(xi);
    const V3 p = bb_add(bb_mul(cs, nn), bb_mul(sn, m));
    const float s = lb / g.l0;
    c = bb_add(bb_add(a, bb_mul(s * g.ac, u)), bb_mul(g.rc, p));
    o = bb_add(bb_add(a, bb_mul(s * g.ao, u)), bb_mul(g.ro, p));
    n = bb_add(bb_add(b, bb_mul(s * g.an, u)), bb_mul(g.rn, p));
    return ok;
}

__global__ __launch_bounds__(BB_THREADS) void backbone_build_kernel(float* __restrict__ atoms, int* __restrict__ built, const float* __restrict__ x,
                                                                    long long x_ss, int x_rs, const float* __restrict__ mask,
                                                                    const float* __restrict__ link, const float* __restrict__ table, BbParams g, int N) {
    __shared__ BbShared sh;
    const int tid = threadIdx.x, s = blockIdx.y, r0 = blockIdx.x * BB_TILE;
    const float* xs = x + (long long)s * x_ss;
    for (int k = tid; k < BB_SLOTS; k += BB_THREADS) {
        const int j = r0 - BB_HALO + k;
        float4 p = make_float4(0.f, 0.f, 0.f, 0.f);             // before the start and past the end: unmasked, unlinked
        float l = 0.f;
        if (j >= 0 && j < N) {
            const float* px = xs + (long long)j * x_rs;
            p = make_float4(px[0], px[1], px[2], mask[j]);
            if (j < N - 1) l = link[j];                         // link[N - 1] is never read as a bond
        }
        sh.p[k] = p;
        sh.link[k] = l;
    }
    __syncthreads();
    const int i = r0 + tid;
    if (i >= N) return;
    // qa .. qg: rows i - 3 .. i + 3 (ca: row i is a C-alpha); c0 .. c5: rows i + k and i + k + 1 belong to one run, k = -3 .. 2
    const float4 qa = sh.p[tid], qb = sh.p[tid + 1], qc = sh.p[tid + 2], qd = sh.p[tid + 3], qe = sh.p[tid + 4], qf = sh.p[tid + 5], qg = sh.p[tid + 6];
    const bool ma = qa.w > 0.5f, mb = qb.w > 0.5f, mc = qc.w > 0.5f, ca = qd.w > 0.5f, me = qe.w > 0.5f, mf = qf.w > 0.5f, mg = qg.w > 0.5f;
    const bool c0 = sh.link[tid] > 0.5f && ma && mb, c1 = sh.link[tid + 1] > 0.5f && mb && mc, c2 = sh.link[tid + 2] > 0.5f && mc && ca;
    const bool c3 = sh.link[tid + 3] > 0.5f && ca && me, c4 = sh.link[tid + 4] > 0.5f && me && mf, c5 = sh.link[tid + 5] > 0.5f && mf && mg;
    const int left = c2 ? (c1 ? (c0 ? 3 : 2) : 1) : 0;          // rows of the run before row i, counted up to 3
    const int right = c3 ? (c4 ? (c5 ? 3 : 2) : 1) : 0;         // and after it
    const V3 q0 = bb_xyz(qd);
    V3 vn = {0.f, 0.f, 0.f}, vc = vn, vo = vn, vb = vn;
    bool has_n = false, has_c = false;
    if (ca && left + right >= 3) {                              // a run of at least 4 rows
        V3 qm1 = bb_xyz(qc), qm2 = bb_xyz(qb), qp1 = bb_xyz(qe), qp2 = bb_xyz(qf);
        bool dm1 = true, dm2 = true, dp1 = true, dp2 = true;    // the points are defined
        if (left == 0) {                                        // P_-1 = dyad(P_1; P_0, P_2; P_3)
            dm1 = bb_vertex(q0, qp1, qp2, g.sin2);
            qm1 = bb_dyad(qp1, q0, qp2, bb_xyz(qg));
        }
        if (left <= 1) {                                        // P_-2 = dyad(P_0; P_-1, P_1; P_2), seen from P_0 or from P_1
            dm2 = dm1 && bb_vertex(qm1, q0, qp1, g.sin2);
            qm2 = bb_dyad(q0, qm1, qp1, qp2);
        }
        if (right == 0) {                                       // the mirror image at the other end
            dp1 = bb_vertex(q0, qm1, qm2, g.sin2);
            qp1 = bb_dyad(qm1, q0, qm2, bb_xyz(qa));
        }
        if (right <= 1) {
            dp2 = dp1 && bb_vertex(qp1, q0, qm1, g.sin2);
            qp2 = bb_dyad(q0, qp1, qm1, qm2);
        }
        V3 c_, o_, n_;
        const bool ok_a = bb_peptide(qm2, qm1, q0, qp1, g, table, c_, o_, vn);       // peptide i - 1: N_i
        const bool ok_b = bb_peptide(qm1, q0, qp1, qp2, g, table, vc, vo, n_);       // peptide i: C_i, O_i
        has_n = ok_a && dm2 && dm1 && dp1;
        has_c = ok_b && dm1 && dp1 && dp2;
        const V3 b = bb_sub(q0, vn), c = bb_sub(vc, q0);
        vb = bb_add(bb_add(bb_add(q0, bb_mul(g.ka, bb_cross(b, c))), bb_mul(g.kb, b)), bb_mul(g.kc, c));
    }
    const bool has_b = has_n && has_c;
    const V3 zero = {0.f, 0.f, 0.f};
    const V3 wn = has_n ? vn : zero, wa = ca ? q0 : zero, wc = has_c ? vc : zero, wb = has_b ? vb : zero, wo = has_c ? vo : zero;
    const size_t row = (size_t)s * N + i;
    float* o = atoms + row * 15;                                // one 60-byte record: N, CA, C, CB, O
    o[0] = wn.x, o[1] = wn.y, o[2] = wn.z;
    o[3] = wa.x, o[4] = wa.y, o[5] = wa.z;
    o[6] = wc.x, o[7] = wc.y, o[8] = wc.z;
    o[9] = wb.x, o[10] = wb.y, o[11] = wb.z;
    o[12] = wo.x, o[13] = wo.y, o[14] = wo.z;
    built[row] = (has_n ? 1 : 0) | (ca ? 2 : 0) | (has_c ? 4 : 0) | (has_b ? 8 : 0) | (has_c ? 16 : 0);
}

bool bb_finite(float v) { return v > -__builtin_inff() && v < __builtin_inff(); }     // NaN fails both comparisons

}  // namespace

extern "C" int prd_backbone_version(void) { return PRD_BACKBONE_VERSION; }

extern "C" int prd_backbone_build(float* atoms, int* built, const float* x, long long x_struct_stride, int x_row_stride, const float* mask,
                                  const float* link, const float* xi_table, float l0, float ac, float rc, float ao, float ro, float an, float rn,
                                  float ka, float kb, float kc, float bond_lo2, float bond_hi2, float sin2_min, int S, int N, hipStream_t stream) {
    if (!atoms || !built || !x || !mask || !link || !xi_table || S <= 0 || N <= 0 || x_row_stride < 3 || x_struct_stride < 0) return PRD_BACKBONE_ERR_ARG;
    const BbParams g = {l0, ac, rc, ao, ro, an, rn, ka, kb, kc, bond_lo2, bond_hi2, sin2_min};
    const float scalars[13] = {l0, ac, rc, ao, ro, an, rn, ka, kb, kc, bond_lo2, bond_hi2, sin2_min};
    for (int k = 0; k < 13; ++k)
        if (!bb_finite(scalars[k])) return PRD_BACKBONE_ERR_ARG;
    if (!(l0 > 0.f) || !(ka < 0.f) || !(bond_lo2 > 0.f) || !(bond_lo2 < bond_hi2) || !(sin2_min >= 0.f) || !(sin2_min < 1.f)) return PRD_BACKBONE_ERR_ARG;
    if (N > PRD_BACKBONE_MAX_N || S > PRD_BACKBONE_MAX_S) return PRD_BACKBONE_ERR_UNSUPPORTED;
    return prd_launch<backbone_build_kernel>(dim3((N + BB_TILE - 1) / BB_TILE, S), dim3(BB_THREADS), 0, stream, atoms, built, x, x_struct_stride,
                                             x_row_stride, mask, link, xi_table, g, N);
}
