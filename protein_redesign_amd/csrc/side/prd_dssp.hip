// Secondary structure of samples on the device (include/prd_dssp.h): the Kabsch-Sander hydrogen bonds and the DSSP classes.
//   dssp_hbonds_kernel   grid (row tiles, S, 2 roles), 256 threads.  The sweep of quality_contacts_kernel: a workgroup owns DS_ROWS = 64
//                        residues of one sample, lane l of EVERY wave holding residue tile * 64 + l in registers -- its N and H in role 0
//                        (the residue as donor), its C and O in role 1 (as acceptor).  The other side passes through the LDS in tiles of
//                        DS_COLS = 256 columns as two float4 per column (C and O of an acceptor, N and H of a donor), staged by the 256
//                        threads, one column each; a column that is no candidate is staged at infinity, where its energy is 0 and no
//                        list keeps it.  Wave w sweeps the w-th quarter of the tile, every lane reading the SAME column in the same
//                        iteration (a broadcast read, no bank conflict), and keeps a running best two (energy, index).  The four
//                        partial lists of a row meet in the LDS and wave 0 merges them in a fixed order by (energy, index).
//   dssp_flags_kernel    grid (row tiles, S), 256 threads: ONE thread owns one residue.  {CA, link} of the tile and a halo of DS_HALO
//                        rows pass through the LDS; the turns, the two lowest bridge partners with their types, the ladder bit and
//                        the bend come from the residue's own lists and those of the rows its partners name, read from memory.
//   dssp_classes_kernel  the same tiling over the flags the launch before wrote: the class of a row from the flags of rows r-10 .. r+6.
// Nothing passes between threads beyond the staging and the merge, and every output element has one writer.  Static LDS only, stated once per kernel below.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../../include/prd_dssp.h"
#include "../prd_launch.h"
#include "prd_dssp_energy.h"

namespace {

constexpr int DS_ROWS = 64;                     // residues of a workgroup of the sweep: one per lane
constexpr int DS_WAVES = 4;                     // its waves: each sweeps a quarter of a column tile
constexpr int DS_COLS = DS_ROWS * DS_WAVES;     // columns of a tile: one per thread when it is staged
constexpr int DS_HB_LDS_BYTES = 12304;          // the sweep's static LDS: the struct below

struct HbShared {
    float4 a[DS_COLS], b[DS_COLS];              // C and O of an acceptor column / N and H of a donor column; .w unused
    float pe[DS_WAVES][2][DS_ROWS];             // the partial lists of the four waves: energy
    int pj[DS_WAVES][2][DS_ROWS];               // and partner
    int any[4];                                 // [0]: some row of the workgroup is a candidate (the rest keeps the struct a multiple of 16 bytes)
};
static_assert(sizeof(HbShared) == DS_HB_LDS_BYTES, "DS_HB_LDS_BYTES states the kernel's LDS");

constexpr int DS_TILE = PRD_DSSP_TILE;          // rows of a tile of the per-residue kernels: one per thread
constexpr int DS_HALO = PRD_DSSP_HALO;          // rows before and after a tile that its outermost residues reach
constexpr int DS_SLOTS = DS_TILE + 2 * DS_HALO; // staged rows
constexpr int DS_FLAGS_LDS_BYTES = DS_SLOTS * 16;   // dssp_flags_kernel: {x, y, z of CA, link} of every staged row
constexpr int DS_CLASSES_LDS_BYTES = DS_SLOTS * 4;  // dssp_classes_kernel: the flags word of every staged row
constexpr int DS_NONE = 0x7fffffff;             // an empty list entry, before it is written as -1
constexpr int DS_BRIDGED = 1 << 16;             // in the staged word of dssp_classes_kernel only: bridge[r][0] >= 0

__device__ __forceinline__ DsspV3 ds_atom(const float* __restrict__ atoms, size_t row, int k) {
    const float* p = atoms + row * 15 + k * 3;
    return {p[0], p[1], p[2]};
}

__device__ __forceinline__ bool ds_less(float e, int j, float f, int k) { return e < f || (e == f && j < k); }

__global__ __launch_bounds__(DS_COLS) void dssp_hbonds_kernel(int* __restrict__ partner, float* __restrict__ energy, const float* __restrict__ atoms,
                                                              const int* __restrict__ built, const float* __restrict__ link,
                                                              const float* __restrict__ donor, float q, float e_min, int N) {
    __shared__ HbShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, s = blockIdx.y, role = blockIdx.z;
    const int i = blockIdx.x * DS_ROWS + lane;
    const size_t base = (size_t)s * N;
    const float inf = __builtin_inff();
    // acceptor: C and O present.  donor: N present, link[d-1] set, C and O of d-1 present, donor[d] allows it
    auto acceptor = [&](int a) { return (built[base + a] & 20) == 20; };
    auto donates = [&](int d) {
        return d >= 1 && (built[base + d] & 1) && link[d - 1] > 0.5f && (built[base + d - 1] & 20) == 20 && (!donor || donor[d] > 0.5f);
    };
    // the row: p = N (role 0) or C (role 1), r = H or O
    DsspV3 p = {0.f, 0.f, 0.f}, r = p;
    const bool active = i < N && (role == 0 ? donates(i) : acceptor(i));
    if (active) {
        if (role == 0) {
            p = ds_atom(atoms, base + i, 0);
            r = dssp_hydrogen(p, ds_atom(atoms, base + i - 1, 2), ds_atom(atoms, base + i - 1, 4));
        } else {
            p = ds_atom(atoms, base + i, 2);
            r = ds_atom(atoms, base + i, 4);
        }
    }
    const int skip = role == 0 ? i - 1 : i + 1;                 // the excluded neighbour: the acceptor d-1 of a donor, the donor a+1 of an acceptor
    float e0 = 0.f, e1 = 0.f;                                   // the running best two, e0 <= e1; only E < 0 enters
    int j0 = DS_NONE, j1 = DS_NONE;
    if (tid == 0) sh.any[0] = 0;
    __syncthreads();
    if (active) sh.any[0] = 1;                                  // every writer writes the same value
    __syncthreads();
    if (sh.any[0]) {                                            // uniform over the workgroup: a tile of ligand rows sweeps nothing
        for (int c0 = 0; c0 < N; c0 += DS_COLS) {
            const int j = c0 + tid;
            float4 a = make_float4(inf, inf, inf, 0.f), b = a;  // at infinity: E = 0, never kept
            if (j < N && (role == 0 ? acceptor(j) : donates(j))) {
                if (role == 0) {
                    const DsspV3 c = ds_atom(atoms, base + j, 2), o = ds_atom(atoms, base + j, 4);
                    a = make_float4(c.x, c.y, c.z, 0.f);
                    b = make_float4(o.x, o.y, o.z, 0.f);
                } else {
                    const DsspV3 n = ds_atom(atoms, base + j, 0);
                    const DsspV3 h = dssp_hydrogen(n, ds_atom(atoms, base + j - 1, 2), ds_atom(atoms, base + j - 1, 4));
                    a = make_float4(n.x, n.y, n.z, 0.f);
                    b = make_float4(h.x, h.y, h.z, 0.f);
                }
            }
            __syncthreads();                                    // the sweep of the tile before is over
            sh.a[tid] = a;
            sh.b[tid] = b;
            __syncthreads();
            const int cb = wave * DS_ROWS, jb = c0 + cb;
            const int kn = N - jb < DS_ROWS ? N - jb : DS_ROWS; // wave-uniform; <= 0: nothing of this quarter is a column
#pragma unroll 2
            for (int k = 0; k < kn; ++k) {
                const float4 ca = sh.a[cb + k], cc = sh.b[cb + k];
                const DsspV3 u = {ca.x, ca.y, ca.z}, v = {cc.x, cc.y, cc.z};
                const float e = role == 0 ? dssp_energy(u, v, p, r, q, e_min) : dssp_energy(p, r, u, v, q, e_min);
                const int jj = jb + k;
                if (active && e < e1 && jj != i && jj != skip) {        // columns come in rising order: an equal energy keeps the lower index
                    if (e < e0) {
                        e1 = e0, j1 = j0;
                        e0 = e, j0 = jj;
                    } else {
                        e1 = e, j1 = jj;
                    }
                }
            }
        }
    }
    sh.pe[wave][0][lane] = e0, sh.pe[wave][1][lane] = e1;
    sh.pj[wave][0][lane] = j0, sh.pj[wave][1][lane] = j1;
    __syncthreads();
    if (wave == 0 && i < N) {                                   // one owner per output element; the merge in a fixed order
        float m0 = 0.f, m1 = 0.f;
        int k0 = DS_NONE, k1 = DS_NONE;
#pragma unroll
        for (int w = 0; w < DS_WAVES; ++w)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float e = sh.pe[w][t][lane];
                const int j = sh.pj[w][t][lane];
                if (j != DS_NONE && ds_less(e, j, m1, k1)) {
                    if (ds_less(e, j, m0, k0)) {
                        m1 = m0, k1 = k0;
                        m0 = e, k0 = j;
                    } else {
                        m1 = e, k1 = j;
                    }
                }
            }
        const size_t o = (base + i) * 4 + role * 2;
        partner[o] = k0 == DS_NONE ? -1 : k0;
        partner[o + 1] = k1 == DS_NONE ? -1 : k1;
        energy[o] = k0 == DS_NONE ? 0.f : m0;
        energy[o + 1] = k1 == DS_NONE ? 0.f : m1;
    }
}

// ---- the per-residue logic --------------------------------------------------------------------------------------------------------------

struct DsLists {                                // the lists of one sample
    const int* partner;
    const float* energy;
    const float* link;
    float cutoff;
    int N;
};

__device__ __forceinline__ bool ds_lk(const DsLists& L, int k) { return k >= 0 && k < L.N - 1 && L.link[k] > 0.5f; }

// the mutual two-best rule
__device__ __forceinline__ bool ds_bond(const DsLists& L, int a, int d) {
    if (a < 0 || d < 0 || a >= L.N || d >= L.N) return false;
    const int* pd = L.partner + (size_t)d * 4;
    const float* ed = L.energy + (size_t)d * 4;
    const bool listed = (pd[0] == a && ed[0] < L.cutoff) || (pd[1] == a && ed[1] < L.cutoff);
    if (!listed) return false;
    const int* pa = L.partner + (size_t)a * 4;
    return pa[2] == d || pa[3] == d;
}

// bit 0: Bridge(i, j) parallel, bit 1: antiparallel
__device__ __forceinline__ int ds_bridge(const DsLists& L, int i, int j) {
    if (i < 1 || j < 1 || i >= L.N - 1 || j >= L.N - 1) return 0;
    const int gap = i > j ? i - j : j - i;
    if (gap < 3 || !ds_lk(L, i - 1) || !ds_lk(L, i) || !ds_lk(L, j - 1) || !ds_lk(L, j)) return 0;
    const bool par = (ds_bond(L, i - 1, j) && ds_bond(L, j, i + 1)) || (ds_bond(L, j - 1, i) && ds_bond(L, i, j + 1));
    const bool anti = (ds_bond(L, i, j) && ds_bond(L, j, i)) || (ds_bond(L, i - 1, j + 1) && ds_bond(L, j - 1, i + 1));
    return (par ? 1 : 0) | (anti ? 2 : 0);
}

__global__ __launch_bounds__(DS_TILE) void dssp_flags_kernel(int* __restrict__ flags, int* __restrict__ bridge, const int* __restrict__ partner,
                                                             const float* __restrict__ energy, const float* __restrict__ atoms,
                                                             const int* __restrict__ built, const float* __restrict__ link, float cutoff,
                                                             float cos_bend, int N) {
    __shared__ float4 sp[DS_SLOTS];                             // {x, y, z of CA (NaN-free zeros when absent), link}; .w < 0: CA absent
    static_assert(sizeof(sp) == DS_FLAGS_LDS_BYTES, "DS_FLAGS_LDS_BYTES states the kernel's LDS");
    const int tid = threadIdx.x, s = blockIdx.y, r0 = blockIdx.x * DS_TILE;
    const size_t base = (size_t)s * N;
    for (int k = tid; k < DS_SLOTS; k += DS_TILE) {
        const int j = r0 - DS_HALO + k;
        float4 p = make_float4(0.f, 0.f, 0.f, -1.f);            // before the start and past the end: no CA, unlinked
        if (j >= 0 && j < N) {
            const bool ca = (built[base + j] & 2) != 0;
            const bool l = j < N - 1 && link[j] > 0.5f;         // link[N - 1] is never read as a bond
            const DsspV3 c = ds_atom(atoms, base + j, 1);
            p = make_float4(c.x, c.y, c.z, (ca ? 1.f : -1.f) * (l ? 2.f : 1.f));     // |w| = 2: linked to the next row; w > 0: CA present
        }
        sp[k] = p;
    }
    __syncthreads();
    const int i = r0 + tid;
    if (i >= N) return;
    const DsLists L = {partner + base * 4, energy + base * 4, link, cutoff, N};
    auto lk = [&](int k) { return fabsf(sp[tid + DS_HALO + k].w) > 1.5f; };     // lk(i + k), k in -HALO .. HALO
    int f = 0;
    // turns: cont(i, n) and Bond(i, i + n)
    const bool c3 = lk(0) && lk(1) && lk(2), c4 = c3 && lk(3), c5 = c4 && lk(4);
    if (c3 && ds_bond(L, i, i + 3)) f |= PRD_DSSP_FLAG_TURN3;
    if (c4 && ds_bond(L, i, i + 4)) f |= PRD_DSSP_FLAG_TURN3 << 1;
    if (c5 && ds_bond(L, i, i + 5)) f |= PRD_DSSP_FLAG_TURN3 << 2;
    // bridges: every Bridge(i, j) has a bond in the lists of row i or row i-1 -- Bond(j-1, i): j-1 among the acceptors of i;
    // Bond(i, j): j among the donors of i; Bond(i-1, j) and Bond(i-1, j+1): j or j+1 among the donors of i-1
    int b0 = DS_NONE, b1 = DS_NONE, t0 = 0, t1 = 0;
    if (lk(-1) && lk(0)) {
        int cand[8];
        const int* pi = L.partner + (size_t)i * 4;
        const int* pm = L.partner + (size_t)(i - 1) * 4;        // lk(-1): i >= 1
        cand[0] = pi[0] < 0 ? -1 : pi[0] + 1, cand[1] = pi[1] < 0 ? -1 : pi[1] + 1;
        cand[2] = pi[2], cand[3] = pi[3];
        cand[4] = pm[2], cand[5] = pm[3];
        cand[6] = pm[2] < 0 ? -1 : pm[2] - 1, cand[7] = pm[3] < 0 ? -1 : pm[3] - 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = cand[k];
            if (j < 0 || j == b0 || j == b1) continue;
            const int t = ds_bridge(L, i, j);
            if (!t) continue;
            if (j < b0) {
                b1 = b0, t1 = t0;
                b0 = j, t0 = t;
            } else if (j < b1) {
                b1 = j, t1 = t;
            }
        }
    }
    f |= (t0 & 1 ? PRD_DSSP_FLAG_PAR0 : 0) | (t0 & 2 ? PRD_DSSP_FLAG_ANTI0 : 0) | (t1 & 1 ? PRD_DSSP_FLAG_PAR1 : 0) | (t1 & 2 ? PRD_DSSP_FLAG_ANTI1 : 0);
    // ladder: a bridge of the same type next to one of the two
    bool ladder = false;
    if (b0 != DS_NONE) {
        if (t0 & 1) ladder |= (ds_bridge(L, i + 1, b0 + 1) & 1) || (ds_bridge(L, i - 1, b0 - 1) & 1);
        if (t0 & 2) ladder |= (ds_bridge(L, i + 1, b0 - 1) & 2) || (ds_bridge(L, i - 1, b0 + 1) & 2);
    }
    if (b1 != DS_NONE) {
        if (t1 & 1) ladder |= (ds_bridge(L, i + 1, b1 + 1) & 1) || (ds_bridge(L, i - 1, b1 - 1) & 1);
        if (t1 & 2) ladder |= (ds_bridge(L, i + 1, b1 - 1) & 2) || (ds_bridge(L, i - 1, b1 + 1) & 2);
    }
    if (ladder) f |= PRD_DSSP_FLAG_LADDER;
    // bend
    const float4 qa = sp[tid + DS_HALO - 2], qc = sp[tid + DS_HALO], qe = sp[tid + DS_HALO + 2];
    if (lk(-2) && lk(-1) && lk(0) && lk(1) && qa.w > 0.f && qc.w > 0.f && qe.w > 0.f) {
        const float ux = qc.x - qa.x, uy = qc.y - qa.y, uz = qc.z - qa.z, vx = qe.x - qc.x, vy = qe.y - qc.y, vz = qe.z - qc.z;
        const float uv = (ux * vx + uy * vy) + uz * vz, uu = (ux * ux + uy * uy) + uz * uz, vv = (vx * vx + vy * vy) + vz * vz;
        if (uv / (sqrtf(uu) * sqrtf(vv)) < cos_bend) f |= PRD_DSSP_FLAG_BEND;
    }
    flags[base + i] = f;
    bridge[(base + i) * 2] = b0 == DS_NONE ? -1 : b0;
    bridge[(base + i) * 2 + 1] = b1 == DS_NONE ? -1 : b1;
}

__global__ __launch_bounds__(DS_TILE) void dssp_classes_kernel(uint8_t* __restrict__ classes, const int* __restrict__ flags,
                                                               const int* __restrict__ bridge, const int* __restrict__ built, int N) {
    __shared__ int sf[DS_SLOTS];                                // the flags word of a row, DS_BRIDGED with it
    static_assert(sizeof(sf) == DS_CLASSES_LDS_BYTES, "DS_CLASSES_LDS_BYTES states the kernel's LDS");
    const int tid = threadIdx.x, s = blockIdx.y, r0 = blockIdx.x * DS_TILE;
    const size_t base = (size_t)s * N;
    for (int k = tid; k < DS_SLOTS; k += DS_TILE) {
        const int j = r0 - DS_HALO + k;
        int f = 0;                                              // before the start and past the end: nothing
        if (j >= 0 && j < N) f = flags[base + j] | (bridge[(base + j) * 2] >= 0 ? DS_BRIDGED : 0);
        sf[k] = f;
    }
    __syncthreads();
    const int i = r0 + tid;
    if (i >= N) return;
    auto fl = [&](int k) { return sf[tid + DS_HALO + k]; };     // the word of row i + k, k in -HALO .. HALO
    // minimal n-helix starting at row i + k: Turn_n(i + k - 1) and Turn_n(i + k)
    auto starts = [&](int k, int bit) { return (fl(k - 1) & bit) && (fl(k) & bit); };
    auto is_h = [&](int k) { return starts(k - 3, 2) || starts(k - 2, 2) || starts(k - 1, 2) || starts(k, 2); };
    auto hbe = [&](int k) { return is_h(k) || (fl(k) & DS_BRIDGED); };
    auto g_at = [&](int k) { return starts(k, 1) && !hbe(k) && !hbe(k + 1) && !hbe(k + 2); };      // a 3-helix k .. k+2 that stands
    auto is_g = [&](int k) { return g_at(k - 2) || g_at(k - 1) || g_at(k); };
    auto i_at = [&](int k) {
        if (!starts(k, 4)) return false;
        for (int m = 0; m < 5; ++m)
            if (hbe(k + m) || is_g(k + m)) return false;
        return true;
    };
    const int me = fl(0);
    int c = 0;
    if (is_h(0)) c = 1;
    else if (me & DS_BRIDGED) c = me & PRD_DSSP_FLAG_LADDER ? 3 : 2;
    else if (is_g(0)) c = 4;
    else if (i_at(-4) || i_at(-3) || i_at(-2) || i_at(-1) || i_at(0)) c = 5;
    else if ((fl(-1) & 7) || (fl(-2) & 7) || (fl(-3) & 6) || (fl(-4) & 4)) c = 6;      // Turn_n(i - k), 1 <= k < n
    else if (me & PRD_DSSP_FLAG_BEND) c = 7;
    if (!(built[base + i] & 2)) c = 0;
    classes[base + i] = (uint8_t)c;
}

bool ds_finite(float v) { return v > -__builtin_inff() && v < __builtin_inff(); }     // NaN fails both comparisons

}  // namespace

extern "C" int prd_dssp_version(void) { return PRD_DSSP_VERSION; }

extern "C" int prd_dssp_hbonds(int* partner, float* energy, const float* atoms, const int* built, const float* link, const float* donor,
                               float q, float e_min, int S, int N, hipStream_t stream) {
    if (!partner || !energy || !atoms || !built || !link || S <= 0 || N <= 0) return PRD_DSSP_ERR_ARG;
    if (!ds_finite(q) || !ds_finite(e_min) || !(q > 0.f) || !(e_min < 0.f)) return PRD_DSSP_ERR_ARG;
    if (N > PRD_DSSP_MAX_N || S > PRD_DSSP_MAX_S) return PRD_DSSP_ERR_UNSUPPORTED;
    return prd_launch<dssp_hbonds_kernel>(dim3((N + DS_ROWS - 1) / DS_ROWS, S, 2), dim3(DS_COLS), 0, stream, partner, energy, atoms, built, link,
                                          donor, q, e_min, N);
}

extern "C" int prd_dssp_assign(uint8_t* classes, int* flags, int* bridge, const int* partner, const float* energy, const float* atoms,
                               const int* built, const float* link, float cutoff, float cos_bend, int S, int N, hipStream_t stream) {
    if (!classes || !flags || !bridge || !partner || !energy || !atoms || !built || !link || S <= 0 || N <= 0) return PRD_DSSP_ERR_ARG;
    if (!ds_finite(cutoff) || !ds_finite(cos_bend) || !(cutoff < 0.f) || !(cos_bend > -1.f) || !(cos_bend < 1.f)) return PRD_DSSP_ERR_ARG;
    if (N > PRD_DSSP_MAX_N || S > PRD_DSSP_MAX_S) return PRD_DSSP_ERR_UNSUPPORTED;
    const dim3 grid((N + DS_TILE - 1) / DS_TILE, S);
    PRD_TRY(prd_launch<dssp_flags_kernel>(grid, dim3(DS_TILE), 0, stream, flags, bridge, partner, energy, atoms, built, link, cutoff, cos_bend, N));
    return prd_launch<dssp_classes_kernel>(grid, dim3(DS_TILE), 0, stream, classes, (const int*)flags, (const int*)bridge, built, N);
}
