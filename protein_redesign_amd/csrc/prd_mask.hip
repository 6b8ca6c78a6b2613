// Redesign masks on the device (include/prd_hip.h: prd_mask_lowest_k).  Training mode (reference model.py:442-458,
// mask_utils.py:16-69, 72-108; the first kernel) and the design regions of inference around the ligand (the second kernel).  Training mode:  All three branches of the reference's prepare_batch are one operation per sample: among the VALID
// residues, mark the k with the smallest key.  One workgroup per sample; k is computed on the device from the residue counts, so no
// count ever travels to the host; selection by rank counting with the keys tiled through the LDS; one owner per output element, no
// atomics, plain vector stores.  A few microseconds of work: nothing here is tuned.
#include "prd_common.h"
#include "../../include/prd_hip.h"
#include "prd_launch.h"

namespace {

constexpr int MASK_WG = 256;            // threads per workgroup = owners per pass = largest batch (one thread per sample for the median)
constexpr int MASK_TILE = 2048;         // keys resident in the LDS at a time (8 KB)

PRD_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// key of position j of the sample: NaN for a position that is not a valid residue (every comparison with it is false, so it is
// never counted and never selected); the given key (random mode), or the distance of the residue's C-alpha to the centroid
// (spatial mode: safe_norm, mask_utils.py:12-14 -- sqrt((dx^2 + dy^2 + dz^2) + 1e-12), products and sums rounded one by one)
PRD_DEV float key_at(const float* __restrict__ rm, const float* __restrict__ key, const float* __restrict__ ca, int ld_ca,
                     float cx, float cy, float cz, int j) {
    if (!(rm[j] > 0.5f)) return __builtin_nanf("");
    if (key) return key[j];
    const float dx = cx - ca[(long)j * ld_ca], dy = cy - ca[(long)j * ld_ca + 1], dz = cz - ca[(long)j * ld_ca + 2];
    return sqrtf(((dx * dx + dy * dy) + dz * dz) + 1e-12f);
}

__global__ __launch_bounds__(MASK_WG) void mask_lowest_k_kernel(float* __restrict__ extra, float* __restrict__ inv, int64_t* __restrict__ tokens,
                                                               const float* __restrict__ residue_mask, const float* __restrict__ key,
                                                               const float* __restrict__ atom_pos, const float* __restrict__ atom_mask,
                                                               const float* __restrict__ ca_pos, int ld_ca, const float* __restrict__ p,
                                                               int spatial, int b, int N) {
    __shared__ __attribute__((aligned(16))) float tile[MASK_TILE];
    __shared__ int cnt[MASK_WG];
    __shared__ float red[MASK_WG / 64][4];
    __shared__ int median;
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* rm = residue_mask + (long)bb * N;

    // ---- residue counts: all b of them in spatial mode (every workgroup recomputes them: b is small), the sample's own otherwise
    // (sums of 0 / 1 below 2^24: exact in any order)
    if (spatial) {
        for (int s = wave; s < b; s += MASK_WG / 64) {  // a wave per sample
            float c = 0.f;
            for (int i = lane; i < N; i += 64) c += residue_mask[(long)s * N + i] > 0.5f ? 1.f : 0.f;
            c = wave_sum(c);
            if (lane == 0) cnt[s] = (int)c;
        }
    } else {
        float c = 0.f;
        for (int i = tid; i < N; i += MASK_WG) c += rm[i] > 0.5f ? 1.f : 0.f;
        c = wave_sum(c);
        if (lane == 0) red[wave][0] = c;
    }
    __syncthreads();
    int count;
    if (spatial) {
        // the LOWER median of the b counts (what torch.median returns, mask_utils.py:36): the count whose rank, ties broken by the
        // sample index, is (b - 1) / 2
        if (tid < b) {
            const int ci = cnt[tid];
            int r = 0;
            for (int j = 0; j < b; ++j) r += (cnt[j] < ci) || (cnt[j] == ci && j < tid);
            if (r == (b - 1) / 2) median = ci;
        }
        count = cnt[bb];
    } else {
        count = (int)(((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]);
    }
    __syncthreads();

    // ---- k (see prd_hip.h)
    const float pf = p[bb];
    int k = 0;
    if (spatial) {
        const float kf = pf * (float)median;            // fp32 product, as the reference's fp32 tensor times a Python double
        if (kf > 0.f) k = kf >= 2147483648.f ? 0x7fffffff : (int)kf;
    } else {
        const double kd = (double)count * (double)pf;
        if (kd > 0.0) k = kd >= 2147483648.0 ? 0x7fffffff : (int)kd;
    }
    if (k > count) k = count;

    // ---- spatial mode: ligand centroid = sum(atom_mask * atom_pos) / sum(atom_mask), fixed summation order
    float cx = 0.f, cy = 0.f, cz = 0.f;
    const float* ca = ca_pos ? ca_pos + (long)bb * N * ld_ca : nullptr;
    if (spatial && k > 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int i = tid; i < N; i += MASK_WG) {
            const float m = atom_mask[(long)bb * N + i];
            const float* q = atom_pos + ((long)bb * N + i) * 3;
            s0 += m * q[0]; s1 += m * q[1]; s2 += m * q[2]; s3 += m;
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
        if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; }
        __syncthreads();
        const float n = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
        cx = (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / n;
        cy = (((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]) / n;
        cz = (((red[0][2] + red[1][2]) + red[2][2]) + red[3][2]) / n;
    }
    const float* kp = spatial ? nullptr : key + (long)bb * N;

    // ---- selection: thread tid owns positions tid, tid + 256, ...; rank of a valid residue = number of valid residues with a smaller
    // key, ties broken by the lower index; selected when rank < k.  The loops are uniform over the workgroup (barriers inside).
    const bool one_tile = N <= MASK_TILE;
    for (int i0 = 0; i0 < N; i0 += MASK_WG) {
        const int i = i0 + tid;
        float ki = __builtin_nanf("");
        if (k > 0 && i < N) ki = key_at(rm, kp, ca, ld_ca, cx, cy, cz, i);
        int rank = 0;
        for (int j0 = 0; k > 0 && j0 < N; j0 += MASK_TILE) {
            if (!one_tile || i0 == 0) {
                __syncthreads();                        // the previous tile has been read by every thread
                for (int j = tid; j < MASK_TILE; j += MASK_WG) tile[j] = j0 + j < N ? key_at(rm, kp, ca, ld_ca, cx, cy, cz, j0 + j) : __builtin_nanf("");
                __syncthreads();
            }
            const int nj = min(MASK_TILE, (N - j0 + 3) & ~3);   // the tile is NaN beyond N: whole 16-byte groups (same address in every lane: a broadcast)
            for (int j = 0; j < nj; j += 4) {
                const float4 v = *reinterpret_cast<const float4*>(tile + j);
                const int jj = j0 + j;
                rank += (v.x < ki || (v.x == ki && jj < i)) ? 1 : 0;
                rank += (v.y < ki || (v.y == ki && jj + 1 < i)) ? 1 : 0;
                rank += (v.z < ki || (v.z == ki && jj + 2 < i)) ? 1 : 0;
                rank += (v.w < ki || (v.w == ki && jj + 3 < i)) ? 1 : 0;
            }
        }
        if (i < N) {
            const float m = rm[i];
            const bool sel = ki == ki && rank < k;      // ki is NaN unless i is a valid residue (and k > 0)
            extra[(long)bb * N + i] = sel ? 0.f : m;
            inv[(long)bb * N + i] = sel ? 1.f : 0.f;
            if (tokens) {
                // mask_utils.py:52-55, 65-69: tokens *= int(extra); tokens += int(esm_mask), esm_mask = 1 - residue_mask with 32 at the selected positions
                const int64_t tk = tokens[(long)bb * N + i];
                tokens[(long)bb * N + i] = tk * (int64_t)(int)(sel ? 0.f : m) + (int64_t)(sel ? 32 : (int)(1.f - m));
            }
        }
    }
}

// ---- inference-time design regions (prd_hip.h: PRD_MASK_LIGAND_NEAREST / PRD_MASK_LIGAND_WITHIN) ---------------------------------
// The key of a valid residue is its C-alpha's distance to the NEAREST ligand atom: O(atoms) per residue, so it is computed ONCE per
// residue and kept in a key store -- the LDS tile for N <= MASK_TILE, the sample's row of `extra` (an output nobody has written
// yet) for longer rows -- where only its owner touches it until a barrier.  The ligand atoms pass through the LDS in tiles of
// MASK_ATOMS, one float4 (x, y, z, validity) per atom, read as broadcasts.
constexpr int MASK_ATOMS = MASK_WG;                 // positions staged per atom tile: one per thread of a fill (4 KB)
constexpr int MASK_LIGAND_MAX_N = 64 * MASK_WG;     // NEAREST: a thread keeps its verdicts as one bit per owned position in a 64-bit word

// extra / inv / tokens of one position, as the kernel above writes them
PRD_DEV void mask_store(float* __restrict__ extra, float* __restrict__ inv, int64_t* __restrict__ tokens, long o, float m, bool sel) {
    extra[o] = sel ? 0.f : m;
    inv[o] = sel ? 1.f : 0.f;
    if (tokens) {
        const int64_t tk = tokens[o];
        tokens[o] = tk * (int64_t)(int)(sel ? 0.f : m) + (int64_t)(sel ? 32 : (int)(1.f - m));
    }
}

__global__ __launch_bounds__(MASK_WG) void mask_ligand_kernel(float* __restrict__ extra, float* __restrict__ inv, int64_t* __restrict__ tokens,
                                                             const float* __restrict__ residue_mask, const float* __restrict__ atom_pos,
                                                             const float* __restrict__ atom_mask, const float* __restrict__ ca_pos, int ld_ca,
                                                             const float* __restrict__ p, int within, int N) {
    __shared__ __attribute__((aligned(16))) float tile[MASK_TILE];
    __shared__ float4 atoms[MASK_ATOMS];
    __shared__ float red[MASK_WG / 64][2];
    const int bb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row = (long)bb * N;
    const float* rm = residue_mask + row;
    const float* am = atom_mask + row;
    const float* ap = atom_pos + row * 3;
    const float* ca = ca_pos + row * ld_ca;
    float* ks = extra + row;                            // the key store of a long row
    const bool one_tile = N <= MASK_TILE;

    // ---- the sample's numbers of valid residues and of ligand atoms (sums of 0 / 1 below 2^24: exact in any order)
    float c = 0.f, a = 0.f;
    for (int i = tid; i < N; i += MASK_WG) {
        c += rm[i] > 0.5f ? 1.f : 0.f;
        a += am[i] > 0.5f ? 1.f : 0.f;
    }
    c = wave_sum(c); a = wave_sum(a);
    if (lane == 0) { red[wave][0] = c; red[wave][1] = a; }
    __syncthreads();
    const int count = (int)(((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]);
    const int natoms = (int)(((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]);

    // ---- what the mode asks for: k of the sample (NEAREST, the random mode's convention) or the radius p itself (WITHIN)
    const float pf = p[bb];
    int k = 0;
    if (!within) {
        const double kd = (double)count * (double)pf;
        if (kd > 0.0) k = kd >= 2147483648.0 ? 0x7fffffff : (int)kd;
        if (k > count) k = count;
    }
    // anything to select at all?  (no ligand atom, k = 0, a negative or NaN radius: nothing is, and no key is formed.)  Uniform over
    // the workgroup, like every loop below that has a barrier inside.
    const bool work = natoms > 0 && count > 0 && (within ? pf >= 0.f : k > 0);

    // ---- keys: +inf at a valid residue, NaN elsewhere (never counted, never selected), then lowered atom tile by atom tile
    if (work) {
        for (int i = tid; i < (one_tile ? (N + 3) & ~3 : N); i += MASK_WG) {      // the LDS tile is NaN up to a whole 16-byte group
            const float v = i < N && rm[i] > 0.5f ? __builtin_inff() : __builtin_nanf("");
            if (one_tile) tile[i] = v; else ks[i] = v;
        }
        for (int a0 = 0; a0 < N; a0 += MASK_ATOMS) {
            const int ja = a0 + tid;
            const bool valid = ja < N && am[ja] > 0.5f;
            atoms[tid] = valid ? make_float4(ap[(long)ja * 3], ap[(long)ja * 3 + 1], ap[(long)ja * 3 + 2], 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
            const int any = __syncthreads_or(valid ? 1 : 0);       // the tile is written; does it hold an atom at all?
            if (any) {
                const int na = min(MASK_ATOMS, N - a0);
                for (int i = tid; i < N; i += MASK_WG) {            // the owner alone reads and writes key i
                    float key = one_tile ? tile[i] : ks[i];
                    if (!(key == key)) continue;
                    const float x = ca[(long)i * ld_ca], y = ca[(long)i * ld_ca + 1], z = ca[(long)i * ld_ca + 2];
                    for (int j = 0; j < na; ++j) {
                        const float4 q = atoms[j];                  // the same address in every lane: a broadcast
                        const float dx = x - q.x, dy = y - q.y, dz = z - q.z;
                        const float d = sqrtf(((dx * dx + dy * dy) + dz * dz) + 1e-12f);
                        if (q.w > 0.5f && d < key) key = d;
                    }
                    if (one_tile) tile[i] = key; else ks[i] = key;
                }
            }
            __syncthreads();                            // the tile has been read by every thread; after the last one: the keys are complete
        }
    }

    // ---- WITHIN: no ranking; every owner compares its own key and overwrites it
    if (within) {
        for (int i = tid; i < N; i += MASK_WG) {
            bool sel = false;
            if (work) sel = (one_tile ? tile[i] : ks[i]) <= pf;    // false for a NaN key
            mask_store(extra, inv, tokens, row + i, rm[i], sel);
        }
        return;
    }

    // ---- NEAREST, ranking pass: as in the kernel above (rank = number of smaller keys, ties to the lower index; selected when
    // rank < k), the verdicts kept in registers -- bit q of `bits` belongs to position tid + 256 q -- because a long row's keys lie
    // where the store pass writes
    unsigned long long bits = 0ull;
    if (work) {
        for (int i0 = 0, q = 0; i0 < N; i0 += MASK_WG, ++q) {
            const int i = i0 + tid;
            const float ki = i < N ? (one_tile ? tile[i] : ks[i]) : __builtin_nanf("");
            int rank = 0;
            for (int j0 = 0; j0 < N; j0 += MASK_TILE) {
                if (!one_tile) {
                    __syncthreads();                    // the previous tile has been read by every thread
                    for (int j = tid; j < MASK_TILE; j += MASK_WG) tile[j] = j0 + j < N ? ks[j0 + j] : __builtin_nanf("");
                    __syncthreads();
                }
                const int nj = min(MASK_TILE, (N - j0 + 3) & ~3);
                for (int j = 0; j < nj; j += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(tile + j);
                    const int jj = j0 + j;
                    rank += (v.x < ki || (v.x == ki && jj < i)) ? 1 : 0;
                    rank += (v.y < ki || (v.y == ki && jj + 1 < i)) ? 1 : 0;
                    rank += (v.z < ki || (v.z == ki && jj + 2 < i)) ? 1 : 0;
                    rank += (v.w < ki || (v.w == ki && jj + 3 < i)) ? 1 : 0;
                }
            }
            if (ki == ki && rank < k) bits |= 1ull << q;
        }
        __syncthreads();                                // no key is overwritten before its last reader
    }
    // ---- store pass
    for (int i0 = 0, q = 0; i0 < N; i0 += MASK_WG, ++q) {
        const int i = i0 + tid;
        if (i < N) mask_store(extra, inv, tokens, row + i, rm[i], (bits >> q) & 1ull);
    }
}

}  // namespace

extern "C" int prd_mask_lowest_k(float* extra, float* inv, int64_t* tokens, const float* residue_mask, const float* key,
                                 const float* atom_pos, const float* atom_mask, const float* ca_pos, int ld_ca, const float* p,
                                 int mode, int b, int N, hipStream_t stream) {
    if (!extra || !inv || !residue_mask || !p || b <= 0 || N <= 0) return PRD_ERR_ARG;
    const bool ligand = mode == PRD_MASK_LIGAND_NEAREST || mode == PRD_MASK_LIGAND_WITHIN;
    if (mode != PRD_MASK_RANDOM && mode != PRD_MASK_SPATIAL && !ligand) return PRD_ERR_ARG;
    if (mode == PRD_MASK_RANDOM && !key) return PRD_ERR_ARG;
    if ((mode == PRD_MASK_SPATIAL || ligand) && (!atom_pos || !atom_mask || !ca_pos || ld_ca < 3)) return PRD_ERR_ARG;
    if (ligand) {
        if (mode == PRD_MASK_LIGAND_NEAREST && N > MASK_LIGAND_MAX_N) return PRD_ERR_UNSUPPORTED;   // one verdict bit per owned position
        return prd_launch<mask_ligand_kernel>(dim3(b), dim3(MASK_WG), 0, stream, extra, inv, tokens, residue_mask, atom_pos, atom_mask,
                                              ca_pos, ld_ca, p, mode == PRD_MASK_LIGAND_WITHIN ? 1 : 0, N);
    }
    if (b > MASK_WG) return PRD_ERR_UNSUPPORTED;        // one thread per sample finds the median of the counts
    return prd_launch<mask_lowest_k_kernel>(dim3(b), dim3(MASK_WG), 0, stream, extra, inv, tokens, residue_mask, key, atom_pos, atom_mask,
                                            ca_pos, ld_ca, p, mode == PRD_MASK_SPATIAL ? 1 : 0, b, N);
}
