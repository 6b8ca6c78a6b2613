"""The yardstick of the chirality tests: prd_chirality.h restated in float64 numpy, and the inputs the CPU and GPU tests share.

The device compares fp32 quantities with window edges, so it may disagree with float64 on a comparison whose sides are closer than the
fp32 error of the quantity.  That error is derivable: bond vectors of ~3.8 Angstrom are differences of fp32 coordinates within 200
Angstrom (half an ulp of 200 is 7.6e-6), so a bond length is good to ~1e-5 Angstrom, a cosine and a dihedral to ~1e-5, a signed volume of
such vectors to ~1e-4 Angstrom^3.  A comparison is AMBIGUOUS when its sides are within BAND_TAU = 1e-4 rad, BAND_COS = 1e-4, BAND_BOND =
1e-4 Angstrom or BAND_VOLUME = 1e-3 Angstrom^3 -- about ten times those errors.  ``census`` gives every count three times: as float64
decides, with every ambiguous comparison false (``counts_lo``) and with every one true (``counts_hi``); the device must lie between."""
import math

import numpy as np

BAND_TAU, BAND_COS, BAND_BOND, BAND_VOLUME = 1e-4, 1e-4, 1e-4, 1e-3
COLUMNS = ("helix_right", "helix_left", "extended_native", "extended_mirror", "quads", "centres_kept", "centres_inverted", "centres_flat")
MIRROR_COLUMNS = [1, 0, 3, 2, 4, 6, 5, 7]
DEFAULT_EDGES_DEG = dict(helix_theta=(75.0, 110.0), helix_tau=(30.0, 80.0), extended_theta=(105.0, 150.0), extended_tau=(120.0, 180.0))
IDEAL = dict(bond=3.83, theta=90.37, tau=50.04)         # the ideal alpha-helix's C-alpha virtual geometry (degrees)


def edges_f32(deg=DEFAULT_EDGES_DEG):
    """the eight fp32 arguments of the launch, restated independently of chirality.Windows: (cos theta_hi, cos theta_lo, tau_lo, tau_hi) of
    the helical and of the extended class, float64 rounded once"""
    out = []
    for th, ta in ((deg["helix_theta"], deg["helix_tau"]), (deg["extended_theta"], deg["extended_tau"])):
        out += [np.float32(math.cos(math.radians(th[1]))), np.float32(math.cos(math.radians(th[0]))), np.float32(math.radians(ta[0])),
                np.float32(math.radians(ta[1]))]
    return [float(v) for v in out]


# ---- chains ---------------------------------------------------------------------------------------------------------------------------

def nerf(bonds, thetas, taus):
    """[L,3] float64: the chain whose virtual bonds are ``bonds`` [L-1] (Angstrom), whose angles at rows 1 .. L-2 are ``thetas`` [L-2] and
    whose dihedrals of rows (i, i+1, i+2, i+3) are ``taus`` [L-3] (radians), by the natural extension of a reference frame"""
    L = len(bonds) + 1
    p = np.zeros((L, 3))
    if L > 1:
        p[1] = [bonds[0], 0.0, 0.0]
    if L > 2:
        p[2] = p[1] + bonds[1] * np.array([-math.cos(thetas[0]), math.sin(thetas[0]), 0.0])
    for k in range(3, L):
        a, b, c = p[k - 3], p[k - 2], p[k - 1]
        bc = (c - b) / np.linalg.norm(c - b)
        n = np.cross(b - a, bc)
        n /= np.linalg.norm(n)
        m = np.cross(n, bc)
        R, th, ta = bonds[k - 1], thetas[k - 2], taus[k - 3]
        p[k] = c + R * (-math.cos(th) * bc + math.sin(th) * math.cos(ta) * m + math.sin(th) * math.sin(ta) * n)
    return p


def ideal_helix(L, hand=1.0, radius=2.3, turn=100.0, rise=1.5):
    """the parametric helix: right-handed for hand = +1, its mirror image for -1"""
    k = np.arange(L)
    a = np.radians(turn) * k
    return np.stack([radius * np.cos(a), hand * radius * np.sin(a), rise * k], 1)


PALETTE = {                       # (theta range, |tau| range, sign of tau) in degrees; every value >= 5 degrees from every window edge
    "helix_r": ((80.0, 105.0), (35.0, 75.0), +1), "helix_l": ((80.0, 105.0), (35.0, 75.0), -1),
    "ext_n": ((112.0, 145.0), (125.0, 175.0), -1), "ext_m": ((112.0, 145.0), (125.0, 175.0), +1),
    "none": ((112.0, 145.0), (85.0, 115.0), +1),
}


def segment(rng, L, kinds, run=(5, 12), ideal=False):
    """a chain of L rows whose (theta, tau) run through ``kinds`` of the palette in runs of random length; bonds within [3.4, 4.2].
    ``ideal``: constant values -- the ideal helix's for a helical kind, (120, -+165) degrees for an extended one"""
    th, ta = np.zeros(max(L - 2, 0)), np.zeros(max(L - 3, 0))
    k = 0
    while k < max(L - 2, 0):
        kind = kinds[int(rng.integers(len(kinds)))]
        (t0, t1), (a0, a1), sign = PALETTE[kind]
        n = int(rng.integers(run[0], run[1] + 1))
        for j in range(k, min(k + n, L - 2)):
            if ideal:
                th[j] = IDEAL["theta"] if kind.startswith("helix") else 120.0
                if j < L - 3:
                    ta[j] = sign * (IDEAL["tau"] if kind.startswith("helix") else 165.0)
            else:
                th[j] = rng.uniform(t0, t1)
                if j < L - 3:
                    ta[j] = sign * rng.uniform(a0, a1)
        k += n
    bonds = np.full(max(L - 1, 0), IDEAL["bond"]) if ideal else rng.uniform(3.4, 4.2, max(L - 1, 0))
    return nerf(bonds, np.radians(th), np.radians(ta))


def structure(rng, N, kinds, seg=30, ideal=False):
    """[N,3] float64 and link [N]: segments of ``seg`` rows, each rotated at random and centred on a random point of a 120 Angstrom box, so
    that coordinates stay within ~100 Angstrom of the origin whatever N is.  Rows of different segments are not linked -- except after
    every third segment, where the link is SET and the bond window is what refuses the quad (the next segment is far away)."""
    x, link = np.zeros((N, 3)), np.ones(N)
    for n, r0 in enumerate(range(0, N, seg)):
        L = min(seg, N - r0)
        s = segment(rng, L, kinds, ideal=ideal)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))                          # a proper rotation: the hand is the palette's
        # segments whose neighbours are linked sit >= 10 Angstrom apart: centres are lattice points of a coarse grid
        x[r0: r0 + L] = (s - s.mean(0)) @ q.T + rng.integers(-3, 4, 3) * 20.0 + rng.uniform(-2, 2, 3)
        link[r0 + L - 1] = 1.0 if n % 3 == 2 else 0.0
    return x, link


# ---- the census -------------------------------------------------------------------------------------------------------------------------

def _dot(u, v):
    return (u * v).sum(-1)


def _lt(a, b, band, mode):
    """a < b; mode -1: every comparison within ``band`` false, +1: every one true"""
    return a < b + mode * band


def verdict_rule(counts, has_ref, min_helix=4, min_extended=12):
    """(verdict, basis) of one row of counts, as the header states the rule"""
    hr, hl, en, em, _, kept, inv, _ = (int(v) for v in counts)
    h, e = hr - hl, en - em
    if h != 0 and abs(h) >= min_helix:
        return (1 if h > 0 else -1), 1
    if has_ref and kept + inv >= 1 and (kept == 0 or inv == 0):
        return (1 if inv == 0 else -1), 2
    if e != 0 and abs(e) >= min_extended:
        return (1 if e > 0 else -1), 3
    return 0, 0


def signed_volume(x, centres):
    c = np.asarray(centres, np.int64).reshape(-1, 4)
    a, b, d = (x[..., c[:, k], :] - x[..., c[:, 0], :] for k in (1, 2, 3))
    return _dot(a, np.cross(b, d))


def census(x, mask, link, centres=None, centre_ref=None, edges=None, bond=(3.3, 4.3), vmin=0.5, min_helix=4, min_extended=12):
    """x [S,N,3] (the fp32 values the device reads), everything else as prd_chirality_census takes it.  Returns a dict: ``tau`` [S,N] (NaN where
    float64 sees no quad), ``classes``, ``valid``, ``counts`` / ``counts_lo`` / ``counts_hi`` [S,8], ``ambiguous`` [S] (the quads of
    counts_hi on which any comparison, validity included, is ambiguous), ``verdict``, ``basis`` (from ``counts``), ``volume`` [S,C]"""
    x = np.asarray(x, np.float64)
    S, N = x.shape[:2]
    hc_lo, hc_hi, ht_lo, ht_hi, ec_lo, ec_hi, et_lo, et_hi = edges_f32() if edges is None else edges
    m, lk = np.asarray(mask) > 0.5, np.asarray(link) > 0.5
    out = {"tau": np.full((S, N), np.nan), "classes": np.zeros((S, N), np.int32), "valid": np.zeros((S, N), bool)}
    cnt = {mode: np.zeros((S, 8), np.int64) for mode in (-1, 0, 1)}
    amb = np.zeros(S, np.int64)
    Q = N - 3
    if Q > 0:
        i = np.arange(Q)
        p0, p1, p2, p3 = x[:, i], x[:, i + 1], x[:, i + 2], x[:, i + 3]
        b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
        d1, d2, d3 = (np.sqrt(_dot(b, b)) for b in (b1, b2, b3))
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        with np.errstate(invalid="ignore", divide="ignore"):
            tau = np.arctan2(d2 * _dot(b1, n2), _dot(n1, n2))
            c1, c2 = -_dot(b1, b2) / (d1 * d2), -_dot(b2, b3) / (d2 * d3)
        at = np.abs(tau)
        rows = (m[i] & m[i + 1] & m[i + 2] & m[i + 3] & lk[i] & lk[i + 1] & lk[i + 2])[None]
        cls = {}
        for mode in (-1, 0, 1):
            ok = rows
            for d in (d1, d2, d3):
                ok = ok & _lt(bond[0], d, BAND_BOND, mode) & _lt(d, bond[1], BAND_BOND, mode)
            near = (at < BAND_TAU) | (at > math.pi - BAND_TAU)                  # the sign of tau itself is within the band
            plus = (tau > 0) & ~near if mode < 0 else (tau > 0) | near if mode > 0 else tau > 0
            minus = (tau < 0) & ~near if mode < 0 else (tau < 0) | near if mode > 0 else tau < 0
            helix = ok
            for c in (c1, c2):
                helix = helix & _lt(hc_lo, c, BAND_COS, mode) & _lt(c, hc_hi, BAND_COS, mode)
            helix = helix & _lt(ht_lo, at, BAND_TAU, mode) & _lt(at, ht_hi, BAND_TAU, mode)
            ext = ok
            for c in (c1, c2):
                ext = ext & _lt(ec_lo, c, BAND_COS, mode) & _lt(c, ec_hi, BAND_COS, mode)
            ext = ext & _lt(et_lo, at, BAND_TAU, mode) & _lt(at, et_hi, BAND_TAU, mode)
            if mode == 0:
                ext = ext & ~helix                              # the helical window is looked at first (the default windows are disjoint)
            cls[mode] = (ok, helix & plus, helix & minus, ext & minus, ext & plus)
            for col, sel in zip((4, 0, 1, 2, 3), cls[mode]):
                cnt[mode][:, col] = sel.sum(1)
        ok, hr, hl, en, em = cls[0]
        out["valid"][:, :Q] = ok
        out["tau"][:, :Q] = np.where(ok, tau, np.nan)
        out["classes"][:, :Q] = np.where(hr, 1, np.where(hl, 2, np.where(en, 3, np.where(em, 4, 0))))
        amb = sum((a != b) for a, b in zip(cls[-1], cls[1]))
        amb = (amb > 0).sum(1)
    C = 0 if centres is None else len(np.asarray(centres).reshape(-1, 4))
    out["volume"] = np.zeros((S, C))
    amb_c = np.zeros(S, np.int64)
    if C:
        v = signed_volume(x, centres)
        out["volume"] = v
        for mode in (-1, 0, 1):
            flat = _lt(np.abs(v), vmin, BAND_VOLUME, mode)
            solid = ~_lt(np.abs(v), vmin, BAND_VOLUME, -mode)
            cnt[mode][:, 7] = flat.sum(1)
            if centre_ref is not None:
                same = (v > 0) == (np.asarray(centre_ref, np.float64) > 0)[None]
                cnt[mode][:, 5] = (solid & same).sum(1)
                cnt[mode][:, 6] = (solid & ~same).sum(1)
        amb_c = (_lt(np.abs(v), vmin, BAND_VOLUME, 1) != _lt(np.abs(v), vmin, BAND_VOLUME, -1)).sum(1)
    out.update(counts=cnt[0], counts_lo=cnt[-1], counts_hi=cnt[1], ambiguous=np.asarray(amb), ambiguous_centres=amb_c)
    vb = [verdict_rule(row, centre_ref is not None and C > 0, min_helix, min_extended) for row in cnt[0]]
    out["verdict"], out["basis"] = np.array([v for v, _ in vb], np.int32), np.array([b for _, b in vb], np.int32)
    return out


# ---- the cases the CPU and GPU tests share --------------------------------------------------------------------------------------------------

KINDS = ("helix_r", "helix_l", "ext_n", "ext_m", "mixed", "sigma0.3", "sigma1")
ALL = ("helix_r", "helix_l", "ext_n", "ext_m", "none")
# (N, S, first kind, mask, strided, C, centre reference): the kernel's row tile is 256 with a halo of 3; its centres go 256 to a pass
CASES = [(1, 1, 0, "ones", False, 0, False), (3, 1, 0, "ones", False, 0, False), (4, 5, 0, "ones", False, 1, True), (5, 1, 4, "ones", False, 1, False),
         (64, 5, 0, "ones", False, 0, False), (255, 1, 4, "ones", False, 64, True), (256, 5, 0, "gap7", False, 65, True),
         (257, 5, 2, "ones", True, 64, False), (259, 1, 4, "tile", False, 1, True), (259, 5, 3, "alt", False, 0, False),
         (300, 7, 0, "ones", False, 65, True), (1100, 5, 4, "ones", True, 65, True)]
IDS = ["N%d-S%d-%s%s-C%d%s" % (c[0], c[1], c[3], "-strided" if c[4] else "", c[5], "-ref" if c[6] else "") for c in CASES]
SEEDS = {}                              # case -> seed, where the default 1000 N + S has an ambiguous comparison in a small case


def case_masks(kind, N, link):
    i = np.arange(N)
    mask, link = np.ones(N), link.copy()
    if kind == "alt":
        mask = (i % 2 == 0).astype(np.float64)                  # no four consecutive rows: no quad at all
    elif kind == "gap7":
        mask = (i % 7 != 6).astype(np.float64)
    elif kind == "tile":
        link[:] = 1.0
        link[[255, 256]] = 0.0                                  # the links broken at the tile edge, and only there
    return mask, link


def case_inputs(case):
    """the inputs of a case as the device takes them (fp32 / int32 numpy) and their float64 census; the kinds of the S structures cycle
    through KINDS from the case's first kind: ideal chains of one class, a mixed chain off every edge, and Gaussian-perturbed mixed chains"""
    N, S, first, mkind, _, C, with_ref = case
    rng = np.random.default_rng(SEEDS.get(case, 1000 * N + S))
    xs, kinds, link = [], [], None
    seg = N if mkind == "tile" and N <= 300 else 30
    for s in range(S):
        kind = KINDS[(first + s) % len(KINDS)]
        kinds.append(kind)
        if kind.startswith("sigma"):
            base, lk = structure(rng, N, ALL, seg)
            base = base + float(kind[5:]) * rng.normal(size=base.shape)
        elif kind == "mixed":
            base, lk = structure(rng, N, ALL, seg)
        else:
            base, lk = structure(rng, N, (kind,), seg, ideal=True)
        link = lk if link is None else link
        xs.append(base)
    x = np.stack(xs).astype(np.float32)
    mask, link = case_masks(mkind, N, link)
    centres = None
    if C:
        base = (np.arange(C) * 5) % max(N - 3, 1)
        centres = np.stack([base + 1, base, base + 2, base + 3], 1).astype(np.int32)
    ref = None
    if C and with_ref:
        ref = signed_volume(x[0].astype(np.float64), centres).astype(np.float32)
        ref[np.abs(ref) < 0.5] = 1.0                            # a reference is never flat (centre_reference drops those)
    exact = [k for k, kind in enumerate(kinds) if not kind.startswith("sigma")]
    return dict(x=x, kinds=kinds, exact=exact, mask=mask.astype(np.float32), link=link.astype(np.float32), centres=centres, centre_ref=ref,
                ref=census(x, mask, link, centres, ref))


def mirror(x, axis=0):
    y = np.array(x, copy=True)
    y[..., axis] = -y[..., axis]
    return y


# ---- the complex and the prepared samples of the generate_samples tests ---------------------------------------------------------------------

NA, NR = 6, 40
TETRA = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0]]) * (1.5 / np.sqrt(3.0))     # |V| = 2.6 Angstrom^3


def complex_and_samples():
    """a complex of 6 ligand atoms (atom 0 a tagged centre bonded to atoms 1, 2, 3, with input coordinates: a tetrahedron) and 40 residues
    of one chain whose input is a right-handed helix, and six prepared samples: right helices, left helices and undecided random walks,
    the ligand tetrahedron kept in the first of each pair and inverted in the second"""
    import torch
    from protein_redesign_amd.synthetic import synthetic_sample
    rng = np.random.default_rng(21)
    data = synthetic_sample(NA, NR, esm_dim=64, seed=2)
    data["atom_feats"][:, 1] = 0
    data["atom_feats"][0, 1] = 1
    bd = torch.full((NA, NA), 5, dtype=torch.long)
    bd.fill_diagonal_(0)
    for j in (1, 2, 3):
        bd[0, j] = bd[j, 0] = 1
    data["bond_distance"] = bd
    lig = np.concatenate([TETRA, [[3.0, 0.0, 0.0], [4.0, 1.0, 0.0]]]) + [0.0, 12.0, 0.0]
    data["atom_pos"] = torch.from_numpy(lig.astype(np.float32))
    data["residue_chain_index"] = torch.zeros(NR, dtype=torch.long)
    helix = ideal_helix(NR) - ideal_helix(NR).mean(0)
    data["residue_atom_pos"] = torch.zeros(NR, 37, 3)
    data["residue_atom_pos"][:, 1] = torch.from_numpy(helix.astype(np.float32))
    walk = np.cumsum(rng.normal(size=(NR, 3)) * 3.8 / np.sqrt(3.0), 0)
    rows = []
    for k, prot in enumerate((helix, helix, mirror(helix, 1), mirror(helix, 1), walk, walk)):
        rows.append(np.concatenate([lig if k % 2 == 0 else mirror(lig - lig.mean(0), 2) + lig.mean(0), prot]))
    return data, np.stack(rows).astype(np.float32)


class Prepared:
    """a model whose samples are prepared device structures, in the order of the keyed sources; logits from the sources' generators"""

    def __init__(self, samples, device):
        import torch
        self.device, self.samples, self.calls = torch.device(device), torch.from_numpy(samples).to(device), 0

    def sample(self, batch, sources, redesign=None, scaffold=None):
        import torch
        n = batch["atom_mask"].shape[1]
        pos = self.samples[self.calls: self.calls + len(sources)].clone()
        self.calls += len(sources)
        return pos, torch.stack([torch.randn(n, 21, generator=s.g) for s in sources]).to(self.device)
