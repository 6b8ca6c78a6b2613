"""float64 numpy yardstick of protein_redesign_amd.quality, written from the definitions of include/prd_quality.h (not from the kernel),
and the inputs of its tests.

Comparisons sit on thresholds, so an fp32 sweep and this one may disagree on a pair whose margin is below the fp32 distance error
(~2e-5 Angstrom for coordinates within 100 Angstrom of each other).  A comparison is AMBIGUOUS when its two sides are within ``BAND`` =
1e-4 Angstrom; every count comes three ways: exact in float64, with every ambiguous comparison false (``_lo``) and with every one true
(``_hi``).  The device must land between the last two, and the tests cap how many pairs may be ambiguous at all."""
import numpy as np

BAND = 1e-4
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
MIRROR = np.diag([1.0, 1.0, -1.0])


def distances(p):
    p = np.asarray(p, dtype=np.float64)
    return np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(-1))


def lddt_counts(x, y, row_mask, col_mask, radius, band=BAND):
    """x [S,N,3], y [N,3], masks [N] (> 0.5: set).  Per row: ``total`` [N] / ``preserved`` [S,N] (exact), their ``_lo`` / ``_hi`` brackets,
    ``near_radius`` [N] bool (some reference distance of an otherwise included pair is ambiguous against the radius), and the numbers
    of included and of ambiguous pairs per sample (``included`` [S], ``ambiguous`` [S])."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    S, N = x.shape[:2]
    pair = (np.asarray(row_mask) > 0.5)[:, None] & (np.asarray(col_mask) > 0.5)[None, :] & ~np.eye(N, dtype=bool)
    D = distances(y)
    inc, inc_lo, inc_hi = pair & (D < radius), pair & (D < radius - band), pair & (D < radius + band)
    out = {"total": inc.sum(1), "total_lo": inc_lo.sum(1), "total_hi": inc_hi.sum(1), "near_radius": (inc_hi & ~inc_lo).any(1),
           "preserved": np.zeros((S, N), np.int64), "preserved_lo": np.zeros((S, N), np.int64), "preserved_hi": np.zeros((S, N), np.int64),
           "included": np.full(S, int(inc.sum())), "ambiguous": np.zeros(S, np.int64)}
    for s in range(S):
        diff = np.abs(distances(x[s]) - D)
        amb = inc_hi & ~inc_lo
        for t in THRESHOLDS:
            out["preserved"][s] += (inc & (diff < t)).sum(1)
            out["preserved_lo"][s] += (inc_lo & (diff < t - band)).sum(1)
            out["preserved_hi"][s] += (inc_hi & (diff < t + band)).sum(1)
            amb |= inc_hi & (np.abs(diff - t) < band)
        out["ambiguous"][s] = amb.sum()
    return out


def lddt_scores(preserved, total):
    """(per position [S,N], NaN where total is 0; pooled per structure [S]) from the integer counts"""
    preserved, total = np.asarray(preserved, dtype=np.float64), np.asarray(total, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return preserved / (4.0 * total), preserved.sum(1) / (4.0 * total.sum())


def lddt(x, y, row_mask, col_mask=None, radius=15.0):
    c = lddt_counts(x, y, row_mask, row_mask if col_mask is None else col_mask, radius)
    return lddt_scores(c["preserved"], c["total"])


def _once(M):
    """pairs of the boolean [N,N] relation M, one that holds in both orders counted once"""
    return int(M.sum()) - int(np.triu(M & M.T, 1).sum())


def contacts_counts(x, a_mask, b_mask, cutoff, exclude=None, band=BAND):
    """x [S,N,3].  ``count`` [S] with ``count_lo`` / ``count_hi``, ``nearest`` [S,N] (+inf without a partner and outside A), ``qualifying`` (the
    number of qualifying pairs, both orders once) and ``ambiguous`` [S]."""
    x = np.asarray(x, dtype=np.float64)
    S, N = x.shape[:2]
    Q = (np.asarray(a_mask) > 0.5)[:, None] & (np.asarray(b_mask) > 0.5)[None, :] & ~np.eye(N, dtype=bool)
    if exclude is not None:
        Q &= np.asarray(exclude) == 0
    out = {"count": np.zeros(S, np.int64), "count_lo": np.zeros(S, np.int64), "count_hi": np.zeros(S, np.int64),
           "nearest": np.full((S, N), np.inf), "qualifying": _once(Q), "ambiguous": np.zeros(S, np.int64)}
    for s in range(S):
        d = distances(x[s])
        out["count"][s], out["count_lo"][s], out["count_hi"][s] = _once(Q & (d < cutoff)), _once(Q & (d < cutoff - band)), _once(Q & (d < cutoff + band))
        out["ambiguous"][s] = _once(Q & (np.abs(d - cutoff) < band))
        out["nearest"][s] = np.where(Q, d, np.inf).min(1)
    return out


def assess(pos, na, nr, ca_marked, bond_distance, residue_index, chain_index, ref=None, ref_has_ligand=True):
    """The named metrics of quality.assess with its documented defaults; pos [S,N,3] over rows [0, na) ligand, [na, na + nr) residues;
    ``ca_marked`` [N] bool; ``bond_distance`` [N,N]; ``residue_index`` / ``chain_index`` [N]."""
    pos = np.asarray(pos, dtype=np.float64)
    S, N = pos.shape[:2]
    rows = np.arange(N)
    lig = rows < na
    res = (rows >= na) & (rows < na + nr) & np.asarray(ca_marked, dtype=bool)
    bd = np.asarray(bond_distance)
    bonded = (bd == 1) & lig[:, None] & lig[None, :]
    out = {"ca_clashes": contacts_counts(pos, res, res, 3.0)["count"], "ligand_clashes": contacts_counts(pos, lig, res, 2.5)["count"],
           "ligand_self_clashes": contacts_counts(pos, lig, lig, 2.0, exclude=bd < 4)["count"],
           "ligand_bond_outliers": np.zeros(S, np.int64), "chain_breaks": np.zeros(S, np.int64)}
    ri, ch = np.asarray(residue_index), np.asarray(chain_index)
    step = res[1:] & res[:-1] & (ch[1:] == ch[:-1]) & (ri[1:] - ri[:-1] == 1)
    for s in range(S):
        d = distances(pos[s])
        out["ligand_bond_outliers"][s] = int(np.triu(bonded & ((d < 0.9) | ~(d < 2.1)), 1).sum())
        out["chain_breaks"][s] = int((step & (np.abs(np.diagonal(d, 1) - 3.8) > 0.5)).sum())
    near = contacts_counts(pos, res, lig, 8.0)["nearest"]
    out["pocket"] = (near < 8.0).astype(np.int64)
    out["pocket_size"] = out["pocket"].sum(1)
    if ref is not None:
        per, out["lddt_ca"] = lddt(pos, ref, res, radius=15.0)
        out["lddt_ca_per_residue"] = per[:, na: na + nr]
        if ref_has_ligand:
            out["lddt_pli"] = lddt(pos, ref, lig, res, radius=10.0)[1]
            out["lddt_ligand"] = lddt(pos, ref, lig, radius=15.0)[1]
            ref_pocket = contacts_counts(np.asarray(ref)[None], res, lig, 8.0)["nearest"][0] < 8.0
            with np.errstate(invalid="ignore", divide="ignore"):
                out["pocket_recall"] = (out["pocket"].astype(bool) & ref_pocket).sum(1) / np.float64(ref_pocket.sum())
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------

def walk(rng, N):
    """A compact, roughly self-avoiding random walk of 3.8 Angstrom steps confined to a sphere of radius 2.6 N^(1/3) Angstrom (the density of
    a folded chain; never below 4 so that a step fits), centred; float32 [N,3].  Coordinates stay well inside +-100 Angstrom."""
    radius = max(2.6 * N ** (1.0 / 3.0), 4.0)
    p = np.zeros((N, 3))
    for i in range(1, N):
        best, best_clear = None, -1.0
        for _ in range(60):
            v = rng.normal(size=3)
            q = p[i - 1] + 3.8 * v / np.linalg.norm(v)
            if np.linalg.norm(q) > radius:
                continue
            clear = np.sqrt(((p[:i] - q) ** 2).sum(1)).min()
            if clear >= 3.0:
                best = q
                break
            if clear > best_clear:
                best, best_clear = q, clear
        if best is None:                        # no try stayed inside: step towards the centre
            best = p[i - 1] - 3.8 * p[i - 1] / max(np.linalg.norm(p[i - 1]), 1e-9)
        p[i] = best
    return (p - p.mean(0)).astype(np.float32)


def samples(rng, ref, S, start=0):
    """S variants of ``ref`` [N,3] float32, cycling through: the reference itself (sigma 0), its exact mirror image, the reference moved by
    1000 Angstrom as a whole, and Gaussian noise of sigma 0.3, 1 and 3 Angstrom -- from kind ``start`` on.  Returns (float32 [S,N,3], the kind of each)."""
    kinds = ["exact", "mirror", "far", "sigma0.3", "sigma1", "sigma3"]
    out, names = [], []
    for s in range(S):
        kind = kinds[(start + s) % len(kinds)]
        if kind == "exact":
            v = ref.copy()
        elif kind == "mirror":
            v = ref * np.array([1.0, 1.0, -1.0], dtype=np.float32)
        elif kind == "far":
            v = ref + np.float32(1000.0)
        else:
            v = ref + (float(kind[5:]) * rng.normal(size=ref.shape)).astype(np.float32)
        out.append(v.astype(np.float32))
        names.append(kind)
    return np.stack(out), names
