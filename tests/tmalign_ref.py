"""Float64 numpy statement of the structural alignment of include/prd_tmalign.h (a cut of TM-align: secondary structure, three initial
alignments, Needleman-Wunsch refinement with Kabsch fits, the TM-score search of prd_align.h on the aligned pairs) -- the yardstick of
the tests, not product code.  Every step is written as the header words it.  ``f32_scores=True`` rounds every DP score matrix to
float32 before the (float64) recurrence: the tests keep a case only where that leaves the mapping unchanged."""
import numpy as np

import align_ref as AR

MIN_L = 5
MAX_ROUNDS = 30
GAPS = (-0.6, 0.0)
COIL, HELIX, STRAND, TURN = 0, 1, 2, 3


def d8_of(Ly):
    return 1.5 * Ly ** 0.3 + 3.5


def sec_classes(x):
    """[L] classes of the C-alpha trace x [L,3] (header, step 1)"""
    L = len(x)
    out = np.zeros(L, np.int64)
    if L < 5:
        return out
    c = np.arange(2, L - 2)

    def d(a, b):
        return np.sqrt(((x[c + a] - x[c + b]) ** 2).sum(-1))
    d13, d14, d15, d24, d25, d35 = d(-2, 0), d(-2, 1), d(-2, 2), d(-1, 1), d(-1, 2), d(0, 2)
    helix = (np.abs(d15 - 6.37) < 2.1) & (np.abs(d14 - 5.18) < 1.42) & (np.abs(d25 - 5.18) < 1.42) \
        & (np.abs(d13 - 5.45) < 0.81) & (np.abs(d24 - 5.45) < 0.81) & (np.abs(d35 - 5.45) < 0.81)
    strand = (np.abs(d15 - 13.0) < 1.42) & (np.abs(d14 - 10.4) < 1.42) & (np.abs(d25 - 10.4) < 1.42) \
        & (np.abs(d13 - 6.1) < 1.42) & (np.abs(d24 - 6.1) < 1.42) & (np.abs(d35 - 6.1) < 1.42)
    out[c] = np.where(helix, HELIX, np.where(strand, STRAND, np.where(d15 < 8.0, TURN, COIL)))
    return out


def dp(s, gap):
    """mapping [Lx] (j or -1) of the DP of the header's step 3 on the score matrix s [Lx,Ly]"""
    Lx, Ly = s.shape
    val = np.zeros((Lx + 1, Ly + 1))
    dg = np.zeros((Lx + 1, Ly + 1), bool)
    dr = np.zeros((Lx + 1, Ly + 1), np.int8)
    for d in range(2, Lx + Ly + 1):
        i = np.arange(max(1, d - Ly), min(Lx, d - 1) + 1)
        j = d - i
        D = val[i - 1, j - 1] + s[i - 1, j - 1]
        H = val[i - 1, j] + np.where(dg[i - 1, j], gap, 0.0)
        V = val[i, j - 1] + np.where(dg[i, j - 1], gap, 0.0)
        isd = (D >= H) & (D >= V)
        val[i, j] = np.maximum(D, np.maximum(H, V))
        dg[i, j] = isd
        dr[i, j] = np.where(isd, 0, np.where(H >= V, 1, 2))
    amap = np.full(Lx, -1, np.int64)
    i, j = Lx, Ly
    while i > 0 and j > 0:
        if dr[i, j] == 0:
            amap[i - 1] = j - 1
            i, j = i - 1, j - 1
        elif dr[i, j] == 1:
            i -= 1
        else:
            j -= 1
    return amap


def seeds(n, levels=None):
    """AR.seeds(n), cut to the first ``levels`` fragment lengths"""
    sd = AR.seeds(n)
    if levels is None:
        return sd
    keep = []
    for _, Lf in sd:
        if Lf not in keep:
            keep.append(Lf)
    keep = keep[:levels]
    return [(a, Lf) for a, Lf in sd if Lf in keep]


def search(x, y, d0, levels=None):
    """(sum of TM terms, R, t): the search of prd_align.h steps 1-4 over the aligned pairs x[k] <-> y[k] with the d0 given"""
    n = len(x)
    d0s = min(max(d0, 4.5), 8.0)
    best = (-1.0, None, None)
    for start, Lf in seeds(n, levels):
        sub = np.zeros(n, bool)
        sub[start:start + Lf] = True
        for it in range(20):
            R, t = AR.kabsch(x[sub], y[sub])
            d = AR.dist(x, y, R, t)
            sc = float((1.0 / (1.0 + (d / d0) ** 2)).sum())
            if sc > best[0]:
                best = (sc, R, t)
            cut = d0s - 1.0 if it == 0 else d0s + 1.0
            while (d < cut).sum() < 3:
                cut += 0.5
            new = d < cut
            if np.array_equal(new, sub):
                break
            sub = new
    return best


def score_matrix(x, y, R, t, d0):
    xt = t + x @ R
    d2 = ((xt[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    return 1.0 / (1.0 + d2 / d0 ** 2)


def threading(x, y, d0):
    """(mapping, R, t) of the best gapless offset (header, step 2 A)"""
    Lx, Ly = len(x), len(y)
    need = max(min(Lx, Ly) // 2, 5)
    best = (-1.0, None, None, None)
    for k in range(-(Lx - 1), Ly):
        i0, i1 = max(0, -k), min(Lx, Ly - k)
        if i1 - i0 < need:
            continue
        R, t = AR.kabsch(x[i0:i1], y[i0 + k:i1 + k])
        sc = float((1.0 / (1.0 + (AR.dist(x[i0:i1], y[i0 + k:i1 + k], R, t) / d0) ** 2)).sum())
        if sc > best[0]:
            best = (sc, k, R, t)
    _, k, R, t = best
    amap = np.full(Lx, -1, np.int64)
    i0, i1 = max(0, -k), min(Lx, Ly - k)
    amap[i0:i1] = np.arange(i0 + k, i1 + k)
    return amap, R, t


def refine(x, y, amap, d0, rnd):
    """(score, mapping, R, t) or None: the header's step 4 from the initial mapping"""
    if (amap >= 0).sum() < 3:
        return None
    a = amap >= 0
    sc, R, t = search(x[a], y[amap[a]], d0, levels=2)
    best = (sc, amap, R, t)
    for gap in GAPS:
        for _ in range(MAX_ROUNDS):
            new = dp(rnd(score_matrix(x, y, R, t, d0)), gap)
            if np.array_equal(new, amap) or (new >= 0).sum() < 3:
                break
            amap = new
            a = amap >= 0
            sc, R, t = search(x[a], y[amap[a]], d0, levels=2)
            if sc > best[0]:
                best = (sc, amap, R, t)
    return best


def align_unmirrored(x, y, rnd):
    Lx, Ly = len(x), len(y)
    d0 = AR.d0_of(Ly)
    sx, sy = sec_classes(x), sec_classes(y)
    same = (sx[:, None] == sy[None, :]).astype(np.float64)
    mapA, RA, tA = threading(x, y, d0)
    inits = [mapA, dp(same, -1.0), dp(rnd(0.5 * same + score_matrix(x, y, RA, tA, d0)), -1.0)]
    best = None
    for m in inits:
        r = refine(x, y, m, d0, rnd)
        if r is not None and (best is None or r[0] > best[0]):
            best = r
    _, amap, R, t = best
    a = np.nonzero(amap >= 0)[0]
    near = AR.dist(x[a], y[amap[a]], R, t) <= d8_of(Ly)
    if near.sum() >= 3:
        amap = amap.copy()
        amap[a[~near]] = -1
    a = amap >= 0
    sc, R, t = search(x[a], y[amap[a]], d0)
    return sc / Ly, amap, R, t


def score_of(x, y, amap, R, t):
    """(tm, rmsd, n_aligned) of a mapping under a transform: TM normalised by len(y) with d0(len(y))"""
    a = amap >= 0
    n = int(a.sum())
    if n == 0:
        return 0.0, 0.0, 0
    d = AR.dist(x[a], y[amap[a]], R, t)
    return float((1.0 / (1.0 + (d / AR.d0_of(len(y))) ** 2)).sum() / len(y)), float(np.sqrt((d ** 2).mean())), n


def align(x, y, mirror=True, f32_scores=False):
    """dict(tm, rmsd, n_aligned, rotation, translation, mirrored, mapping) for ONE pair of compacted structures [Lx,3], [Ly,3]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    Lx, Ly = len(x), len(y)
    if Lx < MIN_L or Ly < MIN_L:
        return dict(tm=0.0, rmsd=0.0, n_aligned=0, rotation=np.eye(3), translation=np.zeros(3), mirrored=0, mapping=np.full(Lx, -1, np.int64))
    rnd = (lambda s: s.astype(np.float32).astype(np.float64)) if f32_scores else (lambda s: s)
    cands = []
    for m in ([0, 1] if mirror else [0]):
        tm, amap, R, t = align_unmirrored(x @ AR.MIRROR if m else x, y, rnd)
        cands.append((tm, amap, AR.MIRROR @ R if m else R, t, m))
    tm, amap, R, t, m = cands[1] if len(cands) == 2 and cands[1][0] > cands[0][0] else cands[0]
    tm, rmsd, n = score_of(x, y, amap, R, t)
    return dict(tm=tm, rmsd=rmsd, n_aligned=n, rotation=R, translation=t, mirrored=m, mapping=amap)


# ---- the planted cases of the tests --------------------------------------------------------------------------------------------

def ss_chain(rng, L):
    """C-alpha trace of 3.8 Angstrom steps: helical stretches (2.3 Angstrom radius, 1.5 rise, 100 degrees per residue), extended ones
    (a 3.2 / 2.05 zigzag) and random-walk coil in between, each in a random orientation; centred and scaled as AR.chain"""
    pts = [np.zeros(3)]
    while len(pts) < L:
        kind = int(rng.integers(0, 3))
        n = int(rng.integers(6, 15))
        k = np.arange(1, n + 1)
        if kind == 0:
            a = np.deg2rad(100.0) * k
            seg = np.stack([2.3 * (np.cos(a) - 1.0), 2.3 * np.sin(a), 1.5 * k], 1)
        elif kind == 1:
            seg = np.stack([3.2 * k, 2.05 * (k % 2), np.zeros(n)], 1)
        else:
            st = rng.normal(size=(n, 3))
            seg = np.cumsum(st * (3.8 / np.linalg.norm(st, axis=1, keepdims=True)), 0)
        seg = seg @ AR.random_rotation(rng)
        seg *= 3.8 / np.linalg.norm(seg[0])             # the joining step is 3.8 too (helix and zigzag start with a shorter chord)
        pts += list(pts[-1] + seg)
    c = np.array(pts[:L])
    c -= c.mean(0)
    r = np.abs(c).max()
    return c * (60.0 / r) if r > 60.0 else c


def planted(rng, Lx, Ly, core_fraction, mirrored=False, indels=True, noise=0.5):
    """(x [Lx,3], y [Ly,3], R0, t0, mapping [Lx]): y is a rigid motion of x (of its mirror image if asked) with an N-terminal
    deletion, an internal deletion and an internal insertion of 3-12 residues each where the lengths allow (what is left of Ly - Lx
    is a C-terminal truncation or extension), 0.5 Angstrom noise on a contiguous core of the planted pairs and an unrelated chain
    elsewhere.  ``mapping`` is the planted alignment: the pairs of the core (outside it y is an unrelated chain: nothing is planted)."""
    x = ss_chain(rng, Lx)
    R0 = AR.random_rotation(rng)
    t0 = rng.uniform(-8.0, 8.0, size=3)
    src = list(range(Lx))                               # x index of each y row, -1 for an inserted residue
    if indels and min(Lx, Ly) >= 40:
        a, b, c = (int(v) for v in rng.integers(3, 13, size=3))
        src = src[a:]
        p = int(rng.integers(5, len(src) - b - 5))
        src = src[:p] + src[p + b:]
        q = int(rng.integers(5, len(src) - 5))
        src = src[:q] + [-1] * c + src[q:]
    elif indels and Lx > Ly:
        a = int(rng.integers(0, Lx - Ly + 1))
        src = src[a:]
    if len(src) > Ly:
        src = src[:Ly]
    src = np.array(src + [-1] * (Ly - len(src)), np.int64)
    xm = x @ AR.MIRROR if mirrored else x
    img = t0 + xm @ R0
    y = ss_chain(rng, Ly)
    pairs = np.nonzero(src >= 0)[0]
    n = len(pairs) if core_fraction >= 1.0 else max(3, int(round(core_fraction * len(pairs))))
    start = int(rng.integers(0, len(pairs) - n + 1))
    core = pairs[start:start + n]
    y[core] = img[src[core]] + noise * rng.normal(size=(n, 3))
    if core_fraction >= 1.0:                            # inserted residues continue the chain from the residue before them
        for j in np.nonzero(src < 0)[0]:
            st = rng.normal(size=3)
            y[j] = (y[j - 1] if j > 0 else img[0]) + st * (3.8 / np.linalg.norm(st))
    amap = np.full(Lx, -1, np.int64)
    amap[src[core]] = core
    return x, y, (AR.MIRROR @ R0 if mirrored else R0), t0, amap
