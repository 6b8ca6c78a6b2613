"""The yardstick of the backbone tests: prd_backbone.h restated in numpy, and the inputs the CPU and GPU tests share.

``build`` is the header's definition, formula by formula, in the dtype it is given: float64 is the yardstick, float32 is the same
restatement in the device's number format, whose deviation E from the yardstick on the very inputs of the GPU tests sets their
tolerance (tests/test_backbone.py).  ``built`` comes back as integers.

The device compares fp32 quantities, so it may disagree with float64 on a validity comparison whose two sides nearly coincide.  A
comparison a < b is AMBIGUOUS when |a - b| < BAND * max(|a|, |b|) with BAND = 1e-4 -- squared bond lengths of fp32 coordinates within
100 Angstrom are good to about 1e-5 relative, cross products of such bonds likewise.  A residue is ambiguous when any comparison that
either of its two peptides, or a virtual point they use, depends on is; ambiguous residues are left out of the comparisons, and the
inputs are seeded so that there are none in the exact family and at most CAP of the residues in the perturbed one."""
import functools
import math

import numpy as np

from protein_redesign_amd import backbone as BB

BAND, CAP = 1e-4, 0.005
# E: the largest deviation in Angstrom of the float32 restatement from the float64 one over the atoms of every case below, for the exact
# and for the perturbed family -- measured 1.19e-5 and 1.23e-5 (``measured_E``; tests/test_backbone_cpu.py holds the measurement to
# [E / 2, E]), about one and a half ulps of a coordinate of 100 Angstrom.  The device is allowed 4 E.
E = (1.5e-5, 1.5e-5)
TILE, HALO = 256, 3                     # the kernel's row tile and its halo (csrc/prd_backbone.hip)
N_, CA_, C_, CB_, O_ = range(5)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _less(a, b):
    """(a < b, the comparison is ambiguous)"""
    return a < b, np.abs(a - b) < BAND * np.maximum(np.abs(a), np.abs(b))


def _vertex(a, c, b, sin2):
    u, v = a - c, b - c
    w = _cross(u, v)
    return _less(sin2 * _dot(u, u) * _dot(v, v), _dot(w, w))


def _dyad(c, a, b, x):
    e = _unit(_unit(a - c) + _unit(b - c))
    d = x - c
    two = d.dtype.type(2.0)
    return c + two * e * _dot(e, d)[..., None] - d


def _peptide(pm, a, b, pn, table, g, dtype):
    """C and O from a, N from b, (valid, ambiguous) of the comparisons on the four points themselves"""
    l0, ac, rc, ao, ro, an, rn = g[:7]
    lo2, hi2, sin2 = g[10:13]
    bm, bb, bp = a - pm, b - a, pn - b
    ok, amb = np.ones(a.shape[:-1], bool), np.zeros(a.shape[:-1], bool)
    for v in (bm, bb, bp):
        for t, q in (_less(lo2, _dot(v, v)), _less(_dot(v, v), hi2)):
            ok, amb = ok & t, amb | q
    for t, q in (_vertex(pm, a, b, sin2), _vertex(a, b, pn, sin2)):
        ok, amb = ok & t, amb | q
    lb = np.sqrt(_dot(bb, bb))
    u = bb / lb[..., None]
    n = _unit(_cross(bm, bb))
    m = _cross(u, n)
    w = _cross(bb, bp)
    tau = np.arctan2(lb * _dot(bm, w), _dot(_cross(bm, bb), w))
    tau = np.where(tau < 0, tau + dtype(2.0 * math.pi), tau)
    f = tau * dtype(72.0 / (2.0 * math.pi))
    k = np.clip(np.nan_to_num(f, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int64), 0, 71)
    xi = table[k] + (f - k.astype(dtype)) * (table[k + 1] - table[k])
    p = np.cos(xi)[..., None] * n + np.sin(xi)[..., None] * m
    s = lb / l0
    c = a + (s * ac)[..., None] * u + rc * p
    o = a + (s * ao)[..., None] * u + ro * p
    nn = b + (s * an)[..., None] * u + rn * p
    return c, o, nn, ok, amb


def build(x, mask, link, spec=None, dtype=np.float64):
    """x [S,N,3] (the fp32 values the device reads), mask [N], link [N]; ``spec``: a backbone.Backbone (default: Backbone()).  Returns
    ``atoms`` [S,N,5,3] in ``dtype``, ``built`` [S,N] int32 and ``ambiguous`` [S,N] bool."""
    spec = BB.Backbone() if spec is None else spec
    g = [dtype(v) for v in spec.scalars()]
    table = spec.orientation.table().astype(dtype)
    x = np.asarray(x).astype(dtype)
    S, N = x.shape[:2]
    m = np.asarray(mask) > 0.5
    conn = np.zeros(N + 6, bool)                                 # conn[3 + k]: rows k and k + 1 belong to one run
    conn[3: N + 2] = (np.asarray(link)[:-1] > 0.5) & m[:-1] & m[1:]
    i = np.arange(N) + 3
    left = conn[i - 1].astype(int) * (1 + conn[i - 2] * (1 + conn[i - 3]))        # rows of the run before row i, counted up to 3
    right = conn[i].astype(int) * (1 + conn[i + 1] * (1 + conn[i + 2]))
    run = m & (left + right >= 3)
    xp = np.zeros((S, N + 6, 3), dtype)
    xp[:, 3: N + 3] = x
    q = {k: xp[:, i + k] for k in range(-3, 4)}
    sin2 = g[12]
    yes, no = np.ones((S, N), bool), np.zeros((S, N), bool)
    sel = lambda cond, a, b: np.where(np.broadcast_to(cond, (S, N))[..., None], a, b)       # noqa: E731
    with np.errstate(all="ignore"):
        # the left end: Q_-1 virtual where left == 0, Q_-2 virtual where left <= 1; the right end is its mirror image
        v1, a1 = _vertex(q[0], q[1], q[2], sin2)
        qm1 = sel(left == 0, _dyad(q[1], q[0], q[2], q[3]), q[-1])
        dm1, am1 = np.where(left == 0, v1, yes), np.where(left == 0, a1, no)
        v2, a2 = _vertex(qm1, q[0], q[1], sin2)
        qm2 = sel(left <= 1, _dyad(q[0], qm1, q[1], q[2]), q[-2])
        dm2, am2 = np.where(left <= 1, dm1 & v2, yes), np.where(left <= 1, am1 | a2, no)
        v1, a1 = _vertex(q[0], q[-1], q[-2], sin2)
        qp1 = sel(right == 0, _dyad(q[-1], q[0], q[-2], q[-3]), q[1])
        dp1, ap1 = np.where(right == 0, v1, yes), np.where(right == 0, a1, no)
        v2, a2 = _vertex(qp1, q[0], q[-1], sin2)
        qp2 = sel(right <= 1, _dyad(q[0], qp1, q[-1], q[-2]), q[2])
        dp2, ap2 = np.where(right <= 1, dp1 & v2, yes), np.where(right <= 1, ap1 | a2, no)
        _, _, nn, ok_a, amb_a = _peptide(qm2, qm1, q[0], qp1, table, g, dtype)           # peptide i - 1: N_i
        cc, oo, _, ok_b, amb_b = _peptide(qm1, q[0], qp1, qp2, table, g, dtype)          # peptide i: C_i, O_i
        has_n = run & ok_a & dm2 & dm1 & dp1
        has_c = run & ok_b & dm1 & dp1 & dp2
        b, c = q[0] - nn, cc - q[0]
        cb = q[0] + g[7] * _cross(b, c) + g[8] * b + g[9] * c
    atoms = np.zeros((S, N, 5, 3), dtype)
    zero = np.zeros((S, N, 3), dtype)
    atoms[:, :, N_] = sel(has_n, nn, zero)
    atoms[:, :, CA_] = sel(m[None], q[0], zero)
    atoms[:, :, C_] = sel(has_c, cc, zero)
    atoms[:, :, O_] = sel(has_c, oo, zero)
    atoms[:, :, CB_] = sel(has_n & has_c, cb, zero)
    built = has_n * 1 + np.broadcast_to(m[None], (S, N)) * 2 + has_c * 4 + (has_n & has_c) * 8 + has_c * 16
    ambiguous = run & (amb_a | amb_b | am1 | am2 | ap1 | ap2)
    return {"atoms": atoms, "built": built.astype(np.int32), "ambiguous": ambiguous}


def flags(built):
    """[...,5] bool from the bit mask"""
    return (np.asarray(built)[..., None] >> np.arange(5)) & 1 == 1


def dihedral(a, b, c, d):
    b1, b2, b3 = b - a, c - b, d - c
    return np.arctan2(np.sqrt(_dot(b2, b2)) * _dot(b1, _cross(b2, b3)), _dot(_cross(b1, b2), _cross(b2, b3)))


def rms(a, b):
    return float(np.sqrt(((a - b) ** 2).sum(-1).mean()))


def cb_volume(atoms):
    """(N - CA) . ((C - CA) x (CB - CA)): positive for an L-residue"""
    ca = atoms[..., CA_, :]
    return _dot(atoms[..., N_, :] - ca, _cross(atoms[..., C_, :] - ca, atoms[..., CB_, :] - ca))


# ---- the cases the CPU and GPU tests share ----------------------------------------------------------------------------------------------

WEIGHTS = (0.4, 0.1, 0.15, 0.1, 0.15, 0.1)            # how often a stretch takes each of backbone.ANCHORS: helix-heavy keeps chains compact


def chain(rng, L, noise=10.0):
    """[L,5,3]: an ideal chain whose (phi, psi) run through the anchors in stretches of 5 to 12 residues, with Gaussian noise of ``noise``
    degrees on every angle.  Its virtual bonds are all L0 and its C-alpha vertices lie between about 80 and 150 degrees."""
    phi, psi = np.zeros(L), np.zeros(L)
    k = 0
    while k < L:
        a = BB.ANCHORS[int(rng.choice(len(BB.ANCHORS), p=WEIGHTS))]
        n = int(rng.integers(5, 13))
        phi[k: k + n], psi[k: k + n] = a[0], a[1]
        k += n
    return BB.ideal_chain(phi + noise * rng.normal(size=L), psi + noise * rng.normal(size=L))


def run_lengths(layout, na, N):
    """the lengths of the runs that fill rows na .. N-1, and whether the link after each run is SET although the next run is far away
    (the bond window then refuses the peptides round it)"""
    nr = N - na
    if layout == "one":
        want = [nr]
    elif layout == "two4":
        want = [4, 4]
    elif layout in ("tileA", "tileB"):                 # one link broken exactly at T-1 | T (A) or at T | T+1 (B); the runs round it are long
        cut = (TILE if layout == "tileA" else TILE + 1) - na
        first = [40] * ((cut - 50) // 40)
        want = first + [cut - sum(first)] + [60] * ((nr - cut) // 60 + 1)
    elif layout == "short":                             # runs of 1, 2 and 3 between longer ones
        want = [6, 1, 9, 2, 5, 3, 12, 4] * (nr // 42 + 1)
    else:                                               # "seg": runs of 60, which cross every tile edge of N = 1100
        want = [60] * (nr // 60 + 1)
    out, left = [], nr
    for n in want:
        if left <= 0:
            break
        out.append(min(n, left))
        left -= out[-1]
    if left > 0:
        out.append(left)
    joined = [layout == "seg" and k % 3 == 2 for k in range(len(out))]
    return out, joined


# (N, S, ligand rows in front, layout, strided)
CASES = [(1, 1, 0, "one", False), (3, 1, 0, "one", False), (4, 5, 0, "one", False), (5, 1, 0, "one", False), (7, 1, 3, "one", False),
         (8, 5, 0, "two4", False), (TILE - 1, 1, 17, "short", False), (TILE, 5, 3, "seg", False), (TILE + 1, 5, 0, "tileA", True),
         (TILE + 3, 7, 17, "tileB", False), (TILE + 3, 1, 3, "tileA", False), (1100, 5, 17, "seg", True), (1100, 1, 0, "short", False),
         (1100, 1, 3, "tileB", False)]
IDS = ["N%d-S%d-na%d-%s%s" % (c[0], c[1], c[2], c[3], "-strided" if c[4] else "") for c in CASES]
SEEDS = {}                              # case -> seed, where the default has an ambiguous comparison in the exact family
SIGMA = 0.3                             # Angstrom: the Gaussian noise of the perturbed family


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """the inputs of a case as the device takes them (fp32 numpy), with the float64 yardstick and the float32 restatement of them.
    Structure s is EXACT (an ideal chain per run) for even s and PERTURBED (sigma = 0.3 Angstrom on every coordinate) for odd s."""
    N, S, na, layout, _ = case
    rng = np.random.default_rng(SEEDS.get(case, 1000 * N + 10 * S + na))
    lengths, joined = run_lengths(layout, na, N)
    mask, link = np.zeros(N), np.zeros(N)
    mask[na:] = 1.0
    r0 = na
    for L, j in zip(lengths, joined):
        link[r0: r0 + L - 1] = 1.0
        link[r0 + L - 1] = 1.0 if j and r0 + L < N else 0.0
        r0 += L
    x = np.zeros((S, N, 3))
    for s in range(S):
        x[s, :na] = rng.uniform(-30.0, 30.0, (na, 3))
        r0 = na
        for L in lengths:
            ca = chain(rng, L)[:, CA_]
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            q *= np.sign(np.linalg.det(q))
            # runs sit on a coarse grid, the long ones near the origin: every coordinate stays within 100 Angstrom
            x[s, r0: r0 + L] = (ca - ca.mean(0)) @ q.T + rng.integers(-2, 3, 3) * (15.0 if L <= 60 else 5.0) + rng.uniform(-2, 2, 3)
            r0 += L
        if s % 2 == 1:
            x[s] += SIGMA * rng.normal(size=(N, 3))
    x = x.astype(np.float32)
    mask, link = mask.astype(np.float32), link.astype(np.float32)
    return dict(x=x, mask=mask, link=link, exact=[s for s in range(S) if s % 2 == 0], ref=build(x, mask, link),
                f32=build(x, mask, link, dtype=np.float32))


def deviation(a, b, keep):
    """the maximum absolute deviation in Angstrom of atoms ``a`` from ``b`` over the atoms ``keep`` [S,N,5] marks"""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)).max(-1)
    return float(d[keep].max(initial=0.0))


def comparable(I):
    """[S,N,5] bool: the atoms both restatements build, outside the ambiguity band"""
    return flags(I["ref"]["built"]) & flags(I["f32"]["built"]) & ~I["ref"]["ambiguous"][..., None]


@functools.lru_cache(maxsize=None)
def measured_E():
    """E: the deviation of the float32 restatement from the float64 one over every case, (exact family, perturbed family)"""
    e = [0.0, 0.0]
    for case in CASES:
        I = case_inputs(case)
        keep = comparable(I)
        for s in range(case[1]):
            k = 0 if s in I["exact"] else 1
            e[k] = max(e[k], deviation(I["f32"]["atoms"][s], I["ref"]["atoms"][s], keep[s]))
    return tuple(e)


def mirror(x, axis=0):
    y = np.array(x, copy=True)
    y[..., axis] = -y[..., axis]
    return y
