"""The yardstick of the secondary-structure tests: include/prd_dssp.h restated in numpy, O(N^2), and the inputs the CPU and GPU tests share.

``hbonds`` and ``assign`` are the header's definitions in the dtype they are given: float64 is the yardstick, float32 the same
restatement in the device's number format, whose deviation E_TOL from the yardstick on the very inputs of the GPU tests sets their
tolerance.  The yardstick knows nothing of the device's method: the lists come from a full sort of the N x N energies, the bridges from
the N x N bond matrix.

AMBIGUITY.  The device decides on fp32 energies, so it may disagree with float64 wherever two sides of a comparison nearly coincide.
The band is B = 1e-3 kcal/mol (DSSP's own print granularity; the CPU test holds B >= 8 E_TOL, so the band cannot hide a wrong
decision).  A near-tie has one of two reaches, and the yardstick reports them apart:
  ``ambiguous`` [S,N]: the residue is an endpoint of a candidate pair on which a BOND may be decided otherwise --
    - its energy lies within B of ``cutoff``;
    - it is among the first three of one of its lists, two neighbouring ranks of those three lie within B of each other, and the lower
      of the two energies lies below ``cutoff`` + B (who is listed decides a bond);
    - one of its four distances lies within 1e-4 Angstrom of 0.5;
    or the residue's bend cosine lies within 1e-5 of ``cos_bend``.
  ``loose`` [S,N,4]: the slot may be FILLED otherwise although no bond depends on it -- the slots of a list in which two neighbouring
    ranks of the first three lie within B of each other above the cutoff (ranks 2 and 3 decide who is listed, ranks 1 and 2 the order),
    or in which an energy within B of 0 would rank in the first two.  Such a tie changes what the list's owner reports in those two
    slots and nothing else: no list of another residue, and no bond, since a bond needs an energy below the cutoff.
``partner`` and ``energy`` are compared on every slot that is not loose of every residue that is not ambiguous; classes, bridges and
flags on every residue farther than EXCLUDE = 10 rows from an ambiguous one -- the reach of one bond decision through bridge, ladder and
the emptiness tests of G and I.  The caps (none in the exact family, 2 % in the perturbed one) hold for ``ambiguous``."""
import functools
import os

import numpy as np

import backbone_ref as BR
from protein_redesign_amd import backbone as BB
from protein_redesign_amd import dssp as DS

B = 1e-3                                # kcal/mol: the ambiguity band
# E_TOL: the largest deviation in kcal/mol of the float32 restatement's reported energies from the float64 ones over every case below
# (``measured_E``; tests/test_dssp_cpu.py holds the measurement to [E_TOL / 2, E_TOL]).  The device is allowed 4 E_TOL.
E_TOL = 3.5e-5
EXCLUDE = 10
CAP_AMBIGUOUS, CAP_EXCLUDED = 0.02, 0.25
ROWS, COLS, TILE, HALO = 64, 256, 256, 10       # the sweep's row and column tile, the per-residue tile and its halo (csrc/side/prd_dssp.hip)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dssp_sheets.npz")
N_, CA_, C_, CB_, O_ = range(5)


def _dist(a, b):
    d = b - a
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _roles(atoms, built, link, donor):
    """acceptor [S,N], donor [S,N], hydrogen [S,N,3] (zeros where there is none)"""
    S, N = built.shape
    lk = np.zeros(N, bool)
    lk[: N - 1] = np.asarray(link)[: N - 1] > 0.5
    acc = (built & 20) == 20
    don = np.zeros((S, N), bool)
    don[:, 1:] = ((built[:, 1:] & 1) == 1) & lk[None, : N - 1] & acc[:, : N - 1]
    if donor is not None:
        don &= (np.asarray(donor) > 0.5)[None]
    h = np.zeros_like(atoms[:, :, 0])
    with np.errstate(all="ignore"):
        co = atoms[:, : N - 1, C_] - atoms[:, : N - 1, O_]
        l = np.sqrt((co[..., 0] * co[..., 0] + co[..., 1] * co[..., 1]) + co[..., 2] * co[..., 2])
        h[:, 1:] = atoms[:, 1:, N_] + co / l[..., None]
    h[~don] = 0
    return acc, don, h, lk


def energies(atoms, built, link, donor=None, spec=None, dtype=np.float64):
    """E [S,N(acceptor),N(donor)] in ``dtype`` (0 where the pair is no candidate), the candidate mask, and the mask of pairs with a distance
    within 1e-4 Angstrom of 0.5"""
    spec = DS.Dssp() if spec is None else spec
    q, e_min = (dtype(v) for v in spec.scalars()[:2])
    atoms, built = np.asarray(atoms).astype(dtype), np.asarray(built)
    S, N = built.shape
    acc, don, h, lk = _roles(atoms, built, link, donor)
    idx = np.arange(N)
    cand = acc[:, :, None] & don[:, None, :] & (idx[:, None] != idx[None, :])[None]
    cand &= ~((idx[:, None] == idx[None, :] - 1) & lk[:, None])[None]
    c, o, n = atoms[:, :, None, C_], atoms[:, :, None, O_], atoms[:, None, :, N_]
    hh = h[:, None, :]
    one, half = dtype(1.0), dtype(0.5)
    with np.errstate(all="ignore"):
        r = [_dist(o, n), _dist(c, hh), _dist(o, hh), _dist(c, n)]
        e = q * (((one / r[0] + one / r[1]) - one / r[2]) - one / r[3])
        close = (r[0] < half) | (r[1] < half) | (r[2] < half) | (r[3] < half)
        e = np.where(close, e_min, np.maximum(e, e_min))
        edge = np.zeros_like(close)
        for x in r:
            edge |= np.abs(x.astype(np.float64) - 0.5) < 1e-4
    e = np.where(cand, e, dtype(0.0))
    return e, cand, edge & cand


def _lists(e, cand):
    """partner [S,N,4], energy [S,N,4] from the full sort of every list by (energy, index)"""
    S, N = e.shape[:2]
    partner, energy = np.full((S, N, 4), -1, np.int32), np.zeros((S, N, 4), e.dtype)
    for s in range(S):
        for role, m, ok in ((0, e[s].T, cand[s].T), (1, e[s], cand[s])):       # role 0: row = donor, columns = acceptors
            keep = ok & (m < 0)
            key = np.where(keep, m, np.inf)
            order = np.argsort(key, axis=1, kind="stable")[:, :2]               # stable: equal energies go by the lower index
            for k in range(min(2, N)):
                j = order[:, k]
                have = keep[np.arange(N), j]
                partner[s, have, role * 2 + k] = j[have]
                energy[s, have, role * 2 + k] = m[np.arange(N), j][have]
    return partner, energy


def _list_ambiguity(e, cand, cutoff):
    """ambiguous [S,N] and loose [S,N,4] of the lists (the head of this file)"""
    S, N = e.shape[:2]
    amb, loose = np.zeros((S, N), bool), np.zeros((S, N, 4), bool)
    e = e.astype(np.float64)
    for s in range(S):
        near = cand[s] & (np.abs(e[s] - cutoff) < B)
        amb[s] |= near.any(1) | near.any(0)
        for role, m, ok in ((0, e[s].T, cand[s].T), (1, e[s], cand[s])):
            key = np.where(ok, m, np.inf)
            order = np.argsort(key, axis=1, kind="stable")
            srt = np.take_along_axis(key, order, 1)
            second = srt[:, min(1, N - 1)][:, None]                         # fewer than two energies of the list lie below m: m <= the second
            zero = (ok & (np.abs(m) < B) & (m <= second)).any(1)            # an energy near 0 that would rank in the first two
            loose[s, zero, 2 * role: 2 * role + 2] = True
            for k in range(min(2, N - 1)):                                  # ranks k+1 and k+2 of the first three
                a, b = srt[:, k], srt[:, k + 1]
                with np.errstate(invalid="ignore"):                         # inf - inf: a list with fewer entries
                    tie = np.isfinite(a) & np.isfinite(b) & (a < 0) & (np.abs(a - b) < B)
                loose[s, tie, 2 * role: 2 * role + 2] = True
                deep = tie & (a < cutoff + B)                               # a bond may depend on it: the owner and both partners
                amb[s] |= deep
                for col in (order[:, k], order[:, k + 1]):
                    amb[s, col[deep]] = True
    return amb, loose


def hbonds(atoms, built, link, donor=None, spec=None, dtype=np.float64):
    spec = DS.Dssp() if spec is None else spec
    e, cand, edge = energies(atoms, built, link, donor, spec, dtype)
    partner, energy = _lists(e, cand)
    amb, loose = _list_ambiguity(e, cand, spec.scalars()[2])
    return {"partner": partner, "energy": energy, "ambiguous": amb | edge.any(1) | edge.any(2), "loose": loose}


def assign(atoms, built, link, donor=None, spec=None, dtype=np.float64):
    """the whole definition: ``classes`` [S,N] uint8, ``flags`` [S,N] int32, ``bridge`` [S,N,2] int32, ``partner``, ``energy`` [S,N,4],
    ``ambiguous`` [S,N], ``loose`` [S,N,4] and ``excluded`` [S,N] (within EXCLUDE rows of an ambiguous residue)"""
    spec = DS.Dssp() if spec is None else spec
    hb = hbonds(atoms, built, link, donor, spec, dtype)
    cutoff, cos_bend = (dtype(v) for v in spec.scalars()[2:])
    atoms, built = np.asarray(atoms).astype(dtype), np.asarray(built)
    S, N = built.shape
    lkv = np.zeros(N + 12, bool)                                # lk(k) at lkv[k + 6]
    lkv[6: 6 + N - 1] = np.asarray(link)[: N - 1] > 0.5
    lk = lambda k: lkv[np.asarray(k) + 6]                       # noqa: E731
    classes, flags, bridge = np.zeros((S, N), np.uint8), np.zeros((S, N), np.int32), np.full((S, N, 2), -1, np.int32)
    amb = hb["ambiguous"].copy()
    I, J = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    for s in range(S):
        p, en = hb["partner"][s], hb["energy"][s]
        bd = np.zeros((N, N), bool)                             # bd[a, d]
        for k in (0, 1):
            d = np.nonzero((p[:, k] >= 0) & (en[:, k] < cutoff))[0]
            a = p[d, k]
            mutual = (p[a, 2] == d) | (p[a, 3] == d)
            bd[a[mutual], d[mutual]] = True

        def bond(a, d):
            ok = (a >= 0) & (a < N) & (d >= 0) & (d < N)
            return bd[np.clip(a, 0, N - 1), np.clip(d, 0, N - 1)] & ok
        ok = (np.abs(I - J) >= 3) & lk(I - 1) & lk(I) & lk(J - 1) & lk(J)
        par = ok & ((bond(I - 1, J) & bond(J, I + 1)) | (bond(J - 1, I) & bond(I, J + 1)))
        anti = ok & ((bond(I, J) & bond(J, I)) | (bond(I - 1, J + 1) & bond(J - 1, I + 1)))

        def at(m, i, j):
            return 0 <= i < N and 0 <= j < N and bool(m[i, j])
        turn = np.zeros((3, N + 12), bool)                      # Turn_n(k) at turn[n - 3, k + 6]
        f = np.zeros(N, np.int32)
        for i in range(N):
            for n in (3, 4, 5):
                if all(lk(i + k) for k in range(n)) and i + n < N and bd[i, i + n]:
                    turn[n - 3, i + 6] = True
                    f[i] |= DS.FLAG_TURN3 << (n - 3)
            js = np.nonzero(par[i] | anti[i])[0][:2]
            ladder = False
            for k, j in enumerate(js):
                bridge[s, i, k] = j
                if par[i, j]:
                    f[i] |= DS.FLAG_BRIDGE[2 * k]
                    ladder |= at(par, i + 1, j + 1) or at(par, i - 1, j - 1)
                if anti[i, j]:
                    f[i] |= DS.FLAG_BRIDGE[2 * k + 1]
                    ladder |= at(anti, i + 1, j - 1) or at(anti, i - 1, j + 1)
            if ladder:
                f[i] |= DS.FLAG_LADDER
            if 2 <= i < N - 2 and all(lk(i + k) for k in (-2, -1, 0, 1)) and all(built[s, i + k] & 2 for k in (-2, 0, 2)):
                u, v = atoms[s, i, CA_] - atoms[s, i - 2, CA_], atoms[s, i + 2, CA_] - atoms[s, i, CA_]
                dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]      # noqa: E731
                with np.errstate(all="ignore"):
                    cos = dot(u, v) / (np.sqrt(dot(u, u)) * np.sqrt(dot(v, v)))
                if cos < cos_bend:
                    f[i] |= DS.FLAG_BEND
                if abs(float(cos) - float(cos_bend)) < 1e-5:
                    amb[s, i] = True
        flags[s] = f
        t = lambda n, k: bool(turn[n - 3, k + 6])               # noqa: E731
        bridged, ladder = bridge[s, :, 0] >= 0, (f & DS.FLAG_LADDER) != 0
        c = np.zeros(N + 12, np.uint8)                          # class of row k at c[k]; rows past the end stay 0
        for r in range(N):
            if any(t(4, i - 1) and t(4, i) for i in range(r - 3, r + 1)):
                c[r] = 1
            elif bridged[r]:
                c[r] = 3 if ladder[r] else 2
        for i in range(N):                                      # G: a minimal 3-helix none of whose residues is H, B or E
            if t(3, i - 1) and t(3, i) and not any(c[i + k] in (1, 2, 3) for k in range(3)):
                for k in range(3):
                    c[i + k] = 4 if c[i + k] in (0, 4) else c[i + k]
        g = c.copy()
        for i in range(N):                                      # I: the same with five residues, none H, B, E or G
            if t(5, i - 1) and t(5, i) and not any(g[i + k] in (1, 2, 3, 4) for k in range(5)):
                for k in range(5):
                    c[i + k] = 5
        for r in range(N):
            if c[r] == 0:
                if any(t(n, r - k) for n in (3, 4, 5) for k in range(1, n)):
                    c[r] = 6
                elif f[r] & DS.FLAG_BEND:
                    c[r] = 7
        c = c[:N]
        c[(built[s] & 2) == 0] = 0
        classes[s] = c
    excluded = np.zeros((S, N), bool)
    for s, i in zip(*np.nonzero(amb)):
        excluded[s, max(0, i - EXCLUDE): i + EXCLUDE + 1] = True
    return {"classes": classes, "flags": flags, "bridge": bridge, "partner": hb["partner"], "energy": hb["energy"], "ambiguous": amb,
            "loose": hb["loose"], "excluded": excluded}


def strings(classes):
    return ["".join(DS.ALPHABET[k] for k in row) for row in classes]


# ---- chains and fixtures ------------------------------------------------------------------------------------------------------------------

ALPHA, THREE10, STRAND = (-57.0, -47.0), (-49.0, -26.0), (-139.0, 135.0)


def regular(phi_psi, L):
    """[L,5,3]: the ideal chain of one conformation"""
    return BB.ideal_chain([phi_psi[0]] * L, [phi_psi[1]] * L)


def whole(chain, link=None):
    """(atoms [1,L,5,3] fp32, built [1,L] all 31, link [L]) of one all-atom chain"""
    L = len(chain)
    return np.asarray(chain, np.float32)[None], np.full((1, L), 31, np.int32), (np.ones(L, np.float32) if link is None else link)


@functools.lru_cache(maxsize=None)
def sheets():
    """{"anti": [16,5,3], "par": [16,5,3]}: two ideal 8-residue strands each, rows 0 .. 7 and 8 .. 15, placed rigidly by a search on the
    CPU so that they pair (tests/golden/dssp_sheets.npz; float64)"""
    with np.load(GOLDEN) as z:
        return {k: z[k].copy() for k in ("anti", "par")}


SHEET_LINK = np.r_[np.ones(7), 0.0, np.ones(7), 0.0].astype(np.float32)


# a segment: (kind, length).  "chain": an ideal chain wandering through the anchors; "alpha" / "310" / "strand": one conformation;
# "anti" / "par": the first (A) or second (B) strand of a sheet fixture, the two of a sample keeping their relative pose
def _segments(layout, nr):
    if layout == "one":
        want = [("chain", nr)]
    elif layout == "breaks":                            # a chain break at 63 | 64 and at 255 | 256 (ROWS and COLS edges), na = 0
        want = [("chain", 64), ("alpha", 60), ("chain", 60), ("chain", 72), ("chain", nr)]
    elif layout == "helix_edge":                        # a helix straddling the tile edge: rows 244 .. 267
        want = [("chain", 60)] * 4 + [("chain", 4), ("alpha", 24)] + [("chain", 60)] * 10
    elif layout == "sheet_edge":                        # a strand pair whose partners sit in different tiles: rows 240 .. 247 and 262 .. 269
        want = [("chain", 60)] * 4 + [("antiA", 8), ("chain", 14), ("antiB", 8), ("parA", 8), ("310", 12), ("parB", 8)] + [("chain", 60)] * 10
    elif layout == "short":                             # runs of 1 .. 4 between longer ones
        want = [("chain", 30), ("chain", 1), ("alpha", 12), ("chain", 2), ("310", 9), ("chain", 3), ("chain", 25), ("chain", 4)] * (nr // 86 + 1)
    else:
        raise ValueError(layout)
    out, left = [], nr
    for kind, n in want:
        if left <= 0:
            break
        if kind[:-1] in ("anti", "par") and left < n:
            kind = "chain"
        out.append((kind, min(n, left)))
        left -= out[-1][1]
    return out


# (N, S, ligand rows in front, layout, donor mask)
HB_CASES = [(1, 1, 0, "one", False), (2, 1, 0, "one", False), (5, 3, 0, "one", False), (63, 1, 3, "one", False), (64, 3, 0, "one", False),
            (65, 1, 17, "one", False), (255, 1, 0, "short", False), (256, 3, 3, "short", True), (257, 1, 17, "short", False),
            (300, 3, 0, "breaks", False)]
AS_CASES = [(255, 1, 3, "short", False), (256, 3, 0, "helix_edge", False), (257, 1, 17, "short", False), (256 + HALO, 3, 0, "helix_edge", False),
            (600, 3, 0, "sheet_edge", True)]
ids = lambda cases: ["N%d-S%d-na%d-%s%s" % (c[0], c[1], c[2], c[3], "-donor" if c[4] else "") for c in cases]      # noqa: E731
# case -> seed, where the default has an ambiguous residue in the exact family
SEEDS = {(64, 3, 0, "one", False): 448032, (255, 1, 3, "short", False): 1785014, (256, 3, 0, "helix_edge", False): 1792035,
         (600, 3, 0, "sheet_edge", True): 4200056}
SIGMA = 0.1                             # Angstrom: the Gaussian noise of the perturbed family, on every atom


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """the inputs of a case as the device takes them (fp32 atoms, int32 built, fp32 link and donor) and the float64 yardstick of them.
    Structure s is EXACT for even s (true atoms of ideal chains) and PERTURBED for odd s (sigma = 0.1 Angstrom on every atom).  The
    segments sit on a coarse grid round the origin: every coordinate stays within 100 Angstrom."""
    N, S, na, layout, masked = case
    rng = np.random.default_rng(SEEDS.get(case, 7000 * N + 10 * S + na))
    segs = _segments(layout, N - na)
    link = np.zeros(N, np.float32)
    r0 = na
    for _, L in segs:
        link[r0: r0 + L - 1] = 1.0
        r0 += L
    built = np.zeros((S, N), np.int32)
    built[:, na:] = 31
    atoms = np.zeros((S, N, 5, 3))
    fixtures = sheets()
    cells = [np.array(c) for c in np.ndindex(5, 5, 5)]
    for s in range(S):
        order = rng.permutation(len(cells))
        pose = {}
        r0 = na
        for k, (kind, L) in enumerate(segs):
            if kind[:-1] in ("anti", "par"):
                half = fixtures[kind[:-1]][:8] if kind[-1] == "A" else fixtures[kind[:-1]][8:]
                if kind[:-1] not in pose:                                   # both strands of a pair share the rigid motion
                    pose[kind[:-1]] = (_rotation(rng), fixtures[kind[:-1]][:, CA_].mean(0), (cells[order[k % 125]] - 2) * 18.0 + rng.uniform(-2, 2, 3))
                q, centre, shift = pose[kind[:-1]]
                seg = (half - centre) @ q.T + shift
            else:
                seg = BR.chain(rng, L) if kind == "chain" else regular({"alpha": ALPHA, "310": THREE10, "strand": STRAND}[kind], L)
                seg = (seg - seg[:, CA_].mean(0)) @ _rotation(rng).T + (cells[order[k % 125]] - 2) * 18.0 + rng.uniform(-2, 2, 3)
            atoms[s, r0: r0 + L] = seg
            r0 += L
        if s % 2 == 1:
            atoms[s, na:] += SIGMA * rng.normal(size=(N - na, 5, 3))
    atoms = atoms.astype(np.float32)
    donor = None
    if masked:
        donor = (rng.uniform(size=N) > 0.15).astype(np.float32)             # "proline" on about one residue in seven
    ref = assign(atoms, built, link, donor)
    return dict(atoms=atoms, built=built, link=link, donor=donor, exact=[s for s in range(S) if s % 2 == 0], ref=ref, na=na, segments=segs)


@functools.lru_cache(maxsize=None)
def measured_E():
    """the largest deviation of the float32 restatement's reported energies from the float64 ones, over the slots both restatements fill
    with the same partner on non-ambiguous residues of every case"""
    worst = 0.0
    for case in dict.fromkeys(HB_CASES + AS_CASES):
        I = case_inputs(case)
        f32 = hbonds(I["atoms"], I["built"], I["link"], I["donor"], dtype=np.float32)
        same = (f32["partner"] == I["ref"]["partner"]) & ~I["ref"]["ambiguous"][..., None] & ~I["ref"]["loose"]
        d = np.abs(f32["energy"].astype(np.float64) - I["ref"]["energy"])
        worst = max(worst, float(d[same].max(initial=0.0)))
    return worst


def mirror(atoms):
    y = np.array(atoms, copy=True)
    y[..., 0] = -y[..., 0]
    return y
