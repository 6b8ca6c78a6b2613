"""Float64 numpy statement of the TM-score superposition search of include/prd_align.h -- the yardstick of the alignment tests, not
product code.  Kabsch by SVD with determinant correction; every step of the search is written as the header words it."""
import numpy as np

MIRROR = np.diag([1.0, 1.0, -1.0])


def d0_of(L):
    return 1.24 * np.cbrt(L - 15.0) - 1.8 if L > 21 else 0.5


def kabsch(x, y):
    """(R, t) with y ~ t + x @ R, R a proper rotation minimising the RMSD of the rows given"""
    xc, yc = x.mean(0), y.mean(0)
    U, _, Vt = np.linalg.svd((x - xc).T @ (y - yc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0])
    R = U @ D @ Vt
    return R, yc - xc @ R


def dist(x, y, R, t):
    return np.sqrt(((t + x @ R - y) ** 2).sum(-1))


def tm_of(x, y, R, t):
    L = len(x)
    if L < 3:
        return 0.0
    return float((1.0 / (1.0 + (dist(x, y, R, t) / d0_of(L)) ** 2)).sum() / L)


def rmsd_of(x, y, R, t):
    return float(np.sqrt((dist(x, y, R, t) ** 2).mean())) if len(x) else 0.0


def seeds(L):
    """[(start, Lf)] in seed order"""
    lengths = []                # L, L/2, L/4, ... while they exceed 4, then 4 itself: every halving of the issue's list that is >= 4
    Lf = L                      # is in it, and the shortest fragment is always 4 (TM-score's own convention)
    while Lf > 4:
        lengths.append(Lf)
        Lf //= 2
    lengths.append(4)
    if L <= 21:                 # d0 = 0.5 against d_cut >= 3.5: the rounds cannot shed an outlier of so small a chain, the seed must avoid it
        lengths.append(3)
    if L < 4:
        lengths = [L]
    out = []
    for Lf in lengths:
        step = max(1, Lf // 2)
        starts = list(range(0, L - Lf + 1, step))
        if starts[-1] != L - Lf:
            starts.append(L - Lf)
        out += [(s, Lf) for s in starts]
    return out


def tm_search(x, y, seed_filter=None, with_seed=False):
    """(tm, R, t) of the search on the rows given (all of them count: pass compacted, masked coordinates).  ``seed_filter``: a
    predicate on the seed index (position in ``seeds(L)``); seeds it rejects are left out -- the tests' model of a search that skips
    seeds.  ``with_seed``: also return the index of the winning seed (the lowest one among equal scores)."""
    L = len(x)
    d0 = d0_of(L)
    d0s = min(max(d0, 4.5), 8.0)
    best = (-1.0, None, None, -1)
    for k, (start, Lf) in enumerate(seeds(L)):
        if seed_filter is not None and not seed_filter(k):
            continue
        sub = np.zeros(L, bool)
        sub[start:start + Lf] = True
        for it in range(20):
            R, t = kabsch(x[sub], y[sub])
            d = dist(x, y, R, t)
            tm = float((1.0 / (1.0 + (d / d0) ** 2)).sum() / L)
            if tm > best[0]:
                best = (tm, R, t, k)
            cut = d0s - 1.0 if it == 0 else d0s + 1.0
            while (d < cut).sum() < 3:
                cut += 0.5
            new = d < cut
            if np.array_equal(new, sub):
                break
            sub = new
    return best if with_seed else best[:3]


def superimpose(x, y, mirror=True, mode="tm"):
    """dict(tm, rmsd, rotation, translation, mirrored) for ONE pair of compacted structures [L,3]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    L = len(x)
    if L < 3:
        return dict(tm=0.0, rmsd=0.0, rotation=np.eye(3), translation=np.zeros(3), mirrored=0)
    cands = []
    for m in ([0, 1] if mirror else [0]):
        xm = x @ MIRROR if m else x
        if mode == "tm":
            tm, R, t = tm_search(xm, y)
        else:
            R, t = kabsch(xm, y)
            tm = tm_of(xm, y, R, t)
        R = MIRROR @ R if m else R
        cands.append(dict(tm=tm, rmsd=rmsd_of(x, y, R, t), rotation=R, translation=t, mirrored=m))
    if len(cands) == 2 and (cands[1]["tm"] > cands[0]["tm"] if mode == "tm" else cands[1]["rmsd"] < cands[0]["rmsd"]):
        return cands[1]
    return cands[0]


# ---- the planted cases of the tests --------------------------------------------------------------------------------------------

def random_rotation(rng):
    q = rng.normal(size=4)
    w, a, b, c = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b)],
                     [2 * (a * b + w * c), 1 - 2 * (a * a + c * c), 2 * (b * c - w * a)],
                     [2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)]])


def chain(rng, L):
    """random walk of 3.8 Angstrom steps, centred, scaled down if needed to stay within 60 Angstrom of the origin"""
    steps = rng.normal(size=(L, 3))
    steps *= 3.8 / np.linalg.norm(steps, axis=1, keepdims=True)
    c = np.cumsum(steps, 0)
    c -= c.mean(0)
    r = np.abs(c).max()
    return c * (60.0 / r) if r > 60.0 else c


def planted(rng, L, core_fraction, mirrored=False, noise=0.3):
    """(x, y, R0, t0, core): y = t0 + x' @ R0 + noise on a contiguous core of the chain (x' = x mirrored if asked), an unrelated chain
    elsewhere.  |t0| <= 15 Angstrom keeps every coordinate within 100 Angstrom of the origin."""
    x = chain(rng, L)
    R0 = random_rotation(rng)
    t0 = rng.uniform(-8.0, 8.0, size=3)
    n = L if core_fraction >= 1.0 else max(3, int(round(core_fraction * L)))
    start = int(rng.integers(0, L - n + 1))
    core = np.zeros(L, bool)
    core[start:start + n] = True
    y = chain(rng, L)
    xm = x @ MIRROR if mirrored else x
    y[core] = (t0 + xm @ R0 + noise * rng.normal(size=(L, 3)))[core]
    return x, y, (MIRROR @ R0 if mirrored else R0), t0, core


def core3_case(L, p):
    """(x, y) float32-rounded [L,3]: two unrelated chains, y moved 20 to 30 Angstrom away, except that y[p:p+3] is the exact image of
    x[p:p+3] under a random rigid motion -- a core that only a seed lying on it can find"""
    rng = np.random.default_rng(900 + 100 * L + p)
    x, y = chain(rng, L), chain(rng, L)
    u = rng.normal(size=3)
    y += u / np.linalg.norm(u) * rng.uniform(20.0, 30.0)
    y[p:p + 3] = rng.uniform(-8.0, 8.0, size=3) + x[p:p + 3] @ random_rotation(rng)
    return x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)


def decisive_cases(lengths=(12, 20, 21), drop=1e-3):
    """the core3_case's in which ONE seed decides: the search without its own winning seed ends at least ``drop`` lower.
    [dict(L, p, x, y, tm, seed, tm_without)]"""
    out = []
    for L in lengths:
        for p in range(L - 2):
            x, y = core3_case(L, p)
            tm, _, _, k = tm_search(x, y, with_seed=True)
            without = tm_search(x, y, seed_filter=lambda j: j != k)[0]
            if tm - without >= drop:
                out.append(dict(L=L, p=p, x=x, y=y, tm=tm, seed=k, tm_without=without))
    return out
