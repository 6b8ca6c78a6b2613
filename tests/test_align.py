"""GPU: libprd_align.so through protein_redesign_amd.align against the float64 yardstick tests/align_ref.py.  The GPU result is never
compared with itself: every case asserts (1) honest numbers -- tm and rmsd recomputed in float64 from the returned transform --,
(2) a rigid motion, (3) a result at least as good as the yardstick's, the float64 Kabsch fit's and the planted transform's.

Tolerances (the issue's): coordinates stay within 100 Angstrom of the origin, where fp32 leaves ~1e-5 Angstrom on a transformed
coordinate, hence at most ~4e-5 on a TM term at the smallest d0 = 0.5: 1e-4 on tm, 1e-4 Angstrom + 1e-5 relative on rmsd, 1e-5 on
|rot^T rot - 1|."""
import functools
import warnings

import numpy as np
import pytest
import torch

import align_ref as AR
from no_host_sync import run_without_host_sync
from protein_redesign_amd import align
from protein_redesign_amd import pipeline as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = [3, 4, 5, 21, 22, 63, 64, 65, 130, 257, 1025]
LIGAND, TAIL = 7, 5


def fractions(L):
    return [1.0] if L < 5 else [1.0, 0.6, 0.35]         # at L = 3, 4 only the fully rigid case is meaningful


def layout(L):
    """(N, mask [N], rows of the masked positions): a ligand prefix of 7 rows, two holes in the mask, a padded tail"""
    N = LIGAND + L + 2 + TAIL
    mask = np.zeros(N, np.float32)
    mask[LIGAND: LIGAND + L + 2] = 1.0
    mask[[LIGAND + 1, LIGAND + 2 + L // 2]] = 0.0
    return N, mask, np.nonzero(mask)[0]


def embed(rng, compact, N, rows):
    """[K,L,3] -> [K,N,3] float32 with junk (within range) where the mask is 0"""
    full = rng.uniform(-90.0, 90.0, size=(compact.shape[0], N, 3))
    full[:, rows] = compact
    return full.astype(np.float32)


def strided_ref(y):
    """[R,N,3] float32 -> a device view of it whose row stride is 15 floats (the C-alpha column of an [R,N,5,3] tensor)"""
    wide = torch.full((y.shape[0], y.shape[1], 5, 3), 77.0)
    wide[:, :, 1] = torch.from_numpy(y)
    view = wide.to(DEV)[:, :, 1]
    assert view.stride() == (y.shape[1] * 15, 15, 1)
    return view


def run(x, y, mask, **kw):
    """superimpose on the device; fields as numpy"""
    ref = strided_ref(y)
    out = align.superimpose(torch.from_numpy(x).to(DEV), ref[0] if kw.pop("single", False) else ref, torch.from_numpy(mask).to(DEV), **kw)
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in ("tm", "rmsd", "rotation", "translation", "mirrored")}


def check_entry(got, idx, xc, yc, what):
    """properties 1 and 2 of one pair; xc, yc: the compacted float32 inputs as float64.  Returns (tm, rmsd, mirrored)."""
    R, t = got["rotation"][idx].astype(np.float64), got["translation"][idx].astype(np.float64)
    tm, rmsd, mir = float(got["tm"][idx]), float(got["rmsd"][idx]), int(got["mirrored"][idx])
    tm64, rmsd64 = AR.tm_of(xc, yc, R, t), AR.rmsd_of(xc, yc, R, t)
    print(f"{what}: tm {tm:.6f} (f64 from the transform {tm64:.6f}) rmsd {rmsd:.5f} ({rmsd64:.5f}) mirrored {mir} "
          f"|RtR-1| {np.abs(R.T @ R - np.eye(3)).max():.2e} det {np.linalg.det(R):+.6f}")
    assert abs(tm - tm64) <= 1e-4, what
    assert abs(rmsd - rmsd64) <= 1e-4 + 1e-5 * rmsd64, what
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-5, what
    assert abs(np.linalg.det(R) - (-1.0 if mir else 1.0)) <= 1e-4, what
    return tm, rmsd, mir


@functools.lru_cache(maxsize=None)
def planted_case(L, frac, mirrored=False):
    """one planted pair, float32-rounded, compacted [L,3] float64 + the planted transform + the yardstick's results (computed once)"""
    rng = np.random.default_rng(7000 + 10 * L + int(10 * frac) + (5 if mirrored else 0))
    x, y, R0, t0, _ = AR.planted(rng, L, frac, mirrored=mirrored)
    x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    return dict(x=x, y=y, R0=R0, t0=t0, rng=rng)


@functools.lru_cache(maxsize=None)
def yardstick(L, frac, mirrored, mirror, mode):
    c = planted_case(L, frac, mirrored)
    return AR.superimpose(c["x"], c["y"], mirror=mirror, mode=mode)


def device_case(L, frac, mirrored=False, **kw):
    c = planted_case(L, frac, mirrored)
    N, mask, rows = layout(L)
    rng = np.random.default_rng(1)
    got = run(embed(rng, c["x"][None], N, rows), embed(rng, c["y"][None], N, rows), mask, **kw)
    return c, got


@pytest.mark.parametrize("L", LENGTHS)
def test_tm_mode_is_at_least_as_good_as_the_yardstick(L):
    mirror = True
    for frac in fractions(L):
        c, got = device_case(L, frac, mirror=mirror)
        tm, _, mir = check_entry(got, (0, 0), c["x"], c["y"], f"L={L} core={frac}")
        ref = yardstick(L, frac, False, mirror, "tm")
        Rk, tk = AR.kabsch(c["x"], c["y"])
        print(f"    yardstick {ref['tm']:.6f}  kabsch {AR.tm_of(c['x'], c['y'], Rk, tk):.6f}  planted {AR.tm_of(c['x'], c['y'], c['R0'], c['t0']):.6f}")
        assert tm >= ref["tm"] - 1e-4, (L, frac)
        assert tm >= AR.tm_of(c["x"], c["y"], Rk, tk) - 1e-4, (L, frac)
        assert tm >= AR.tm_of(c["x"], c["y"], c["R0"], c["t0"]) - 1e-4, (L, frac)
        if frac == 1.0 and L >= 21:         # (three points are coplanar: a core of three fits its mirror image just as well)
            assert mir == 0, (L, frac)


@pytest.mark.parametrize("L", LENGTHS)
def test_rmsd_mode_reaches_the_float64_kabsch_fit(L):
    for frac in fractions(L):
        c, got = device_case(L, frac, mirror=False, mode="rmsd", single=True)
        assert got["tm"].shape == (1,)
        _, rmsd, mir = check_entry(got, (0,), c["x"], c["y"], f"L={L} core={frac} rmsd mode")
        Rk, tk = AR.kabsch(c["x"], c["y"])
        print(f"    kabsch {AR.rmsd_of(c['x'], c['y'], Rk, tk):.6f}")
        assert rmsd <= AR.rmsd_of(c["x"], c["y"], Rk, tk) + 1e-4 and mir == 0, (L, frac)


@pytest.mark.parametrize("L", [65, 130])
def test_mirror(L):
    c, on = device_case(L, 1.0, mirrored=True, mirror=True)
    tm_on, _, mir = check_entry(on, (0, 0), c["x"], c["y"], f"L={L} mirrored input, mirror on")
    assert mir == 1 and tm_on >= AR.tm_of(c["x"], c["y"], c["R0"], c["t0"]) - 1e-4
    assert tm_on >= yardstick(L, 1.0, True, True, "tm")["tm"] - 1e-4
    _, off = device_case(L, 1.0, mirrored=True, mirror=False)
    tm_off, _, mir = check_entry(off, (0, 0), c["x"], c["y"], f"L={L} mirrored input, mirror off")
    assert mir == 0 and tm_on - tm_off > 0.3
    assert tm_off >= yardstick(L, 1.0, True, False, "tm")["tm"] - 1e-4
    c, plain = device_case(L, 1.0, mirror=True)
    assert check_entry(plain, (0, 0), c["x"], c["y"], f"L={L} plain input, mirror on")[2] == 0


def family(L, K, seed):
    """K float32-rounded variants [K,L,3] (float64) of one fold: rigid moves of a base chain, noise growing with the index, every
    third one mirrored, the last third of every second one replaced by an unrelated chain"""
    rng = np.random.default_rng(seed)
    base = AR.chain(rng, L) * 0.8
    out = []
    for k in range(K):
        v = base @ AR.MIRROR if k % 3 == 2 else base.copy()
        v = rng.uniform(-8.0, 8.0, 3) + v @ AR.random_rotation(rng) + (0.2 + 0.15 * k) * rng.normal(size=(L, 3))
        if k % 2 == 1:
            v[2 * L // 3:] = AR.chain(rng, L)[2 * L // 3:] * 0.8
        out.append(v)
    return np.stack(out).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("S,R", [(1, 1), (5, 1), (1, 3), (5, 3)])
def test_cross_product_of_structures(S, R):
    L = 65
    N, mask, rows = layout(L)
    xs, ys = family(L, 5, 31)[:S], family(L, 3, 32)[:R]
    rng = np.random.default_rng(2)
    got = run(embed(rng, xs, N, rows), embed(rng, ys, N, rows), mask)
    assert got["tm"].shape == (S, R) and got["rotation"].shape == (S, R, 3, 3) and got["mirrored"].dtype == np.int32
    for s in range(S):
        for r in range(R):
            tm, _, mir = check_entry(got, (s, r), xs[s], ys[r], f"pair ({s},{r})")
            ref = cross_yardstick(s, r)
            Rk, tk = AR.kabsch(xs[s], ys[r])
            assert tm >= ref["tm"] - 1e-4 and tm >= AR.tm_of(xs[s], ys[r], Rk, tk) - 1e-4, (s, r)
            assert mir == ref["mirrored"], (s, r)           # the families are mirrored or not by a wide margin


@functools.lru_cache(maxsize=None)
def cross_yardstick(s, r):
    return AR.superimpose(family(65, 5, 31)[s], family(65, 3, 32)[r], mirror=True)


@functools.lru_cache(maxsize=None)
def pair_yardstick(s, r):
    f = family(63, 7, 41)
    return AR.superimpose(f[s], f[r], mirror=True)


@pytest.mark.parametrize("S", [1, 2, 7])
def test_pairwise_matrix_and_diversity(S):
    L = 63
    N, mask, rows = layout(L)
    xs = family(L, 7, 41)[:S]
    x = torch.from_numpy(embed(np.random.default_rng(3), xs, N, rows)).to(DEV)
    m = torch.from_numpy(mask).to(DEV)
    full = align.pairwise(x, m)
    tm = align.pairwise_tm(x, m)
    div = align.diversity(x, m)
    torch.cuda.synchronize()
    got = {k: getattr(full, k).cpu().numpy() for k in ("tm", "rmsd", "rotation", "translation", "mirrored")}
    tm = tm.cpu().numpy()
    assert tm.shape == (S, S) and np.array_equal(tm, got["tm"]) and np.array_equal(tm, tm.T) and np.array_equal(np.diag(tm), np.ones(S, np.float32))
    assert np.array_equal(got["rmsd"], got["rmsd"].T) and np.array_equal(got["mirrored"], got["mirrored"].T)
    off = []
    for s in range(S):
        assert np.array_equal(got["rotation"][s, s], np.eye(3)) and not got["translation"][s, s].any() and got["rmsd"][s, s] == 0
        for r in range(S):
            if s == r:
                continue
            v, _, _ = check_entry(got, (s, r), xs[s], xs[r], f"pair ({s},{r}) of {S}")          # (r, s) holds the inverse: honest too
            ref = pair_yardstick(min(s, r), max(s, r))
            Rk, tk = AR.kabsch(xs[s], xs[r])
            assert v >= ref["tm"] - 1e-4 and v >= AR.tm_of(xs[s], xs[r], Rk, tk) - 1e-4, (s, r)
            off.append(v)
    if S == 1:
        assert np.isnan(float(div))
    else:
        assert abs(float(div) - np.mean(off)) <= 1e-6


def test_two_calls_are_bit_equal():
    L = 130
    N, mask, rows = layout(L)
    xs = family(L, 5, 51)
    x, m = torch.from_numpy(embed(np.random.default_rng(4), xs, N, rows)).to(DEV), torch.from_numpy(mask).to(DEV)
    a, b = align.superimpose(x, x[:3], m), align.superimpose(x, x[:3], m)
    pa, pb = align.pairwise(x, m), align.pairwise(x, m)
    torch.cuda.synchronize()
    for u, v in ((a, b), (pa, pb)):
        for k in ("tm", "rmsd", "rotation", "translation", "mirrored"):
            assert torch.equal(getattr(u, k), getattr(v, k)), k
    assert np.array_equal(np.diagonal(a.tm[:3].cpu().numpy()), np.ones(3, np.float32)) or float(a.tm[0, 0]) > 1 - 1e-6


def test_limits():
    x = torch.from_numpy(np.random.default_rng(5).uniform(-50, 50, size=(2, 12, 3)).astype(np.float32)).to(DEV)
    for ones in ([], [4], [4, 9]):                      # L = 0, 1, 2
        m = torch.zeros(12, device=DEV)
        m[ones] = 1.0
        for out in (align.superimpose(x, x[:1] + 1.0, m), align.pairwise(x, m), align.superimpose(x, x[0], m, mode="rmsd")):
            torch.cuda.synchronize()
            assert not out.tm.any() and not out.rmsd.any() and not out.mirrored.any() and not out.translation.any()
            assert torch.equal(out.rotation, torch.eye(3, device=DEV).expand_as(out.rotation))
    with pytest.raises(ValueError, match="4096"):
        align.superimpose(torch.zeros(1, 4097, 3, device=DEV), torch.zeros(4097, 3, device=DEV), torch.ones(4097, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        align.superimpose(x, x[0], torch.ones(12, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="expected 12"):
        align.superimpose(x, torch.zeros(11, 3, device=DEV), torch.ones(12, device=DEV))
    with pytest.raises(ValueError, match="mode"):
        align.superimpose(x, x[0], torch.ones(12, device=DEV), mode="gdt")


def test_no_host_synchronisation():
    """Mechanism as in tests/test_redesign_region.py: ``set_sync_debug_mode("error")`` where this torch build honours it (probed with an
    ``.item()``), otherwise a single-stream capture, where a synchronisation fails the capture.  Which one ran is printed."""
    L = 65
    N, mask, rows = layout(L)
    xs = family(L, 5, 61)
    x, m = torch.from_numpy(embed(np.random.default_rng(6), xs, N, rows)).to(DEV), torch.from_numpy(mask).to(DEV)
    ref = strided_ref(embed(np.random.default_rng(7), xs[:1], N, rows))[0]

    def work():
        return align.superimpose(x, ref, m), align.pairwise_tm(x, m), align.apply(x, torch.eye(3, device=DEV).expand(5, 3, 3), torch.zeros(5, 3, device=DEV))
    warm = work()                                       # library, allocator
    got = run_without_host_sync(work)
    assert torch.equal(got[0].tm, warm[0].tm) and torch.equal(got[1], warm[1]) and torch.equal(got[0].rotation, warm[0].rotation)
    assert torch.equal(got[2], x)                       # identity transform: t + x @ 1 with t = 0 is x bit for bit


def test_apply_equals_the_float64_transform():
    rng = np.random.default_rng(8)
    pos = rng.uniform(-80, 80, size=(3, 301, 3)).astype(np.float32)
    rot = np.stack([AR.random_rotation(rng) for _ in range(3)]).astype(np.float32)
    tr = rng.uniform(-10, 10, size=(3, 3)).astype(np.float32)
    got = align.apply(torch.from_numpy(pos).to(DEV), torch.from_numpy(rot).to(DEV), torch.from_numpy(tr).to(DEV)).cpu().numpy()
    want = tr[:, None].astype(np.float64) + pos.astype(np.float64) @ rot.astype(np.float64)
    assert np.abs(got - want).max() <= 5e-5             # three products of magnitude <= 80 and three sums in fp32: 6 x 2^-24 x 140
    one = align.apply(torch.from_numpy(pos[1]).to(DEV), torch.from_numpy(rot[1]).to(DEV), torch.from_numpy(tr[1]).to(DEV)).cpu().numpy()
    assert np.array_equal(one, got[1])


def test_generate_samples_end_to_end(tmp_path):
    """the small synthetic model of smoke(), align_to="input", S = 3"""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    args = make_args(single_dim=128, pair_dim=64, num_blocks=2, esm_dim=64, num_steps=16, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    data = synthetic_sample(8, 40, esm_dim=64, seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=tmp_path / "plain")
        out = PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=tmp_path / "aligned", align_to="input")
    assert len(plain) == 4 and len(out) == 5
    pos0, logits0, proteins0, ligands0 = plain
    pos, logits, proteins, ligands, info = out
    assert sorted(info) == ["diversity", "mirrored", "rmsd", "rotation", "tmscore", "translation"]
    assert info["tmscore"].shape == (3,) and info["rotation"].shape == (3, 3, 3) and isinstance(info["diversity"], float)
    # the returned positions are the unaligned run's under the returned transforms
    moved = align.apply(torch.from_numpy(pos0).to(DEV), torch.from_numpy(info["rotation"]).to(DEV), torch.from_numpy(info["translation"]).to(DEV))
    assert np.array_equal(pos, moved.cpu().numpy())
    # the rest of the 4-tuple is the align_to=None run's except for the frame
    assert np.array_equal(logits, logits0) and all(np.array_equal(a.aatype, b.aatype) for a, b in zip(proteins, proteins0))
    for k in range(3):
        assert np.array_equal(proteins[k].atom_pos[:, 1], pos[k, 8:48]) and np.array_equal(ligands[k], pos[k, :8])
    # honest scores: recomputed in float64 from the inputs and the returned transform, over the residues with a C-alpha
    ca = np.asarray(data["residue_atom_mask"])[:, 1] > 0.5
    ref = np.asarray(data["residue_atom_pos"], dtype=np.float32)[:, 1].astype(np.float64)[ca]
    got = {"tm": info["tmscore"], "rmsd": info["rmsd"], "rotation": info["rotation"], "translation": info["translation"], "mirrored": info["mirrored"]}
    for k in range(3):
        check_entry(got, (k,), pos0[k, 8:48].astype(np.float64)[ca], ref, f"sample {k}")
    lines = (tmp_path / "aligned" / "sample_tmscores.txt").read_text().splitlines()
    assert len(lines) == 3 and [float(v) for v in lines] == [float(v) for v in info["tmscore"]]
    z = np.load(tmp_path / "aligned" / "sample_alignment.npz")
    assert sorted(z.files) == sorted(info) and np.array_equal(z["rotation"], info["rotation"])
    assert not (tmp_path / "plain" / "sample_tmscores.txt").exists()
    assert 0.0 < info["diversity"] <= 1.0
