"""GPU: libprd_tmalign.so through protein_redesign_amd.tmalign against the float64 yardstick tests/tmalign_ref.py.  The device result is
never compared with itself.  Every case asserts (1) honest numbers -- tm, rmsd and n_aligned recomputed in float64 from the returned
transform and mapping agree to 1e-4 (coordinates stay within 100 Angstrom: the tolerances and the reason are those of
tests/test_align.py), the mapping strictly increasing and inside the masked rows of both sides --, (2) a rigid motion whose determinant
matches ``mirrored``, (3) tm at least that of the planted alignment under the planted transform and at least the yardstick's, both
minus 1e-4."""
import warnings

import numpy as np
import pytest
import torch

import tmalign_cases as TC
import tmalign_ref as TR
from protein_redesign_amd import align, tmalign
from protein_redesign_amd import pipeline as PL
from test_align import embed, layout, strided_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIELDS = ("tm", "rmsd", "n_aligned", "rotation", "translation", "mirrored", "mapping")


def run(x, y, mx, my, strided=True, **kw):
    ref = strided_ref(y) if strided else torch.from_numpy(y).to(DEV)
    out = tmalign.align(torch.from_numpy(x).to(DEV), ref, torch.from_numpy(mx).to(DEV), torch.from_numpy(my).to(DEV), **kw)
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in FIELDS}


def check_entry(got, idx, xc, yc, rows_x, rows_y, Nx, what):
    """properties 1 and 2 of one pair; xc, yc: the compacted float32 inputs as float64.  Returns (tm, compacted mapping)."""
    R, t = got["rotation"][idx].astype(np.float64), got["translation"][idx].astype(np.float64)
    tm, rmsd, n, mir = float(got["tm"][idx]), float(got["rmsd"][idx]), int(got["n_aligned"][idx]), int(got["mirrored"][idx])
    mp = got["mapping"][idx]
    assert mp.shape == (Nx,) and mp.dtype == np.int32
    on = np.nonzero(mp >= 0)[0]
    assert np.isin(on, rows_x).all() and np.isin(mp[on], rows_y).all(), what          # inside the masked rows of both sides
    assert (np.diff(mp[on]) > 0).all(), what                                          # strictly increasing
    amap = np.full(len(xc), -1, np.int64)
    amap[np.searchsorted(rows_x, on)] = np.searchsorted(rows_y, mp[on])
    tm64, rmsd64, n64 = TR.score_of(xc, yc, amap, R, t)
    print(f"{what}: tm {tm:.6f} (f64 {tm64:.6f}) rmsd {rmsd:.5f} ({rmsd64:.5f}) n {n} ({n64}) mirrored {mir} "
          f"|RtR-1| {np.abs(R.T @ R - np.eye(3)).max():.2e} det {np.linalg.det(R):+.6f}")
    assert abs(tm - tm64) <= 1e-4 and abs(rmsd - rmsd64) <= 1e-4 + 1e-5 * rmsd64 and n == n64, what
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-5, what
    assert abs(np.linalg.det(R) - (-1.0 if mir else 1.0)) <= 1e-4, what
    return tm, amap


def device_case(case, **kw):
    Lx, Ly = case[:2]
    c = TC.planted_case(*case)
    Nx, mx, rx = layout(Lx)
    Ny, my, ry = layout(Ly)
    rng = np.random.default_rng(1)
    got = run(embed(rng, c["x"][None], Nx, rx), embed(rng, c["y"][None], Ny, ry), mx, my, **kw)
    return c, got, (rx, ry, Nx)


@pytest.mark.parametrize("case", TC.CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}{'-m' if c[3] else ''}")
def test_at_least_as_good_as_the_planted_alignment_and_the_yardstick(case):
    ref = TC.yardstick(*case)
    c, got, (rx, ry, Nx) = device_case(case)
    assert got["tm"].shape == (1, 1) and got["mapping"].shape == (1, 1, Nx)
    tm, _ = check_entry(got, (0, 0), c["x"], c["y"], rx, ry, Nx, f"{case}")
    print(f"    yardstick {ref['tm']:.6f} (n {ref['n_aligned']}, mirrored {ref['mirrored']})  planted {c['planted_tm']:.6f}")
    assert tm >= c["planted_tm"] - 1e-4, case
    assert tm >= ref["tm"] - 1e-4, case


@pytest.mark.parametrize("case", TC.LONG_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_diagonals_longer_than_the_workgroup(case):
    """more DP rows than threads: a thread owns 1, 2 or 3 rows (Lx below and above 512 and 1024).  All three properties on all four;
    the yardstick takes 10 to 40 s each here, once (cached, shared with tests/test_tmalign_cpu.py)."""
    ref = TC.yardstick(*case)
    c, got, (rx, ry, Nx) = device_case(case)
    tm, _ = check_entry(got, (0, 0), c["x"], c["y"], rx, ry, Nx, f"{case}")
    print(f"    yardstick {ref['tm']:.6f} (n {ref['n_aligned']}, mirrored {ref['mirrored']})  planted {c['planted_tm']:.6f}")
    assert tm >= c["planted_tm"] - 1e-4, case
    assert tm >= ref["tm"] - 1e-4, case


def test_the_limit_2048():
    """Nx = Ny = 2048: properties 1 and 2 and the planted bound only (the yardstick is too slow here)"""
    L = 2048 - 14
    c = TC.planted_case(L, L - 9, 1.0, False, 30000)
    Nx, mx, rx = layout(L)
    Ny, my, ry = layout(L - 9)
    mx, my = np.concatenate([mx, np.zeros(2048 - Nx, np.float32)]), np.concatenate([my, np.zeros(2048 - Ny, np.float32)])
    rng = np.random.default_rng(2)
    got = run(embed(rng, c["x"][None], 2048, rx), embed(rng, c["y"][None], 2048, ry), mx, my, mirror=False)
    tm, _ = check_entry(got, (0, 0), c["x"], c["y"], rx, ry, 2048, "N = 2048")
    print(f"    planted {c['planted_tm']:.6f}")
    assert tm >= c["planted_tm"] - 1e-4
    with pytest.raises(ValueError, match="2048"):
        tmalign.align(torch.zeros(1, 2049, 3, device=DEV), torch.zeros(8, 3, device=DEV), torch.ones(2049, device=DEV), torch.ones(8, device=DEV))
    with pytest.raises(ValueError, match="2048"):
        tmalign.align(torch.zeros(1, 8, 3, device=DEV), torch.zeros(2049, 3, device=DEV), torch.ones(8, device=DEV), torch.ones(2049, device=DEV))


def test_short_chains_give_the_documented_zeros():
    x = torch.from_numpy(np.random.default_rng(5).uniform(-50, 50, size=(2, 12, 3)).astype(np.float32)).to(DEV)
    full = torch.ones(12, device=DEV)
    short = torch.zeros(12, device=DEV)
    short[[1, 4, 6, 9]] = 1.0
    for mx, my in ((short, full), (full, short), (torch.zeros(12, device=DEV), full)):
        out = tmalign.align(x, x[:1] + 1.0, mx, my)
        torch.cuda.synchronize()
        assert not out.tm.any() and not out.rmsd.any() and not out.n_aligned.any() and not out.mirrored.any() and not out.translation.any()
        assert torch.equal(out.rotation, torch.eye(3, device=DEV).expand_as(out.rotation)) and bool((out.mapping == -1).all())


def _bits(got):
    return [got[k].tobytes() for k in FIELDS if k != "mapping"]


def test_embedding_masked_rows_strides_determinism():
    """one pair embedded in rows of N = L ... 2048, junk / NaN / inf / 1e30 in masked-out rows, a strided ref, two runs: bit-equal"""
    case = TC.CASES[6]
    Lx, Ly = case[:2]
    c = TC.planted_case(*case)
    ones_x, ones_y = np.ones(Lx, np.float32), np.ones(Ly, np.float32)
    x32, y32 = c["x"][None].astype(np.float32), c["y"][None].astype(np.float32)
    plain = run(x32, y32, ones_x, ones_y, strided=False)
    again = run(x32, y32, ones_x, ones_y, strided=False)
    assert _bits(plain) == _bits(again) and np.array_equal(plain["mapping"], again["mapping"])
    check_entry(plain, (0, 0), c["x"], c["y"], np.arange(Lx), np.arange(Ly), Lx, "plain")
    pm = plain["mapping"][0, 0]
    for (Nx, Ny), junk in (((Lx + 1, Ly + 3), np.nan), ((600, 513), np.inf), ((1100, 200), 1e30), ((2048, 2048), -np.inf)):
        rng = np.random.default_rng(Nx)
        rx, ry = np.sort(rng.choice(Nx, Lx, replace=False)), np.sort(rng.choice(Ny, Ly, replace=False))
        mx, my = np.zeros(Nx, np.float32), np.zeros(Ny, np.float32)
        mx[rx], my[ry] = 1.0, 1.0
        xe, ye = np.full((1, Nx, 3), junk, np.float32), np.full((1, Ny, 3), junk, np.float32)
        xe[:, rx], ye[:, ry] = x32, y32
        got = run(xe, ye, mx, my, strided=True)
        assert _bits(got) == _bits(plain), (Nx, Ny)
        gm = got["mapping"][0, 0]
        want = np.full(Nx, -1, np.int32)
        want[rx[pm >= 0]] = ry[pm[pm >= 0]]
        assert np.array_equal(gm, want), (Nx, Ny)


def test_guard_bytes_around_outputs_and_workspace():
    case = TC.CASES[4]
    Lx, Ly = case[:2]
    c = TC.planted_case(*case)
    Nx, mx, rx = layout(Lx)
    Ny, my, ry = layout(Ly)
    rng = np.random.default_rng(3)
    S, R, G = 2, 2, 256
    x = torch.from_numpy(embed(rng, np.stack([c["x"], c["x"][::-1]]), Nx, rx)).to(DEV)
    y = torch.from_numpy(embed(rng, np.stack([c["y"], c["y"] + 1.0]), Ny, ry)).to(DEV)
    mxd, myd = torch.from_numpy(mx).to(DEV), torch.from_numpy(my).to(DEV)
    want = tmalign.align(x, y, mxd, myd)
    L = tmalign.lib()
    nbytes = L.prd_tmalign_workspace_bytes(S, R, Nx, Ny, 1)
    sizes = dict(tm=4 * S * R, rmsd=4 * S * R, rot=36 * S * R, trans=12 * S * R, n=4 * S * R, mir=4 * S * R, map=4 * S * R * Nx, ws=nbytes)
    bufs = {k: torch.full((G + ((v + 15) // 16) * 16 + G,), 0xA5, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    p = {k: b.data_ptr() + G for k, b in bufs.items()}
    assert all(v % 16 == 0 for v in p.values())
    code = L.prd_tmalign_align(p["tm"], p["rmsd"], p["rot"], p["trans"], p["n"], p["mir"], p["map"], x.data_ptr(), x.stride(0), x.stride(1),
                               mxd.data_ptr(), y.data_ptr(), y.stride(0), y.stride(1), myd.data_ptr(), S, R, Nx, Ny, 1, p["ws"], nbytes,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert code == 0
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:G] == 0xA5).all() and (h[G + sizes[k]:] == 0xA5).all(), k
    for k, f in (("tm", want.tm), ("rot", want.rotation), ("n", want.n_aligned), ("map", want.mapping)):
        assert bufs[k].cpu().numpy()[G:G + sizes[k]].tobytes() == f.cpu().numpy().tobytes(), k
    for s in range(S):
        for r in range(R):
            xs, ys = x[s].cpu().numpy()[rx].astype(np.float64), y[r].cpu().numpy()[ry].astype(np.float64)
            check_entry({k: getattr(want, k).cpu().numpy() for k in FIELDS}, (s, r), xs, ys, rx, ry, Nx, f"pair ({s},{r})")


@pytest.mark.parametrize("case", [TC.CASES[3], TC.LONG_CASES[2]], ids=["63x64", "1010x1040-above-48KiB-of-LDS"])
def test_graph_capture_and_replay(case):
    c, warm, _ = device_case(case)
    Nx, mx, rx = layout(case[0])
    Ny, my, ry = layout(case[1])
    rng = np.random.default_rng(1)
    x, y = torch.from_numpy(embed(rng, c["x"][None], Nx, rx)).to(DEV), strided_ref(embed(rng, c["y"][None], Ny, ry))
    mxd, myd = torch.from_numpy(mx).to(DEV), torch.from_numpy(my).to(DEV)
    tmalign.align(x, y, mxd, myd)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tmalign.align(x, y, mxd, myd)
    graph.replay()
    torch.cuda.synchronize()
    for k in FIELDS:
        assert np.array_equal(getattr(out, k).cpu().numpy(), warm[k]), k


@pytest.mark.parametrize("L", [64, 130])
def test_equal_length_rigid_pairs_map_to_the_identity(L):
    rng = np.random.default_rng(4000 + L)
    x, y, R0, t0, amap = TR.planted(rng, L, L, 1.0, indels=False)
    assert np.array_equal(amap, np.arange(L))
    x, y = x.astype(np.float32), y.astype(np.float32)
    N, mask, rows = layout(L)
    xe, ye = embed(rng, x[None], N, rows), embed(rng, y[None], N, rows)
    got = run(xe, ye, mask, mask)
    tm, cm = check_entry(got, (0, 0), x.astype(np.float64), y.astype(np.float64), rows, rows, N, f"L={L} rigid")
    assert np.array_equal(cm, np.arange(L))
    sup = align.superimpose(torch.from_numpy(xe).to(DEV), strided_ref(ye), torch.from_numpy(mask).to(DEV))
    assert tm >= float(sup.tm[0, 0]) - 1e-4


def test_generate_samples_end_to_end(tmp_path):
    """the small synthetic model of smoke(), a Protein of another length as the reference, S = 3"""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    args = make_args(single_dim=128, pair_dim=64, num_blocks=2, esm_dim=64, num_steps=16, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    data = synthetic_sample(8, 40, esm_dim=64, seed=0)
    ref = PL.protein_from_sequence("ACDEFGHIKLMNPQRSTVWYACDEFGHIKLMNPQR")            # 35 residues against the complex's 40
    ref.atom_pos[:, 1] = np.asarray(data["residue_atom_pos"], dtype=np.float32)[3:38, 1] + 0.5
    ref.atom_mask[:, 1] = 1.0
    ref.atom_mask[7, 1] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=tmp_path / "plain")
        out = PL.generate_samples(model, data, num_samples=3, batch_size=2, seed=4, output_dir=tmp_path / "aligned", align_to=ref,
                                  correspondence="structure")
    assert len(plain) == 4 and len(out) == 5
    pos0, pos, info = plain[0], out[0], out[4]
    assert sorted(info) == ["diversity", "mapping", "mirrored", "n_aligned", "rmsd", "rotation", "tmscore", "translation"]
    assert info["n_aligned"].shape == (3,) and info["mapping"].shape == (3, 40) and info["mapping"].max() < 35 and (info["mapping"] != 7).all()
    moved = align.apply(torch.from_numpy(pos0).to(DEV), torch.from_numpy(info["rotation"]).to(DEV), torch.from_numpy(info["translation"]).to(DEV))
    assert np.array_equal(pos, moved.cpu().numpy())
    ca = np.nonzero(np.asarray(data["residue_atom_mask"])[:, 1] > 0.5)[0]
    rca = np.nonzero(ref.atom_mask[:, 1] > 0.5)[0]
    yc = ref.atom_pos[rca, 1].astype(np.float64)
    got = dict(tm=info["tmscore"], rmsd=info["rmsd"], n_aligned=info["n_aligned"], rotation=info["rotation"], translation=info["translation"],
               mirrored=info["mirrored"], mapping=info["mapping"])
    for k in range(3):
        check_entry(got, (k,), pos0[k, 8:48].astype(np.float64)[ca], yc, ca, rca, 40, f"sample {k}")
    lines = (tmp_path / "aligned" / "sample_tmscores.txt").read_text().splitlines()
    assert len(lines) == 3 and [float(v) for v in lines] == [float(v) for v in info["tmscore"]]
    z = np.load(tmp_path / "aligned" / "sample_alignment.npz")
    assert sorted(z.files) == sorted(info) and np.array_equal(z["mapping"], info["mapping"]) and np.array_equal(z["n_aligned"], info["n_aligned"])
