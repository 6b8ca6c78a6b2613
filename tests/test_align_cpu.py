"""CPU: the yardstick of the alignment tests (tests/align_ref.py) on planted cases, the header / build / export list of
libprd_align.so, and the ``align_to`` argument of pipeline.generate_samples as far as it goes without a GPU."""
import os

import numpy as np
import pytest
import torch

import align_ref as AR
from protein_redesign_amd import _lib, build
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.synthetic import synthetic_sample
from sample_stubs import _NoDevice, _Stub, header_entries

LENGTHS = [3, 4, 5, 21, 22, 63, 64, 65, 130, 257, 1025]
HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


def cases(L):
    """core fractions per length: at L = 3, 4 only the fully rigid case is meaningful"""
    return [1.0] if L < 5 else [1.0, 0.6, 0.35]


@pytest.mark.parametrize("L", LENGTHS)
def test_reference_search_recovers_the_planted_transform(L):
    rng = np.random.default_rng(1000 + L)
    for frac in cases(L):
        x, y, R0, t0, core = AR.planted(rng, L, frac)
        got = AR.superimpose(x, y, mirror=False)
        R, t = got["rotation"], got["translation"]
        assert got["tm"] >= AR.tm_of(x, y, R0, t0) - 1e-4, (L, frac)
        assert abs(got["tm"] - AR.tm_of(x, y, R, t)) < 1e-12 and abs(got["rmsd"] - AR.rmsd_of(x, y, R, t)) < 1e-12
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
        Rk, tk = AR.kabsch(x, y)
        assert got["tm"] >= AR.tm_of(x, y, Rk, tk) - 1e-12          # the first seed is the whole-set fit
        if frac < 1.0 and L >= 21:
            assert AR.tm_of(x, y, Rk, tk) < got["tm"]                # the search is really exercised
        assert AR.superimpose(x, y, mirror=False, mode="rmsd")["rmsd"] <= got["rmsd"] + 1e-12


@pytest.mark.parametrize("L", [63, 130])
def test_reference_mirror(L):
    rng = np.random.default_rng(2000 + L)
    x, y, R0, t0, _ = AR.planted(rng, L, 1.0, mirrored=True)
    on, off = AR.superimpose(x, y, mirror=True), AR.superimpose(x, y, mirror=False)
    assert on["mirrored"] == 1 and abs(np.linalg.det(on["rotation"]) + 1.0) < 1e-12 and on["tm"] >= AR.tm_of(x, y, R0, t0) - 1e-4
    assert off["mirrored"] == 0 and on["tm"] - off["tm"] > 0.3
    x, y, *_ = AR.planted(rng, L, 1.0)
    assert AR.superimpose(x, y, mirror=True)["mirrored"] == 0


def test_reference_seeds_and_short_chains():
    assert AR.seeds(3) == [(0, 3)] and AR.seeds(4) == [(0, 4), (0, 3), (1, 3)]
    assert AR.seeds(5) == [(0, 5), (0, 4), (1, 4), (0, 3), (1, 3), (2, 3)]
    assert AR.seeds(22)[:6] == [(0, 22), (0, 11), (5, 11), (10, 11), (11, 11), (0, 5)] and min(Lf for _, Lf in AR.seeds(22)) == 4
    s = AR.seeds(320)
    assert [Lf for _, Lf in s if _ == 0] == [320, 160, 80, 40, 20, 10, 5, 4] and all(0 <= a and a + Lf <= 320 for a, Lf in s)
    assert AR.superimpose(np.zeros((2, 3)), np.ones((2, 3))) == dict(tm=0.0, rmsd=0.0, rotation=pytest.approx(np.eye(3)),
                                                                      translation=pytest.approx(np.zeros(3)), mirrored=0)
    assert AR.d0_of(21) == 0.5 and abs(AR.d0_of(22) - (1.24 * 7 ** (1 / 3) - 1.8)) < 1e-12


def test_seed_filter_leaves_the_default_search_alone_and_decisive_seeds_exist():
    """The condition tests/test_align_range.py relies on, without a GPU: among the planted 3-residue cores (AR.core3_case, L = 12, 20,
    21) there are at least 8 in which the float64 search drops by 1e-3 or more once its own winning seed is left out, with at least 5
    distinct winning seeds.  A later change of the yardstick cannot hollow the device test out without failing here."""
    rng = np.random.default_rng(3000)
    x, y, *_ = AR.planted(rng, 21, 0.35)
    full = AR.tm_search(x, y)
    same = AR.tm_search(x, y, seed_filter=lambda k: True, with_seed=True)
    assert len(full) == 3 and full[0] == same[0] and np.array_equal(full[1], same[1]) and 0 <= same[3] < len(AR.seeds(21))
    assert AR.tm_search(x, y, seed_filter=lambda k: k == 0)[0] == pytest.approx(AR.tm_of(x, y, *AR.kabsch(x, y)), abs=1e-12) or \
        AR.tm_search(x, y, seed_filter=lambda k: k == 0)[0] > AR.tm_of(x, y, *AR.kabsch(x, y))     # seed 0, round 0 is the Kabsch fit
    cases = AR.decisive_cases()
    seeds = {c["seed"] for c in cases}
    assert len(cases) >= 8 and len(seeds) >= 5, (len(cases), sorted(seeds))
    for c in cases:
        assert c["tm"] - c["tm_without"] >= 1e-3 and np.abs(c["x"]).max() < 100.0 and np.abs(c["y"]).max() < 100.0
        start, Lf = AR.seeds(c["L"])[c["seed"]]
        assert AR.tm_search(c["x"], c["y"], seed_filter=lambda k: k == c["seed"])[0] == c["tm"]     # that seed alone reaches it
        assert np.array_equal(c["x"], c["x"].astype(np.float32)) and Lf <= c["L"]


# ---- header, build, export list ---------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("align")
    assert sorted(e) == ["prd_align_apply", "prd_align_superimpose", "prd_align_version", "prd_align_workspace_bytes"]
    assert all(x.inject is None for x in e.values())            # no parameter is an injected word
    assert e["prd_align_workspace_bytes"].restype is _lib.cz and len(e["prd_align_superimpose"].argtypes) == 21
    from protein_redesign_amd import align
    assert align.ENTRIES == e
    assert not set(e) & set(_lib.ENTRIES)                       # nothing of it is part of the denoiser ABI


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_new_kernels_are_reported_apart():
    mine = build.resource_usage(sources=build.SIDE_LIBS["align"].sources)
    assert sorted(mine) == ["align_apply_kernel", "align_compact_kernel", "align_finalize_kernel", "align_search_kernel"]
    assert all(u["scratch"] == 0 for u in mine.values())
    assert mine["align_search_kernel"]["occupancy"] >= 2        # 8 waves per workgroup, one workgroup per CU at the least


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_workspace_bytes_refusals_growth_and_lower_bound():
    """prd_align_workspace_bytes is host code: 0 for what prd_align_superimpose refuses, never smaller for a longer row, and in the cross
    mode at least the header and the (S + R) x 3 planes of N floats that the kernels index."""
    from protein_redesign_amd import align
    build.build_side("align", verbose=False)
    ws = align.lib().prd_align_workspace_bytes
    TM, RMSD, CROSS, SELF = align.MODES["tm"], align.MODES["rmsd"], align.PAIRS_CROSS, align.PAIRS_SELF
    assert ws(2, 3, 4096, CROSS, TM, 1) > 0 and ws(2, 3, 4097, CROSS, TM, 1) == 0
    assert ws(3, 3, 64, SELF, TM, 1) > 0 and ws(3, 2, 64, SELF, TM, 1) == 0 and ws(2, 3, 64, SELF, RMSD, 0) == 0
    assert ws(2, 3, 64, CROSS, 2, 1) == 0 and ws(2, 3, 64, CROSS, -1, 1) == 0          # unknown mode
    assert ws(2, 3, 64, 2, TM, 1) == 0 and ws(2, 3, 64, -1, TM, 1) == 0                # unknown pairs
    assert ws(0, 3, 64, CROSS, TM, 1) == 0 and ws(2, 0, 64, CROSS, TM, 1) == 0 and ws(2, 3, 0, CROSS, TM, 1) == 0
    for S, R, pairs, mode, mirror in ((1, 1, CROSS, TM, 1), (2, 3, CROSS, TM, 0), (2, 3, CROSS, RMSD, 1), (4, 4, SELF, TM, 1), (1, 1, SELF, TM, 1)):
        sizes = [ws(S, R, N, pairs, mode, mirror) for N in range(3, 4097)]
        assert all(b > 0 and b % 16 == 0 for b in sizes), (S, R, pairs, mode)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (S, R, pairs, mode)
        if pairs == CROSS:
            assert all(b >= 16 * 4 + (S + R) * 3 * N * 4 for N, b in zip(range(3, 4097), sizes)), (S, R, mode)


def test_host_argument_checks_of_the_python_side():
    from protein_redesign_amd import align
    x, m = torch.zeros(2, 5, 3), torch.ones(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        align.superimpose(x, x[0], m)
    with pytest.raises(ValueError, match="float32"):
        align.superimpose(x.double(), x[0], m)
    with pytest.raises(ValueError, match=r"\[K,N,3\]"):
        align.superimpose(torch.zeros(5, 3), x[0], m)
    with pytest.raises(ValueError, match="mode"):
        align._run((x, 15, 3), None, m, 2, 2, 5, align.PAIRS_SELF, "gdt", True)
    with pytest.raises(ValueError, match="4096"):
        align._run((x, 15, 3), None, m, 2, 2, 4097, align.PAIRS_SELF, "tm", True)


# ---- pipeline.generate_samples(align_to=...) ---------------------------------------------------------------------------------------

def test_align_to_input_is_refused_without_coordinates_before_the_model_is_touched():
    lig = {k: v for k, v in synthetic_sample(5, 9, esm_dim=16, seed=8).items() if k.startswith(("atom_", "bond_")) or k == "num_atoms"}
    data = PL.protein_to_data(PL.protein_from_sequence("ACDEFGHIK"), **lig)
    with pytest.raises(ValueError, match="coordinates"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, align_to="input")
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with pytest.raises(ValueError, match="C-alpha"):
        PL.generate_samples(_NoDevice(), dict(full, residue_atom_mask=torch.zeros(9, 37)), num_samples=1, align_to="input")


def test_unknown_align_to_raises():
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with pytest.raises(ValueError, match="align_to"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, align_to="reference")
    with pytest.raises(ValueError, match="9 residues"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, align_to=np.zeros((8, 3)))
    with pytest.raises(ValueError, match="9 residues"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, align_to=PL.protein_from_sequence("ACD"))


def test_align_to_none_takes_the_old_path(tmp_path, monkeypatch):
    import warnings
    from protein_redesign_amd import align
    for name in ("superimpose", "pairwise", "apply", "lib"):
        monkeypatch.setattr(align, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("the alignment ran")))
    data = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        out = PL.generate_samples(_Stub(), data, num_samples=3, batch_size=2, seed=1, output_dir=tmp_path)
    assert len(out) == 4
    pos, logits, proteins, ligands = out
    from protein_redesign_amd.synthetic import NoiseSource
    want = torch.stack([torch.randn(14, 3, generator=NoiseSource(1, k).g) for k in range(3)]).numpy()
    assert np.array_equal(pos, want) and logits.shape == (3, 14, 21)
    assert np.array_equal(proteins[2].atom_pos[:, 1], want[2, 5:14]) and np.array_equal(ligands[1], want[1, :5])
    assert sorted(os.listdir(tmp_path)) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
