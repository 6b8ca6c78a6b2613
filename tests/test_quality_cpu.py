"""CPU: the yardstick of the quality tests (tests/quality_ref.py) on hand-made cases, the header / build / export list of
libprd_quality.so, the Python-side argument checks, and the ``assess`` argument of pipeline.generate_samples as far as it goes without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import quality_ref as QR
from protein_redesign_amd import _lib, build
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.synthetic import synthetic_sample
from sample_stubs import _NoDevice, _Stub, header_entries

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
ONES3 = np.ones(3)


# ---- the yardstick on hand-made cases ----------------------------------------------------------------------------------------------

def test_three_collinear_points_have_the_counts_worked_out_by_hand():
    """reference 0, 1, 3 on a line (distances 1, 3, 2); sample 0, 1, 4.2 (distances 1, 4.2, 3.2).  Radius 2.5 includes (0,1) and (1,2) in both
    orders.  |d - D|: pair (0,1) 0 -> all 4 thresholds; pair (1,2) 1.2 -> thresholds 2 and 4."""
    y = np.array([[0.0, 0, 0], [1.0, 0, 0], [3.0, 0, 0]])
    x = np.array([[[0.0, 0, 0], [1.0, 0, 0], [4.2, 0, 0]]])
    c = QR.lddt_counts(x, y, ONES3, ONES3, 2.5)
    assert c["total"].tolist() == [1, 2, 1] and c["preserved"].tolist() == [[4, 6, 2]]
    assert c["total_lo"].tolist() == c["total_hi"].tolist() == [1, 2, 1] and c["ambiguous"].tolist() == [0] and c["included"].tolist() == [4]
    per, score = QR.lddt_scores(c["preserved"], c["total"])
    assert np.allclose(per, [[1.0, 0.75, 0.5]]) and np.allclose(score, [12 / 16])            # pooled over pairs, not mean(per) = 0.75 by chance
    c = QR.lddt_counts(x, y, ONES3, ONES3, 3.5)                 # now (0,2) too: |4.2 - 3| = 1.2
    assert c["total"].tolist() == [2, 2, 2] and c["preserved"].tolist() == [[6, 6, 4]]
    per, score = QR.lddt_scores(c["preserved"], c["total"])
    assert np.allclose(score, [16 / 24]) and np.allclose(per.mean(), 16 / 24)
    # rows = point 2 alone, columns = points 0 and 1: the protein-ligand form; a row outside the mask has nothing and scores NaN
    c = QR.lddt_counts(x, y, [0, 0, 1], [1, 1, 0], 3.5)
    assert c["total"].tolist() == [0, 0, 2] and c["preserved"].tolist() == [[0, 0, 4]]
    per, score = QR.lddt_scores(c["preserved"], c["total"])
    assert np.isnan(per[0, :2]).all() and per[0, 2] == 0.5 and score[0] == 0.5
    # contacts on the same sample: below 1.5 only (0,1); A = B counts it once, A = {0}, B = {1} once, and the nearest partners
    k = QR.contacts_counts(x, ONES3, ONES3, 1.5)
    assert k["count"].tolist() == [1] and np.allclose(k["nearest"], [[1.0, 1.0, 3.2]]) and k["qualifying"] == 3
    k = QR.contacts_counts(x, [1, 0, 0], [0, 1, 1], 1.5)
    assert k["count"].tolist() == [1] and k["nearest"][0].tolist() == [1.0, np.inf, np.inf]
    ex = np.zeros((3, 3), np.uint8)
    ex[0, 1] = 1                                                # only the order (0,1) is excluded: the pair still qualifies as (1,0)
    k = QR.contacts_counts(x, ONES3, ONES3, 1.5, exclude=ex)
    assert k["count"].tolist() == [1] and np.allclose(k["nearest"], [[4.2, 1.0, 3.2]])
    ex[1, 0] = 1
    assert QR.contacts_counts(x, ONES3, ONES3, 1.5, exclude=ex)["count"].tolist() == [0]


def test_a_structure_scores_one_against_itself_and_against_its_mirror_image():
    rng = np.random.default_rng(5)
    y = QR.walk(rng, 65)
    assert np.abs(np.linalg.norm(np.diff(y.astype(np.float64), axis=0), axis=1) - 3.8).max() < 1e-5 and np.abs(y).max() < 100.0
    x = np.stack([y, y @ QR.MIRROR.astype(np.float32)])
    m = np.ones(65)
    c = QR.lddt_counts(x, y, m, m, 15.0)
    assert (c["preserved"] == 4 * c["total"][None]).all() and c["total"].min() > 0
    per, score = QR.lddt_scores(c["preserved"], c["total"])
    assert (per == 1.0).all() and (score == 1.0).all()
    noisy = y + rng.normal(size=y.shape).astype(np.float32)
    assert 0.3 < QR.lddt(noisy[None], y, m)[1][0] < 0.98


def test_a_pair_exactly_at_a_threshold_is_not_preserved():
    y = np.array([[0.0, 0, 0], [2.0, 0, 0]])
    for t, want in ((0.5, 3), (1.0, 2), (2.0, 1), (4.0, 0)):    # |d - D| == t exactly: the strict < fails for t and holds above it
        x = np.array([[[0.0, 0, 0], [2.0 + t, 0, 0]]])
        c = QR.lddt_counts(x, y, np.ones(2), np.ones(2), 15.0)
        assert c["preserved"].tolist() == [[want, want]], t
        assert c["preserved_lo"].tolist() == [[want, want]] and c["preserved_hi"].tolist() == [[want + 1, want + 1]] and c["ambiguous"].tolist() == [2]
    c = QR.lddt_counts(y[None], y, np.ones(2), np.ones(2), 2.0)                 # D == radius exactly: not included
    assert c["total"].tolist() == [0, 0] and c["total_hi"].tolist() == [1, 1] and c["near_radius"].all()
    k = QR.contacts_counts(y[None], np.ones(2), np.ones(2), 2.0)                # d == cutoff exactly: no contact
    assert k["count"].tolist() == [0] and k["count_hi"].tolist() == [1] and k["ambiguous"].tolist() == [1]


def test_the_inputs_keep_the_ambiguous_pairs_far_below_the_cap():
    """what tests/test_quality.py asserts per case on the device, here once without one: at most 0.2 % of the included pairs ambiguous"""
    rng = np.random.default_rng(11)
    y = QR.walk(rng, 257)
    x, kinds = QR.samples(rng, y, 6)
    assert kinds == ["exact", "mirror", "far", "sigma0.3", "sigma1", "sigma3"]
    c = QR.lddt_counts(x, y, np.ones(257), np.ones(257), 15.0)
    assert (c["ambiguous"] <= 0.002 * c["included"]).all() and c["included"][0] > 257 * 20
    per, score = QR.lddt_scores(c["preserved"], c["total"])
    assert score[0] == score[1] == 1.0 and score[2] > 0.999 and score[3] > score[4] > score[5] > 0.05     # every threshold sees both outcomes


# ---- header, build, export list ---------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    from protein_redesign_amd import align, quality, tmalign
    e = header_entries("quality")
    assert sorted(e) == ["prd_quality_contacts", "prd_quality_lddt", "prd_quality_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    assert len(e["prd_quality_lddt"].argtypes) == 13 and len(e["prd_quality_contacts"].argtypes) == 12
    assert e["prd_quality_lddt"].argtypes[9] is _lib.cf and e["prd_quality_lddt"].argtypes[3] is _lib.cll
    assert quality.ENTRIES == e
    assert not set(e) & (set(_lib.ENTRIES) | set(align.ENTRIES) | set(tmalign.ENTRIES))
    assert quality.MAX_N == 32768 >= align.MAX_N and quality.MAX_S == 65535 and quality.ABI_VERSION == 100


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_new_kernels():
    mine = build.resource_usage(sources=build.SIDE_LIBS["quality"].sources)
    assert sorted(mine) == ["quality_contacts_kernel", "quality_lddt_kernel"]
    assert all(u["scratch"] == 0 and u["agprs"] == 0 for u in mine.values())
    assert all(u["occupancy"] == 8 and u["lds"] <= 16 * 1024 for u in mine.values())      # 4-wave workgroups, 8 of them per CU


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """the refusals of prd_quality.h are host code that runs before the first HIP call: every one of them is reachable without a GPU, with
    pointers that are never followed"""
    from protein_redesign_amd import quality
    build.build_side("quality", verbose=False)
    L, D = quality.lib(), quality._DEFINES
    assert L.prd_quality_version() == 100
    p = ctypes.c_void_p(4096)
    inf, nan = float("inf"), float("nan")

    def lddt(pres=p, tot=p, x=p, xs=30, xr=3, y=p, yr=3, rm=p, cm=p, radius=15.0, S=2, N=5):
        return L.prd_quality_lddt(pres, tot, x, xs, xr, y, yr, rm, cm, radius, S, N, None)

    def contacts(cnt=p, near=p, x=p, xs=30, xr=3, a=p, b=p, ex=None, cutoff=3.0, S=2, N=5):
        return L.prd_quality_contacts(cnt, near, x, xs, xr, a, b, ex, cutoff, S, N, None)
    for kw in (dict(pres=None), dict(tot=None), dict(x=None), dict(y=None), dict(rm=None), dict(cm=None), dict(S=0), dict(N=0), dict(S=-1),
               dict(xr=2), dict(yr=2), dict(xs=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf)):
        assert lddt(**kw) == D["ERR_ARG"], kw
    for kw in (dict(cnt=None), dict(near=None), dict(x=None), dict(a=None), dict(b=None), dict(S=0), dict(N=-3), dict(xr=1), dict(xs=-5),
               dict(cutoff=0.0), dict(cutoff=nan), dict(cutoff=-inf), dict(cutoff=inf)):
        assert contacts(**kw) == D["ERR_ARG"], kw
    for kw in (dict(N=quality.MAX_N + 1), dict(S=quality.MAX_S + 1)):
        assert lddt(**kw) == contacts(**kw) == D["ERR_UNSUPPORTED"], kw


def test_host_argument_checks_of_the_python_side():
    from protein_redesign_amd import quality
    x, m = torch.zeros(2, 5, 3), torch.ones(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        quality.lddt(x, x[0], m)
    with pytest.raises(RuntimeError, match="GPU only"):
        quality.contacts(x, m, m, 3.0)
    with pytest.raises(ValueError, match="float32"):
        quality.lddt(x.double(), x[0], m)
    with pytest.raises(ValueError, match=r"\[S,N,3\]"):
        quality.contacts(torch.zeros(5, 3), m, m, 3.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            quality.lddt(x, x[0], m, radius=bad)
        with pytest.raises(ValueError, match="cutoff"):
            quality.contacts(x, m, m, bad)
    assert quality.SCALAR_COLUMNS[:6] == ("ca_clashes", "ligand_clashes", "ligand_self_clashes", "ligand_bond_outliers", "chain_breaks", "pocket_size")
    assert "mirror image scores exactly like the original" in quality.__doc__


# ---- pipeline.generate_samples(assess=...) -----------------------------------------------------------------------------------------

def test_assess_input_is_refused_without_coordinates_before_the_model_is_touched():
    lig = {k: v for k, v in synthetic_sample(5, 9, esm_dim=16, seed=8).items() if k.startswith(("atom_", "bond_")) or k == "num_atoms"}
    data = PL.protein_to_data(PL.protein_from_sequence("ACDEFGHIK"), **lig)
    with pytest.raises(ValueError, match="coordinates"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, assess="input")
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with pytest.raises(ValueError, match="C-alpha"):
        PL.generate_samples(_NoDevice(), dict(full, residue_atom_mask=torch.zeros(9, 37)), num_samples=1, assess="input")


def test_unknown_assess_and_a_protein_of_another_length_raise():
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with pytest.raises(ValueError, match="assess must be"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, assess="reference")
    with pytest.raises(ValueError, match="assess must be"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, assess=np.zeros((9, 3)))
    with pytest.raises(ValueError, match="9 residues"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, assess=PL.protein_from_sequence("ACD"))


def test_the_reference_of_assess_is_laid_out_over_the_rows_of_a_sample():
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    assert PL._quality_reference(full, "self") is None
    ref, ligand = PL._quality_reference(full, "input")
    assert ligand and ref.shape == (14, 3) and ref.dtype == np.float32
    assert np.array_equal(ref[:5], full["atom_pos"].numpy()) and np.array_equal(ref[5:], full["residue_atom_pos"][:, 1].numpy())
    no_ligand = {k: v for k, v in full.items() if k != "atom_pos"}
    ref, ligand = PL._quality_reference(no_ligand, "input")
    assert not ligand and not ref[:5].any() and np.array_equal(ref[5:], full["residue_atom_pos"][:, 1].numpy())
    prot = PL.Protein(np.zeros(9, np.int64), np.arange(9), np.zeros(9, np.int64), full["residue_atom_pos"].numpy() + 1.0, np.ones((9, 37), np.float32))
    ref, ligand = PL._quality_reference(full, prot)
    assert not ligand and np.array_equal(ref[5:], prot.atom_pos[:, 1])


def test_assess_none_takes_the_old_path(tmp_path, monkeypatch):
    import warnings
    from protein_redesign_amd import quality
    for name in ("lddt", "contacts", "assess", "lib"):
        monkeypatch.setattr(quality, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("the scoring ran")))
    data = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        out = PL.generate_samples(_Stub(), data, num_samples=3, batch_size=2, seed=1, output_dir=tmp_path)
    assert len(out) == 4
    from protein_redesign_amd.synthetic import NoiseSource
    want = torch.stack([torch.randn(14, 3, generator=NoiseSource(1, k).g) for k in range(3)]).numpy()
    assert np.array_equal(out[0], want) and sorted(os.listdir(tmp_path)) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
