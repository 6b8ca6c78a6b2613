"""GPU: libprd_quality.so through protein_redesign_amd.quality against the float64 yardstick tests/quality_ref.py.

Comparisons sit on thresholds, so the fp32 sweep and float64 may disagree on a pair whose margin is below the fp32 distance error.  That
error is derivable: the inputs are fp32, a difference of coordinates below 200 Angstrom rounds by at most 0.5 ulp(200) ~ 7.6e-6, so a
distance is off by about 2e-5 Angstrom at most.  A comparison whose sides are within 1e-4 Angstrom is AMBIGUOUS; quality_ref gives every
count with the ambiguous comparisons all false and all true, and the device count must lie between the two.  So that this band hides
nothing, every case asserts that the ambiguous pairs are at most 0.2 % of the included ones, and the sigma = 0 sample and the mirror
image must be exact: preserved == 4 total as integers.

Shapes: the row tile of the kernels is 64 (one row per lane) and the column tile 256; N runs over both edges +-1, the smallest sizes,
and one case of 1100 rows (18 row tiles, 5 column tiles, the last a quarter full)."""
import functools
import warnings

import numpy as np
import pytest
import torch

import quality_ref as QR
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd import quality

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 0.002
PAD = 96                # sentinel elements on either side of every output
INT_SENTINEL, FLOAT_SENTINEL = -7777, -1234.5
# (N, S, first sample kind, masks, strided): kinds cycle exact, mirror, far, sigma 0.3, 1, 3 (quality_ref.samples)
CASES = [(1, 1, 0, "ones", False), (2, 1, 3, "ones", False), (3, 5, 0, "ones", False), (63, 1, 4, "alt", False), (64, 5, 1, "ones", False),
         (65, 5, 2, "disjoint", False), (65, 1, 5, "empty", False), (255, 1, 3, "ones", False), (256, 5, 0, "alt", False),
         (257, 6, 0, "ones", True), (257, 5, 1, "disjoint", False), (1100, 3, 3, "ones", True)]
IDS = ["N%d-S%d-%s%s" % (c[0], c[1], c[3], "-strided" if c[4] else "") for c in CASES]


def masks(kind, N):
    i = np.arange(N)
    if kind == "ones":
        return np.ones(N, np.float32), np.ones(N, np.float32)
    if kind == "alt":
        return (i % 2 == 0).astype(np.float32), (i % 3 != 1).astype(np.float32)
    if kind == "empty":
        return np.zeros(N, np.float32), np.ones(N, np.float32)
    return (i < N // 3).astype(np.float32), (i >= N // 3).astype(np.float32)         # disjoint: the protein-ligand form


@functools.lru_cache(maxsize=None)
def inputs(case):
    """the inputs of a case and its float64 references, computed once and shared by the tests (read only)"""
    N, S, start, kind, _ = case
    rng = np.random.default_rng(100 * N + S)
    y = QR.walk(rng, N)
    x, kinds = QR.samples(rng, y, S, start)
    rm, cm = masks(kind, N)
    ex_sym = np.triu(rng.random((N, N)) < 0.3, 1)
    ex_sym = (ex_sym | ex_sym.T).astype(np.uint8)
    ex_few = np.ones((N, N), np.uint8)                          # everything but a few ordered pairs
    for _ in range(6):
        ex_few[rng.integers(N), rng.integers(N)] = 0
    return dict(y=y, x=x, kinds=kinds, rm=rm, cm=cm, ex_sym=ex_sym, ex_few=ex_few,
                lddt=QR.lddt_counts(x, y, rm, cm, 15.0),
                contacts={name: QR.contacts_counts(x, rm, cm, 4.5, ex) for name, ex in (("none", None), ("sym", ex_sym), ("few", ex_few))})


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype, sentinel):
    """(buffer, view of ``shape`` in its middle): the view and PAD elements on either side of it hold the sentinel"""
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[PAD: PAD + n].view(shape)


def intact(buf, sentinel):
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def raw_lddt(x, y, rm, cm, radius, S=None, N=None):
    """prd_quality_lddt itself on sentinel-filled, guarded outputs -> (code, preserved, total, bands intact)"""
    S, N = x.shape[0] if S is None else S, x.shape[1] if N is None else N
    pb, pres = guarded((x.shape[0], x.shape[1]), torch.int32, INT_SENTINEL)
    tb, tot = guarded((x.shape[1],), torch.int32, INT_SENTINEL)
    code = quality.lib().prd_quality_lddt(pres.data_ptr(), tot.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1), y.data_ptr(), y.stride(0),
                                          rm.data_ptr(), cm.data_ptr(), radius, S, N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, pres, tot, intact(pb, INT_SENTINEL) and intact(tb, INT_SENTINEL)


def raw_contacts(x, a, b, cutoff, ex=None, S=None, N=None):
    S, N = x.shape[0] if S is None else S, x.shape[1] if N is None else N
    cb, cnt = guarded((x.shape[0],), torch.int32, INT_SENTINEL)
    nb, near = guarded((x.shape[0], x.shape[1]), torch.float32, FLOAT_SENTINEL)
    code = quality.lib().prd_quality_contacts(cnt.data_ptr(), near.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1), a.data_ptr(), b.data_ptr(),
                                              None if ex is None else ex.data_ptr(), cutoff, S, N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, cnt, near, intact(cb, INT_SENTINEL) and intact(nb, FLOAT_SENTINEL)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lddt_counts(case):
    N, S, _, kind, strided = case
    I = inputs(case)
    ref = I["lddt"]
    x, y, rm, cm = dev(I["x"]), dev(I["y"]), dev(I["rm"]), dev(I["cm"])
    code, pres, tot, bands = raw_lddt(x, y, rm, cm, 15.0)
    assert code == 0 and bands                                  # nothing outside the outputs was written
    pres, tot = pres.cpu().numpy(), tot.cpu().numpy()
    assert (pres != INT_SENTINEL).all() and (tot != INT_SENTINEL).all()           # every element was written
    off = I["rm"] < 0.5
    assert (tot[off] == 0).all() and (pres[:, off] == 0).all()
    share = ref["ambiguous"] / np.maximum(ref["included"], 1)
    print(f"lddt N={N} S={S} {kind}: included {int(ref['included'][0])}, ambiguous {ref['ambiguous'].tolist()} (share max {share.max():.2e}), "
          f"differs from float64 in {int((pres != ref['preserved']).sum())} rows, by at most {int(np.abs(pres - ref['preserved']).max())}")
    assert (share <= CAP).all()                                 # the band below may not hide a failure
    # total: exact wherever no reference distance is within 1e-4 of the radius, bracketed elsewhere
    assert np.array_equal(tot[~ref["near_radius"]], ref["total"][~ref["near_radius"]])
    assert (ref["total_lo"] <= tot).all() and (tot <= ref["total_hi"]).all()
    assert (ref["preserved_lo"] <= pres).all() and (pres <= ref["preserved_hi"]).all()
    for s, name in enumerate(I["kinds"]):
        if name in ("exact", "mirror"):
            assert np.array_equal(pres[s], 4 * tot), name       # as integers, in every row
    # a second launch is bit-identical
    code2, pres2, tot2, _ = raw_lddt(x, y, rm, cm, 15.0)
    assert code2 == 0 and np.array_equal(pres2.cpu().numpy(), pres) and np.array_equal(tot2.cpu().numpy(), tot)
    # the public function: same integers, the scores are their float64 quotients; partner_mask=None means mask
    got = quality.lddt(x, y, rm, partner_mask=cm)
    assert np.array_equal(got.preserved.cpu().numpy(), pres) and np.array_equal(got.total.cpu().numpy(), tot)
    per, score = QR.lddt_scores(pres, tot)
    assert got.per_position.dtype == got.score.dtype == torch.float64
    assert np.array_equal(got.per_position.cpu().numpy(), per, equal_nan=True) and np.array_equal(got.score.cpu().numpy(), score, equal_nan=True)
    assert np.isnan(per[:, tot == 0]).all()
    if kind == "ones":
        same = quality.lddt(x, y, rm)
        assert torch.equal(same.preserved, got.preserved) and torch.equal(same.total, got.total)
    if strided:                                                 # a [N,37,3] view at column 1 as the reference, rows of 5 floats in the samples
        y37 = torch.randn(N, 37, 3, device=DEV)
        y37[:, 1] = y
        x5 = torch.randn(S, N, 5, device=DEV)
        x5[:, :, :3] = x
        view = quality.lddt(x5[:, :, :3], y37[:, 1], rm, partner_mask=cm)
        assert y37[:, 1].stride(0) == 111 and x5[:, :, :3].stride(1) == 5
        assert torch.equal(view.preserved, got.preserved) and torch.equal(view.total, got.total)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_contacts_counts(case):
    N, S, _, kind, strided = case
    I = inputs(case)
    x, a, b = dev(I["x"]), dev(I["rm"]), dev(I["cm"])
    plain = None
    for name, ex in (("none", None), ("sym", I["ex_sym"]), ("few", I["ex_few"])):
        ref = I["contacts"][name]
        exd = None if ex is None else dev(ex)
        code, cnt, near, bands = raw_contacts(x, a, b, 4.5, exd)
        assert code == 0 and bands
        cnt, near = cnt.cpu().numpy(), near.cpu().numpy()
        assert (cnt != INT_SENTINEL).all() and (near != FLOAT_SENTINEL).all()
        print(f"contacts N={N} S={S} {kind} exclude={name}: qualifying {ref['qualifying']}, count {cnt.tolist()} (float64 {ref['count'].tolist()}), "
              f"ambiguous {ref['ambiguous'].tolist()}")
        assert (ref["ambiguous"] <= max(1, CAP * ref["qualifying"])).all()
        assert (ref["count_lo"] <= cnt).all() and (cnt <= ref["count_hi"]).all()
        none = np.isinf(ref["nearest"])
        assert np.array_equal(np.isposinf(near), none)          # +inf exactly where there is no partner, and outside A
        assert none[:, I["rm"] < 0.5].all()
        assert np.abs(near[~none] - ref["nearest"][~none]).max(initial=0.0) < 1e-4
        code2, cnt2, near2, _ = raw_contacts(x, a, b, 4.5, exd)
        assert code2 == 0 and np.array_equal(cnt2.cpu().numpy(), cnt) and np.array_equal(near2.cpu().numpy(), near)
        got = quality.contacts(x, a, b, 4.5, exclude=exd if exd is None or name == "sym" else exd.bool())
        assert np.array_equal(got.count.cpu().numpy(), cnt) and np.array_equal(got.nearest.cpu().numpy(), near)
        plain = got if ex is None else plain
    if strided:                                                 # rows of 5 floats
        x5 = torch.randn(S, N, 5, device=DEV)
        x5[:, :, :3] = x
        view = quality.contacts(x5[:, :, :3], a, b, 4.5)
        assert torch.equal(view.count, plain.count) and torch.equal(view.nearest, plain.nearest)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in (3, 64, 257, 1100) and c[3] == "ones"], ids=lambda c: "N%d" % c[0])
def test_a_pair_that_qualifies_in_both_orders_is_counted_once(case):
    """A = B: with the strict upper triangle excluded only the orders i > j qualify, with the lower one only i < j; each census then
    counts every unordered pair once, and so must the census without an exclusion -- half the ordered count, exactly (d_ij == d_ji bit for bit)"""
    N = case[0]
    I = inputs(case)
    x, ones = dev(I["x"]), torch.ones(N, device=DEV)
    upper = torch.ones(N, N, device=DEV).triu(1).bool()
    both = quality.contacts(x, ones, ones, 4.5).count
    low = quality.contacts(x, ones, ones, 4.5, exclude=upper).count
    up = quality.contacts(x, ones, ones, 4.5, exclude=upper.T.contiguous()).count
    assert torch.equal(low, up) and torch.equal(low + up, 2 * both) and int(both.max()) > 0


def test_refusals_leave_the_outputs_untouched():
    D = quality._DEFINES
    I = inputs(CASES[3])
    x, y, rm, cm = dev(I["x"]), dev(I["y"]), dev(I["rm"]), dev(I["cm"])
    for kw, want in ((dict(N=quality.MAX_N + 1), D["ERR_UNSUPPORTED"]), (dict(S=quality.MAX_S + 1), D["ERR_UNSUPPORTED"]), (dict(S=0), D["ERR_ARG"])):
        code, pres, tot, bands = raw_lddt(x, y, rm, cm, 15.0, **kw)
        assert code == want and bands and bool((pres == INT_SENTINEL).all()) and bool((tot == INT_SENTINEL).all()), kw
        code, cnt, near, bands = raw_contacts(x, rm, cm, 4.5, **kw)
        assert code == want and bands and bool((cnt == INT_SENTINEL).all()) and bool((near == FLOAT_SENTINEL).all()), kw
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        code, pres, tot, _ = raw_lddt(x, y, rm, cm, bad)
        assert code == D["ERR_ARG"] and bool((pres == INT_SENTINEL).all()) and bool((tot == INT_SENTINEL).all()), bad
        code, cnt, near, _ = raw_contacts(x, rm, cm, bad)
        assert code == D["ERR_ARG"] and bool((cnt == INT_SENTINEL).all()) and bool((near == FLOAT_SENTINEL).all()), bad
        with pytest.raises(ValueError, match="radius"):
            quality.lddt(x, y, rm, radius=bad)
        with pytest.raises(ValueError, match="cutoff"):
            quality.contacts(x, rm, cm, bad)
    big = torch.zeros(1, quality.MAX_N + 1, 3, device=DEV)
    with pytest.raises(ValueError, match="PRD_QUALITY_MAX_N"):
        quality.lddt(big, big[0], torch.ones(quality.MAX_N + 1, device=DEV))
    with pytest.raises(ValueError, match="PRD_QUALITY_MAX_N"):
        quality.contacts(big, torch.ones(quality.MAX_N + 1, device=DEV), torch.ones(quality.MAX_N + 1, device=DEV), 3.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        quality.lddt(x.cpu(), y, rm)
    with pytest.raises(ValueError, match="is on"):
        quality.lddt(x, y.cpu(), rm)


# ---- assess: a complex with planted defects -------------------------------------------------------------------------------------------

NA, NR = 8, 40


def planted_complex():
    """A clean complex over the rows of synthetic_batch([(8, 40)]) and a copy with hand-planted defects.  Clean: the residues on a serpentine
    of 3.8 Angstrom steps (4 rows of 10 in the plane z = 0), the ligand a straight chain of 1.5 Angstrom bonds 6 Angstrom above it, everything
    jittered by ~0.03 Angstrom so that no distance sits on a threshold.  Residue 38 has no C-alpha marked.  Planted:
      ligand atom 7 moved onto the C-alpha of residue 35 (0.3 above it)   -> 1 ligand clash, and its bond to atom 6 is torn
      the bond of atoms 0 and 1 stretched to 3 Angstrom                   -> with the torn one, 2 bond outliers
      residue 0 pulled 2.2 Angstrom away from residue 1: a step of 6       -> 1 chain break
      residue 39 placed 2 Angstrom above residue 25                       -> 1 C-alpha clash (its step from 38 does not count: 38 has no C-alpha)"""
    from protein_redesign_amd.synthetic import synthetic_batch
    rng = np.random.default_rng(7)
    batch = synthetic_batch([(NA, NR)], esm_dim=16, seed=3)
    k = np.arange(NA)
    batch["bond_distance"][0, :NA, :NA] = torch.from_numpy(np.abs(k[:, None] - k[None, :]))
    batch["residue_atom_mask"][0, NA + 38, 1] = 0.0
    clean = np.zeros((NA + NR, 3))
    clean[:NA] = np.stack([10.0 + 1.5 * k, np.full(NA, 5.7), np.full(NA, 6.0)], 1)
    for r in range(NR):
        row, col = divmod(r, 10)
        clean[NA + r] = [3.8 * (col if row % 2 == 0 else 9 - col), 3.8 * row, 0.0]
    clean += 0.03 * rng.normal(size=clean.shape)
    bad = clean.copy()
    bad[7] = bad[NA + 35] + [0.0, 0.0, 0.3]
    bad[0] = bad[1] + 3.0 * (bad[0] - bad[1]) / np.linalg.norm(bad[0] - bad[1])
    bad[NA + 0] = bad[NA + 1] + 6.0 * (bad[NA + 0] - bad[NA + 1]) / np.linalg.norm(bad[NA + 0] - bad[NA + 1])
    bad[NA + 39] = bad[NA + 25] + [0.0, 0.0, 2.0]
    pos = np.stack([clean, bad, bad * [1.0, 1.0, -1.0]]).astype(np.float32)
    return batch, pos


def test_assess_names_the_planted_defects():
    batch, pos = planted_complex()
    ca = batch["residue_atom_mask"][0, :, 1].numpy() > 0.5
    want = QR.assess(pos, NA, NR, ca, batch["bond_distance"][0].numpy(), batch["residue_index"][0].numpy(), batch["residue_chain_index"][0].numpy(),
                     ref=pos[0])
    # the fixture keeps clear of every threshold, so that float64 and fp32 must agree exactly
    rows = np.arange(NA + NR)
    lig, res = rows < NA, (rows >= NA) & ca
    for rmask, cmask, radius in ((res, res, 15.0), (lig, res, 10.0), (lig, lig, 15.0)):
        assert QR.lddt_counts(pos, pos[0], rmask, cmask, radius)["ambiguous"].sum() == 0
    got = quality.assess(torch.from_numpy(pos).to(DEV), batch, torch.from_numpy(pos[0]).to(DEV))
    got = {k: v.cpu().numpy() for k, v in got.items()}
    print({k: v.tolist() for k, v in got.items() if v.ndim == 1})
    assert sorted(got) == sorted(want) == sorted(["ca_clashes", "ligand_clashes", "ligand_self_clashes", "ligand_bond_outliers", "chain_breaks", "pocket",
                                                   "pocket_size", "lddt_ca", "lddt_ca_per_residue", "lddt_pli", "lddt_ligand", "pocket_recall"])
    planted = {"ca_clashes": [0, 1, 1], "ligand_clashes": [0, 1, 1], "ligand_self_clashes": [0, 0, 0], "ligand_bond_outliers": [0, 2, 2],
               "chain_breaks": [0, 1, 1]}
    for name, numbers in planted.items():
        assert got[name].tolist() == numbers == want[name].tolist(), name
    assert got["pocket"].shape == (3, NA + NR) and np.array_equal(got["pocket"], want["pocket"]) and np.array_equal(got["pocket_size"], want["pocket_size"])
    assert 0 < got["pocket_size"][0] < NR - 1 and not got["pocket"][:, :NA].any() and not got["pocket"][:, NA + 38].any()
    for name in ("lddt_ca", "lddt_pli", "lddt_ligand", "pocket_recall"):
        assert got[name].dtype == np.float64 and got[name].shape == (3,) and np.array_equal(got[name], want[name]), name
    assert got["lddt_ca_per_residue"].shape == (3, NR) and np.array_equal(got["lddt_ca_per_residue"], want["lddt_ca_per_residue"], equal_nan=True)
    assert got["lddt_ca"][0] == got["lddt_pli"][0] == got["lddt_ligand"][0] == got["pocket_recall"][0] == 1.0
    assert got["lddt_ca"][1] < 1.0 and got["lddt_pli"][1] < 1.0 and got["lddt_ligand"][1] < 1.0
    assert np.isnan(got["lddt_ca_per_residue"][:, 38]).all()                        # no C-alpha: no included pair
    # a mirror image scores exactly like the original, in every metric
    for name, v in got.items():
        assert np.array_equal(v[1], v[2], equal_nan=True), name
    # without ligand coordinates in the reference, and without a reference
    no_lig = quality.assess(torch.from_numpy(pos).to(DEV), batch, torch.from_numpy(pos[0]).to(DEV), ref_has_ligand=False, num_atoms=NA, num_residues=NR)
    assert sorted(set(got) - set(no_lig)) == ["lddt_ligand", "lddt_pli", "pocket_recall"] and np.array_equal(no_lig["lddt_ca"].cpu().numpy(), got["lddt_ca"])
    alone = quality.assess(torch.from_numpy(pos).to(DEV), batch)
    assert sorted(set(got) - set(alone)) == ["lddt_ca", "lddt_ca_per_residue", "lddt_ligand", "lddt_pli", "pocket_recall"]
    # a keyword moves a cutoff: at 1.9 Angstrom the planted 2 Angstrom pair is no clash
    assert quality.assess(torch.from_numpy(pos).to(DEV), batch, ca_clash=1.9)["ca_clashes"].tolist() == [0, 0, 0]


# ---- generate_samples(assess=...) with the small model of smoke() ------------------------------------------------------------------------

SELF_KEYS = ["ca_clashes", "chain_breaks", "ligand_bond_outliers", "ligand_clashes", "ligand_self_clashes", "pocket", "pocket_size"]
INPUT_KEYS = sorted(SELF_KEYS + ["lddt_ca", "lddt_ca_per_residue", "lddt_pli", "lddt_ligand", "pocket_recall"])


def test_generate_samples_end_to_end(tmp_path):
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    args = make_args(single_dim=128, pair_dim=64, num_blocks=2, esm_dim=64, num_steps=16, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    data = synthetic_sample(NA, NR, esm_dim=64, seed=0)
    kw = dict(num_samples=2, batch_size=2, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(model, data, output_dir=tmp_path / "plain", **kw)
        alone = PL.generate_samples(model, data, output_dir=tmp_path / "self", assess="self", **kw)
        scored = PL.generate_samples(model, data, output_dir=tmp_path / "input", assess="input", **kw)
        both = PL.generate_samples(model, data, output_dir=tmp_path / "both", assess="input", align_to="input", **kw)
        prot = PL.generate_samples(model, data, assess=PL.Protein(np.zeros(NR, np.int64), np.arange(NR), np.zeros(NR, np.int64),
                                                                  data["residue_atom_pos"].numpy(), np.ones((NR, 37), np.float32)), **kw)
    # assess=None: exactly today's tuple and files
    assert len(plain) == 4 and sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    assert len(alone) == 5 and len(scored) == 5 and len(both) == 6 and len(prot) == 5
    for out in (alone, scored, prot):                           # scoring changes nothing else
        assert np.array_equal(out[0], plain[0]) and np.array_equal(out[1], plain[1])
    q_self, q, q_both, q_prot = alone[4], scored[4], both[5], prot[4]
    assert sorted(q_self) == SELF_KEYS and sorted(q) == INPUT_KEYS == sorted(q_both)
    assert sorted(q_prot) == sorted(SELF_KEYS + ["lddt_ca", "lddt_ca_per_residue"])
    assert "tmscore" in both[4] and "mirrored" in both[4]       # the alignment dict first, then the quality dict
    for name in INPUT_KEYS:
        want = (2, NR) if name in ("pocket", "lddt_ca_per_residue") else (2,)
        assert isinstance(q[name], np.ndarray) and q[name].shape == want, name
    for name in SELF_KEYS:
        assert np.array_equal(q_self[name], q[name]) and q[name].dtype == np.int32, name
    # the yardstick on the samples that came back
    batch = PL.collate_fn([data])
    ref = np.concatenate([data["atom_pos"].numpy(), data["residue_atom_pos"][:, 1].numpy()]).astype(np.float32)
    want = QR.assess(plain[0], NA, NR, batch["residue_atom_mask"][0, :, 1].numpy() > 0.5, batch["bond_distance"][0].numpy(),
                     batch["residue_index"][0].numpy(), batch["residue_chain_index"][0].numpy(), ref=ref)
    for name in SELF_KEYS:
        assert np.array_equal(q[name], want[name][:, NA:] if name == "pocket" else want[name]), name
    assert np.array_equal(q["pocket_recall"], want["pocket_recall"], equal_nan=True)
    # lDDT = P / (4 T): a pair on a threshold moves P by at most 4 and T by at most 1, so k ambiguous pairs move the score by at most 2 k / T_lo.
    # The same bound holds between the runs with and without align_to: its transform rounds a coordinate by ~1e-5, far inside the band
    lig, res = np.r_[np.ones(NA), np.zeros(NR)], np.r_[np.zeros(NA), np.ones(NR)]
    for name, rmask, cmask, radius in (("lddt_ca", res, res, 15.0), ("lddt_pli", lig, res, 10.0), ("lddt_ligand", lig, lig, 15.0)):
        c = QR.lddt_counts(plain[0], ref, rmask, cmask, radius)
        slack = 2.0 * c["ambiguous"] / np.maximum(c["total_lo"].sum(), 1) + 1e-12
        print(name, q[name].tolist(), want[name].tolist(), "ambiguous", c["ambiguous"].tolist(), "of", c["included"].tolist())
        assert (np.abs(q[name] - want[name]) <= slack).all(), name
        assert (np.abs(q_both[name] - q[name]) <= slack).all(), name
    assert np.array_equal(q_prot["lddt_ca"], q["lddt_ca"]) and np.array_equal(q_prot["lddt_ca_per_residue"], q["lddt_ca_per_residue"], equal_nan=True)
    # scoring commutes with align_to: the integer metrics exactly
    for name in SELF_KEYS:
        assert np.array_equal(q_both[name], q[name]), name
    assert np.array_equal(q_both["pocket_recall"], q["pocket_recall"], equal_nan=True)
    # the files round-trip
    z = np.load(tmp_path / "input" / "sample_quality.npz")
    assert sorted(z.files) == INPUT_KEYS and all(np.array_equal(z[k], q[k], equal_nan=True) for k in z.files)
    lines = (tmp_path / "input" / "sample_quality.txt").read_text().splitlines()
    cols = [c for c in quality.SCALAR_COLUMNS if c in q]
    assert lines[0] == "# " + " ".join(cols) and len(lines) == 3 and len(cols) == 10
    table = np.loadtxt(tmp_path / "input" / "sample_quality.txt", ndmin=2)
    assert table.shape == (2, 10) and all(np.array_equal(table[:, j], q[c].astype(np.float64), equal_nan=True) for j, c in enumerate(cols))
    assert (tmp_path / "both" / "sample_alignment.npz").exists() and (tmp_path / "both" / "sample_quality.txt").exists()
    assert (tmp_path / "self" / "sample_quality.txt").read_text().splitlines()[0] == "# " + " ".join(quality.SCALAR_COLUMNS[:6])
