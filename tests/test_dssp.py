"""GPU: libprd_dssp.so, called directly and through protein_redesign_amd.dssp, against the float64 yardstick tests/dssp_ref.py.

Two families of input (dssp_ref.case_inputs): EXACT -- true atoms of ideal chains wandering through the builder's anchor conformations,
with helices, 3-10 helices and the two-strand sheet fixtures of tests/golden/dssp_sheets.npz laid across the tile edges -- and PERTURBED,
the same with Gaussian noise of sigma = 0.1 Angstrom on every atom.  Coordinates stay within 100 Angstrom.

TOLERANCE.  E_TOL is the largest deviation of a float32 numpy restatement of the header's formulas from the float64 one on these very
inputs, measured on the CPU: 2.9e-5 kcal/mol, stated as 3.5e-5 (dssp_ref.E_TOL; tests/test_dssp_cpu.py holds the measurement to
[E_TOL / 2, E_TOL]).  The device uses the same IEEE square roots and divisions in the same order, so it is allowed 4 E_TOL = 1.4e-4 on
every reported energy.  Decisions are compared exactly outside the ambiguity of dssp_ref (band B = 1e-3 kcal/mol >= 8 E_TOL): ``partner``
on every slot that is not loose of every residue that is not ambiguous, ``classes``, ``bridge`` and ``flags`` on every residue farther
than 10 rows from an ambiguous one.  The exact family has no ambiguous residue; the caps of the perturbed one are asserted on the CPU.

Shapes: the sweep's row tile is 64 and its column tile 256, so N runs over 1, 2, 5, 63, 64, 65, 255, 256, 257 and 300, S over 1 and 3,
with 0, 3 and 17 ligand rows in front, a chain break at 63 | 64 and 255 | 256 and a donor mask; the per-residue kernels' tile is 256
with a halo of 10, so N runs over 255, 256, 257, 266 and 600 with a helix across the tile edge, a strand pair whose partners sit in
different tiles, and runs of 1 to 4 residues between longer ones."""
import warnings

import numpy as np
import pytest
import torch

import backbone_ref as BR
import dssp_ref as DR
from no_host_sync import run_without_host_sync
from protein_redesign_amd import backbone as BB
from protein_redesign_amd import chirality as CH
from protein_redesign_amd import dssp as DS
from protein_redesign_amd import pipeline as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 96                # sentinel elements on either side of every output
INT_SENTINEL, FLOAT_SENTINEL, BYTE_SENTINEL = -7777, -1234.5, 0xAB
ALLOWED = 4.0 * DR.E_TOL


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype, sentinel):
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[PAD: PAD + n].view(shape)


def intact(buf, sentinel):
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def ptr(t):
    return None if t is None else t.data_ptr()


def raw_hbonds(atoms, built, link, donor=None, spec=None, S=None, N=None, null=(), **scalars):
    """prd_dssp_hbonds itself on sentinel-filled, guarded outputs -> (code, partner, energy, guard bands intact)"""
    S0, N0 = built.shape
    q, e_min = (scalars.pop(n, v) for n, v in zip(("q", "e_min"), DS.Dssp.of("assign" if spec is None else spec).scalars()[:2]))
    assert not scalars
    pbuf, partner = guarded((S0, N0, 4), torch.int32, INT_SENTINEL)
    ebuf, energy = guarded((S0, N0, 4), torch.float32, FLOAT_SENTINEL)
    arg = lambda name, t: None if name in null else ptr(t)         # noqa: E731
    code = DS.lib().prd_dssp_hbonds(arg("partner", partner), arg("energy", energy), arg("atoms", atoms), arg("built", built), arg("link", link),
                                    ptr(donor), q, e_min, S0 if S is None else S, N0 if N is None else N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, partner, energy, intact(pbuf, INT_SENTINEL) and intact(ebuf, FLOAT_SENTINEL)


def raw_assign(partner, energy, atoms, built, link, spec=None, S=None, N=None, null=(), **scalars):
    """prd_dssp_assign itself on guarded outputs -> (code, classes, flags, bridge, guard bands intact)"""
    S0, N0 = built.shape
    cutoff, cos_bend = (scalars.pop(n, v) for n, v in zip(("cutoff", "cos_bend"), DS.Dssp.of("assign" if spec is None else spec).scalars()[2:]))
    assert not scalars
    cbuf, classes = guarded((S0, N0), torch.uint8, BYTE_SENTINEL)
    fbuf, flags = guarded((S0, N0), torch.int32, INT_SENTINEL)
    bbuf, bridge = guarded((S0, N0, 2), torch.int32, INT_SENTINEL)
    arg = lambda name, t: None if name in null else ptr(t)         # noqa: E731
    code = DS.lib().prd_dssp_assign(arg("classes", classes), arg("flags", flags), arg("bridge", bridge), arg("partner", partner), arg("energy", energy),
                                    arg("atoms", atoms), arg("built", built), arg("link", link), cutoff, cos_bend, S0 if S is None else S,
                                    N0 if N is None else N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, classes, flags, bridge, intact(cbuf, BYTE_SENTINEL) and intact(fbuf, INT_SENTINEL) and intact(bbuf, INT_SENTINEL)


def check_lists(p, e, ref, label):
    """partner equal on every slot that is not loose of every residue that is not ambiguous; energy within 4 E_TOL there"""
    keep = ~ref["ambiguous"][..., None] & ~ref["loose"]
    assert np.array_equal(p[keep], ref["partner"][keep]), label
    worst = float(np.abs(e.astype(np.float64) - ref["energy"])[keep].max(initial=0.0))
    print(f"{label}: {int(keep.sum())} slots compared, {int((~keep).sum())} left out, {int((p[keep] >= 0).sum())} filled, "
          f"max energy deviation {worst:.3e} kcal/mol (allowed {ALLOWED:.1e})")
    assert worst <= ALLOWED, label
    # whatever the slot: an empty one is -1 with energy 0, a filled one has a negative energy, the lower energy comes first
    assert ((p == -1) == (e == 0)).all() and (e <= 0).all() and (p >= -1).all() and (p < p.shape[1]).all()
    for r in (0, 2):
        both = (p[..., r] >= 0) & (p[..., r + 1] >= 0)
        assert (e[..., r][both] <= e[..., r + 1][both]).all() and (p[..., r][both] != p[..., r + 1][both]).all()
        assert not ((p[..., r] < 0) & (p[..., r + 1] >= 0)).any()


@pytest.mark.parametrize("case", DR.HB_CASES, ids=DR.ids(DR.HB_CASES))
def test_hbonds_against_float64(case):
    N, S, na, layout, masked = case
    I = DR.case_inputs(case)
    ref = I["ref"]
    atoms, built, link, donor = dev(I["atoms"]), dev(I["built"]), dev(I["link"]), dev(I["donor"])
    code, partner, energy, bands = raw_hbonds(atoms, built, link, donor)
    assert code == 0 and bands                                  # nothing outside the outputs was written
    p, e = partner.cpu().numpy(), energy.cpu().numpy()
    assert (p != INT_SENTINEL).all() and (e != FLOAT_SENTINEL).all()          # every element was written
    for s in I["exact"]:
        assert not ref["ambiguous"][s].any(), (s, "the case's seed must keep the exact family unambiguous")
    check_lists(p, e, ref, f"N={N} S={S} na={na} {layout}")
    assert (p[:, :na] == -1).all()                              # ligand rows hold no atoms
    # the same bond carries the same bits in the donor's list and in the acceptor's
    for s, d, k in zip(*np.nonzero(p[..., :2] >= 0)):
        a = p[s, d, k]
        for m in (2, 3):
            if p[s, a, m] == d:
                assert bits(e[s, a, m]) == bits(e[s, d, k])
    # the mirror image: bit-equal energies, equal partners
    codem, pm, em, _ = raw_hbonds(dev(DR.mirror(I["atoms"])), built, link, donor)
    assert codem == 0 and np.array_equal(pm.cpu().numpy(), p) and np.array_equal(bits(em.cpu().numpy()), bits(e))
    # determinism: a second launch gives equal bits; the public function gives the same
    code2, p2, e2, _ = raw_hbonds(atoms, built, link, donor)
    assert code2 == 0 and np.array_equal(p2.cpu().numpy(), p) and np.array_equal(bits(e2.cpu().numpy()), bits(e))
    pub = DS.hbonds(atoms, built, link, donor)
    assert pub.partner.shape == (S, N, 4) and pub.partner.dtype == torch.int32 and pub.energy.dtype == torch.float32
    assert np.array_equal(pub.partner.cpu().numpy(), p) and np.array_equal(bits(pub.energy.cpu().numpy()), bits(e))
    if masked:                                                  # a cleared donor donates nothing and is nobody's donor
        off = I["donor"] < 0.5
        assert (p[:, off, :2] == -1).all() and not np.isin(p[..., 2:], np.nonzero(off)[0]).any()


@pytest.mark.parametrize("case", DR.AS_CASES, ids=DR.ids(DR.AS_CASES))
def test_assign_against_float64(case):
    N, S, na, layout, masked = case
    I = DR.case_inputs(case)
    ref = I["ref"]
    atoms, built, link, donor = dev(I["atoms"]), dev(I["built"]), dev(I["link"]), dev(I["donor"])
    code, partner, energy, bands = raw_hbonds(atoms, built, link, donor)
    assert code == 0 and bands
    check_lists(partner.cpu().numpy(), energy.cpu().numpy(), ref, f"N={N} S={S} {layout}")
    code, classes, flags, bridge, bands = raw_assign(partner, energy, atoms, built, link)
    assert code == 0 and bands
    c, f, b = classes.cpu().numpy(), flags.cpu().numpy(), bridge.cpu().numpy()
    assert (f != INT_SENTINEL).all() and (b != INT_SENTINEL).all() and (c < 8).all()          # every element was written
    keep = ~ref["excluded"]
    for s in I["exact"]:
        assert keep[s].all()
    print(f"N={N} S={S} {layout}: {int(keep.sum())} residues compared, {int((~keep).sum())} excluded; classes "
          + " ".join(f"{DS.ALPHABET[k]}={int((c == k).sum())}" for k in range(8)))
    assert np.array_equal(c[keep], ref["classes"][keep]), [(DR.strings(c)[s], DR.strings(ref["classes"])[s]) for s in range(S)]
    assert np.array_equal(b[keep], ref["bridge"][keep]) and np.array_equal(f[keep], ref["flags"][keep])
    assert (c[:, :na] == 0).all() and (b >= -1).all() and (b < N).all() and (f >= 0).all() and (f < 512).all()
    if layout == "helix_edge" and N > 256:
        assert all(DR.strings(c)[s][250:262] == "H" * 12 for s in I["exact"])
    if layout == "sheet_edge":
        assert all((c[s, 240:248] == 3).sum() >= 2 and (b[s, 240:248, 0] >= 256).sum() >= 2 for s in I["exact"])
    # the mirror image is assigned alike; a second run gives equal bits; the public function gives the same
    pub = DS.assign(dev(DR.mirror(I["atoms"])), built, link, donor)
    assert np.array_equal(pub.classes.cpu().numpy(), c) and np.array_equal(pub.bridge.cpu().numpy(), b) and np.array_equal(pub.flags.cpu().numpy(), f)
    assert np.array_equal(bits(pub.energy.cpu().numpy()), bits(energy.cpu().numpy()))
    code2, c2, f2, b2, _ = raw_assign(partner, energy, atoms, built, link)
    assert code2 == 0 and torch.equal(c2, classes) and torch.equal(f2, flags) and torch.equal(b2, bridge)
    pub = DS.assign(atoms, built, link, donor)
    assert pub.classes.dtype == torch.uint8 and torch.equal(pub.classes, classes) and torch.equal(pub.flags, flags) and torch.equal(pub.bridge, bridge)
    # the census is plain arithmetic on the classes
    mask = dev((np.arange(N) >= na).astype(np.float32))
    got = DS.census(pub, mask)
    assert np.array_equal(got["counts"].cpu().numpy(), np.stack([(c[:, na:] == k).sum(1) for k in range(8)], 1))
    assert np.allclose(got["helix_fraction"].cpu().numpy(), np.isin(c[:, na:], [1, 4, 5]).mean(1))
    assert np.allclose(got["strand_fraction"].cpu().numpy(), np.isin(c[:, na:], [2, 3]).mean(1))
    e = pub.energy.cpu().numpy()
    assert np.array_equal(got["hbonds"].cpu().numpy(), (e[:, na:, :2] < np.float32(-0.5)).sum((1, 2)))


def test_a_spec_moves_the_cutoff_and_the_bend():
    I = DR.case_inputs(DR.AS_CASES[1])                          # N = 256, S = 3
    atoms, built, link = dev(I["atoms"]), dev(I["built"]), dev(I["link"])
    for spec in (DS.Dssp(cutoff=-1.0), DS.Dssp(bend=40.0), DS.Dssp(coupling=20.0, floor=-5.0)):
        ref = DR.assign(I["atoms"], I["built"], I["link"], None, spec)
        got = DS.assign(atoms, built, link, None, spec)
        check_lists(got.partner.cpu().numpy(), got.energy.cpu().numpy(), ref, repr(spec))
        keep = ~ref["excluded"]
        assert keep.mean() > 0.7 and np.array_equal(got.classes.cpu().numpy()[keep], ref["classes"][keep])
        assert np.array_equal(got.flags.cpu().numpy()[keep], ref["flags"][keep])
    loose, tight = DS.assign(atoms, built, link).classes, DS.assign(atoms, built, link, None, DS.Dssp(cutoff=-2.5)).classes
    assert int((loose == 1).sum()) > int((tight == 1).sum())
    assert int((DS.assign(atoms, built, link, None, DS.Dssp(bend=40.0)).flags & DS.FLAG_BEND).ne(0).sum()) > int((DS.assign(atoms, built, link).flags & DS.FLAG_BEND).ne(0).sum())


def test_built_backbones_of_ideal_traces_are_h_and_g_end_to_end():
    """backbone.build -> dssp.assign on the device: H on residues 1 .. 22 of an ideal alpha C-alpha trace of 24, G on the interior of
    the 3-10 trace; the float64 side rests on tests/backbone_ref.py for the built atoms"""
    ones = torch.ones(24, device=DEV)
    for conf, letter in ((DR.ALPHA, "H"), (DR.THREE10, "G")):
        ca = DR.regular(conf, 24)[:, BR.CA_]
        x = dev(np.stack([ca, ca + [30.0, -20.0, 10.0]]).astype(np.float32))
        built = BB.build(x, ones, ones)
        got = DS.assign(built.atoms, built.built, ones)
        assert DS.strings(got.classes) == ["-" + letter * 22 + "-"] * 2
        # the reflection of the BUILT atoms is assigned alike, with bit-equal energies
        flipped = DS.assign(built.atoms * torch.tensor([-1.0, 1.0, 1.0], device=DEV), built.built, ones)
        assert torch.equal(flipped.classes, got.classes) and torch.equal(flipped.energy, got.energy) and torch.equal(flipped.partner, got.partner)
        r = BR.build(x.cpu().numpy(), np.ones(24), np.ones(24))
        ref = DR.assign(r["atoms"].astype(np.float32), r["built"], np.ones(24, np.float32))
        assert DR.strings(ref["classes"]) == ["-" + letter * 22 + "-"] * 2 and not ref["ambiguous"].any()
        keep = ~ref["loose"]
        assert np.array_equal(got.partner.cpu().numpy()[keep], ref["partner"][keep])
        # the device's atoms differ from the yardstick's by up to the builder's own 4 E (tests/test_backbone.py), which the energy
        # magnifies: four terms of slope q / r^2 <= 27.9 / 1.9^2 = 7.7 kcal/mol per Angstrom, each between two such atoms
        assert np.abs(got.energy.cpu().numpy() - ref["energy"])[keep].max() < 4 * 7.7 * 2 * 4 * max(BR.E) + ALLOWED


def test_refusals_leave_the_outputs_untouched():
    D = DS._DEFINES
    I = DR.case_inputs(DR.HB_CASES[2])                          # N = 5, S = 3
    atoms, built, link = dev(I["atoms"]), dev(I["built"]), dev(I["link"])
    nan, inf = float("nan"), float("inf")
    for kw, want in ((dict(null=("partner",)), "ERR_ARG"), (dict(null=("energy",)), "ERR_ARG"), (dict(null=("atoms",)), "ERR_ARG"), (dict(null=("built",)), "ERR_ARG"),
                     (dict(null=("link",)), "ERR_ARG"), (dict(S=0), "ERR_ARG"), (dict(N=-1), "ERR_ARG"), (dict(q=0.0), "ERR_ARG"), (dict(q=nan), "ERR_ARG"),
                     (dict(e_min=0.0), "ERR_ARG"), (dict(e_min=-inf), "ERR_ARG"), (dict(N=DS.MAX_N + 1), "ERR_UNSUPPORTED"), (dict(S=DS.MAX_S + 1), "ERR_UNSUPPORTED")):
        code, partner, energy, bands = raw_hbonds(atoms, built, link, **kw)
        assert code == D[want] and bands, kw
        assert bool((partner == INT_SENTINEL).all()) and bool((energy == FLOAT_SENTINEL).all()), kw
    hb = DS.hbonds(atoms, built, link)
    for kw, want in ((dict(null=("classes",)), "ERR_ARG"), (dict(null=("flags",)), "ERR_ARG"), (dict(null=("bridge",)), "ERR_ARG"), (dict(null=("partner",)), "ERR_ARG"),
                     (dict(null=("energy",)), "ERR_ARG"), (dict(null=("atoms",)), "ERR_ARG"), (dict(null=("built",)), "ERR_ARG"), (dict(null=("link",)), "ERR_ARG"),
                     (dict(S=0), "ERR_ARG"), (dict(N=0), "ERR_ARG"), (dict(cutoff=0.0), "ERR_ARG"), (dict(cutoff=nan), "ERR_ARG"), (dict(cos_bend=1.0), "ERR_ARG"),
                     (dict(cos_bend=-1.0), "ERR_ARG"), (dict(cos_bend=inf), "ERR_ARG"), (dict(N=DS.MAX_N + 1), "ERR_UNSUPPORTED"),
                     (dict(S=DS.MAX_S + 1), "ERR_UNSUPPORTED")):
        code, classes, flags, bridge, bands = raw_assign(hb.partner, hb.energy, atoms, built, link, **kw)
        assert code == D[want] and bands, kw
        assert bool((classes == BYTE_SENTINEL).all()) and bool((flags == INT_SENTINEL).all()) and bool((bridge == INT_SENTINEL).all()), kw
    with pytest.raises(ValueError, match="PRD_DSSP_MAX_N"):
        DS.hbonds(torch.zeros(1, DS.MAX_N + 1, 5, 3, device=DEV), torch.zeros(1, DS.MAX_N + 1, dtype=torch.int32, device=DEV), torch.ones(DS.MAX_N + 1, device=DEV))
    with pytest.raises(RuntimeError, match="GPU only"):
        DS.assign(atoms.cpu(), built, link)
    with pytest.raises(ValueError, match="is on"):
        DS.assign(atoms, built, link.cpu())
    with pytest.raises(ValueError, match="built must be"):
        DS.assign(atoms, built.float(), link)


def test_the_calls_are_capturable_and_never_synchronise():
    I = DR.case_inputs(DR.AS_CASES[3])                          # N = 266, S = 3
    a0, built, link = dev(I["atoms"]), dev(I["built"]), dev(I["link"])
    eager = DS.assign(a0, built, link)                          # also the warm-up: library, allocator
    torch.cuda.synchronize()
    for spec in (None, "assign", DS.Dssp()):
        got = run_without_host_sync(lambda spec=spec: DS.assign(a0, built, link, None, spec))
        assert torch.equal(got.classes, eager.classes) and torch.equal(got.energy, eager.energy) and torch.equal(got.bridge, eager.bridge)
    hb = run_without_host_sync(lambda: DS.hbonds(a0, built, link))
    assert torch.equal(hb.partner, eager.partner)
    mask = torch.ones(a0.shape[1], device=DEV)
    counted = run_without_host_sync(lambda: DS.census(eager, mask))
    assert int(counted["counts"].sum()) == a0.shape[0] * a0.shape[1]
    # the two calls captured into a graph and replayed on other data in the same buffers
    static = a0.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = DS.assign(static, built, link)
    static.copy_(a0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g.classes, eager.classes) and torch.equal(g.partner, eager.partner) and torch.equal(g.energy, eager.energy)
    assert torch.equal(g.flags, eager.flags) and torch.equal(g.bridge, eager.bridge)
    static[:, :, 4] += 1.5                                      # every oxygen moved: other bonds
    graph.replay()
    torch.cuda.synchronize()
    moved = DS.assign(static, built, link)
    assert torch.equal(g.classes, moved.classes) and torch.equal(g.energy, moved.energy) and not torch.equal(g.energy, eager.energy)


# ---- generate_samples(secondary=...) --------------------------------------------------------------------------------------------------------

def test_generate_samples_assigns_the_real_models_samples(tmp_path):
    """the real model at the tiny shape of the other GPU pipeline tests: the stage runs on the device tensors of the backbone stage"""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    args = make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=4, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    na, nr = 5, 12
    data = synthetic_sample(na, nr, esm_dim=64, seed=0)
    kw = dict(num_samples=2, batch_size=2, seed=4, handedness="fix", align_to="first")
    loose = BB.Backbone(bond=(0.01, 1000.0), min_angle=0.0)     # an untrained model's C-alphas are not 3.8 Angstrom apart
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        before = PL.generate_samples(model, data, backbone=loose, **kw)
        out = PL.generate_samples(model, data, output_dir=tmp_path / "out", backbone=loose, secondary="assign", **kw)
    assert len(before) == 7 and len(out) == 8
    assert np.array_equal(bits(out[0]), bits(before[0])) and np.array_equal(bits(out[1]), bits(before[1]))
    for k in (4, 5, 6):                                         # every earlier element is what it was without the keyword
        assert all(np.array_equal(out[k][key], before[k][key], equal_nan=True) for key in before[k])
    d = out[7]
    assert d["classes"].shape == (2, nr) and d["classes"].dtype == np.uint8 and d["partner"].shape == d["energy"].shape == (2, nr, 4)
    assert d["bridge"].shape == (2, nr, 2) and d["counts"].shape == (2, 8) and (d["counts"].sum(1) == nr).all() and len(d["strings"]) == 2
    one = PL.collate_fn([data])
    mask, link = (t[: na + nr].contiguous().to(DEV) for t in CH.trace_links(one, 0, na, nr))
    again = BB.build(dev(out[0]), mask, link, loose)            # the stage saw the atoms of the RETURNED positions
    assert np.array_equal(bits(out[6]["atoms"]), bits(again.atoms[:, na:].cpu().numpy()))
    want = DS.assign(again.atoms, again.built, link)
    assert np.array_equal(d["classes"], want.classes[:, na:].cpu().numpy()) and np.array_equal(bits(d["energy"]), bits(want.energy[:, na:].cpu().numpy()))
    p = want.partner[:, na:].cpu().numpy()
    assert np.array_equal(d["partner"], np.where(p >= 0, p - na, -1)) and d["partner"].max() < nr and d["strings"] == DS.strings(d["classes"])
    assert sorted(set(("sample_secondary.npz", "sample_secondary.txt")) & set(p.name for p in (tmp_path / "out").iterdir())) == ["sample_secondary.npz", "sample_secondary.txt"]
    with np.load(tmp_path / "out" / "sample_secondary.npz") as z:
        assert sorted(z.files) == sorted(d) and all(np.array_equal(z[key], d[key]) for key in z.files)
    lines = (tmp_path / "out" / "sample_secondary.txt").read_text().splitlines()
    assert lines[0].startswith("#") and lines[1:] == d["strings"]
