"""GPU: libprd_backbone.so, called directly and through protein_redesign_amd.backbone, against the float64 yardstick tests/backbone_ref.py.

Two families of input (backbone_ref.case_inputs): EXACT -- every run an ideal chain whose (phi, psi) wander through the anchors, so every
virtual bond is L0 and every C-alpha vertex lies between 20 and 160 degrees, far from every validity edge -- and PERTURBED -- the same
with Gaussian noise of sigma = 0.3 Angstrom on every coordinate, which pushes about a tenth of the virtual bonds out of the window.
Coordinates stay within 100 Angstrom.  ``built`` must equal the yardstick's exactly on every residue outside the ambiguity band (there
is none in the exact family; at most 0.5 % of the residues may be in the perturbed one, and that cap is asserted).

TOLERANCE.  E is the largest deviation of a float32 numpy restatement of the same formulas from the float64 one on these very inputs,
measured on the CPU: 1.19e-5 Angstrom in the exact family and 1.23e-5 in the perturbed one, stated as E = 1.5e-5 for both
(backbone_ref.E; tests/test_backbone_cpu.py holds the measurement to [E / 2, E]).  The device's atan2f / sinf / cosf and its order of
operations differ from numpy's by a few ulps, not by a factor, so the device is allowed 4 E = 6.0e-5 Angstrom of maximum absolute
deviation from float64 on every built atom.

Shapes: the kernel's row tile T is 256 with a halo of 3 rows on either side; N runs over 1, 3, 4 (the first run that is built), 5, 7, 8
(two runs of 4), T - 1, T, T + 1, T + 3 and 1100 (five tiles), S over 1, 5 and 7, with 0, 3 and 17 ligand rows in front so that runs start
mid-tile, a link broken exactly at T-1 | T and at T | T+1, runs of 1, 2 and 3 between longer ones, and a strided view of x."""
import warnings

import numpy as np
import pytest
import torch

import backbone_ref as BR
from no_host_sync import run_without_host_sync
from protein_redesign_amd import backbone as BB
from protein_redesign_amd import chirality as CH
from protein_redesign_amd import pipeline as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 96                # sentinel elements on either side of every output
INT_SENTINEL, FLOAT_SENTINEL = -7777, -1234.5
ALLOWED = tuple(4.0 * e for e in BR.E)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype, sentinel):
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[PAD: PAD + n].view(shape)


def intact(buf, sentinel):
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def table(spec=None):
    return BB.upload("build" if spec is None else spec, DEV)


def raw_build(x, mask, link, spec=None, S=None, N=None, xr=None, null=(), **scalars):
    """prd_backbone_build itself on sentinel-filled, guarded outputs -> (code, atoms, built, guard bands intact); ``null``: the pointers
    handed over as NULL; ``scalars``: the scalar arguments that differ from the spec's"""
    S0, N0 = x.shape[:2]
    up = table(spec)
    names = ("l0", "ac", "rc", "ao", "ro", "an", "rn", "ka", "kb", "kc", "lo2", "hi2", "sin2")
    g = [scalars.pop(n, v) for n, v in zip(names, up.spec.scalars())]
    assert not scalars and set(null) <= {"atoms", "built", "x", "mask", "link", "table"}
    abuf, atoms = guarded((S0, N0, 5, 3), torch.float32, FLOAT_SENTINEL)
    bbuf, built = guarded((S0, N0), torch.int32, INT_SENTINEL)
    ptr = lambda name, t: None if name in null else t.data_ptr()         # noqa: E731
    code = BB.lib().prd_backbone_build(ptr("atoms", atoms), ptr("built", built), ptr("x", x), x.stride(0), x.stride(1) if xr is None else xr,
                                       ptr("mask", mask), ptr("link", link), ptr("table", up.table), *g, S0 if S is None else S,
                                       N0 if N is None else N, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, atoms, built, intact(abuf, FLOAT_SENTINEL) and intact(bbuf, INT_SENTINEL)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("case", BR.CASES, ids=BR.IDS)
def test_build_against_float64(case):
    N, S, na, layout, strided = case
    I = BR.case_inputs(case)
    ref = I["ref"]
    x, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    code, atoms, built, bands = raw_build(x, mask, link)
    assert code == 0 and bands                                  # nothing outside the outputs was written
    a, b = atoms.cpu().numpy(), built.cpu().numpy()
    assert (b != INT_SENTINEL).all() and (a != FLOAT_SENTINEL).all()          # every element was written
    amb = ref["ambiguous"]
    # built: the yardstick's integers outside the band; the band is empty in the exact family and narrow in the perturbed one
    for s in range(S):
        if s in I["exact"]:
            assert not amb[s].any(), (s, "the case's seed must keep the exact family unambiguous")
        else:
            assert amb[s].sum() <= BR.CAP * (N - na), s
    assert np.array_equal(b[~amb], ref["built"][~amb])
    assert ((b >= 0) & (b < 32)).all() and (((b >> 3) & 1) == ((b & 1) & ((b >> 2) & 1))).all() and (((b >> 4) & 1) == ((b >> 2) & 1)).all()
    # atoms: the maximum absolute deviation from float64 over the built atoms, per family
    on = BR.flags(b)
    keep = on & BR.flags(ref["built"]) & ~amb[..., None]
    dev_e = [max([BR.deviation(a[s], ref["atoms"][s], keep[s]) for s in range(S) if (s in I["exact"]) == (k == 0)], default=0.0) for k in (0, 1)]
    print(f"N={N} S={S} na={na} {layout}: residues built whole {(b == 31).sum(1).tolist()}, ambiguous {amb.sum(1).tolist()}, max deviation "
          f"exact {dev_e[0]:.3e} perturbed {dev_e[1]:.3e} Angstrom (allowed {ALLOWED[0]:.1e} / {ALLOWED[1]:.1e})")
    assert dev_e[0] <= ALLOWED[0] and dev_e[1] <= ALLOWED[1]
    # rows without mask and unbuilt atoms are exactly zero; CA is the input's bits
    assert not a[~on].any() and not a[:, I["mask"] < 0.5].any() and not b[:, I["mask"] < 0.5].any()
    assert np.array_equal(bits(a[:, I["mask"] > 0.5, BR.CA_]), bits(I["x"][:, I["mask"] > 0.5]))
    # L-residues on every built residue of the sample and of its reflection
    whole = on[..., BR.CB_]
    assert (BR.cb_volume(a.astype(np.float64))[whole] > 0).all()
    codem, am, bm, _ = raw_build(dev(BR.mirror(I["x"])), mask, link)
    am, bm = am.cpu().numpy(), bm.cpu().numpy()
    assert codem == 0 and (BR.cb_volume(am.astype(np.float64))[BR.flags(bm)[..., BR.CB_]] > 0).all()
    assert np.array_equal(bm[~amb], b[~amb])                    # validity is made of lengths and angles: the mirror image's is the same
    # determinism: a second launch gives equal bits
    code2, a2, b2, _ = raw_build(x, mask, link)
    assert code2 == 0 and np.array_equal(bits(a2.cpu().numpy()), bits(a)) and np.array_equal(b2.cpu().numpy(), b)
    # the public function: the same bits; a strided x is taken as it is
    pub = BB.build(x, mask, link)
    assert pub.atoms.shape == (S, N, 5, 3) and pub.built.shape == (S, N) and pub.built.dtype == torch.int32
    assert np.array_equal(bits(pub.atoms.cpu().numpy()), bits(a)) and np.array_equal(pub.built.cpu().numpy(), b)
    assert np.array_equal(pub.flags.cpu().numpy(), on)
    if strided:
        x4 = torch.randn(S + 1, N + 2, 4, device=DEV)[:S, :N]   # row stride 4, a padded structure stride
        x4[:, :, :3] = x
        view = x4[:, :, :3]
        assert view.stride(1) == 4 and view.stride(0) == 4 * (N + 2)
        got = BB.build(view, mask, link, table())
        assert np.array_equal(bits(got.atoms.cpu().numpy()), bits(a)) and np.array_equal(got.built.cpu().numpy(), b)
        codes, as_, bs, bands = raw_build(view, mask, link)
        assert codes == 0 and bands and np.array_equal(bits(as_.cpu().numpy()), bits(a))


def test_a_spec_moves_the_thresholds_and_the_table():
    I = BR.case_inputs(BR.CASES[7])                             # N = 256, S = 5
    x, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    for spec in (BB.Backbone(bond=(3.0, 4.6)), BB.Backbone(min_angle=25.0), BB.Backbone(orientation=BB.Orientation.constant(40.0)),
                 BB.Backbone(geometry=BB.Geometry(c_n=1.34, cb=(-0.5, 0.5, -0.5)))):
        ref = BR.build(I["x"], I["mask"], I["link"], spec)
        got = BB.build(x, mask, link, spec)
        a, b = got.atoms.cpu().numpy(), got.built.cpu().numpy()
        amb = ref["ambiguous"]
        assert amb.sum() <= BR.CAP * amb.size and np.array_equal(b[~amb], ref["built"][~amb])
        keep = BR.flags(b) & BR.flags(ref["built"]) & ~amb[..., None]
        assert BR.deviation(a, ref["atoms"], keep) <= max(ALLOWED) and keep.sum() > 1000
    wide = BB.build(x, mask, link, BB.Backbone(bond=(3.0, 4.6))).built
    assert int((wide == 31).sum()) > int((BB.build(x, mask, link).built == 31).sum())


def test_refusals_leave_the_outputs_untouched():
    D = BB._DEFINES
    I = BR.case_inputs(BR.CASES[5])                             # N = 8, S = 5
    x, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    nan, inf = float("nan"), float("inf")
    for kw, want in ((dict(null=("atoms",)), "ERR_ARG"), (dict(null=("built",)), "ERR_ARG"), (dict(null=("x",)), "ERR_ARG"), (dict(null=("mask",)), "ERR_ARG"),
                     (dict(null=("link",)), "ERR_ARG"), (dict(null=("table",)), "ERR_ARG"), (dict(S=0), "ERR_ARG"), (dict(S=-2), "ERR_ARG"), (dict(N=0), "ERR_ARG"),
                     (dict(N=-1), "ERR_ARG"), (dict(xr=2), "ERR_ARG"), (dict(lo2=18.49, hi2=10.89), "ERR_ARG"), (dict(lo2=0.0), "ERR_ARG"),
                     (dict(hi2=nan), "ERR_ARG"), (dict(sin2=1.0), "ERR_ARG"), (dict(sin2=-0.5), "ERR_ARG"), (dict(l0=0.0), "ERR_ARG"), (dict(ka=0.5), "ERR_ARG"),
                     (dict(rc=inf), "ERR_ARG"), (dict(N=BB.MAX_N + 1), "ERR_UNSUPPORTED"), (dict(S=BB.MAX_S + 1), "ERR_UNSUPPORTED")):
        code, atoms, built, bands = raw_build(x, mask, link, **kw)
        assert code == D[want] and bands, kw
        assert bool((atoms == FLOAT_SENTINEL).all()) and bool((built == INT_SENTINEL).all()), kw
    with pytest.raises(ValueError, match="PRD_BACKBONE_MAX_N"):
        BB.build(torch.zeros(1, BB.MAX_N + 1, 3, device=DEV), torch.ones(BB.MAX_N + 1, device=DEV), torch.ones(BB.MAX_N + 1, device=DEV))
    with pytest.raises(RuntimeError, match="GPU only"):
        BB.build(x.cpu(), mask, link)
    with pytest.raises(ValueError, match="is on"):
        BB.build(x, mask.cpu(), link)
    with pytest.raises(ValueError, match="the table is on"):
        BB.build(x, mask, link, BB.upload("build", "cpu"))


def test_build_is_capturable_and_never_synchronises():
    I = BR.case_inputs(BR.CASES[9])                             # N = 259, S = 7
    x0, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    up = BB.upload("build", DEV)                                # the one copy that waits for the host, outside the region
    assert up is BB.upload(BB.Backbone(), x0.device)
    eager = BB.build(x0, mask, link, up)                        # also the warm-up: library, allocator
    torch.cuda.synchronize()
    for spec in (up, "build", None, BB.Backbone()):             # an uploaded spec is found again, nothing is copied
        got = run_without_host_sync(lambda spec=spec: BB.build(x0, mask, link, spec))
        assert torch.equal(got.atoms, eager.atoms) and torch.equal(got.built, eager.built)
    # captured into a graph and replayed on other data in the same buffers
    static = x0.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = BB.build(static, mask, link, up)
    static.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g.atoms, eager.atoms) and torch.equal(g.built, eager.built)
    static.copy_(dev(BR.mirror(I["x"])))
    graph.replay()
    torch.cuda.synchronize()
    rows = mask > 0.5
    assert torch.equal(g.atoms[:, rows, 1], static[:, rows]) and not torch.equal(g.atoms, eager.atoms)


# ---- generate_samples(backbone=...) ---------------------------------------------------------------------------------------------------------

def _records(pdb_text):
    models = []
    for line in pdb_text.splitlines():
        if line.startswith("MODEL"):
            models.append({})
        elif line.startswith("ATOM"):
            models[-1].setdefault((int(line[22:26]), line[17:20]), []).append(line[12:16].strip())
    return models


def test_generate_samples_builds_the_backbone_of_the_real_models_samples(tmp_path):
    """the real model at the tiny shape of the other GPU pipeline tests: the stage runs last, on the positions that are returned"""
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
    # an untrained model's C-alphas are not 3.8 Angstrom apart: beside the default, a window that takes whatever it draws
    loose = BB.Backbone(bond=(0.01, 1000.0), min_angle=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        before = PL.generate_samples(model, data, **kw)
        out = PL.generate_samples(model, data, output_dir=tmp_path / "build", backbone="build", **kw)
        wide = PL.generate_samples(model, data, output_dir=tmp_path / "wide", backbone=loose, **kw)
    assert len(before) == 6 and len(out) == len(wide) == 7
    for got in (out, wide):                                     # every earlier element is what it was without the keyword
        assert np.array_equal(bits(got[0]), bits(before[0])) and np.array_equal(bits(got[1]), bits(before[1]))
        assert all(np.array_equal(got[4][k], before[4][k], equal_nan=True) for k in before[4])
        assert all(np.array_equal(got[5][k], before[5][k], equal_nan=True) for k in before[5])
    one = PL.collate_fn([data])
    mask, link = (t[: na + nr].contiguous().to(DEV) for t in CH.trace_links(one, 0, na, nr))
    for got, spec, name in ((out, BB.Backbone(), "build"), (wide, loose, "wide")):
        d = got[6]
        again = BB.build(dev(got[0]), mask, link, spec)        # the builder applied to the RETURNED positions: final frame, final hand
        assert np.array_equal(bits(d["atoms"]), bits(again.atoms[:, na:].cpu().numpy())) and np.array_equal(d["built"], again.flags[:, na:].cpu().numpy())
        assert d["atoms"].shape == (2, nr, 5, 3) and d["built"].shape == (2, nr, 5) and d["unbuilt_residues"].shape == (2,)
        assert np.array_equal(bits(d["atoms"][:, :, 1]), bits(got[0][:, na:]))
        assert np.array_equal(d["unbuilt_residues"], (~(d["built"][:, :, 0] & d["built"][:, :, 2] & d["built"][:, :, 4])).sum(1))
        models = _records((tmp_path / name / "sample_protein.pdb").read_text())
        assert len(models) == 2
        for k, model_records in enumerate(models):
            assert len(model_records) == nr
            for r, ((_, resn), names) in enumerate(model_records.items()):
                if d["built"][k, r].all():                      # a built residue: 4 or 5 records in the order N, CA, C, CB, O
                    assert names == (["N", "CA", "C", "O"] if resn in ("GLY", "UNK") else ["N", "CA", "C", "CB", "O"])
                assert "CB" not in names or d["built"][k, r, 3]
        with np.load(tmp_path / name / "sample_backbone.npz") as z:
            assert sorted(z.files) == sorted(d) and all(np.array_equal(z[key], d[key]) for key in z.files)
    print("unbuilt residues: default window", out[6]["unbuilt_residues"].tolist(), "loose window", wide[6]["unbuilt_residues"].tolist())
    assert wide[6]["built"].all() and (wide[6]["unbuilt_residues"] == 0).all()     # with the loose window every residue of the chain is built
