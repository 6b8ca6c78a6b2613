"""GPU: libprd_chirality.so through protein_redesign_amd.chirality against the float64 yardstick tests/chirality_ref.py.

Three families of input (chirality_ref.case_inputs): (a) chains built by NeRF from chosen (bond, theta, tau) sequences that keep every
value at least 5 degrees / 0.1 Angstrom from every window edge -- counts, classes, verdict and basis must equal float64's exactly; (b)
Gaussian-perturbed copies (sigma 0.3 and 1 Angstrom), whose comparisons may sit on an edge -- the device count must lie between the
yardstick's count with every ambiguous comparison false and with every one true, and so that this band hides nothing the ambiguous quads
are at most 0.5 % of the valid ones wherever there are 200 or more (the bands and their derivation: the head of chirality_ref.py); (c)
the exact mirror image of every case -- the hands of counts swapped as integers, tau negated bit for bit, the verdict negated.

Shapes: the census kernel's row tile is 256 with a halo of 3 rows and its centres go 256 to a pass; N runs over 1, 3, 4 (the first quad), 5,
the tile +-1 and +3, and 1100 (five tiles), S over 1, 5 and 7, C over 0, 1, 64 and 65."""
import functools
import warnings

import numpy as np
import pytest
import torch

import chirality_ref as CR
from no_host_sync import run_without_host_sync
from protein_redesign_amd import chirality as CH
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd import quality

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 96                # sentinel elements on either side of every output
INT_SENTINEL, FLOAT_SENTINEL = -7777, -1234.5
CAP = 0.005


@functools.lru_cache(maxsize=None)
def inputs(case):
    """computed once and shared by the tests (read only)"""
    return CR.case_inputs(case)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(shape, dtype, sentinel):
    n = int(np.prod(shape))
    buf = torch.full((PAD + n + PAD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[PAD: PAD + n].view(shape)


def intact(buf, sentinel):
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def raw_census(x, mask, link, centres=None, centre_ref=None, S=None, N=None, optional=True, min_helix=4, min_extended=12, vmin=0.5,
               edges=None, bond=(3.3, 4.3)):
    """prd_chirality_census itself on sentinel-filled, guarded outputs -> (code, dict of outputs, bands intact)"""
    S0, N0 = x.shape[:2]
    C = 0 if centres is None else centres.shape[0]
    shapes = dict(counts=((S0, 8), torch.int32), verdict=((S0,), torch.int32), basis=((S0,), torch.int32), tau=((S0, N0), torch.float32),
                  cls=((S0, N0), torch.int32), volume=((S0, max(C, 1)), torch.float32))
    bufs, out = {}, {}
    for name, (shape, dtype) in shapes.items():
        bufs[name], out[name] = guarded(shape, dtype, INT_SENTINEL if dtype == torch.int32 else FLOAT_SENTINEL)
    cd = None if centres is None else dev(centres)
    opt = lambda name: out[name].data_ptr() if optional else None       # noqa: E731
    code = CH.lib().prd_chirality_census(out["counts"].data_ptr(), out["verdict"].data_ptr(), out["basis"].data_ptr(), opt("tau"), opt("cls"),
                                         opt("volume"), x.data_ptr(), x.stride(0), x.stride(1), mask.data_ptr(), link.data_ptr(),
                                         None if cd is None else cd.data_ptr(), None if centres is None else centres.ctypes.data,
                                         None if centre_ref is None else centre_ref.data_ptr(), C, *(CR.edges_f32() if edges is None else edges),
                                         bond[0], bond[1], vmin, min_helix, min_extended, S0 if S is None else S, N0 if N is None else N,
                                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ok = all(intact(bufs[n], INT_SENTINEL if shapes[n][1] == torch.int32 else FLOAT_SENTINEL) for n in shapes)
    if C == 0 or not optional:
        assert bool((out["volume"] == FLOAT_SENTINEL).all())
    if C:
        out["volume"] = out["volume"][:, :C] if optional else out["volume"]
    return code, out, ok


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("case", CR.CASES, ids=CR.IDS)
def test_census_against_float64_and_under_reflection(case):
    N, S, _, mkind, strided, C, with_ref = case
    I = inputs(case)
    ref = I["ref"]
    x, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    centres = np.ascontiguousarray(I["centres"]) if C else None
    cref = dev(I["centre_ref"]) if I["centre_ref"] is not None else None
    code, out, bands = raw_census(x, mask, link, centres, cref)
    assert code == 0 and bands                                  # nothing outside the outputs was written
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for name in ("counts", "verdict", "basis", "cls"):
        assert (got[name] != INT_SENTINEL).all(), name          # every element was written
    assert (got["tau"] != FLOAT_SENTINEL).all() and (C == 0 or (got["volume"] != FLOAT_SENTINEL).all())
    quads = ref["counts"][:, 4]
    print(f"N={N} S={S} {mkind} C={C}: kinds {I['kinds']}, quads {quads.tolist()}, ambiguous {ref['ambiguous'].tolist()} (centres "
          f"{ref['ambiguous_centres'].tolist()}), device counts {got['counts'].tolist()}, float64 {ref['counts'].tolist()}, verdict "
          f"{got['verdict'].tolist()} basis {got['basis'].tolist()}")
    # (a) exact where nothing sits on an edge; (b) bracketed elsewhere, and the band is narrow
    for s in range(S):
        if s in I["exact"] or quads[s] < 200:
            assert ref["ambiguous"][s] == 0 and ref["ambiguous_centres"][s] == 0, (s, "the case's seed must keep small cases unambiguous")
        else:
            assert ref["ambiguous"][s] <= CAP * ref["counts_hi"][s, 4], s
        if ref["ambiguous"][s] == 0 and ref["ambiguous_centres"][s] == 0:
            assert np.array_equal(got["counts"][s], ref["counts"][s]), s
            assert np.array_equal(got["cls"][s], ref["classes"][s]) and np.array_equal(np.isnan(got["tau"][s]), ~ref["valid"][s]), s
            assert got["verdict"][s] == ref["verdict"][s] and got["basis"][s] == ref["basis"][s], s
    assert (ref["counts_lo"] <= got["counts"]).all() and (got["counts"] <= ref["counts_hi"]).all()
    # the verdict is the rule applied to the device's own counts, whatever they are
    for s in range(S):
        assert (got["verdict"][s], got["basis"][s]) == CR.verdict_rule(got["counts"][s], cref is not None), s
    both = ~np.isnan(got["tau"]) & ref["valid"]
    diff = np.abs(got["tau"][both] - ref["tau"][both])
    assert np.minimum(diff, 2 * np.pi - diff).max(initial=0.0) < CR.BAND_TAU
    assert ((got["cls"] == 0) | ~np.isnan(got["tau"])).all() and got["counts"][:, :4].sum(1).tolist() == (got["cls"] > 0).sum(1).tolist()
    if C:
        scale = 1e-5 * np.maximum(np.abs(ref["volume"]), 100.0)     # vectors of <= ~6 Angstrom within a segment; relative beyond
        assert (np.abs(got["volume"] - ref["volume"]) <= scale).all()
    # determinism: a second launch gives equal bits
    code2, out2, _ = raw_census(x, mask, link, centres, cref)
    assert code2 == 0 and all(np.array_equal(bits(out2[k].cpu().numpy()), bits(got[k])) for k in got)
    # NULL optional outputs: the rest is what it was
    code3, out3, bands3 = raw_census(x, mask, link, centres, cref, optional=False)
    assert code3 == 0 and bands3 and all(np.array_equal(out3[k].cpu().numpy(), got[k]) for k in ("counts", "verdict", "basis"))
    assert bool((out3["tau"] == FLOAT_SENTINEL).all()) and bool((out3["cls"] == INT_SENTINEL).all())
    # (c) the exact mirror image, about either of two axes
    for axis in (0, 2):
        codem, outm, _ = raw_census(dev(CR.mirror(I["x"], axis)), mask, link, centres, cref)
        m = {k: v.cpu().numpy() for k, v in outm.items()}
        assert codem == 0 and np.array_equal(m["counts"][:, CR.MIRROR_COLUMNS], got["counts"]) and np.array_equal(m["verdict"], -got["verdict"])
        assert np.array_equal(m["basis"], got["basis"])
        valid = ~np.isnan(got["tau"])
        assert np.array_equal(np.isnan(m["tau"]), ~valid) and np.array_equal(bits(m["tau"])[valid], bits(-got["tau"])[valid])
        assert np.array_equal(m["cls"], np.array([0, 2, 1, 4, 3])[got["cls"]])
        if C:
            assert np.array_equal(bits(m["volume"]), bits(-got["volume"]))
    # the public function: the same integers; a strided x is taken as it is
    listed = CH.upload(centres, DEV) if C else None
    pub = CH.census(x, mask, link, centres=listed, centre_ref=cref)
    assert np.array_equal(pub.counts.cpu().numpy(), got["counts"]) and np.array_equal(pub.verdict.cpu().numpy(), got["verdict"])
    assert np.array_equal(bits(pub.tau.cpu().numpy()), bits(got["tau"])) and np.array_equal(pub.classes.cpu().numpy(), got["cls"])
    assert pub.volume.shape == (S, C) and (C == 0 or np.array_equal(bits(pub.volume.cpu().numpy()), bits(got["volume"])))
    assert torch.equal(pub.helix_left, pub.counts[:, 1]) and pub.helix_fraction.dtype == torch.float64
    frac = pub.helix_fraction.cpu().numpy()
    with np.errstate(invalid="ignore"):
        assert np.array_equal(frac, (got["counts"][:, 0] + got["counts"][:, 1]) / got["counts"][:, 4].astype(np.float64), equal_nan=True)
    assert np.isnan(frac[got["counts"][:, 4] == 0]).all()
    if strided:
        x4 = torch.randn(S, N, 4, device=DEV)
        x4[:, :, :3] = x
        view = CH.census(x4[:, :, :3], mask, link, centres=listed, centre_ref=cref)
        assert x4[:, :, :3].stride(1) == 4 and torch.equal(view.counts, pub.counts) and torch.equal(view.classes, pub.classes)
        assert np.array_equal(bits(view.tau.cpu().numpy()), bits(got["tau"]))


def _chain(parts, rng):
    """rows, link: ideal segments of the given (kind, rows), unlinked from each other and 40 Angstrom apart"""
    xs, link = [], []
    for k, (kind, L) in enumerate(parts):
        s = CR.segment(rng, L, (kind,), ideal=True)
        xs.append(s - s.mean(0) + [40.0 * (k - len(parts) / 2), 0.0, 0.0])
        link += [1.0] * (L - 1) + [0.0]
    return np.concatenate(xs), np.array(link)


def test_the_verdict_rule_reaches_every_basis_and_every_tie():
    """hand-made counts: helical segments of n rows give n - 3 helical quads, extended ones n - 3 extended quads, and tetrahedra placed
    after the chain give kept / inverted / flat centres against a reference of the unreflected tetrahedron"""
    rng = np.random.default_rng(3)
    # (segments, tetrahedra: +1 kept, -1 inverted, 0 flat), want (verdict, basis)
    table = [([("helix_r", 7), ("helix_l", 3 + 0)], [], (1, 1)),                                   # h = +4
             ([("helix_l", 9), ("helix_r", 4)], [1], (-1, 1)),                                      # h = -5 beats a kept centre
             ([("helix_r", 6), ("helix_l", 3)], [1, 1], (1, 2)),                                    # |h| = min_helix - 1: rule 2, all kept
             ([("helix_r", 6)], [-1], (-1, 2)),                                                      # all inverted
             ([("helix_r", 5), ("helix_l", 5), ("ext_n", 15)], [1, -1], (1, 3)),                   # h = 0, mixed centres: rule 3, e = +12
             ([("ext_m", 16), ("ext_n", 4)], [0], (-1, 3)),                                         # a flat centre says nothing; e = -12
             ([("ext_n", 14)], [1, -1, 0], (0, 0)),                                                  # |e| = 11: undecided
             ([("helix_r", 5), ("helix_l", 5), ("ext_n", 9), ("ext_m", 9)], [], (0, 0))]            # every tie
    for parts, tets, want in table:
        chain, link = _chain(parts, rng)
        n = len(chain)
        lig = [CR.TETRA * ([1.0, 1.0, float(t)] if t else [1.0, 1.0, 0.0]) + [0.0, 30.0 + 10.0 * k, 0.0] for k, t in enumerate(tets)]
        x = np.concatenate([chain] + lig)[None].astype(np.float32)
        mask = np.r_[np.ones(n), np.zeros(4 * len(tets))].astype(np.float32)
        lk = np.r_[link, np.zeros(4 * len(tets))].astype(np.float32)
        centres = np.array([[n + 4 * k, n + 4 * k + 1, n + 4 * k + 2, n + 4 * k + 3] for k in range(len(tets))], np.int32).reshape(-1, 4)
        cref = np.full(len(tets), float(CR.signed_volume(CR.TETRA, [[0, 1, 2, 3]])[0]), np.float32)
        ref = CR.census(x, mask, lk, centres if len(tets) else None, cref if len(tets) else None)
        got = CH.census(dev(x), dev(mask), dev(lk), centres=centres if len(tets) else None, centre_ref=dev(cref) if len(tets) else None)
        counts = got.counts.cpu().numpy()[0]
        print(parts, tets, counts.tolist(), int(got.verdict), int(got.basis))
        assert np.array_equal(counts, ref["counts"][0]) and ref["ambiguous"][0] == 0
        assert counts[5:].tolist() == [tets.count(1), tets.count(-1), tets.count(0)]
        assert (int(got.verdict), int(got.basis)) == want == CR.verdict_rule(counts, bool(tets))
    # the minima are arguments: with min_helix = 3 the third row is decided by its helices, with min_extended = 11 the seventh by its strand
    chain, link = _chain(table[2][0], rng)
    got = CH.census(dev(chain[None].astype(np.float32)), torch.ones(len(chain), device=DEV), dev(link.astype(np.float32)), min_helix=3)
    assert (int(got.verdict), int(got.basis)) == (1, 1)
    chain, link = _chain(table[6][0], rng)
    got = CH.census(dev(chain[None].astype(np.float32)), torch.ones(len(chain), device=DEV), dev(link.astype(np.float32)), min_extended=11)
    assert (int(got.verdict), int(got.basis)) == (1, 3)


def test_reflect_is_exact_and_distances_keep_their_bits():
    case = CR.CASES[10]                                         # N = 300, S = 7
    I = inputs(case)
    N, S = case[0], case[1]
    x0 = dev(I["x"])
    mask, link = dev(I["mask"]), dev(I["link"])
    buf, x = guarded((S, N, 3), torch.float32, FLOAT_SENTINEL)
    x.copy_(x0)
    flip = torch.tensor([1, 0, 7, 0, -1, 0, 1], dtype=torch.int32, device=DEV)
    assert CH.reflect(x, flip) is x
    torch.cuda.synchronize()
    assert intact(buf, FLOAT_SENTINEL)
    on = flip.cpu().numpy() != 0
    a, b = x.cpu().numpy(), I["x"]
    assert np.array_equal(bits(a[~on]), bits(b[~on])) and np.array_equal(bits(a[on][..., 1:]), bits(b[on][..., 1:]))
    assert np.array_equal(bits(a[on][..., 0]), bits(-b[on][..., 0]))
    # distances: the censuses of prd_quality.h are integer-equal to the original's
    ones = torch.ones(N, device=DEV)
    for cutoff in (4.0, 8.0):
        assert torch.equal(quality.contacts(x, ones, ones, cutoff).count, quality.contacts(x0, ones, ones, cutoff).count)
        assert torch.equal(quality.contacts(x, ones, ones, cutoff).nearest, quality.contacts(x0, ones, ones, cutoff).nearest)
    la, lb = quality.lddt(x, x0[4], ones), quality.lddt(x0, x0[4], ones)
    assert torch.equal(la.preserved, lb.preserved) and torch.equal(la.total, lb.total) and int(lb.total.sum()) > 0
    # twice restores the bits; a bool flip and a strided x work in place; a tensor that would be copied is refused
    CH.reflect(x, flip != 0)
    assert np.array_equal(bits(x.cpu().numpy()), bits(I["x"]))
    x4 = torch.zeros(S, N, 4, device=DEV)
    x4[:, :, :3] = x0
    CH.reflect(x4[:, :, :3], flip)
    assert torch.equal(x4[:, :, 1:3], x0[:, :, 1:]) and torch.equal(x4[on.tolist(), :, 0], -x0[on.tolist(), :, 0]) and float(x4[:, :, 3].abs().max()) == 0.0
    with pytest.raises(ValueError, match="in place"):
        CH.reflect(x0.transpose(1, 2).contiguous().transpose(1, 2), flip)
    with pytest.raises(ValueError, match="flip must be"):
        CH.reflect(x, flip.float())
    # fix: no -1 verdict is left, the +1 and 0 ones are untouched, and the fixed samples' counts are the swapped ones
    before = CH.census(x, mask, link)
    assert int((before.verdict < 0).sum()) >= 2 and int((before.verdict > 0).sum()) >= 2
    assert CH.fix(x, before) is x
    after = CH.census(x, mask, link)
    was = (before.verdict < 0).cpu().numpy()
    assert int((after.verdict < 0).sum()) == 0 and torch.equal(after.verdict, before.verdict.abs())
    assert np.array_equal(after.counts.cpu().numpy()[was], before.counts.cpu().numpy()[was][:, CR.MIRROR_COLUMNS])
    assert np.array_equal(bits(x.cpu().numpy()[~was]), bits(I["x"][~was]))


def test_refusals_leave_the_outputs_untouched():
    D = CH._DEFINES
    I = inputs(CR.CASES[4])
    x, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    centres = np.array([[1, 0, 2, 3]], np.int32)
    e = CR.edges_f32()
    for kw, want in ((dict(N=CH.MAX_N + 1), "ERR_UNSUPPORTED"), (dict(S=CH.MAX_S + 1), "ERR_UNSUPPORTED"), (dict(S=0), "ERR_ARG"), (dict(vmin=0.0), "ERR_ARG"),
                     (dict(min_helix=-1), "ERR_ARG"), (dict(bond=(4.3, 3.3)), "ERR_ARG"), (dict(edges=e[:2] + [e[3], e[2]] + e[4:]), "ERR_ARG"),
                     (dict(edges=[float("nan")] + e[1:]), "ERR_ARG"), (dict(centres=np.array([[1, 0, 2, 64]], np.int32)), "ERR_ARG"),
                     (dict(centres=np.array([[-1, 0, 2, 3]], np.int32)), "ERR_ARG")):
        code, out, bands = raw_census(x, mask, link, **dict(dict(centres=centres), **kw))
        assert code == D[want] and bands, kw
        assert all(bool((out[k] == (FLOAT_SENTINEL if out[k].dtype == torch.float32 else INT_SENTINEL)).all()) for k in out), kw
    buf, y = guarded(tuple(x.shape), torch.float32, FLOAT_SENTINEL)
    flip = torch.ones(x.shape[0], dtype=torch.int32, device=DEV)
    for S, N, want in ((0, 64, "ERR_ARG"), (5, CH.MAX_N + 1, "ERR_UNSUPPORTED"), (CH.MAX_S + 1, 64, "ERR_UNSUPPORTED")):
        assert CH.lib().prd_chirality_reflect(y.data_ptr(), y.stride(0), 3, flip.data_ptr(), S, N, None) == D[want]
    assert CH.lib().prd_chirality_reflect(y.data_ptr(), y.stride(0), 2, flip.data_ptr(), 5, 64, None) == D["ERR_ARG"]
    torch.cuda.synchronize()
    assert bool((buf == FLOAT_SENTINEL).all())
    with pytest.raises(ValueError, match="PRD_CHIRALITY_MAX_N"):
        CH.census(torch.zeros(1, CH.MAX_N + 1, 3, device=DEV), torch.ones(CH.MAX_N + 1, device=DEV), torch.ones(CH.MAX_N + 1, device=DEV))
    with pytest.raises(RuntimeError, match="prd_chirality_census failed: PRD_CHIRALITY_ERR_ARG"):
        CH.census(x, mask, link, centres=np.array([[1, 0, 2, 64]]))         # the library's own check of the host copy
    with pytest.raises(RuntimeError, match="GPU only"):
        CH.census(x.cpu(), mask, link)
    with pytest.raises(ValueError, match="is on"):
        CH.census(x, mask.cpu(), link)


def test_census_and_reflect_are_capturable_and_never_synchronise():
    case = CR.CASES[10]
    I = inputs(case)
    x0, mask, link = dev(I["x"]), dev(I["mask"]), dev(I["link"])
    listed, cref = CH.upload(I["centres"], DEV), dev(I["centre_ref"])
    eager_x = x0.clone()
    eager = CH.census(eager_x, mask, link, centres=listed, centre_ref=cref)          # also the warm-up: library, allocator
    CH.fix(eager_x, eager)
    torch.cuda.synchronize()

    def work():
        y = x0.clone()
        got = CH.census(y, mask, link, centres=listed, centre_ref=cref)
        CH.fix(y, got)
        return y, got
    y, got = run_without_host_sync(work)
    assert torch.equal(y, eager_x) and torch.equal(got.counts, eager.counts) and torch.equal(got.verdict, eager.verdict)
    # captured into a graph and replayed on other data in the same buffers
    static = x0.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = CH.census(static, mask, link, centres=listed, centre_ref=cref)
        CH.fix(static, g)
    static.copy_(x0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager_x) and torch.equal(g.counts, eager.counts) and torch.equal(g.basis, eager.basis)
    assert np.array_equal(bits(g.tau.cpu().numpy()), bits(eager.tau.cpu().numpy()))
    static.copy_(dev(CR.mirror(I["x"])))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g.verdict, -eager.verdict) and torch.equal(g.counts, eager.counts[:, CR.MIRROR_COLUMNS])


# ---- generate_samples(handedness=...) -----------------------------------------------------------------------------------------------

NA, NR, TETRA, complex_and_samples = CR.NA, CR.NR, CR.TETRA, CR.complex_and_samples


def _Prepared(samples):
    return CR.Prepared(samples, DEV)


def test_generate_samples_reports_and_fixes(tmp_path):
    data, samples = complex_and_samples()
    kw = dict(num_samples=6, batch_size=4, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(_Prepared(samples), data, output_dir=tmp_path / "plain", **kw)
        report = PL.generate_samples(_Prepared(samples), data, output_dir=tmp_path / "report", handedness="report", **kw)
        fixed = PL.generate_samples(_Prepared(samples), data, output_dir=tmp_path / "fix", handedness="fix", align_to="input", assess="self", **kw)
        scored = PL.generate_samples(_Prepared(samples), data, align_to="input", assess="self", **kw)
        spec = PL.generate_samples(_Prepared(samples), data, handedness=CH.Handedness(fix=True, min_helix=50), **kw)
        unfixed = PL.generate_samples(_Prepared(samples), data, handedness="fix", **kw)
    assert len(plain) == 4 and len(report) == 5 and len(fixed) == 7 and len(scored) == 6
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    assert np.array_equal(bits(plain[0]), bits(samples)) and np.array_equal(bits(report[0]), bits(plain[0])) and np.array_equal(report[1], plain[1])
    d = report[4]
    assert sorted(d) == sorted(["verdict", "basis", "flipped", "helix_right", "helix_left", "extended_native", "extended_mirror", "quads",
                                "helix_fraction", "extended_fraction", "tau", "classes", "ligand_centres", "ligand_volume", "ligand_kept",
                                "ligand_inverted", "ligand_flat", "input_verdict", "input_basis", "input_counts"])
    print({k: v.tolist() for k, v in d.items() if v.ndim <= 1})
    assert d["verdict"].tolist()[:4] == [1, 1, -1, -1] and d["basis"].tolist()[:4] == [1, 1, 1, 1] and not d["flipped"].any()
    assert d["helix_right"].tolist()[:2] == [37, 37] and d["helix_left"].tolist()[2:4] == [37, 37] and d["quads"].tolist()[:4] == [37] * 4
    assert d["ligand_centres"].tolist() == [0] and d["ligand_kept"].tolist() == [1, 0] * 3 and d["ligand_inverted"].tolist() == [0, 1] * 3
    # the random walks have no helical majority: the ligand's centre decides them, by rule 2
    assert d["basis"].tolist()[4:] == [2, 2] and d["verdict"].tolist()[4:] == [1, -1] and (np.abs(d["helix_right"][4:] - d["helix_left"][4:]) < 4).all()
    assert d["tau"].shape == d["classes"].shape == (6, NR) and d["ligand_volume"].shape == (6, 1) and d["helix_fraction"].tolist()[:4] == [1.0] * 4
    assert np.allclose(np.abs(d["ligand_volume"][:, 0]), 2.598, atol=1e-3) and np.allclose(np.degrees(d["tau"][0, :37]), 50.04, atol=0.01)
    assert (int(d["input_verdict"]), int(d["input_basis"])) == (1, 1) and d["input_counts"].tolist() == [37, 0, 0, 0, 37, 1, 0, 0]
    # fix: x negated exactly where the verdict is -1, nothing else; the census values describe the samples as drawn
    f = fixed[6]
    assert all(np.array_equal(f[k], d[k], equal_nan=True) for k in d if k != "flipped") and np.array_equal(f["flipped"], d["verdict"] < 0)
    assert f["flipped"].tolist() == [False, False, True, True, False, True]
    want = samples.copy()
    want[f["flipped"], :, 0] = -want[f["flipped"], :, 0]
    assert np.array_equal(bits(unfixed[0]), bits(want)) and np.array_equal(unfixed[1], plain[1])
    assert np.array_equal(bits(np.stack(unfixed[3])), bits(want[:, :NA]))
    # the later stages see the fixed samples: the flipped helices need no mirror to fit the input, and distances do not change
    assert fixed[4]["mirrored"].tolist()[:4] == [0, 0, 0, 0] and scored[4]["mirrored"].tolist()[:4] == [0, 0, 1, 1]
    assert (fixed[4]["tmscore"][:4] > 0.99).all() and np.array_equal(fixed[1], plain[1])
    assert all(np.array_equal(fixed[5][k], scored[5][k]) for k in scored[5])
    # a spec moves a threshold: with min_helix = 50 the helices fall through to the ligand's centre
    assert spec[4]["basis"].tolist() == [2] * 6 and spec[4]["verdict"].tolist() == [1, -1] * 3 and spec[4]["flipped"].tolist() == [False, True] * 3
    # the files
    assert sorted(p.name for p in (tmp_path / "report").iterdir()) == ["sample_handedness.npz", "sample_handedness.txt", "sample_ligand_pos.npy",
                                                                        "sample_protein.pdb"]
    with np.load(tmp_path / "fix" / "sample_handedness.npz") as z:
        assert sorted(z.files) == sorted(f) and all(np.array_equal(z[k], f[k], equal_nan=True) for k in z.files)
    lines = (tmp_path / "fix" / "sample_handedness.txt").read_text().splitlines()
    assert lines[0] == "# verdict basis flipped helix_right helix_left extended_native extended_mirror quads centres_kept centres_inverted centres_flat"
    table = np.loadtxt(tmp_path / "fix" / "sample_handedness.txt", ndmin=2)
    cols = ["verdict", "basis", "flipped", "helix_right", "helix_left", "extended_native", "extended_mirror", "quads", "ligand_kept",
            "ligand_inverted", "ligand_flat"]
    assert table.shape == (6, 11) and all(np.array_equal(table[:, j], f[c].astype(np.float64)) for j, c in enumerate(cols))
    # "report" goes with a scaffold, "fix" does not (refused before the model is touched: tests/test_chirality_cpu.py)


def test_the_keyword_does_not_reach_the_real_model():
    """the real model at a tiny shape: "report" leaves every draw and position what it was"""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_sample
    from protein_redesign_amd.weights import spec_tensors
    args = make_args(single_dim=128, pair_dim=64, num_blocks=1, esm_dim=64, num_steps=4, mask_prob=0.3)
    model = ProteinReDiffModel(args)
    model.load_state_dict(deterministic_state_dict(spec_tensors(args), seed=1))
    model = model.to(DEV).eval()
    data = synthetic_sample(5, 12, esm_dim=64, seed=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(model, data, num_samples=2, batch_size=2, seed=4)
        report = PL.generate_samples(model, data, num_samples=2, batch_size=2, seed=4, handedness="report")
    assert len(plain) == 4 and len(report) == 5
    assert np.array_equal(bits(report[0]), bits(plain[0])) and np.array_equal(bits(report[1]), bits(plain[1]))
    assert report[4]["verdict"].shape == (2,) and report[4]["tau"].shape == (2, 12) and not report[4]["flipped"].any()
