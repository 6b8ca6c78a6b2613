"""CPU: the yardstick of the structural-alignment tests (tests/tmalign_ref.py) on the planted cases, the header / build / export list /
workspace query of libprd_tmalign.so, the Python-side argument checks and the ``correspondence`` keyword of pipeline.generate_samples as
far as it goes without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import align_ref as AR
import tmalign_cases as TC
import tmalign_ref as TR
from conftest import ROOT
from protein_redesign_amd import _lib, build
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.synthetic import synthetic_sample
from sample_stubs import _NoDevice, _Stub, header_entries
from test_binding_cpu import Recorder

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------

def test_secondary_structure_classes_and_their_mirror_invariance():
    k = np.arange(12)
    a = np.deg2rad(100.0) * k
    helix = np.stack([2.3 * np.cos(a), 2.3 * np.sin(a), 1.5 * k], 1)
    strand = np.stack([3.2 * k, 2.05 * (k % 2), 0.0 * k], 1)
    assert list(TR.sec_classes(helix)) == [0, 0] + [TR.HELIX] * 8 + [0, 0]
    assert list(TR.sec_classes(strand)) == [0, 0] + [TR.STRAND] * 8 + [0, 0]
    assert list(TR.sec_classes(strand * 0.5)) == [0, 0] + [TR.TURN] * 8 + [0, 0] and not TR.sec_classes(strand * 2.0).any()
    x = TR.ss_chain(np.random.default_rng(1), 200)
    sx = TR.sec_classes(x)
    assert np.array_equal(sx, TR.sec_classes(x @ AR.MIRROR)) and set(sx) == {0, 1, 2, 3}          # classes B and C are exercised
    assert np.abs(np.linalg.norm(np.diff(x, axis=0), axis=1) - 3.8).max() < 1e-9


def test_dp_follows_the_recurrence_on_a_small_matrix():
    s = np.eye(4)[:, [0, 1, 3]]                                     # x_2 has no partner
    assert list(TR.dp(s, -1.0)) == [0, 1, -1, 2]
    assert list(TR.dp(np.zeros((3, 2)), -1.0)) == [-1, 0, 1]        # all ties: D wins, end gaps are free
    assert list(TR.dp(np.array([[0.0, 1.0], [1.0, 0.0]]), 0.0)) == [1, -1]      # H >= V decides a tie of the two gaps: x_2 is left out


@pytest.mark.parametrize("case", TC.CASES + TC.LONG_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}{'-m' if c[3] else ''}")
def test_yardstick_meets_the_planted_bound_and_is_stable_under_float32_scores(case):
    c = TC.planted_case(*case)
    got = TC.yardstick(*case)
    x, y, amap, R, t = c["x"], c["y"], got["mapping"], got["rotation"], got["translation"]
    assert np.abs(x).max() < 100.0 and np.abs(y).max() < 100.0
    assert got["tm"] >= c["planted_tm"] - 1e-4, (case, got["tm"], c["planted_tm"])
    assert (got["tm"], got["rmsd"], got["n_aligned"]) == TR.score_of(x, y, amap, R, t)
    on = amap[amap >= 0]
    assert (np.diff(on) > 0).all() and len(on) == got["n_aligned"] >= 3 and on.max() < case[1]
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - (-1.0 if got["mirrored"] else 1.0)) < 1e-12
    if case[2] == 1.0 and min(case[:2]) >= 40:
        assert got["mirrored"] == int(case[3])
    assert np.array_equal(TC.yardstick(*case, f32_scores=True)["mapping"], amap)         # the rule a kept case obeys


def test_at_most_one_candidate_seed_in_ten_was_dropped():
    assert len(TC.KEPT) == len(TC.SHAPES) == 9 and sum(TC.KEPT) * 10 <= sum(k + 1 for k in TC.KEPT) and max(TC.KEPT) <= 2
    assert len(TC.LONG_KEPT) == len(TC.LONG_SHAPES) == 4 and max(TC.LONG_KEPT) <= 2
    dropped, tried = sum(TC.KEPT) + sum(TC.LONG_KEPT), sum(k + 1 for k in TC.KEPT + TC.LONG_KEPT)
    assert dropped * 10 <= tried and [c[:2] for c in TC.LONG_CASES] == TC.LONG_SHAPES
    assert [c[:2] for c in TC.CASES] == TC.SHAPES and {c[2] for c in TC.CASES} == {1.0, 0.6, 0.35} and any(c[3] for c in TC.CASES)


def test_yardstick_short_chains_and_equal_length_identity():
    z = TR.align(np.zeros((4, 3)), np.ones((9, 3)))
    assert z["tm"] == 0.0 and z["n_aligned"] == 0 and (z["mapping"] == -1).all() and np.array_equal(z["rotation"], np.eye(3))
    rng = np.random.default_rng(4064)
    x, y, R0, t0, amap = TR.planted(rng, 64, 64, 1.0, indels=False)
    got = TR.align(x, y)
    assert np.array_equal(amap, np.arange(64)) and np.array_equal(got["mapping"], np.arange(64))
    assert got["tm"] >= AR.superimpose(x, y)["tm"] - 1e-4


# ---- header, build, export list ---------------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("tmalign")
    assert sorted(e) == ["prd_tmalign_align", "prd_tmalign_version", "prd_tmalign_workspace_bytes"]
    assert all(x.inject is None for x in e.values())
    assert e["prd_tmalign_workspace_bytes"].restype is _lib.cz and len(e["prd_tmalign_workspace_bytes"].argtypes) == 5
    assert len(e["prd_tmalign_align"].argtypes) == 23
    from protein_redesign_amd import align, tmalign
    assert tmalign.ENTRIES == e and not set(e) & set(_lib.ENTRIES) and not set(e) & set(align.ENTRIES)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_shared_fit_header_makes_both_side_libraries_stale_and_not_the_denoiser(monkeypatch):
    """``_stale`` is the real one and no compiler runs: the header of the fit (csrc/prd_superpose.h) is given the newest time stamp, and
    a command that is recorded makes its output newer still, as the compiler would have."""
    build.build(verbose=False)
    build.build_side("align", verbose=False)
    build.build_side("tmalign", verbose=False)
    header, real, written = os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_superpose.h"), os.path.getmtime, []
    assert os.path.exists(header)
    newest = max(real(p) for p in (build.LIB, build.SIDE_LIBS["align"].lib, build.SIDE_LIBS["tmalign"].lib)) + 10.0
    monkeypatch.setattr(os.path, "getmtime", lambda p: newest + 10.0 * (1 + written.index(p)) if p in written else newest if p == header else real(p))

    class Touching(Recorder):
        def __call__(self, kind, cmd, *a, **kw):
            written.extend(cmd[cmd.index("-o") + 1:][:1] if "-o" in cmd else [])
            return super().__call__(kind, cmd, *a, **kw)
    rec = Touching(execute=False)
    rec.install(monkeypatch)
    build.build(verbose=False)
    assert rec.cmds == []
    for name in ("align", "tmalign"):
        build.build_side(name, verbose=False)
        obj = "{ROOT}/protein_redesign_amd/csrc/prd_%s.o" % name
        assert [c[-3:] for c in rec.cmds] == [["{ROOT}/protein_redesign_amd/csrc/prd_%s.hip" % name, "-o", obj],
                                              ["-o", "{ROOT}/protein_redesign_amd/libprd_%s.so" % name, obj]]
        rec.cmds = []


def test_the_fit_is_defined_in_one_file():
    csrc = os.path.join(ROOT, "protein_redesign_amd", "csrc")
    for fn in ("jacobi_rotate", "kabsch_from_sums"):
        defined = []
        for name in sorted(os.listdir(csrc)):
            if name.endswith((".hip", ".h", ".inc")):
                with open(os.path.join(csrc, name)) as f:
                    defined += [name] * len(re.findall(r"\bvoid\s+%s\s*\(" % fn, f.read()))
        assert defined == ["prd_superpose.h"], (fn, defined)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_new_kernels():
    mine = build.resource_usage(sources=build.SIDE_LIBS["tmalign"].sources)
    assert sorted(mine) == ["tmalign_compact_kernel", "tmalign_finalize_kernel", "tmalign_refine_kernel", "tmalign_search_kernel"]
    assert all(u["scratch"] == 0 for u in mine.values())


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_workspace_bytes_refusals_growth_and_lower_bound():
    from protein_redesign_amd import tmalign
    build.build_side("tmalign", verbose=False)
    ws = tmalign.lib().prd_tmalign_workspace_bytes
    assert ws(2, 3, 2048, 2048, 1) > 0 and ws(2, 3, 2049, 64, 1) == 0 and ws(2, 3, 64, 2049, 1) == 0
    assert ws(0, 3, 64, 64, 1) == 0 and ws(2, 0, 64, 64, 1) == 0 and ws(2, 3, 0, 64, 1) == 0 and ws(2, 3, 64, 0, 1) == 0 and ws(-1, 3, 64, 64, 0) == 0
    assert ws(1 << 15, 1 << 15, 8, 8, 1) == 0                   # more problems than PRD_TMALIGN_MAX_PROBLEMS = 2^20
    assert ws(1 << 9, 1 << 9, 8, 8, 0) > 0 and ws(1 << 9, 1 << 9, 8, 8, 1) == 0 and ws((1 << 20) // 3 + 1, 1, 8, 8, 0) == 0

    def floor(S, R, Nx, Ny, nm):
        """what the kernels index: the header, the planes, one mapping per problem, 2 direction bits per cell per problem"""
        nprob = S * R * nm * 3
        return 16 * 4 + (S * 3 * Nx + R * 3 * Ny) * 4 + nprob * Nx * 4 + nprob * (Nx * Ny * 2 + 7) // 8
    sizes = [5, 6, 15, 16, 17, 63, 64, 65, 300, 320, 1023, 1024, 1025, 2047, 2048]
    for S, R, mirror in ((1, 1, 1), (2, 3, 0), (4, 1, 1)):
        for fixed in (5, 100, 2048):
            along_x = [ws(S, R, N, fixed, mirror) for N in range(1, 2049, 7)] + [ws(S, R, 2048, fixed, mirror)]
            along_y = [ws(S, R, fixed, N, mirror) for N in range(1, 2049, 7)] + [ws(S, R, fixed, 2048, mirror)]
            for seq in (along_x, along_y):
                assert all(b > 0 and b % 16 == 0 for b in seq) and all(a <= b for a, b in zip(seq, seq[1:])), (S, R, fixed)
        for Nx in sizes:
            for Ny in sizes:
                assert ws(S, R, Nx, Ny, mirror) >= floor(S, R, Nx, Ny, 2 if mirror else 1), (S, R, Nx, Ny)


def test_host_argument_checks_of_the_python_side():
    from protein_redesign_amd import tmalign
    x, m = torch.zeros(2, 5, 3), torch.ones(5)
    y, my = torch.zeros(7, 3), torch.ones(7)
    with pytest.raises(RuntimeError, match="GPU only"):
        tmalign.align(x, y, m, my)
    with pytest.raises(ValueError, match="float32"):
        tmalign.align(x.double(), y, m, my)
    with pytest.raises(ValueError, match=r"\[K,N,3\]"):
        tmalign.align(torch.zeros(5, 3), y, m, my)
    assert tmalign.MAX_N == 2048 and tmalign.ABI_VERSION == 100
    with open(os.path.join(ROOT, "include", "prd_tmalign.h")) as f:
        text = f.read()
    assert "#define PRD_TMALIGN_MAX_N 2048" in text and "#define PRD_TMALIGN_VERSION 100" in text


# ---- pipeline.generate_samples(correspondence=...) ---------------------------------------------------------------------------------

def _reference(n, marked=None):
    p = PL.protein_from_sequence(("ACDEFGHIKLMNPQRSTVWY" * (n // 20 + 1))[:n])
    p.atom_pos[:, 1] = np.random.default_rng(n).normal(size=(n, 3)) * 10.0
    p.atom_mask[:, 1] = 0.0
    p.atom_mask[: n if marked is None else marked, 1] = 1.0
    return p


def test_structure_requests_are_refused_before_the_model_is_touched():
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)

    def gen(**kw):
        return PL.generate_samples(_NoDevice(), full, num_samples=1, correspondence="structure", **kw)
    for known in ("input", "first", None):
        with pytest.raises(ValueError, match="correspondence"):
            gen(align_to=known)
    with pytest.raises(ValueError, match="correspondence must be"):
        PL.generate_samples(_NoDevice(), full, num_samples=1, align_to=np.zeros((9, 3)), correspondence="sequence")
    with pytest.raises(ValueError, match="4 residues with a C-alpha"):
        gen(align_to=_reference(12, marked=4))
    with pytest.raises(ValueError, match="all zero"):
        gen(align_to=PL.protein_from_sequence("ACDEFGHIK"))
    with pytest.raises(ValueError, match="all zero"):
        gen(align_to=np.zeros((12, 3)))
    with pytest.raises(ValueError, match="2048"):
        gen(align_to=np.ones((2049, 3)))
    with pytest.raises(ValueError, match=r"\[m,3\]"):
        gen(align_to=np.ones((12, 4)))
    with pytest.raises(ValueError, match=r"\[m,3\]"):
        gen(align_to=np.ones((4, 3)))
    big = dict(full, num_residues=2044)                                     # 5 ligand atoms + 2044 residues: 2049 rows on the sample side
    with pytest.raises(ValueError, match="2049 rows"):
        PL.generate_samples(_NoDevice(), big, num_samples=1, correspondence="structure", align_to=_reference(12))
    with pytest.raises(AssertionError, match="the model was touched"):     # a reference of another length passes the host checks
        gen(align_to=_reference(12))


def test_index_correspondence_is_the_untouched_path(tmp_path, monkeypatch):
    import warnings
    from protein_redesign_amd import tmalign
    monkeypatch.setattr(tmalign, "align", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the structural alignment ran")))
    monkeypatch.setattr(tmalign, "lib", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    for kw in (dict(), dict(correspondence="index")):
        with pytest.raises(ValueError, match="9 residues"):
            PL.generate_samples(_NoDevice(), full, num_samples=1, align_to=_reference(12), **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        a = PL.generate_samples(_Stub(), full, num_samples=2, seed=1, output_dir=tmp_path / "a")
        b = PL.generate_samples(_Stub(), full, num_samples=2, seed=1, output_dir=tmp_path / "b", correspondence="index")
    assert len(a) == len(b) == 4 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert sorted(os.listdir(tmp_path / "b")) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
