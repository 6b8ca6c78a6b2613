"""CPU: the accessibility count as far as it goes without a GPU -- the header / build / export list of libprd_sasa.so and its host
refusals, its row of the third build table, the yardstick tests/sasa_ref.py on closed forms, the lattice's quadrature error, the band the
GPU tests rely on, the reference area, the host spec, and the ``accessibility=`` keyword of pipeline.generate_samples: its refusals, and
its whole path with the launch replaced by the yardstick."""
import inspect
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import backbone_ref as BR
import chirality_ref as CR
import sasa_ref as SR
from conftest import ROOT
from protein_redesign_amd import _lib, build
from protein_redesign_amd import backbone as BB
from protein_redesign_amd import chirality as CH
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd import sasa as SA
from sample_stubs import _NoDevice, header_entries
from test_backbone_cpu import _yardstick_build
from test_binding_cpu import Recorder, exported
from test_chirality_cpu import _host_reflect, _yardstick_census
from test_generate_samples_combinations_cpu import fakes

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
CSRC = os.path.join(ROOT, "protein_redesign_amd", "csrc")
SOURCE = os.path.join(CSRC, "sasa", "prd_sasa.hip")


# ---- header, build, export list, host refusals ------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("sasa")
    assert sorted(e) == ["prd_sasa_count", "prd_sasa_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    vp, ci, cll = _lib.vp, _lib.ci, _lib.cll
    assert e["prd_sasa_count"].argtypes == [vp, vp, cll, cll, vp, vp, vp, vp, ci, ci, ci, ci, vp] and e["prd_sasa_version"].argtypes == []
    assert SA.ENTRIES == e and not set(e) & set(_lib.ENTRIES)
    assert SA._DEFINES == {"VERSION": 100, "ERR_ARG": -1, "ERR_UNSUPPORTED": -3, "MAX_P": 1024, "MAX_A": 65536, "MAX_S": 65535, "ALL": 0, "SAME_GROUP": 1}
    assert SA.ABI_VERSION == 100 and (SA.MAX_P, SA.MAX_A, SA.MAX_S, SA.ALL, SA.SAME_GROUP) == (1024, 65536, 65535, 0, 1)
    with open(SOURCE) as f:
        text = f.read()
    assert '#include "../prd_launch.h"' in text and '#include "../../../include/prd_sasa.h"' in text
    for word in ("hipLaunchKernelGGL", "<<<", "asm", "atomic", "getenv", "hipMalloc", "Synchronize", "__builtin_amdgcn_rcp", "__builtin_amdgcn_rsq", "rsqrtf",
                 "__frcp", "sqrt"):
        assert word not in text, word
    assert text.count("prd_launch<") == 1                       # one launch per call
    assert "(ex * ex + ey * ey) + ez * ez" in text and "rr = n.w * n.w" in text       # the operation order the band is measured against
    assert "SA_WAVES = 4" in text and "SA_TILE = 64 * SA_WAVES" in text
    with open(os.path.join(ROOT, "include", "prd_sasa.h")) as f:
        head = f.read()
    assert head.lstrip().startswith("/* libprd_sasa.so")
    for words in ("DEFINITION", "(strictly)", "ARITHMETIC, part of the definition", "RELATIVE frame", "no cap on the number of neighbours", "NaN included",
                  "Every refusal happens on the host", "not mirror-symmetric"):
        assert words in head, words
    for words in ("WHAT IS CLAIMED", "OVERESTIMATE exposure", "poly-alanine", "not mirror-symmetric", "no bit-exact reflection claim"):
        assert words in SA.__doc__, words


def all_stale(monkeypatch):
    monkeypatch.delenv("HIPCC", raising=False)
    monkeypatch.setattr(build, "_stale", lambda out, deps: True)
    rec = Recorder(execute=False)
    rec.install(monkeypatch)
    return rec


def test_the_row_of_the_third_table_and_its_one_compile_and_one_link(monkeypatch):
    assert "sasa" in build.LATER_SIDE_LIBS and "sasa" not in build.SIDE_LIBS and "sasa" not in build.MORE_SIDE_LIBS
    s = build.LATER_SIDE_LIBS["sasa"]
    assert isinstance(s, build.SideLib) and s.sources == ["sasa/prd_sasa.hip"] and s.flag == "--sasa" and s.traced is False
    assert s.lib == os.path.join(ROOT, "protein_redesign_amd", "libprd_sasa.so")
    assert s.headers == [os.path.join(ROOT, "include", "prd_sasa.h"), os.path.join(CSRC, "prd_launch.h")]
    assert build._headers(s.sources[0]) == s.headers and all(os.path.exists(p) for p in s.headers + [SOURCE])
    # lookups: side_lib finds a row of any table; all_side_libs stays the first two tables; every_side_lib is all three, in their order
    assert build.side_lib("sasa") is s and build.side_lib("dssp") is build.MORE_SIDE_LIBS["dssp"] and build.side_lib("backbone") is build.SIDE_LIBS["backbone"]
    assert "sasa" not in build.all_side_libs() and list(build.all_side_libs()) == list(build.SIDE_LIBS) + list(build.MORE_SIDE_LIBS)
    every = build.every_side_lib()
    assert every["sasa"] is s and list(every) == list(build.SIDE_LIBS) + list(build.MORE_SIDE_LIBS) + list(build.LATER_SIDE_LIBS)
    with pytest.raises(KeyError):
        build.side_lib("nothing")
    rec = all_stale(monkeypatch)
    build.build(verbose=False)
    shipped, rec.cmds = rec.cmds[0], []
    build.build_side("sasa", verbose=False)
    src, obj, lib = (f"{{ROOT}}/protein_redesign_amd/{f}" for f in ("csrc/sasa/prd_sasa.hip", "csrc/sasa/prd_sasa.o", "libprd_sasa.so"))
    assert rec.cmds == [shipped[:-3] + [src, "-o", obj], shipped[:1] + ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj]]
    assert "-ffp-contract=off" in rec.cmds[0]
    # a variant's object lies under <variant objdir>/sasa/
    rec.cmds = []
    build.build_side("sasa", verbose=False, variant="asan")
    assert rec.cmds[0][-1] == "{ROOT}/protein_redesign_amd/csrc/asan/sasa/prd_sasa.o" and rec.cmds[1][rec.cmds[1].index("-o") + 1].endswith("libprd_sasa_asan.so")
    # no other build names it
    for other in [None] + [n for n in build.every_side_lib() if n != "sasa"]:
        rec.cmds = []
        build.build(verbose=False) if other is None else build.build_side(other, verbose=False)
        assert rec.cmds and not any("prd_sasa" in t for c in rec.cmds for t in c), other
    # the comment above the table says what the next library is
    with open(os.path.join(ROOT, "protein_redesign_amd", "build.py")) as f:
        text = f.read()
    above = text[text.index("# The third table"): text.index("LATER_SIDE_LIBS = ")]
    assert "csrc/<name>/" in above and "No fourth table" in above and "#   sasa  " in text


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_cross_compiled_exports_resources_and_stated_lds():
    lib = build.build_side("sasa", verbose=False)
    assert lib == build.LATER_SIDE_LIBS["sasa"].lib and exported(lib) == set(header_entries("sasa"))
    mine = build.resource_usage(sources=build.LATER_SIDE_LIBS["sasa"].sources)
    assert sorted(mine) == ["sasa_count_kernel"]
    assert not set(mine) & set(build.resource_usage()) and not set(mine) & set(build.resource_usage(sources=build.MORE_SIDE_LIBS["dssp"].sources))
    with open(SOURCE) as f:
        text = f.read()
    stated = int(re.search(r"constexpr int SA_LDS_BYTES = (\d+);", text).group(1))
    u = mine["sasa_count_kernel"]
    assert stated == 256 * 16 + 256 * 4 == u["lds"]
    assert u["scratch"] == 0 and u["agprs"] == 0, u


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """every refusal of prd_sasa.h is host code that runs before the first HIP call: reachable without a GPU, with device pointers that
    are never followed"""
    import ctypes
    build.build_side("sasa", verbose=False)
    L, D = SA.lib(), SA._DEFINES
    assert L.prd_sasa_version() == 100
    p = ctypes.c_void_p(4096)

    def call(count=p, pos=p, stride_s=15, stride_a=3, reach=p, present=p, group=p, sphere=p, mode=SA.SAME_GROUP, S=2, A=5, P=256):
        return L.prd_sasa_count(count, pos, stride_s, stride_a, reach, present, group, sphere, mode, S, A, P, None)
    for kw in [dict(count=None), dict(pos=None), dict(reach=None), dict(present=None), dict(sphere=None), dict(group=None), dict(S=0), dict(A=0), dict(P=0),
               dict(S=-1), dict(A=-4), dict(P=-64), dict(mode=2), dict(mode=-1), dict(stride_a=2), dict(stride_a=0), dict(stride_a=-3), dict(stride_s=14),
               dict(stride_s=0), dict(stride_s=-15), dict(stride_a=4, stride_s=18), dict(stride_a=2 ** 63 - 1, stride_s=2 ** 63 - 1),
               dict(P=100, reach=None)]:
        assert call(**kw) == D["ERR_ARG"], kw
    for kw in [dict(P=100), dict(P=63), dict(P=SA.MAX_P + 64), dict(A=SA.MAX_A + 1, stride_s=3 * (SA.MAX_A + 1)), dict(S=SA.MAX_S + 1),
               dict(mode=SA.ALL, group=None, P=100)]:
        assert call(**kw) == D["ERR_UNSUPPORTED"], kw
    # a single structure has no structure stride to overlap with
    assert call(S=1, stride_s=0, P=100) == D["ERR_UNSUPPORTED"]
    # the launch geometry the bounds promise: grid (A / 4, S), and every index fits
    assert SA.MAX_S <= 65535 and (SA.MAX_A + 3) // 4 < 2 ** 31 and SA.MAX_P % 64 == 0


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_host_side_of_the_library_under_address_sanitizer():
    """the same refusals from a stand-alone C program (tests/native/sasa_abi_check.c) against the library's host code built with
    AddressSanitizer.  Needs hipcc only (no GPU)."""
    exe = build.build_side_check("sasa", verbose=False)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    assert out.returncode == 0 and "sasa_abi_check OK" in text and "AddressSanitizer" not in text and "FAIL" not in text, text[-2000:]
    assert os.path.dirname(exe) == build.VARIANTS["asan"].objdir and os.path.exists(build.LATER_SIDE_LIBS["sasa"].lib.replace(".so", "_asan.so"))


# ---- the host spec ------------------------------------------------------------------------------------------------------------------------

def test_spec_is_validated_and_immutable():
    a = SA.Accessibility()
    assert (a.probe, a.points, a.buried_below) == (1.4, 256, 0.2) and a.radii == SA.Radii()
    assert dict(zip(SA.ATOMS, a.radii.backbone)) == {"N": 1.65, "CA": 1.87, "C": 1.76, "O": 1.40, "CB": 1.87}
    assert dict(a.radii.ligand) == {1: 1.20, 6: 1.70, 7: 1.55, 8: 1.52, 9: 1.47, 15: 1.80, 16: 1.80, 17: 1.75, 35: 1.85, 53: 1.98} and a.radii.other == 1.80
    t = a.radii.by_element()
    assert t.shape == (119,) and t[0] == 1.20 and t[5] == 1.70 and t[7] == 1.52 and t[52] == 1.98 and t[118] == 1.80 and t[25] == 1.80
    bb, el = a.reaches()
    assert bb.dtype == el.dtype == np.float32 and np.array_equal(bb, (np.array(a.radii.backbone) + 1.4).astype(np.float32)) and np.array_equal(el, (t + 1.4).astype(np.float32))
    assert SA.Accessibility.of("measure") == a and SA.Accessibility.of(a) is a and hash(a) == hash(SA.Accessibility())
    with pytest.raises(Exception):
        a.probe = 1.0
    with pytest.raises(ValueError, match="'measure'"):
        SA.Accessibility.of("sasa")
    for bad in (True, 1, dict()):
        with pytest.raises(TypeError, match="sasa.Accessibility"):
            SA.Accessibility.of(bad)
    for kw, what in ((dict(probe=-0.1), "probe"), (dict(probe=float("nan")), "probe"), (dict(probe="big"), "probe"), (dict(probe=True), "probe"),
                     (dict(points=100), "points"), (dict(points=0), "points"), (dict(points=2048), "points"), (dict(points=256.0), "points"),
                     (dict(points=True), "points"), (dict(buried_below=-0.1), "buried_below"), (dict(buried_below=1.5), "buried_below"),
                     (dict(buried_below=float("inf")), "buried_below"), (dict(radii=(1.0, 2.0)), "radii")):
        with pytest.raises(ValueError, match=what):
            SA.Accessibility(**kw)
    for kw in (dict(backbone=(1.6, 1.8)), dict(backbone=(1.6, 1.8, 1.7, 1.8, float("nan"))), dict(backbone=(1.6, 1.8, 1.7, 1.8, 9.0)), dict(ligand=((0, 1.5),)),
               dict(ligand=((119, 1.5),)), dict(ligand=((6, 1.7), (6, 1.8))), dict(ligand=((6, -1.0),)), dict(ligand=5), dict(other=float("inf"))):
        with pytest.raises(ValueError, match="radi"):
            SA.Radii(**kw)
    assert SA.Accessibility(points=64, probe=0).points == 64 and SA.Radii(ligand=[(8, 1.5)]).by_element()[7] == 1.5
    assert sorted(a.describe()) == ["backbone_radii", "buried_below", "ligand_radii", "points", "probe", "reference_area"]
    for bad in ([1.0, float("nan")], [1.0, -0.5], [float("inf")], [[1.0]]):
        with pytest.raises(ValueError, match="reach"):
            SA.check_reach(bad)
    # the lattice: unit vectors, the stated formula, rounded once
    for P in (64, 256, 1024):
        u = SA.sphere(P)
        assert u.shape == (P, 3) and u.dtype == np.float32 and np.abs(np.linalg.norm(u.astype(np.float64), axis=1) - 1).max() < 2e-7
        k = np.arange(P)
        assert np.array_equal(u[:, 2], (1 - (2 * k + 1) / P).astype(np.float32)) and np.abs(u.astype(np.float64).mean(0)).max() < 2.0 / P
    with pytest.raises(ValueError, match="positive integer"):
        SA.sphere(0)
    # area: the quotient in float64, tensors and arrays alike
    c, r = np.array([[0, 128, 256]]), np.array([1.0, 2.0, 3.0], np.float32)
    want = 4 * np.pi * np.array([[0.0, 4 * 0.5, 9.0]])
    assert np.allclose(SA.area(c, r, 256), want, rtol=1e-15) and SA.area(c, r, 256).dtype == np.float64
    got = SA.area(torch.from_numpy(c), torch.from_numpy(r), 256)
    assert got.dtype == torch.float64 and np.allclose(got.numpy(), want, rtol=1e-15)
    # a CPU tensor is refused: there is no fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        SA.count(torch.zeros(1, 4, 3), torch.ones(4), torch.ones(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="float32"):
        SA.count(torch.zeros(1, 4, 3, dtype=torch.float64), torch.ones(4), torch.ones(1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[S,nr,5,3\]"):
        SA.measure(torch.zeros(2, 5, 3), torch.zeros(2, 5, dtype=torch.int32), torch.zeros(2, 0, 3), torch.zeros(0))


# ---- the yardstick on its own ---------------------------------------------------------------------------------------------------------------

def _pair(r1, r2, d, P, dtype=np.float64):
    """count of atom 0 (reach r1) with atom 1 (reach r2) at distance d along a skew direction"""
    axis = np.array([0.36, -0.48, 0.8])
    pos = np.stack([np.zeros(3), d * axis])[None].astype(np.float32)
    return SR.count(pos, np.array([r1, r2], np.float32), np.ones((1, 2), np.int32), sphere=SA.sphere(P), dtype=dtype)


def test_closed_forms_of_the_yardstick():
    for P in (64, 256, 1024):
        one = SR.count(np.zeros((1, 1, 3), np.float32), np.array([3.0], np.float32), np.ones((1, 1), np.int32), sphere=SA.sphere(P))
        assert one["count"].tolist() == [[P]] and one["sure"].tolist() == [[P]] and one["ambiguous"].tolist() == [[0]]       # an isolated atom
        inside = _pair(2.0, 4.5, 1.0, P)
        assert inside["count"].tolist() == [[0, P]] and inside["sure"].tolist() == [[0, P]]      # an atom inside a larger one; the larger one is untouched
        apart = _pair(2.0, 3.0, 5.5, P)
        assert apart["count"].tolist() == [[P, P]]
    # an absent atom: count 0, buries nobody, and its coordinates -- NaN -- are never looked at
    pos = np.array([[[0, 0, 0], [np.nan, np.nan, np.nan], [1.0, 0, 0]]], np.float32)
    r = SR.count(pos, np.array([3.0, 9.0, 3.0], np.float32), np.array([[1, 0, 1]], np.int32))
    both = SR.count(pos[:, [0, 2]], np.array([3.0, 3.0], np.float32), np.ones((1, 2), np.int32))
    assert r["count"][0, 1] == 0 and np.array_equal(r["count"][0, [0, 2]], both["count"][0]) and 0 < r["count"][0, 0] < 256
    # groups: only the own group buries
    pos = np.array([[[0, 0, 0], [2.0, 0, 0], [0, 2.0, 0]]], np.float32)
    reach, ones = np.full(3, 3.0, np.float32), np.ones((1, 3), np.int32)
    g = SR.count(pos, reach, ones, np.array([0, 0, 1], np.int32), SR.SAME_GROUP)
    assert g["count"][0, 2] == 256 and np.array_equal(g["count"][0, :2], SR.count(pos[:, :2], reach[:2], ones[:, :2])["count"][0])
    # coincident atoms of equal reach: every margin is exactly 0 -- not buried (the test is strict), and all of it ambiguous
    tie = SR.count(np.zeros((1, 2, 3), np.float32), np.array([2.0, 2.0], np.float32), np.ones((1, 2), np.int32), sphere=SA.sphere(64))
    assert tie["sure"].tolist() == [[0, 0]] and tie["ambiguous"].tolist() == [[64, 64]]


PAIRS = [(r1, r2, f) for r1 in (2.6, 2.92, 3.1, 3.38) for r2 in (2.6, 3.0, 3.27) for f in (0.08, 0.21, 0.35, 0.5, 0.64, 0.77, 0.93)]


def test_the_lattice_quadrature_error_on_two_spheres():
    """A property of the lattice, not of the device: the worst |exposed fraction - analytic cap| of the yardstick over PAIRS -- 84 pairs of
    reaches met in practice, the second centre at |r1 - r2| + f (2 min(r1, r2)) along a skew axis -- is 0.0375 at P = 64, 0.0110 at
    P = 256 and 0.0043 at P = 1024 (measured here; over 2000 random pairs the figures were 0.052, 0.019 and 0.0066).  The assertion is
    1.5 times each figure; the computation is deterministic, the margin covers a later change of the list alone."""
    measured = {64: 0.0375, 256: 0.0110, 1024: 0.0043}
    for P, figure in measured.items():
        worst = 0.0
        for r1, r2, f in PAIRS:
            d = abs(r1 - r2) + f * 2 * min(r1, r2)
            got = _pair(r1, r2, d, P)["count"][0, 0] / P
            worst = max(worst, abs(got - SR.two_spheres(float(np.float32(r1)), float(np.float32(r2)), d)))
        print(f"P = {P}: worst quadrature error {worst:.4f} (stated {figure})")
        assert worst <= 1.5 * figure and worst >= 0.5 * figure, (P, worst)


def test_the_band_covers_the_fp32_restatement_and_the_cap_holds():
    """what tests/test_sasa.py relies on, checked here without a device: the fp32 restatement of the header's arithmetic -- what the
    kernel computes -- keeps within the rule against float64 on the shared inputs, the yardstick's own ambiguous share is under the cap,
    and the fp32 margin deviates from the float64 one by less than a third of the band, with and without a far offset"""
    assert SR.BAND == 1e-4 and SR.CAP == 1e-3
    I = SR.case_inputs(200, 1, 256)
    for offset in (0.0, 150.0, 1000.0):
        m = SR.measured_margin(I["pos"][0] + np.float32(offset), I["reach"], I["sphere"])
        print(f"offset {offset}: largest |fp32 margin - float64 margin| = {m:.3e} Angstrom^2 (band {SR.BAND:.0e})")
        assert m <= 3e-5
    for A, S, P, offset in ((200, 1, 256, 0.0), (65, 3, 64, 0.0), (257, 1, 64, 1000.0)):
        I = SR.case_inputs(A, S, P, offset=offset)
        ref = I["ref"]
        assert SR.capped(ref, P) and ref["ambiguous"].sum() <= 3
        got = SR.count(I["pos"], I["reach"], I["present"], sphere=I["sphere"], dtype=np.float32)
        assert SR.within(got["count"], ref) and np.array_equal(got["count"], ref["count"])
        assert (ref["count"] == 0).any() and ((ref["count"] > 0) & (ref["count"] < P)).sum() >= A // 8       # buried and partly buried atoms both occur
    # exact ties fall under the cap like any other case: two coincident atoms among 257
    pos, reach = np.array(I["pos"][:1]), np.array(I["reach"])
    pos[0, 7], reach[7] = pos[0, 3], reach[3]
    ref = SR.count(pos, reach, np.ones((1, 257), np.int32), sphere=I["sphere"])
    assert SR.capped(ref, 64) and SR.within(SR.count(pos, reach, np.ones((1, 257), np.int32), sphere=I["sphere"], dtype=np.float32)["count"], ref)


def test_reference_area_is_what_the_yardstick_measures():
    assert SA.REFERENCE_AREA == SR.reference_area() and 100.0 < SA.REFERENCE_AREA < 125.0
    # the middle residue of the extended chain is, by construction, at relative 1
    x = torch.from_numpy(BB.ideal_chain([-120.0] * 3, [130.0] * 3).astype(np.float32))[None]
    orig = SA.count
    SA.count = SR.fake_count
    try:
        got = SA.measure(x, torch.full((1, 3), 31, dtype=torch.int32), torch.zeros(1, 0, 3), torch.zeros(0, dtype=torch.long))
    finally:
        SA.count = orig
    assert abs(float(got["relative"][0, 1]) - 1.0) < 1e-14 and bool(got["complete"].all()) and not bool(got["buried"].any())
    assert np.isnan(float(got["ligand_buried_fraction"][0])) and float(got["interface_area"][0]) == 0.0 and got["ligand_area"].shape == (1, 0)


# ---- pipeline.generate_samples(accessibility=...) -------------------------------------------------------------------------------------------

def test_generate_samples_refuses_before_the_model_is_touched():
    data, _ = CR.complex_and_samples()
    with pytest.raises(ValueError, match='backbone="build"'):
        PL.generate_samples(_NoDevice(), data, num_samples=2, accessibility="measure")
    with pytest.raises(ValueError, match="'measure' or a sasa.Accessibility, got 'sasa'"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, backbone="build", accessibility="sasa")
    with pytest.raises(TypeError, match="sasa.Accessibility, got bool"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, backbone="build", accessibility=True)
    p = inspect.signature(PL.generate_samples).parameters
    assert p["accessibility"].default is None and p["accessibility"].kind is p["secondary"].kind
    assert "poly-alanine" in PL.generate_samples.__doc__ and "not mirror-symmetric" in PL.generate_samples.__doc__


def test_generate_samples_measures_after_the_backbone_returns_and_writes_with_the_launch_restated_on_the_host(tmp_path, monkeypatch):
    """the whole path of the keyword on the CPU; tests/test_sasa.py runs it with the launch itself"""
    from test_dssp_cpu import _yardstick_assign
    from protein_redesign_amd import dssp as DS
    log = []
    for (module, name), fake in fakes(log).items():
        monkeypatch.setattr(module, name, fake)
    monkeypatch.setattr(CH, "census", _yardstick_census)
    monkeypatch.setattr(CH, "reflect", _host_reflect)
    monkeypatch.setattr(BB, "build", _yardstick_build)
    monkeypatch.setattr(DS, "assign", _yardstick_assign)
    monkeypatch.setattr(SA, "count", SR.fake_count)
    data, samples = CR.complex_and_samples()
    NA, NR = CR.NA, CR.NR
    kw = dict(num_samples=6, batch_size=4, seed=3, handedness="fix", align_to="input")
    spec = SA.Accessibility(points=64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        before = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "before", backbone="build", secondary="assign", **kw)
        again = PL.generate_samples(CR.Prepared(samples, "cpu"), data, backbone="build", secondary="assign", accessibility=None, **kw)
        full = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "full", backbone="build", secondary="assign", accessibility=spec, **kw)
        alone = PL.generate_samples(CR.Prepared(samples, "cpu"), data, backbone="build", accessibility=spec, **kw)
    # nothing changed without the keyword; with it one trailing dict, after the secondary-structure dict
    assert len(before) == len(again) == 8 and len(full) == 9 and len(alone) == 8
    assert not [n for n in os.listdir(tmp_path / "before") if "accessibility" in n]
    for k in range(2):
        assert np.array_equal(before[k], again[k]) and np.array_equal(before[k], full[k])
    for k in (4, 5, 6, 7):
        assert sorted(before[k]) == sorted(full[k]) == sorted(again[k])
        assert all(np.array_equal(before[k][key], full[k][key], equal_nan=True) and np.array_equal(before[k][key], again[k][key], equal_nan=True)
                   for key in before[k] if key != "strings")
    d = full[8]
    assert all(np.array_equal(d[key], alone[7][key], equal_nan=True) for key in d) and sorted(d) == sorted(alone[7])
    assert sorted(d) == sorted(["atom_area", "residue_area", "relative", "buried", "complete", "ligand_area", "ligand_area_free", "ligand_buried_fraction",
                                "interface_area", "interface_residues", "total_area", "buried_residues", "probe", "points", "buried_below",
                                "backbone_radii", "ligand_radii", "reference_area"])
    assert d["atom_area"].shape == (6, NR, 5) and d["atom_area"].dtype == np.float64
    assert d["residue_area"].shape == d["relative"].shape == d["buried"].shape == d["complete"].shape == d["interface_residues"].shape == (6, NR)
    assert d["ligand_area"].shape == d["ligand_area_free"].shape == (6, NA)
    assert all(d[key].shape == (6,) for key in ("ligand_buried_fraction", "interface_area", "total_area", "buried_residues"))
    assert d["points"] == 64 and d["probe"] == 1.4 and d["buried"].dtype == bool and d["complete"].dtype == bool
    # the stage saw the atoms of the backbone stage and the ligand rows of the returned positions: the float64 yardstick on them
    mask, link = np.r_[np.zeros(NA), np.ones(NR)], np.r_[np.zeros(NA), np.ones(NR - 1), 0.0]
    built = BR.build(full[0], mask, link)
    atoms, bits = built["atoms"].astype(np.float32)[:, NA:], built["built"][:, NA:]
    assert np.array_equal(atoms, full[6]["atoms"])
    pos = np.concatenate([atoms.reshape(6, NR * 5, 3), full[0][:, :NA]], 1)
    present = np.concatenate([((bits[:, :, None] >> np.arange(5)) & 1).reshape(6, NR * 5), np.ones((6, NA), np.int64)], 1).astype(np.int32)
    bb, el = spec.reaches()
    reach = np.concatenate([np.tile(bb, NR), el[data["atom_feats"][:NA, 0].numpy()]])
    group = np.r_[np.zeros(NR * 5, np.int32), np.ones(NA, np.int32)]
    sphere = SA.sphere(64)
    ref, free = SR.count(pos, reach, present, sphere=sphere), SR.count(pos, reach, present, group, SR.SAME_GROUP, sphere)
    assert SR.capped(ref, 64) and SR.capped(free, 64)
    got_all = SR.counts_of(np.concatenate([d["atom_area"].reshape(6, NR * 5), d["ligand_area"]], 1), reach, 64)
    got_free = SR.counts_of(d["ligand_area_free"], reach[NR * 5:], 64)
    assert SR.within(got_all, ref) and SR.within(got_free, {k: free[k][:, NR * 5:] for k in ("sure", "ambiguous")})
    a_all = SA.area(got_all, reach, 64)
    assert np.allclose(d["total_area"], a_all.sum(1), rtol=1e-12)
    assert np.allclose(d["residue_area"], d["atom_area"].sum(2), rtol=1e-12) and np.allclose(d["relative"], d["residue_area"] / SA.REFERENCE_AREA, rtol=1e-12)
    lost = SA.area(free["count"] - ref["count"], reach, 64)                    # the area both partners lose, by the yardstick; a point of the band is 1.3 A^2 at most
    slack = SA.area(ref["ambiguous"] + free["ambiguous"], reach, 64).sum(1) + 1e-9
    assert (np.abs(d["interface_area"] - lost.sum(1)) <= slack).all() and (d["interface_area"] >= 0).all() and (d["interface_area"] > 0).any()
    assert np.array_equal(d["complete"], (bits & 23) == 23) and np.array_equal(d["buried"], (d["relative"] < 0.2) & ((bits & 2) != 0))
    assert (d["ligand_area"] <= d["ligand_area_free"]).all() and np.array_equal(d["buried_residues"], d["buried"].sum(1))
    assert np.allclose(d["ligand_buried_fraction"], 1 - d["ligand_area"].sum(1) / d["ligand_area_free"].sum(1), rtol=1e-12)
    sure_lost = (free["sure"] - ref["sure"] - ref["ambiguous"])[:, : NR * 5].reshape(6, NR, 5).sum(2) > 0       # lost beyond the band
    assert (d["interface_residues"] | ~sure_lost).all() and d["interface_residues"].any() and (d["interface_residues"].sum(1) <= NR // 2).all()
    # the helices are built everywhere, the random walks nowhere: those keep their C-alphas alone, which take part with CA's radius
    assert d["complete"][:4].all() and not d["complete"][4:].any() and (d["atom_area"][4:, :, 1] > 0).any() and (d["atom_area"][4:, :, [0, 2, 3, 4]] == 0).all()
    # the input has CA alone: no input_relative
    assert "input_relative" not in d and "burial_agreement" not in d
    assert sorted(os.listdir(tmp_path / "full")) == sorted(os.listdir(tmp_path / "before") + ["sample_accessibility.npz", "sample_accessibility.txt"])
    with np.load(tmp_path / "full" / "sample_accessibility.npz") as z:
        assert sorted(z.files) == sorted(d) and all(np.array_equal(z[k], d[k], equal_nan=True) for k in z.files)
    lines = (tmp_path / "full" / "sample_accessibility.txt").read_text().splitlines()
    assert lines[0] == "# total_area interface_area ligand_buried_fraction buried_residues" and len(lines) == 7
    for k, line in enumerate(lines[1:]):
        assert [float(v) for v in line.split()] == [d["total_area"][k], d["interface_area"][k], d["ligand_buried_fraction"][k], d["buried_residues"][k]]
    # an input with its own N, C and O: its relative areas by the same call, and the share of residues called alike
    import dssp_ref as DR
    helix = DR.regular(DR.ALPHA, NR)
    whole = dict(data, residue_atom_pos=torch.zeros(NR, 37, 3), residue_atom_mask=torch.zeros(NR, 37))
    whole["residue_atom_pos"][:, :5] = torch.from_numpy((helix - helix[:, 1].mean(0)).astype(np.float32))
    whole["residue_atom_mask"][:, :5] = 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        own = PL.generate_samples(CR.Prepared(samples, "cpu"), whole, backbone="build", accessibility=SA.Accessibility(points=64, buried_below=0.6), **kw)[7]
    assert own["input_relative"].shape == (NR,) and own["burial_agreement"].shape == (6,)
    assert (own["input_relative"] > 0).all() and (own["input_relative"][1:-1] < 1.0).all()
    alike = ((own["relative"] < 0.6) == (own["input_relative"] < 0.6)[None]) & own["complete"]
    assert np.allclose(own["burial_agreement"][:4], alike[:4].sum(1) / own["complete"][:4].sum(1), rtol=1e-12) and (own["burial_agreement"][:4] >= 0.5).all()
    assert np.isnan(own["burial_agreement"][4:]).all()           # the walks have no whole residue
