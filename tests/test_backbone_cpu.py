"""CPU: the backbone builder as far as it goes without a GPU -- the header / build / export list of libprd_backbone.so and its host
refusals, the yardstick tests/backbone_ref.py on ideal chains (the accuracy that is claimed, and nothing beyond it), the host specs, the
inputs of the GPU tests, and the ``backbone=`` keyword of pipeline.generate_samples: its refusals, and its whole path with every launch
replaced by its float64 yardstick."""
import inspect
import math
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import backbone_ref as BR
import chirality_ref as CR
from conftest import ROOT
from protein_redesign_amd import _lib, build
from protein_redesign_amd import backbone as BB
from protein_redesign_amd import chirality as CH
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.conditioning import Scaffold
from sample_stubs import _NoDevice, header_entries
from test_chirality_cpu import _host_reflect, _yardstick_census
from test_generate_samples_combinations_cpu import fakes

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
SOURCE = os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_backbone.hip")
ONES = lambda n: np.ones(n)         # noqa: E731


# ---- header, build, export list, host refusals ------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("backbone")
    assert sorted(e) == ["prd_backbone_build", "prd_backbone_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    vp, ci, cf, cll = _lib.vp, _lib.ci, _lib.cf, _lib.cll
    assert e["prd_backbone_build"].argtypes == [vp] * 3 + [cll, ci] + [vp] * 3 + [cf] * 13 + [ci, ci, vp] and e["prd_backbone_version"].argtypes == []
    assert BB.ENTRIES == e and not set(e) & set(_lib.ENTRIES)
    assert BB._DEFINES == {"VERSION": 100, "ERR_ARG": -1, "ERR_UNSUPPORTED": -3, "MAX_N": 32768, "MAX_S": 65535, "TABLE": 73}
    assert BB.ABI_VERSION == 100 and (BB.MAX_N, BB.MAX_S, BB.TABLE) == (32768, 65535, 73)
    with open(SOURCE) as f:
        text = f.read()
    assert '#include "prd_launch.h"' in text and "hipLaunchKernelGGL" not in text and "<<<" not in text and "asm" not in text
    assert "atomic" not in text and "getenv" not in text and "hipMalloc" not in text and "Synchronize" not in text
    assert text.count("prd_launch<") == 1                       # one launch
    with open(os.path.join(ROOT, "include", "prd_backbone.h")) as f:
        head = f.read()
    assert head.lstrip().startswith("/* libprd_backbone.so") and all(w in head for w in ("Padding.", "Validity", "dyad(", "L-residues always"))
    assert (BR.TILE, BR.HALO) == (256, 3) and "BB_TILE = BB_THREADS" in text and "BB_THREADS = 256" in text and "BB_HALO = 3" in text


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_kernel():
    import re
    mine = build.resource_usage(sources=build.SIDE_LIBS["backbone"].sources)
    assert sorted(mine) == ["backbone_build_kernel"]
    u = mine["backbone_build_kernel"]
    with open(SOURCE) as f:
        stated = int(re.search(r"constexpr int BB_LDS_BYTES = (\d+);", f.read()).group(1))
    assert u["lds"] == stated == (256 + 6) * 16 + (256 + 8) * 4 and u["scratch"] == 0 and u["agprs"] == 0 and u["vgprs"] <= 64


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """every refusal of prd_backbone.h is host code that runs before the first HIP call: reachable without a GPU, with device pointers
    that are never followed"""
    import ctypes
    build.build_side("backbone", verbose=False)
    L, D = BB.lib(), BB._DEFINES
    assert L.prd_backbone_version() == 100
    p = ctypes.c_void_p(4096)
    inf, nan = float("inf"), float("nan")
    good = list(BB.Backbone().scalars())
    names = ("l0", "ac", "rc", "ao", "ro", "an", "rn", "ka", "kb", "kc", "lo2", "hi2", "sin2")

    def call(atoms=p, built=p, x=p, xs=30, xr=3, mask=p, link=p, table=p, S=2, N=5, **kw):
        g = [kw.pop(n, v) for n, v in zip(names, good)]
        assert not kw
        return L.prd_backbone_build(atoms, built, x, xs, xr, mask, link, table, *g, S, N, None)
    bad = [dict(atoms=None), dict(built=None), dict(x=None), dict(mask=None), dict(link=None), dict(table=None), dict(S=0), dict(N=0), dict(S=-1),
           dict(N=-4), dict(xr=2), dict(xs=-1), dict(l0=0.0), dict(l0=-3.8), dict(ka=0.0), dict(ka=0.5), dict(lo2=18.49, hi2=10.89),
           dict(lo2=10.89, hi2=10.89), dict(lo2=0.0), dict(lo2=-1.0), dict(sin2=-0.1), dict(sin2=1.0)]
    bad += [{n: v} for n in names for v in (nan, inf, -inf)]
    for kw in bad:
        assert call(**kw) == D["ERR_ARG"], kw
    for kw in (dict(N=BB.MAX_N + 1), dict(S=BB.MAX_S + 1)):
        assert call(**kw) == D["ERR_UNSUPPORTED"], kw
    # the launch geometry the bounds promise: the grid is (N / 256, S), and every output index fits size_t
    assert BB.MAX_S <= 65535 and BB.MAX_N * 15 < 2 ** 31


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_host_side_of_the_library_under_address_sanitizer():
    """the same refusals from a stand-alone C program (tests/native/backbone_abi_check.c) against the library's host code built with
    AddressSanitizer.  Needs hipcc only (no GPU)."""
    exe = build.build_side_check("backbone", verbose=False)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    assert out.returncode == 0 and "backbone_abi_check OK" in text and "AddressSanitizer" not in text and "FAIL" not in text, text[-2000:]
    assert os.path.dirname(exe) == build.VARIANTS["asan"].objdir and os.path.exists(build.SIDE_LIBS["backbone"].lib.replace(".so", "_asan.so"))


# ---- the host specs -------------------------------------------------------------------------------------------------------------------------

def test_geometry_is_recomputed_from_bonds_and_angles():
    g = BB.Geometry().plane()
    assert abs(g["L0"] - 3.80395) < 5e-6
    for key, want in (("C", (1.42842, 0.53408)), ("O", (1.64217, 1.74638)), ("N", (-1.40832, -0.37737))):
        assert np.allclose(g[key], want, atol=5e-6), key
    # the numbers ARE the peptide: bond lengths and angles read back from the plane
    ca, ca2 = np.zeros(2), np.array([g["L0"], 0.0])
    c, o, n = np.array(g["C"]), np.array(g["O"]), ca2 + np.array(g["N"])
    dist = lambda a, b: float(np.linalg.norm(a - b))         # noqa: E731
    ang = lambda a, v, b: math.degrees(math.acos(np.dot(a - v, b - v) / (dist(a, v) * dist(b, v))))      # noqa: E731
    assert np.allclose([dist(ca, c), dist(c, n), dist(n, ca2), dist(c, o)], [1.525, 1.329, 1.458, 1.231], atol=1e-12)
    assert np.allclose([ang(ca, c, n), ang(c, n, ca2), ang(ca, c, o)], [116.2, 121.7, 120.5], atol=1e-9)
    cross = lambda u, v: u[0] * v[1] - u[1] * v[0]           # noqa: E731
    assert cross(n - c, ca - c) * cross(n - c, ca2 - n) < 0   # trans: the two C-alphas on opposite sides of the C-N bond, seen along it
    s = BB.Backbone().scalars()
    assert len(s) == 13 and all(v == float(np.float32(v)) for v in s)
    assert s[:10] == BB.Geometry().scalars() and s[7:10] == tuple(float(np.float32(v)) for v in (-0.58273431, 0.56802827, -0.54067466))
    assert s[10:] == tuple(float(np.float32(v)) for v in (3.3 ** 2, 4.3 ** 2, math.sin(math.radians(10.0)) ** 2))
    other = BB.Geometry(c_n=1.34).plane()
    assert other["L0"] != g["L0"]
    for kw, what in ((dict(n_ca=0.0), "n_ca"), (dict(ca_c_n=200.0), "ca_c_n"), (dict(cb=(0.5, 0.5, -0.5)), "ka < 0"), (dict(cb=(1.0, 2.0)), "cb must"),
                     (dict(c_o=float("nan")), "c_o")):
        with pytest.raises(ValueError, match=what):
            BB.Geometry(**kw)


def test_ideal_chain_places_the_requested_bonds_angles_and_dihedrals():
    rng = np.random.default_rng(0)
    L = 30
    phi, psi = rng.uniform(-180, 180, L), rng.uniform(-180, 180, L)
    ch = BB.ideal_chain(phi, psi)
    assert ch.shape == (L, 5, 3)
    n, ca, c, cb, o = (ch[:, k] for k in range(5))
    norm = lambda v: np.linalg.norm(v, axis=-1)              # noqa: E731
    assert np.allclose(norm(ca - n), 1.458) and np.allclose(norm(c - ca), 1.525) and np.allclose(norm(n[1:] - c[:-1]), 1.329) and np.allclose(norm(o - c), 1.231)
    wrapped = lambda a, b: np.abs((np.degrees(a) - b + 180.0) % 360.0 - 180.0).max()      # noqa: E731
    assert wrapped(BR.dihedral(c[:-1], n[1:], ca[1:], c[1:]), phi[1:]) < 1e-9
    assert wrapped(BR.dihedral(n[:-1], ca[:-1], c[:-1], n[1:]), psi[:-1]) < 1e-9
    assert wrapped(BR.dihedral(ca[:-1], c[:-1], n[1:], ca[1:]), 180.0) < 1e-9
    assert wrapped(BR.dihedral(o[:-1], c[:-1], n[1:], ca[1:]), 0.0) < 1e-9            # O is cis to the next C-alpha: a trans peptide
    assert np.allclose(norm(ca[1:] - ca[:-1]), BB.Geometry().plane()["L0"], atol=1e-12)
    assert (BR.cb_volume(ch) > 0).all() and np.allclose(norm(cb - ca), 1.52, atol=0.02)
    with pytest.raises(ValueError, match="phi and psi"):
        BB.ideal_chain([1.0, 2.0], [1.0])


def test_orientation_is_periodic_takes_the_shorter_arcs_and_passes_through_its_knots():
    o = BB.Orientation.ideal()
    assert o is BB.Orientation.ideal() and BB.Backbone().orientation is o and len(o.knots) == 6
    assert [t for t, _ in o.knots] == sorted(t for t, _ in o.knots) and all(0.0 <= t < 360.0 for t, _ in o.knots)
    measured = sorted(BB.measure(BB.ideal_chain([phi] * 8, [psi] * 8), 3) for phi, psi in BB.ANCHORS)      # another chain, another peptide
    assert np.allclose(measured, o.knots, atol=1e-9)
    t = o.table()
    assert t.dtype == np.float32 and t.shape == (73,) and t[72] == t[0] and np.isfinite(t).all()
    assert np.array_equal(t[:72], np.array([math.radians(o.curve(5.0 * g)) for g in range(72)]).astype(np.float32))
    knots = list(o.knots) + [(o.knots[0][0] + 360.0, o.knots[0][1])]
    for (ta, xa), (tb, xb) in zip(knots, knots[1:]):
        arc = (xb - xa + 180.0) % 360.0 - 180.0                # the shorter of the two ways round
        assert abs(arc) <= 180.0
        for f in (0.0, 0.25, 0.5, 1.0):
            got = o.curve(ta + f * (tb - ta))
            assert abs((got - (xa + f * arc) + 180.0) % 360.0 - 180.0) < 1e-9
    assert abs(o.curve(0.0) - o.curve(360.0)) < 1e-9 and abs(o.curve(-5.0) - o.curve(355.0)) < 1e-9
    # neighbouring table entries never differ by a turn: the device interpolates them linearly
    assert np.abs(np.diff(t.astype(np.float64))).max() < math.radians(45.0)
    # the shorter arc between 170 and -170 degrees passes through 180, not through 0
    two = BB.Orientation(knots=[(180.0, -170.0), (0.0, 170.0)])
    assert two.knots == ((0.0, 170.0), (180.0, -170.0)) and abs(two.curve(90.0) - 180.0) < 1e-9 and abs(abs(two.curve(270.0)) - 180.0) < 1e-9
    assert abs(two.table()[18] - math.pi) < 1e-6
    flat = BB.Orientation.constant(30.0)
    assert np.array_equal(flat.table(), np.full(73, np.float32(math.radians(30.0))))
    for knots, what in (([(0.0, 0.0), (120.0, 120.0), (240.0, 240.0)], "wind"), ([], "at least one"), ([(10.0, 1.0), (370.0, 2.0)], "share a tau"),
                        ([(0.0, float("nan"))], "finite"), ("ab", "knots must")):
        with pytest.raises(ValueError, match=what):
            BB.Orientation(knots=knots)


def test_backbone_spec_is_validated_and_immutable():
    b = BB.Backbone()
    assert (b.geometry, b.bond, b.min_angle) == (BB.Geometry(), (3.3, 4.3), 10.0) and BB.BOND == CH.BOND
    assert BB.Backbone.of("build") == b and BB.Backbone.of(b) is b and hash(b) == hash(BB.Backbone())
    with pytest.raises(Exception):
        b.min_angle = 5.0
    with pytest.raises(ValueError, match="'build'"):
        BB.Backbone.of("full")
    for bad in (True, 1, dict()):
        with pytest.raises(TypeError, match="backbone.Backbone"):
            BB.Backbone.of(bad)
    for kw, what in ((dict(bond=(4.3, 3.3)), "bond must"), (dict(bond=3.8), "bond must"), (dict(min_angle=90.0), "min_angle"), (dict(min_angle=-1.0), "min_angle"),
                     (dict(geometry="ideal"), "geometry must"), (dict(orientation=30.0), "orientation must")):
        with pytest.raises(ValueError, match=what):
            BB.Backbone(**kw)
    d = b.describe()
    assert sorted(d) == ["L0", "bond", "cb", "min_angle", "plane_C", "plane_N", "plane_O", "table"] and d["table"].shape == (73,)
    up = BB.upload("build", "cpu")
    assert up is BB.upload(BB.Backbone(), "cpu") and up.spec == b and up.table.dtype == torch.float32 and np.array_equal(up.table.numpy(), d["table"])
    assert BB.ATOMS == tuple(PL.RESIDUE_ATOMS[:5]) == ("N", "CA", "C", "CB", "O")
    assert "Nothing is claimed about accuracy on real proteins" in PL.generate_samples.__doc__ and "WHAT IS CLAIMED" in BB.__doc__
    x, m = torch.zeros(2, 5, 3), torch.ones(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        BB.build(x, m, m)
    with pytest.raises(ValueError, match="float32"):
        BB.build(x.double(), m, m)
    with pytest.raises(ValueError, match=r"\[S,N,3\]"):
        BB.build(torch.zeros(5, 3), m, m)


# ---- the yardstick on its own ---------------------------------------------------------------------------------------------------------------

def _anchor(phi, psi, L=12):
    ch = BB.ideal_chain([phi] * L, [psi] * L)
    r = BR.build(ch[None, :, 1], ONES(L), ONES(L))
    assert (r["built"] == 31).all() and not r["ambiguous"].any()
    return ch, r["atoms"][0]


def test_anchor_chains_are_rebuilt_to_the_stated_accuracy_ends_included():
    worst = 0.0
    for phi, psi in BB.ANCHORS:
        ch, got = _anchor(phi, psi)
        err = np.linalg.norm(got - ch, axis=-1)                 # [L,5]
        e = {k: BR.rms(got[:, k], ch[:, k]) for k in (BR.N_, BR.C_, BR.O_)}
        print((phi, psi), {BB.ATOMS[k]: round(v, 4) for k, v in e.items()})
        assert e[BR.N_] < 0.02 and e[BR.C_] < 0.02 and e[BR.O_] < 0.1 and err[:, BR.CA_].max() == 0.0
        worst = max(worst, e[BR.O_])
        # the dyad continuation is exact on a regular chain: the terminal N and the terminal C, O are no worse than the interior
        assert err[0, BR.N_] <= err[2:-2, BR.N_].max() + 1e-9 and err[-1, BR.C_] <= err[2:-2, BR.C_].max() + 1e-9
        assert err[-1, BR.O_] <= err[2:-2, BR.O_].max() + 1e-9 and err[1, BR.N_] <= err[2:-2, BR.N_].max() + 1e-9
        assert BR.rms(got[:, BR.CB_], ch[:, BR.CB_]) < 0.05
    assert 0.05 < worst < 0.07                                  # 0.059 on the antiparallel strand: the table's 5-degree sampling
    # off the anchors the table interpolates between six knots, and the carbonyl oxygen is off by about an Angstrom: nothing else is claimed
    ch, got = _anchor(-90.0, 90.0)
    assert 1.0 < BR.rms(got[:, BR.O_], ch[:, BR.O_]) < 1.3 and BR.rms(got[:, BR.N_], ch[:, BR.N_]) < 0.3


def test_the_peptide_keeps_its_bond_lengths_is_planar_and_the_residues_are_l_on_either_hand():
    rng = np.random.default_rng(5)
    g = BB.Geometry()
    for _ in range(4):
        ca = BR.chain(rng, 40)[:, BR.CA_]           # |b| = L0 on every virtual bond
        for x in (ca, BR.mirror(ca)):
            r = BR.build(x[None], ONES(40), ONES(40))
            a = r["atoms"][0]
            assert (r["built"] == 31).all()
            n, c, o = a[:, BR.N_], a[:, BR.C_], a[:, BR.O_]
            norm = lambda v: np.linalg.norm(v, axis=-1)          # noqa: E731
            s = np.array(BB.Backbone().scalars()[:7], np.float64)    # the fp32-rounded plane the yardstick is handed
            assert np.allclose(norm(n - x), math.hypot(s[5], s[6]), atol=1e-9) and abs(math.hypot(s[5], s[6]) - g.n_ca) < 1e-6
            assert np.allclose(norm(c - x), math.hypot(s[1], s[2]), atol=1e-9) and abs(math.hypot(s[1], s[2]) - g.ca_c) < 1e-6
            assert np.allclose(norm(n[1:] - c[:-1]), g.c_n, atol=1e-6) and np.ptp(norm(n[1:] - c[:-1])) < 1e-9
            assert np.allclose(norm(o - c), g.c_o, atol=1e-6) and np.ptp(norm(o - c)) < 1e-9
            omega = np.degrees(BR.dihedral(x[:-1], c[:-1], n[1:], x[1:]))
            assert np.allclose(np.abs(omega), 180.0, atol=1e-6)
            assert (BR.cb_volume(a) > 0).all()                  # L-residues on the trace AND on its mirror image
            angle = np.degrees(np.arccos(((n - x) * (c - x)).sum(-1) / (norm(n - x) * norm(c - x))))
            assert 75.0 < angle.min() and angle.max() < 155.0   # N-CA-C is whatever the trace makes it: no claim, a sanity bound


def test_rotating_and_translating_the_trace_rotates_and_translates_the_atoms():
    rng = np.random.default_rng(6)
    ca = BR.chain(rng, 30)[:, BR.CA_] + 0.2 * rng.normal(size=(30, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q *= np.sign(np.linalg.det(q))
    t = rng.uniform(-20, 20, 3)
    a = BR.build(ca[None], ONES(30), ONES(30))
    b = BR.build((ca @ q.T + t)[None], ONES(30), ONES(30))
    on = BR.flags(a["built"])
    assert np.array_equal(a["built"], b["built"]) and on[0, :, BR.CA_].all() and on.sum() > 100
    assert np.abs(np.where(on[..., None], a["atoms"] @ q.T + t - b["atoms"], 0.0)).max() < 1e-9


def _helix(L, bonds=None, thetas=None, taus=None):
    bonds = np.full(max(L - 1, 0), 3.8) if bonds is None else bonds
    thetas = np.radians(np.full(max(L - 2, 0), 90.37)) if thetas is None else thetas
    taus = np.radians(np.full(max(L - 3, 0), 50.04)) if taus is None else taus
    return CR.nerf(bonds, thetas, taus)


def test_runs_shorter_than_four_are_left_alone_and_a_run_of_four_is_built_whole():
    x = np.concatenate([_helix(n) + [30.0 * k, 0.0, 0.0] for k, n in enumerate((1, 2, 3, 4))])
    link = np.array([0, 1, 0, 1, 1, 0, 1, 1, 1, 0], np.float64)
    r = BR.build(x[None], ONES(10), link)
    assert r["built"][0].tolist() == [2] * 6 + [31] * 4 and not r["ambiguous"].any()
    assert np.array_equal(r["atoms"][0, :, BR.CA_], x) and not r["atoms"][0, :6, [0, 2, 3, 4]].any() and np.abs(r["atoms"][0, 6:]).sum(-1).min() > 0
    # the mask ends a run as a link does, and an unmasked row is zeros altogether
    x = _helix(9)
    mask = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1], np.float64)
    r = BR.build(x[None], mask, ONES(9))
    assert r["built"][0].tolist() == [2, 2, 2, 0, 31, 31, 31, 31, 31] and not r["atoms"][0, 3].any()
    # link[N-1] is never a bond
    assert np.array_equal(BR.build(x[None], ONES(9), np.r_[np.ones(8), 0.0])["built"], BR.build(x[None], ONES(9), ONES(9))["built"])


def test_a_long_bond_or_a_straight_vertex_unbuilds_exactly_the_atoms_the_header_says():
    L = 12
    bonds = np.full(L - 1, 3.8)
    bonds[5] = 4.4                                              # between rows 5 and 6: peptides 4, 5 and 6
    r = BR.build(_helix(L, bonds=bonds)[None], ONES(L), ONES(L))
    assert r["built"][0].tolist() == [31, 31, 31, 31, 3, 2, 2, 22, 31, 31, 31, 31] and not r["ambiguous"].any()
    thetas = np.radians(np.full(L - 2, 90.37))
    thetas[5] = math.radians(175.0)                             # the vertex at row 6: peptides 5 and 6
    r = BR.build(_helix(L, thetas=thetas)[None], ONES(L), ONES(L))
    assert r["built"][0].tolist() == [31] * 5 + [3, 2, 22] + [31] * 4 and not r["ambiguous"].any()
    thetas = np.radians(np.full(L - 2, 90.37))
    thetas[0] = math.radians(175.0)                             # the vertex at row 1: P_-1 and P_-2 are undefined, and peptides -1, 0, 1 with them
    r = BR.build(_helix(L, thetas=thetas)[None], ONES(L), ONES(L))
    assert r["built"][0].tolist() == [2, 2, 22] + [31] * 9
    thetas = np.radians(np.full(L - 2, 90.37))
    thetas[-1] = math.radians(5.0)                              # folded back at row L-2: the mirror image at the other end
    r = BR.build(_helix(L, thetas=thetas)[None], ONES(L), ONES(L))
    assert r["built"][0].tolist() == [31] * 9 + [3, 2, 2]
    # the thresholds are keywords: a window that admits 4.4 Angstrom builds everything again; so does the angle
    wide = BB.Backbone(bond=(3.3, 4.5))
    assert (BR.build(_helix(L, bonds=bonds)[None], ONES(L), ONES(L), wide)["built"] == 31).all()
    thetas[-1] = math.radians(175.0)
    assert (BR.build(_helix(L, thetas=thetas)[None], ONES(L), ONES(L), BB.Backbone(min_angle=2.0))["built"] == 31).all()
    # a comparison on the edge is reported as ambiguous
    bonds[5] = 4.3
    r = BR.build(_helix(L, bonds=bonds)[None], ONES(L), ONES(L))
    assert r["ambiguous"][0].tolist() == [False] * 4 + [True] * 4 + [False] * 4


def test_the_inputs_of_the_gpu_tests_keep_clear_of_the_edges_and_state_the_tolerance():
    """what tests/test_backbone.py relies on, checked here without a device: no ambiguous comparison in the exact family, at most 0.5 %
    of the residues in the perturbed one, coordinates within 100 Angstrom, vertices of at least 20 degrees in the exact family, and E --
    the deviation of the float32 restatement from the float64 one on these very inputs -- no larger than the stated one"""
    seen = set()
    for case in BR.CASES:
        N, S, na, layout, _ = case
        I = BR.case_inputs(case)
        r = I["ref"]
        assert np.abs(I["x"]).max() <= 100.0 and I["mask"][:na].sum() == 0 and I["mask"][na:].all()
        lengths, _ = BR.run_lengths(layout, na, N)
        assert sum(lengths) == N - na
        seen |= {min(n, 4) for n in lengths}
        for s in range(S):
            if s in I["exact"]:
                assert not r["ambiguous"][s].any(), (case, s)
                assert np.array_equal(I["f32"]["built"][s], r["built"][s])
                x = I["x"][s].astype(np.float64)
                u, v = x[:-2] - x[1:-1], x[2:] - x[1:-1]
                inside = (I["link"][:-2] > 0.5) & (I["link"][1:-1] > 0.5) & (np.linalg.norm(u, axis=1) < 4.3) & (np.linalg.norm(v, axis=1) < 4.3)
                cos = (u * v).sum(1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
                assert inside.sum() == 0 or (np.degrees(np.arccos(cos[inside])).min() >= 20.0 and np.degrees(np.arccos(cos[inside])).max() <= 160.0)
            else:
                assert r["ambiguous"][s].sum() <= BR.CAP * (N - na), (case, s)
        if layout == "tileA":
            assert I["link"][BR.TILE - 1] == 0 and I["link"][BR.TILE - 2] == 1 and (N <= BR.TILE + 3 or I["link"][BR.TILE] == 1)
        if layout == "tileB":
            assert I["link"][BR.TILE] == 0 and I["link"][BR.TILE - 1] == 1 and I["link"][BR.TILE + 1] == 1
    assert seen == {1, 2, 3, 4}
    assert sorted({c[0] for c in BR.CASES}) == [1, 3, 4, 5, 7, 8, 255, 256, 257, 259, 1100] and {c[1] for c in BR.CASES} == {1, 5, 7}
    assert {c[2] for c in BR.CASES} == {0, 3, 17} and any(c[4] for c in BR.CASES)
    built = np.concatenate([BR.case_inputs(c)["ref"]["built"].ravel() for c in BR.CASES])
    assert {0, 2, 3, 22, 31} <= set(built.tolist())             # every kind of residue occurs
    e = BR.measured_E()
    print("E (exact, perturbed) =", e, "allowed on the device:", tuple(4 * v for v in BR.E))
    assert all(0.5 * stated <= got <= stated for got, stated in zip(e, BR.E)), (e, BR.E)


# ---- pipeline.generate_samples(backbone=...) ------------------------------------------------------------------------------------------------

def _yardstick_build(x, mask, link, spec=None):
    """backbone.build restated on the host for the stub path (the real one is a launch)"""
    spec = spec.spec if isinstance(spec, BB.Uploaded) else BB.Backbone.of("build" if spec is None else spec)
    r = BR.build(x.numpy(), mask.numpy(), link.numpy(), spec)
    return BB.Built(torch.from_numpy(r["atoms"].astype(np.float32)), torch.from_numpy(r["built"]))


def test_generate_samples_refuses_before_the_model_is_touched():
    data, _ = CR.complex_and_samples()
    with pytest.raises(ValueError, match="'build' or a backbone.Backbone, got 'full'"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, backbone="full")
    with pytest.raises(TypeError, match="backbone.Backbone, got bool"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, backbone=True)
    # with a scaffold nothing is refused: the next thing that fails is the model itself
    with pytest.raises(AssertionError, match="the model was touched"):
        PL.generate_samples(_NoDevice(), data, num_samples=2, backbone="build", scaffold=Scaffold())
    assert inspect.signature(PL.generate_samples).parameters["backbone"].default is None


def _records(pdb_text):
    """[model][(residue number, residue name)] -> atom names in file order"""
    models = []
    for line in pdb_text.splitlines():
        if line.startswith("MODEL"):
            models.append({})
        elif line.startswith("ATOM"):
            models[-1].setdefault((int(line[22:26]), line[17:20]), []).append(line[12:16].strip())
    return models


def test_generate_samples_builds_last_returns_and_writes_with_the_launches_restated_on_the_host(tmp_path, monkeypatch):
    """the whole path of the keyword on the CPU; tests/test_backbone.py runs it with the launches themselves"""
    log = []
    for (module, name), fake in fakes(log).items():
        monkeypatch.setattr(module, name, fake)
    monkeypatch.setattr(CH, "census", _yardstick_census)
    monkeypatch.setattr(CH, "reflect", _host_reflect)
    monkeypatch.setattr(BB, "build", _yardstick_build)
    data, samples = CR.complex_and_samples()
    NA, NR = CR.NA, CR.NR
    kw = dict(num_samples=6, batch_size=4, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "plain", **kw)
        again = PL.generate_samples(CR.Prepared(samples, "cpu"), data, backbone=None, **kw)
        before = PL.generate_samples(CR.Prepared(samples, "cpu"), data, handedness="fix", align_to="input", **kw)
        full = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "full", handedness="fix", align_to="input", backbone="build", **kw)
    # nothing changed without the keyword
    assert len(plain) == len(again) == 4 and sorted(os.listdir(tmp_path / "plain")) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    assert np.array_equal(plain[0], again[0]) and np.array_equal(plain[1], again[1])
    assert all(np.array_equal(a.atom_pos, b.atom_pos) and np.array_equal(a.atom_mask, b.atom_mask) for a, b in zip(plain[2], again[2]))
    assert all(p.atom_mask[:, 1].all() and p.atom_mask.sum() == NR for p in plain[2])
    # the keyword adds one trailing dict and changes no earlier element but the proteins
    assert len(before) == 6 and len(full) == 7
    assert np.array_equal(full[0], before[0]) and np.array_equal(full[1], before[1]) and np.array_equal(np.stack(full[3]), np.stack(before[3]))
    assert all(np.array_equal(full[4][k], before[4][k]) for k in before[4]) and all(np.array_equal(full[5][k], before[5][k], equal_nan=True) for k in before[5])
    d = full[6]
    assert sorted(d) == sorted(["atoms", "built", "unbuilt_residues", "table", "L0", "plane_C", "plane_O", "plane_N", "cb", "bond", "min_angle"])
    assert d["atoms"].shape == (6, NR, 5, 3) and d["atoms"].dtype == np.float32 and d["built"].shape == (6, NR, 5) and d["built"].dtype == bool
    assert d["unbuilt_residues"].shape == (6,) and np.array_equal(d["table"], BB.Backbone().orientation.table())
    # the ordering: the atoms are the builder applied to the RETURNED positions -- after the fix (samples 2, 3 and 5 were reflected) and
    # after align_to (every sample was moved) -- not to the samples as drawn
    assert full[5]["flipped"].tolist() == [False, False, True, True, False, True] and np.abs(full[0] - samples).max() > 1.0
    mask, link = np.r_[np.zeros(NA), np.ones(NR)], np.r_[np.zeros(NA), np.ones(NR - 1), 0.0]
    want = BR.build(full[0], mask, link)
    assert np.array_equal(d["atoms"], want["atoms"][:, NA:].astype(np.float32)) and np.array_equal(d["built"], BR.flags(want["built"])[:, NA:])
    drawn = BR.build(samples, mask, link)
    assert np.abs(d["atoms"] - drawn["atoms"][:, NA:]).max() > 1.0
    assert np.array_equal(d["atoms"][:, :, 1], full[0][:, NA:])
    # the four helices are right-handed now and built whole; the random walks' steps are not chain steps
    assert d["built"][:4].all() and d["unbuilt_residues"].tolist()[:4] == [0] * 4 and (d["unbuilt_residues"][4:] > NR // 2).all()
    assert (BR.cb_volume(d["atoms"].astype(np.float64))[d["built"][:, :, 3]] > 0).all()
    tau = np.degrees(BR.dihedral(*(full[0][:4, NA + k: NA + NR - 3 + k].astype(np.float64) for k in range(4))))
    assert np.allclose(tau, 50.04, atol=0.1)
    # the proteins: N, CA, C, CB, O in atom37 slots 0 .. 4, no CB on a residue decoded as G or left undetermined
    gly = PL.RESIDUE_TYPES.index("G")
    no_cb = 0
    for k, prot in enumerate(full[2]):
        skip = np.isin(prot.aatype, [gly, -1])
        no_cb += int((skip & d["built"][k][:, 3]).sum())
        have = d["built"][k].copy()
        have[:, 3] &= ~skip
        have[:, 1] = True
        assert np.array_equal(prot.atom_mask[:, :5] > 0.5, have) and not prot.atom_mask[:, 5:].any()
        assert np.array_equal(prot.atom_pos[:, :5][have], d["atoms"][k][have]) and not prot.atom_pos[:, :5][~have].any()
        assert np.array_equal(prot.aatype, before[2][k].aatype)
    assert no_cb >= 3                                           # the decoded sequences do hold glycines / undetermined residues on built rows
    # the files: sample_backbone.npz, and the PDB with the atom order N, CA, C, CB, O
    assert sorted(os.listdir(tmp_path / "full")) == ["sample_alignment.npz", "sample_backbone.npz", "sample_handedness.npz", "sample_handedness.txt",
                                                      "sample_ligand_pos.npy", "sample_protein.pdb", "sample_tmscores.txt"]
    with np.load(tmp_path / "full" / "sample_backbone.npz") as z:
        assert sorted(z.files) == sorted(d) and all(np.array_equal(z[k], d[k]) for k in z.files)
    models = _records((tmp_path / "full" / "sample_protein.pdb").read_text())
    assert len(models) == 6
    for k, model in enumerate(models):
        assert len(model) == NR
        for (_, resn), names in model.items():
            assert names in (["CA"], ["N", "CA"], ["N", "CA", "C", "O"], ["N", "CA", "C", "CB", "O"], ["CA", "C", "O"]), names
            assert not (resn in ("GLY", "UNK") and "CB" in names)
        if k < 4:
            assert all(len(names) == (4 if resn in ("GLY", "UNK") else 5) for (_, resn), names in model.items())
    plain_models = _records((tmp_path / "plain" / "sample_protein.pdb").read_text())
    assert all(names == ["CA"] for model in plain_models for names in model.values())
    # the stage ran once, after the superposition
    assert [e[0] for e in log if e[0].startswith("align.")] == ["align.superimpose", "align.diversity", "align.apply"] * 2       # `before` and `full`


def test_the_stage_warns_without_handedness_and_takes_an_input_without_coordinates(monkeypatch):
    monkeypatch.setattr(CH, "census", _yardstick_census)
    monkeypatch.setattr(BB, "build", _yardstick_build)
    data, samples = CR.complex_and_samples()
    kw = dict(num_samples=6, batch_size=4, seed=3)
    with pytest.warns(UserWarning, match="L-residues on a D-trace") as caught:
        out = PL.generate_samples(CR.Prepared(samples, "cpu"), data, backbone="build", **kw)
    assert sum("D-trace" in str(w.message) for w in caught) == 1 and len(out) == 5
    # without the fix the mirror-image helices are built as they are: L-residues on a left-handed helix
    d = out[4]
    assert d["built"][:4].all() and (BR.cb_volume(d["atoms"].astype(np.float64))[:4] > 0).all()
    assert np.array_equal(d["atoms"][:, :, 1], samples[:, CR.NA:])
    with warnings.catch_warnings():
        warnings.simplefilter("error", UserWarning)
        warnings.filterwarnings("ignore", message="samples .* decode to 'X'")
        quiet = PL.generate_samples(CR.Prepared(samples, "cpu"), data, backbone=BB.Backbone(bond=(3.0, 4.5)), handedness="report", **kw)
    assert len(quiet) == 6 and np.array_equal(quiet[5]["bond"], [3.0, 4.5]) and np.array_equal(quiet[5]["built"][:4], d["built"][:4])
    # a protein from its sequence alone (no coordinates anywhere in the input) is fine
    bare = dict(data, atom_pos=torch.zeros(CR.NA, 3), residue_atom_pos=torch.zeros(CR.NR, 37, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        same = PL.generate_samples(CR.Prepared(samples, "cpu"), bare, backbone="build", **kw)[4]
    assert np.array_equal(same["atoms"], d["atoms"]) and np.array_equal(same["built"], d["built"])
