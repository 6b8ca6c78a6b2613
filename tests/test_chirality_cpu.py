"""CPU: the handedness census as far as it goes without a GPU -- the yardstick tests/chirality_ref.py on hand-made chains and the inputs of
the GPU tests, the header / build / export list of libprd_chirality.so and its host refusals, the host helpers on hand-made batches, the
specs, and the ``handedness=`` keyword of pipeline.generate_samples: its refusals, and its whole path with the two launches replaced by
the float64 yardstick."""
import ctypes
import math
import os
import warnings

import numpy as np
import pytest
import torch

import chirality_ref as CR
from conftest import ROOT
from protein_redesign_amd import _lib, build
from protein_redesign_amd import chirality as CH
from protein_redesign_amd import pipeline as PL
from protein_redesign_amd.conditioning import Scaffold
from protein_redesign_amd.synthetic import synthetic_batch, synthetic_sample
from sample_stubs import _NoDevice, header_entries

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
SOURCE = os.path.join(ROOT, "protein_redesign_amd", "csrc", "prd_chirality.hip")


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------

def test_the_ideal_helix_has_the_stated_virtual_geometry_and_its_mirror_image_the_negated_dihedral():
    for hand in (1.0, -1.0):
        x = CR.ideal_helix(12, hand)
        c = CR.census(x[None], np.ones(12), np.ones(12))
        assert np.allclose(np.degrees(c["tau"][0, :9]), hand * 50.04, atol=0.005) and np.isnan(c["tau"][0, 9:]).all()
        assert np.allclose(np.linalg.norm(np.diff(x, axis=0), axis=1), 3.83, atol=0.005)
        b = np.diff(x, axis=0)
        cos = -(b[:-1] * b[1:]).sum(1) / 3.83 ** 2
        assert np.allclose(np.degrees(np.arccos(cos)), 90.37, atol=0.05)
        assert c["counts"][0].tolist() == ([9, 0] if hand > 0 else [0, 9]) + [0, 0, 9, 0, 0, 0] and (c["verdict"][0], c["basis"][0]) == (hand, 1)
        assert c["classes"][0].tolist() == [1 if hand > 0 else 2] * 9 + [0] * 3
    # an ideal sp3 centre with 1.5 Angstrom bonds
    assert abs(abs(CR.signed_volume(CR.TETRA, [[0, 1, 2, 3]])[0]) - 2.598) < 1e-3
    assert np.allclose(np.linalg.norm(CR.TETRA[1:], axis=1), 1.5)


def test_nerf_places_the_requested_angles_and_dihedrals():
    rng = np.random.default_rng(0)
    L = 40
    bonds, th, ta = rng.uniform(3.4, 4.2, L - 1), np.radians(rng.uniform(70, 150, L - 2)), np.radians(rng.uniform(-179, 179, L - 3))
    x = CR.nerf(bonds, th, ta)
    c = CR.census(x[None], np.ones(L), np.ones(L), bond=(3.0, 5.0))
    assert np.allclose(c["tau"][0, :L - 3], ta, atol=1e-9) and np.allclose(np.linalg.norm(np.diff(x, axis=0), axis=1), bonds)
    b = np.diff(x, axis=0)
    cos = -(b[:-1] * b[1:]).sum(1) / (bonds[:-1] * bonds[1:])
    assert np.allclose(np.arccos(cos), th, atol=1e-9)
    # the strands of the inputs: tau = -165 degrees is the native twist, +165 its mirror image
    for kind, col in (("ext_n", 2), ("ext_m", 3), ("helix_r", 0), ("helix_l", 1)):
        s = CR.segment(rng, 20, (kind,), ideal=True)
        assert CR.census(s[None], np.ones(20), np.ones(20))["counts"][0].tolist() == [17 if k in (col, 4) else 0 for k in range(8)]


def test_edges_on_a_window_are_strict_and_the_three_counts_bracket_them():
    e = CR.edges_f32()
    assert np.allclose(e, [math.cos(math.radians(110)), math.cos(math.radians(75)), math.radians(30), math.radians(80),
                           math.cos(math.radians(150)), math.cos(math.radians(105)), math.radians(120), math.radians(180)], atol=1e-7)
    assert list(CH.Windows().edges()) == e                      # the module's own statement, computed independently
    for tau, want, amb in ((30.0, 0, 1), (30.01, 1, 0), (79.99, 1, 0), (80.0, 0, 1), (100.0, 0, 0)):
        # the fp32 edge lies a few 1e-8 beside the double 30 / 80 degrees: inside the band either way
        x = CR.nerf(np.full(3, 3.8), np.radians([90.0, 90.0]), np.radians([tau]))
        c = CR.census(x[None], np.ones(4), np.ones(4))
        assert c["counts_lo"][0, 0] <= c["counts"][0, 0] <= c["counts_hi"][0, 0] and c["ambiguous"][0] == amb, tau
        if not amb:
            assert c["counts"][0, 0] == want == c["counts_lo"][0, 0] == c["counts_hi"][0, 0], tau
        else:
            assert (c["counts_lo"][0, 0], c["counts_hi"][0, 0]) == (0, 1), tau
    # a bond exactly on the window, a mask and a link switch a quad off
    x = CR.nerf(np.array([3.8, 4.3, 3.8]), np.radians([90.0, 90.0]), np.radians([50.0]))
    c = CR.census(x[None], np.ones(4), np.ones(4))
    assert (c["counts_lo"][0, 4], c["counts_hi"][0, 4], c["ambiguous"][0]) == (0, 1, 1)
    x = CR.ideal_helix(8)
    for mask, link, quads in ((np.ones(8), np.ones(8), 5), (np.r_[np.ones(7), 0], np.ones(8), 4), (np.ones(8), np.r_[0, np.ones(7)], 4),
                              (np.ones(8), np.r_[1, 1, 1, 0, 1, 1, 1, 1], 2), (np.ones(8), np.r_[np.ones(7), 0], 5)):
        assert CR.census(x[None], mask, link)["counts"][0, 4] == quads


def test_the_verdict_rule_on_hand_made_counts():
    rule = CR.verdict_rule
    assert rule([4, 0, 0, 0, 9, 0, 0, 0], False) == (1, 1) and rule([1, 6, 0, 20, 9, 3, 0, 0], True) == (-1, 1)
    assert rule([3, 0, 0, 20, 9, 2, 0, 1], True) == (1, 2) and rule([3, 0, 0, 20, 9, 0, 1, 0], True) == (-1, 2)
    assert rule([3, 0, 0, 20, 9, 2, 0, 0], False) == (-1, 3)                 # kept / inverted without a reference are never counted
    assert rule([3, 0, 14, 2, 9, 1, 1, 0], True) == (1, 3) and rule([2, 2, 13, 2, 9, 0, 0, 5], True) == (0, 0)
    assert rule([5, 5, 9, 9, 30, 1, 1, 0], True) == (0, 0) and rule([3, 0, 0, 0, 3, 0, 0, 0], False, min_helix=3) == (1, 1)
    assert rule([0, 0, 0, 0, 0, 0, 0, 0], True, min_helix=0, min_extended=0) == (0, 0)      # a tie decides nothing, whatever the minimum


def test_the_inputs_of_the_gpu_tests_keep_clear_of_the_edges_where_they_must():
    """what tests/test_chirality.py asserts per case on the device, here once without one: the chains placed off the edges and every small case
    have no ambiguous comparison; the perturbed ones with 200 quads or more have at most 0.5 %; the mirror image has the swapped counts"""
    big = 0
    for case in CR.CASES:
        I = CR.case_inputs(case)
        r = I["ref"]
        assert np.abs(I["x"]).max() < 200.0
        for s in range(case[1]):
            if s in I["exact"] or r["counts"][s, 4] < 200:
                assert r["ambiguous"][s] == 0 and r["ambiguous_centres"][s] == 0, (case, s)
                assert np.array_equal(r["counts_lo"][s], r["counts"][s]) and np.array_equal(r["counts_hi"][s], r["counts"][s])
            else:
                big += 1
                assert r["ambiguous"][s] <= 0.005 * r["counts_hi"][s, 4], (case, s)
        m = CR.census(CR.mirror(I["x"]), I["mask"], I["link"], I["centres"], I["centre_ref"])
        assert np.array_equal(m["counts"][:, CR.MIRROR_COLUMNS], r["counts"]) and np.array_equal(m["verdict"], -r["verdict"])
        assert np.array_equal(m["tau"], -r["tau"], equal_nan=True)
    assert big >= 1                                             # the 0.5 % cap is exercised
    kinds = {k for case in CR.CASES for k in CR.case_inputs(case)["kinds"]}
    assert kinds == set(CR.KINDS)
    bases = {int(b) for case in CR.CASES for b in CR.case_inputs(case)["ref"]["basis"]}
    assert bases == {0, 1, 2, 3}


# ---- header, build, export list, host refusals ------------------------------------------------------------------------------------------

def test_header_parses_with_the_derived_binding():
    e = header_entries("chirality")
    assert sorted(e) == ["prd_chirality_census", "prd_chirality_reflect", "prd_chirality_version"]
    assert all(x.inject is None and x.restype is _lib.ci for x in e.values())
    vp, ci, cf, cll = _lib.vp, _lib.ci, _lib.cf, _lib.cll
    assert e["prd_chirality_census"].argtypes == [vp] * 7 + [cll, ci] + [vp] * 5 + [ci] + [cf] * 11 + [ci] * 4 + [vp]
    assert e["prd_chirality_reflect"].argtypes == [vp, cll, ci, vp, ci, ci, vp] and e["prd_chirality_version"].argtypes == []
    assert CH.ENTRIES == e and not set(e) & set(_lib.ENTRIES)
    assert CH._DEFINES == {"VERSION": 100, "ERR_ARG": -1, "ERR_UNSUPPORTED": -3, "MAX_N": 32768, "MAX_S": 65535, "MAX_C": 1024, "BASIS_NONE": 0,
                           "BASIS_HELIX": 1, "BASIS_CENTRES": 2, "BASIS_EXTENDED": 3}
    assert CH.ABI_VERSION == 100 and (CH.MAX_N, CH.MAX_S, CH.MAX_C) == (32768, 65535, 1024)
    with open(SOURCE) as f:
        text = f.read()
    assert '#include "prd_launch.h"' in text and "hipLaunchKernelGGL" not in text and "<<<" not in text and "asm" not in text
    assert "atomic" not in text and "getenv" not in text and "hipMalloc" not in text and "Synchronize" not in text
    assert text.count("prd_launch<") == 2                       # one kernel per entry point
    with open(os.path.join(ROOT, "include", "prd_chirality.h")) as f:
        head = f.read()
    assert head.lstrip().startswith("/* libprd_chirality.so") and "Verdict" in head and "WHO VALIDATES THE ROWS" in head


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_resources_of_the_two_kernels():
    import re
    mine = build.resource_usage(sources=build.SIDE_LIBS["chirality"].sources)
    assert sorted(mine) == ["chirality_census_kernel", "chirality_reflect_kernel"]
    assert all(u["scratch"] == 0 and u["agprs"] == 0 for u in mine.values())
    with open(SOURCE) as f:
        stated = int(re.search(r"constexpr int CH_LDS_BYTES = (\d+);", f.read()).group(1))
    assert mine["chirality_census_kernel"]["lds"] == stated == (256 + 3) * 16 + (256 + 4) * 4 + 4 * 8 * 4 and mine["chirality_reflect_kernel"]["lds"] == 0
    assert mine["chirality_census_kernel"]["vgprs"] <= 64


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_library_refuses_on_the_host_before_any_device_call():
    """every refusal of prd_chirality.h is host code that runs before the first HIP call: reachable without a GPU, with device pointers that
    are never followed.  The centre rows are validated by the LIBRARY, on the host copy the caller passes beside the device list."""
    build.build_side("chirality", verbose=False)
    L, D = CH.lib(), CH._DEFINES
    assert L.prd_chirality_version() == 100
    p = ctypes.c_void_p(4096)
    inf, nan = float("inf"), float("nan")
    host = (ctypes.c_int * 8)(1, 0, 2, 3, 4, 3, 2, 1)
    E = dict(zip(("hcl", "hch", "htl", "hth", "ecl", "ech", "etl", "eth"), CR.edges_f32()))
    names = ("counts", "verdict", "basis", "tau", "cls", "volume")

    def census(xs=30, xr=3, x=p, mask=p, link=p, centres=p, chost=host, cref=p, C=2, lo=3.3, hi=4.3, vmin=0.5, mh=4, me=12, S=2, N=5, **kw):
        out = [kw.pop(n, p) for n in names]
        e = dict(E, **kw)
        return L.prd_chirality_census(*out, x, xs, xr, mask, link, centres, chost, cref, C, e["hcl"], e["hch"], e["htl"], e["hth"], e["ecl"], e["ech"],
                                      e["etl"], e["eth"], lo, hi, vmin, mh, me, S, N, None)
    bad = [dict(counts=None), dict(verdict=None), dict(basis=None), dict(x=None), dict(mask=None), dict(link=None), dict(S=0), dict(N=0), dict(S=-1),
           dict(N=-4), dict(C=-1), dict(xr=2), dict(xs=-1), dict(centres=None), dict(chost=None),
           dict(hcl=nan), dict(hch=inf), dict(htl=-inf), dict(eth=nan), dict(hcl=0.5, hch=0.2), dict(hcl=0.3, hch=0.3), dict(htl=1.4, hth=0.5),
           dict(ecl=-1.5), dict(ech=1.5), dict(etl=-0.1), dict(eth=3.2), dict(etl=2.5, eth=2.5),
           dict(lo=4.3, hi=3.3), dict(lo=3.8, hi=3.8), dict(lo=0.0), dict(lo=-1.0), dict(lo=nan), dict(hi=inf), dict(hi=nan),
           dict(vmin=0.0), dict(vmin=-0.5), dict(vmin=nan), dict(vmin=inf), dict(mh=-1), dict(me=-1),
           dict(chost=(ctypes.c_int * 8)(1, 0, 2, 3, 4, 3, 2, 5)), dict(chost=(ctypes.c_int * 8)(1, 0, -1, 3, 4, 3, 2, 1)),
           dict(chost=(ctypes.c_int * 8)(1, 0, 2, 3, 4, 3, 2, 1), N=4)]
    for kw in bad:
        assert census(**kw) == D["ERR_ARG"], kw
    for kw in (dict(N=CH.MAX_N + 1), dict(S=CH.MAX_S + 1), dict(C=CH.MAX_C + 1)):
        assert census(**kw) == D["ERR_UNSUPPORTED"], kw

    def reflect(x=p, xs=30, xr=3, flip=p, S=2, N=5):
        return L.prd_chirality_reflect(x, xs, xr, flip, S, N, None)
    for kw in (dict(x=None), dict(flip=None), dict(S=0), dict(N=0), dict(N=-1), dict(xr=2), dict(xs=-3)):
        assert reflect(**kw) == D["ERR_ARG"], kw
    for kw in (dict(N=CH.MAX_N + 1), dict(S=CH.MAX_S + 1)):
        assert reflect(**kw) == D["ERR_UNSUPPORTED"], kw
    # the launch geometry the bounds promise: the census grid is S, the reflection's (N / 256, S); every output index fits size_t
    assert CH.MAX_S <= 65535 and CH.MAX_N * 3 < 2 ** 31


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_host_side_of_the_library_under_address_sanitizer():
    """the same refusals from a stand-alone C program (tests/native/chirality_abi_check.c) against the library's host code built with
    AddressSanitizer: the walk over the caller's host copy of the centre list stays inside its 4 * C ints.  Needs hipcc only (no GPU)."""
    import subprocess
    exe = build.build_side_check("chirality", verbose=False)
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    text = out.stdout.decode(errors="replace")
    assert out.returncode == 0 and "chirality_abi_check OK" in text and "AddressSanitizer" not in text and "FAIL" not in text, text[-2000:]
    assert os.path.dirname(exe) == build.VARIANTS["asan"].objdir and os.path.exists(build.SIDE_LIBS["chirality"].lib.replace(".so", "_asan.so"))


# ---- the specs and the python-side checks-------------------------------------------------------------------------------------------------

def test_windows_and_handedness_are_validated_and_immutable():
    w = CH.Windows()
    assert (w.helix_theta, w.helix_tau, w.extended_theta, w.extended_tau) == ((75.0, 110.0), (30.0, 80.0), (105.0, 150.0), (120.0, 180.0))
    with pytest.raises(Exception):
        w.helix_tau = (1.0, 2.0)
    for kw, what in ((dict(helix_tau=(80, 30)), "helix_tau"), (dict(helix_theta=(75, float("nan"))), "helix_theta"), (dict(extended_tau=(120, 181)), "extended_tau"),
                     (dict(extended_theta=5), "extended_theta"), (dict(helix_tau=(-30, 30)), "helix_tau")):
        with pytest.raises(ValueError, match=what):
            CH.Windows(**kw)
    h = CH.Handedness()
    assert (h.fix, h.windows, h.bond, h.vmin, h.min_helix, h.min_extended) == (False, w, (3.3, 4.3), 0.5, 4, 12)
    assert CH.Handedness.of("report") == h and CH.Handedness.of("fix") == CH.Handedness(fix=True) and CH.Handedness.of(h) is h
    assert h.thresholds() == dict(windows=w, bond=(3.3, 4.3), vmin=0.5, min_helix=4, min_extended=12)
    with pytest.raises(Exception):
        h.fix = True
    with pytest.raises(ValueError, match="'report', 'fix'"):
        CH.Handedness.of("mirror")
    for bad in (True, 1, dict(fix=True), ("fix",)):
        with pytest.raises(TypeError, match="chirality.Handedness"):
            CH.Handedness.of(bad)
    for kw, what in ((dict(fix="yes"), "fix must"), (dict(windows=(75, 110)), "windows must"), (dict(bond=(4.3, 3.3)), "bond must"), (dict(bond=(0, 1)), "bond must"),
                     (dict(vmin=0), "vmin must"), (dict(vmin=float("inf")), "vmin must"), (dict(min_helix=-1), "min_helix"), (dict(min_extended=1.5), "min_extended"),
                     (dict(min_helix=True), "min_helix")):
        with pytest.raises(ValueError, match=what):
            CH.Handedness(**kw)
    # the documented defaults are quality.assess's chain-step window
    from protein_redesign_amd import quality
    assert CH.BOND == (quality.CA_STEP - quality.CA_STEP_TOLERANCE, quality.CA_STEP + quality.CA_STEP_TOLERANCE)
    assert CH.COUNT_COLUMNS == CR.COLUMNS and list(CH.MIRROR_COLUMNS) == CR.MIRROR_COLUMNS and CH.BASIS == {0: "none", 1: "helix", 2: "centres", 3: "extended"}
    assert "Nothing is claimed" in PL.generate_samples.__doc__ and "fitted to nothing" in CH.__doc__


def test_host_argument_checks_of_the_python_side():
    x, m = torch.zeros(2, 5, 3), torch.ones(5)
    with pytest.raises(RuntimeError, match="GPU only"):
        CH.census(x, m, m)
    with pytest.raises(RuntimeError, match="GPU only"):
        CH.reflect(x, torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="float32"):
        CH.census(x.double(), m, m)
    with pytest.raises(ValueError, match=r"\[S,N,3\]"):
        CH.census(torch.zeros(5, 3), m, m)
    for kw, what in ((dict(vmin=0.0), "vmin"), (dict(bond=(1.0,)), "bond"), (dict(min_helix=-2), "min_helix"), (dict(windows="wide"), "windows")):
        with pytest.raises(ValueError, match=what):
            CH.census(x, m, m, **kw)
    with pytest.raises(ValueError, match="PRD_CHIRALITY_MAX_C"):
        CH.upload(np.zeros((CH.MAX_C + 1, 4), np.int64), "cpu")
    listed = CH.upload([[1, 0, 2, 3]], "cpu")
    assert listed.host.dtype == listed.device.dtype == torch.int32 and listed.host.tolist() == [[1, 0, 2, 3]]


# ---- the host helpers on hand-made batches --------------------------------------------------------------------------------------------------

def test_trace_links_follow_chains_gaps_and_unmarked_c_alphas():
    batch = synthetic_batch([(4, 12), (2, 5)], esm_dim=16, seed=0)          # complex 0: two chains of 6; N = 16
    batch["residue_index"][0, 4 + 8:4 + 12] += 1                            # a gap in chain 1 between its residues 2 and 3 (rows 11 | 12)
    batch["residue_atom_mask"][0, 4 + 3, 1] = 0.0                           # an unmarked C-alpha in chain 0
    mask, link = CH.trace_links(batch)
    assert mask.dtype == link.dtype == torch.float32 and mask.shape == link.shape == (16,)
    assert mask.tolist() == [0.0] * 4 + [1, 1, 1, 0, 1, 1] + [1.0] * 6
    #                 ligand    chain 0: rows 4..9, row 7 unmarked; the chain ends at 9    chain 1: rows 10..15, gap after 11
    assert link.tolist() == [0.0] * 4 + [1, 1, 0, 0, 1, 0] + [1, 0, 1, 1, 1, 0]
    m1, l1 = CH.trace_links(batch, 1)
    assert m1.tolist() == [0.0] * 2 + [1.0] * 5 + [0.0] * 9 and l1.tolist() == [0.0] * 2 + [1.0] * 4 + [0.0] * 10      # one chain (nr < 8), padded rows
    same = CH.trace_links(batch, 0, num_atoms=4, num_residues=12)
    assert torch.equal(same[0], mask) and torch.equal(same[1], link)
    with pytest.raises(ValueError, match="do not fit"):
        CH.trace_links(batch, 0, num_atoms=4, num_residues=13)
    # the mask is quality.assess's, the link its chain-step condition
    ca = batch["residue_atom_mask"][0, :, 1] > 0.5
    ri, ch = batch["residue_index"][0], batch["residue_chain_index"][0]
    step = ca[1:] & ca[:-1] & (ch[1:] == ch[:-1]) & (ri[1:] - ri[:-1] == 1)
    step[:4] = False                                                        # ligand rows: residue_atom_mask is zero there already
    assert torch.equal(link[:-1] > 0.5, step)


def _ligand_batch():
    """7 ligand atoms: atom 0 tagged with neighbours 1, 2, 3, 4 (four), atom 5 tagged with neighbours 2, 4, 6 (three), atom 6 tagged with
    neighbours 5 and -- one-sided in the matrix -- 1 (two: dropped), atom 3 untagged"""
    batch = synthetic_batch([(7, 4)], esm_dim=16, seed=1)
    batch["atom_feats"][0, :, 1] = 0
    batch["atom_feats"][0, [0, 5, 6], 1] = torch.tensor([1, 2, 2])
    bd = torch.full((11, 11), 3, dtype=torch.long)
    bd.fill_diagonal_(0)
    for i, j in ((0, 1), (0, 2), (0, 3), (0, 4), (5, 2), (5, 4), (5, 6)):
        bd[i, j] = bd[j, i] = 1
    bd[1, 6] = 1                                                            # taken as symmetric
    batch["bond_distance"][0] = bd
    return batch


def test_ligand_centres_select_the_tagged_atoms_with_three_neighbours():
    batch = _ligand_batch()
    centres, atoms = CH.ligand_centres(batch)
    assert centres.dtype == torch.int32 and centres.tolist() == [[0, 1, 2, 3], [5, 2, 4, 6]] and atoms.tolist() == [0, 5]
    batch["bond_distance"][0, 6, 3] = 1                                     # a third neighbour: the atom is a centre now, 1 < 3 < 5
    assert CH.ligand_centres(batch)[0].tolist() == [[0, 1, 2, 3], [5, 2, 4, 6], [6, 1, 3, 5]]
    batch["atom_feats"][0, 5, 1] = 3                                        # another tag value selects nothing
    assert CH.ligand_centres(batch)[1].tolist() == [0, 6]
    none = synthetic_batch([(0, 6)], esm_dim=16, seed=1)
    assert CH.ligand_centres(none)[0].shape == (0, 4) and CH.ligand_centres(none)[1].shape == (0,)


def test_centre_reference_rounds_float64_once_and_drops_a_planar_centre():
    pos = np.zeros((11, 3), np.float32)
    pos[[0, 1, 2, 3]] = CR.TETRA.astype(np.float32)
    pos[[5, 4, 6]] = pos[2] + np.array([[1.0, 0, 0], [1.0, 1.0, 0], [0.0, -1.0, 0]], np.float32)            # centre 5 and its neighbours in one plane
    centres = torch.tensor([[0, 1, 2, 3], [5, 2, 4, 6]], dtype=torch.int32)
    kept, vol = CH.centre_reference(pos, centres)
    want = CR.signed_volume(pos.astype(np.float64), centres.numpy())
    assert abs(want[1]) < 1e-6 and kept.tolist() == [[0, 1, 2, 3]] and vol.dtype == torch.float32
    assert vol.tolist() == [float(np.float32(want[0]))] and abs(abs(vol[0].item()) - 2.598) < 1e-3
    loose, vols = CH.centre_reference(torch.from_numpy(pos), centres, vmin=3.0)        # a tetrahedron of 2.6 Angstrom^3 is flat at 3
    assert loose.shape == (0, 4) and vols.shape == (0,)
    mirrored = CH.centre_reference(CR.mirror(pos), centres)[1]
    assert mirrored.tolist() == [-vol[0].item()]
    with pytest.raises(ValueError, match="vmin"):
        CH.centre_reference(pos, centres, vmin=0.0)
    assert np.allclose(CH.signed_volumes(pos, centres), want, rtol=0, atol=1e-12)


# ---- pipeline.generate_samples(handedness=...) ------------------------------------------------------------------------------------------------

def test_generate_samples_refuses_before_the_model_is_touched():
    full = synthetic_sample(5, 9, esm_dim=16, seed=8)
    with pytest.raises(ValueError, match="'report', 'fix' or a chirality.Handedness, got 'mirror'"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, handedness="mirror")
    with pytest.raises(TypeError, match="chirality.Handedness, got bool"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, handedness=True)
    with pytest.raises(TypeError, match="chirality.Handedness, got dict"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, handedness=dict(fix=True))
    for spec in ("fix", CH.Handedness(fix=True)):
        with pytest.raises(ValueError, match="handedness='fix' cannot be combined with a scaffold"):
            PL.generate_samples(_NoDevice(), full, num_samples=2, handedness=spec, scaffold=Scaffold())
    # "report" with a scaffold passes this refusal: the next thing that fails is the model itself
    with pytest.raises(AssertionError, match="the model was touched"):
        PL.generate_samples(_NoDevice(), full, num_samples=2, handedness="report", scaffold=Scaffold())
    import inspect
    assert inspect.signature(PL.generate_samples).parameters["handedness"].default is None
    assert list(inspect.signature(PL.generate_samples).parameters)[-1] == "handedness"


def _yardstick_census(x, mask, link, *, centres=None, centre_ref=None, windows=CH.Windows(), bond=CH.BOND, vmin=CH.VMIN, min_helix=4, min_extended=12):
    """chirality.census restated on the host for the stub path (the real one is a launch)"""
    if centres is not None and not isinstance(centres, CH.Centres):
        centres = CH.upload(centres, "cpu")
    c = CR.census(x.numpy(), mask.numpy(), link.numpy(), None if centres is None else centres.host.numpy(), None if centre_ref is None else centre_ref.numpy(),
                  edges=list(windows.edges()), bond=bond, vmin=vmin, min_helix=min_helix, min_extended=min_extended)
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a).astype(d))         # noqa: E731
    return CH.Census(t(c["counts"], np.int32), t(c["verdict"], np.int32), t(c["basis"], np.int32), t(c["tau"], np.float32), t(c["classes"], np.int32),
                     t(c["volume"], np.float32))


def _host_reflect(x, flip):
    x[flip != 0, :, 0] = -x[flip != 0, :, 0]
    return x


def test_generate_samples_reports_fixes_and_writes_with_the_launches_restated_on_the_host(tmp_path, monkeypatch):
    """the whole path of the keyword on the CPU; tests/test_chirality.py runs it with the launches themselves"""
    monkeypatch.setattr(CH, "census", _yardstick_census)
    monkeypatch.setattr(CH, "reflect", _host_reflect)
    data, samples = CR.complex_and_samples()
    kw = dict(num_samples=6, batch_size=4, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        plain = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "plain", **kw)
        again = PL.generate_samples(CR.Prepared(samples, "cpu"), data, handedness=None, **kw)
        report = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "report", handedness="report", **kw)
        fixed = PL.generate_samples(CR.Prepared(samples, "cpu"), data, output_dir=tmp_path / "fix", handedness="fix", **kw)
    assert len(plain) == len(again) == 4 and len(report) == len(fixed) == 5
    assert sorted(os.listdir(tmp_path / "plain")) == ["sample_ligand_pos.npy", "sample_protein.pdb"]
    assert np.array_equal(plain[0], samples) and np.array_equal(again[0], samples) and np.array_equal(report[0], samples) and np.array_equal(report[1], plain[1])
    d, f = report[4], fixed[4]
    assert d["verdict"].tolist() == [1, 1, -1, -1, 1, -1] and d["basis"].tolist() == [1, 1, 1, 1, 2, 2] and not d["flipped"].any()
    assert d["helix_right"].tolist()[:4] == [37, 37, 0, 0] and d["helix_left"].tolist()[:4] == [0, 0, 37, 37] and d["quads"].tolist()[:4] == [37] * 4
    assert (np.abs(d["helix_right"][4:] - d["helix_left"][4:]) < 4).all()
    assert d["ligand_centres"].tolist() == [0] and d["ligand_kept"].tolist() == [1, 0] * 3 and d["ligand_inverted"].tolist() == [0, 1] * 3
    assert d["tau"].shape == d["classes"].shape == (6, CR.NR) and d["ligand_volume"].shape == (6, 1)
    assert (int(d["input_verdict"]), int(d["input_basis"])) == (1, 1) and d["input_counts"].tolist() == [37, 0, 0, 0, 37, 1, 0, 0]
    assert f["flipped"].tolist() == [False, False, True, True, False, True] and all(np.array_equal(f[k], d[k], equal_nan=True) for k in d if k != "flipped")
    want = samples.copy()
    want[f["flipped"], :, 0] = -want[f["flipped"], :, 0]
    assert np.array_equal(fixed[0], want) and np.array_equal(fixed[1], plain[1]) and np.array_equal(np.stack(fixed[3]), want[:, :CR.NA])
    assert np.array_equal(np.stack([p.atom_pos[:, 1] for p in fixed[2]]), want[:, CR.NA:])
    assert sorted(os.listdir(tmp_path / "fix")) == ["sample_handedness.npz", "sample_handedness.txt", "sample_ligand_pos.npy", "sample_protein.pdb"]
    lines = (tmp_path / "fix" / "sample_handedness.txt").read_text().splitlines()
    assert lines[0] == "# " + " ".join(CH.TEXT_COLUMNS) and lines[3].split()[:8] == ["-1", "1", "1", "0", "37", "0", "0", "37"] and len(lines) == 7
    # a SMILES-only ligand (no coordinates) and a protein from its sequence: no centre reference, no input census; the volumes are still returned
    bare = dict(data, atom_pos=torch.zeros(CR.NA, 3), residue_atom_pos=torch.zeros(CR.NR, 37, 3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        out = PL.generate_samples(CR.Prepared(samples, "cpu"), bare, handedness="report", **kw)[4]
    assert not any(k.startswith("input_") for k in out) and out["ligand_volume"].shape == (6, 1) and not out["ligand_kept"].any() and not out["ligand_inverted"].any()
    assert out["verdict"].tolist() == [1, 1, -1, -1, 0, 0] and np.array_equal(np.sign(out["ligand_volume"][:, 0]), np.sign(d["ligand_volume"][:, 0]))
