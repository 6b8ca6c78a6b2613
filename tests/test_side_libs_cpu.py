"""CPU: the build of the side libraries (protein_redesign_amd/build.py, SIDE_LIBS) -- the table, what each row holds, the two commands
a row issues and that no other build issues them, the export list of a cross-compiled library against its header, and the kernel names.
Once per row; what is specific to one library (its header, its kernels' figures, its host refusals) is in that library's own test file."""
import os

import pytest

from conftest import ROOT
from protein_redesign_amd import build
from sample_stubs import header_entries
from test_binding_cpu import Recorder, exported

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
NAMES = ["align", "tmalign", "quality", "condition", "sequence", "solver", "guide", "chirality", "multistep", "backbone"]
PKG, CSRC = os.path.join(ROOT, "protein_redesign_amd"), os.path.join(ROOT, "protein_redesign_amd", "csrc")


def all_stale(monkeypatch):
    """everything stale, nothing executed: the recorder of the hipcc commands"""
    monkeypatch.delenv("HIPCC", raising=False)
    monkeypatch.setattr(build, "_stale", lambda out, deps: True)
    rec = Recorder(execute=False)
    rec.install(monkeypatch)
    return rec


def test_the_table_is_the_ten_in_their_order_and_the_first_five_are_traced():
    assert list(build.SIDE_LIBS) == NAMES
    assert [n for n, s in build.SIDE_LIBS.items() if s.traced] == NAMES[:5] and all(s.traced is (n in NAMES[:5]) for n, s in build.SIDE_LIBS.items())
    assert build.SideLib._fields == ("sources", "headers", "lib", "flag", "traced")


def test_the_denoiser_build_issues_the_commands_it_issued_before(monkeypatch):
    """build() knows nothing of the side libraries: one compile per source of its own, in their order, and one link"""
    rec = all_stale(monkeypatch)
    build.build(verbose=False)
    assert len(rec.cmds) == len(build.SOURCES) + 1
    assert [c[-3] for c in rec.cmds[:-1]] == ["{ROOT}/protein_redesign_amd/csrc/" + s for s in build.SOURCES]
    assert build.SOURCES == ["prd_gemm.hip", "prd_pair.hip", "prd_tri.hip", "prd_tri2.hip", "prd_bwd.hip", "prd_spa.hip", "prd_tri_heads.hip",
                             "prd_tri_heads_bwd.hip", "prd_mask.hip"] and sorted(build.VARIANTS) == ["ab", "asan", "shipped", "timing", "trace"]


@pytest.mark.parametrize("name", NAMES)
def test_row_contents(name):
    s = build.SIDE_LIBS[name]
    assert s.sources == [f"prd_{name}.hip"] and s.flag == f"--{name}" and s.lib == os.path.join(PKG, f"libprd_{name}.so")
    fit = [os.path.join(CSRC, "prd_superpose.h")] if name in ("align", "tmalign") else []       # the fit the two share, and nobody else's
    assert s.headers == [os.path.join(ROOT, "include", f"prd_{name}.h"), os.path.join(CSRC, "prd_launch.h")] + fit
    assert build._headers(s.sources[0]) == s.headers
    assert all(os.path.exists(p) for p in s.headers + [os.path.join(CSRC, s.sources[0])])


@pytest.mark.parametrize("name", NAMES)
def test_one_compile_one_link_with_the_denoisers_flags(monkeypatch, name):
    rec = all_stale(monkeypatch)
    build.build(verbose=False)
    shipped, rec.cmds = rec.cmds[0], []
    build.build_side(name, verbose=False)
    src, obj, lib = (f"{{ROOT}}/protein_redesign_amd/{f}" for f in (f"csrc/prd_{name}.hip", f"csrc/prd_{name}.o", f"libprd_{name}.so"))
    assert rec.cmds == [shipped[:-3] + [src, "-o", obj], shipped[:1] + ["--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj]]
    assert shipped[-4] == "-c" and "-ffp-contract=off" in rec.cmds[0]


@pytest.mark.parametrize("name", NAMES)
def test_no_other_build_compiles_or_links_it(monkeypatch, name):
    """by the file stem ``prd_<name>.``: source, object and library carry it (libprd_tmalign.so does not carry prd_align.)"""
    rec = all_stale(monkeypatch)
    for other in [None] + [n for n in NAMES if n != name]:
        rec.cmds = []
        build.build(verbose=False) if other is None else build.build_side(other, verbose=False)
        assert rec.cmds and not any(f"prd_{name}." in t for c in rec.cmds for t in c), other


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("name", NAMES)
def test_forced_cross_compile_exports_the_header_and_a_second_build_is_incremental(monkeypatch, name):
    lib = build.build_side(name, force=True, verbose=False)
    assert lib == build.SIDE_LIBS[name].lib and os.path.exists(lib)
    assert exported(lib) == set(header_entries(name))
    rec = Recorder(execute=True)
    rec.install(monkeypatch)
    assert build.build_side(name, verbose=False) == lib
    assert rec.cmds == []                                       # a second build starts no compiler


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
@pytest.mark.parametrize("name", NAMES)
def test_kernel_names_are_its_own(name):
    mine = set(build.resource_usage(sources=build.SIDE_LIBS[name].sources))
    assert mine and not mine & set(build.resource_usage())      # the denoiser library's table is what it was
    for other in NAMES:
        assert other == name or not mine & set(build.resource_usage(sources=build.SIDE_LIBS[other].sources)), other
