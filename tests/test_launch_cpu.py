"""CPU: the host half of every kernel launch (protein_redesign_amd/csrc/prd_launch.h) -- that it is the only place that raises a kernel's
dynamic-LDS limit or launches a kernel, for the denoiser and for the side libraries, that every object of either depends on it, and
that its launch geometry is the arithmetic the launch sites spelled out before the header existed."""
import os
import re
import subprocess

import pytest

from conftest import ROOT
from protein_redesign_amd import build
from test_binding_cpu import Recorder

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
CSRC = os.path.join(ROOT, "protein_redesign_amd", "csrc")
SIDE = {s for lib in build.SIDE_LIBS.values() for s in lib.sources} | {"prd_superpose.h"}


def denoiser_files():
    """name -> text of every file under csrc/ that is compiled into libprd_hip.so"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".inc")) and name not in SIDE:
            with open(os.path.join(CSRC, name)) as f:
                out[name] = f.read()
    return out


def test_one_raise_one_launcher():
    files = denoiser_files()
    assert set(build.SOURCES) | {"prd_common.h", "prd_launch.h", "prd_tri2_v3_body.inc"} == set(files)
    for word in ("hipFuncSetAttribute", "hipLaunchKernelGGL", "<<<"):
        assert [n for n, t in files.items() if word in t] == ["prd_launch.h"], word
    assert not any(re.search(r"\(void\)\s*hipFuncSetAttribute", t) for t in files.values())   # the result of the raise is kept
    assert not any(re.search(r"#define\s+\w*SET_LDS", t) for t in files.values())
    # std::call_once: the raise, and the CU count of the co-resident launch
    assert sorted(n for n, t in files.items() if "std::once_flag" in t) == ["prd_launch.h", "prd_tri2.hip"]
    assert files["prd_tri2.hip"].count("std::once_flag") == 1 and "prd_cu_count" in files["prd_tri2.hip"]
    # one definition of the geometry
    for fn in ("grid_for", "prd_rows_per_head", "prd_rows_per_head_xcd8"):
        assert [n for n, t in files.items() if re.search(r"\b(?:int|long)\s+%s\s*\(" % fn, t)] == ["prd_launch.h"], fn
    # every denoiser source includes the header, and so does every side source: the same holds for them (prd_superpose.h is device code)
    for src in build.SOURCES:
        assert '#include "prd_launch.h"' in files[src], src
    for name in SIDE:
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        assert ('#include "prd_launch.h"' in text) == name.endswith(".hip"), name
        for word in ("hipFuncSetAttribute", "hipLaunchKernelGGL", "<<<", "hipGetLastError", "hipMemsetAsync", "std::once_flag"):
            assert word not in text, (name, word)


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_the_launch_header_makes_every_object_stale(monkeypatch):
    """``_stale`` is the real one and no compiler runs: csrc/prd_launch.h is given the newest time stamp, and a command that is recorded
    makes its output newer still, as the compiler would have."""
    build.build(verbose=False)
    for side in build.SIDE_LIBS:
        build.build_side(side, verbose=False)
    header, real, written = os.path.join(CSRC, "prd_launch.h"), os.path.getmtime, []
    assert header in build.HEADERS and all(header in s.headers for s in build.SIDE_LIBS.values())
    newest = max(real(p) for p in [build.LIB] + [s.lib for s in build.SIDE_LIBS.values()]) + 10.0
    monkeypatch.setattr(os.path, "getmtime", lambda p: newest + 10.0 * (1 + written.index(p)) if p in written else newest if p == header else real(p))

    class Touching(Recorder):
        def __call__(self, kind, cmd, *a, **kw):
            written.extend(cmd[cmd.index("-o") + 1:][:1] if "-o" in cmd else [])
            return super().__call__(kind, cmd, *a, **kw)
    rec = Touching(execute=False)
    rec.install(monkeypatch)
    for side, s in build.SIDE_LIBS.items():          # a side library: its one object, then its link, and nothing of another library
        src, lib = "{ROOT}/protein_redesign_amd/csrc/" + s.sources[0], s.lib.replace(ROOT, "{ROOT}")
        build.build_side(side, verbose=False)
        assert [c[-3:] for c in rec.cmds] == [[src, "-o", src.replace(".hip", ".o")], ["-o", lib, src.replace(".hip", ".o")]], side
        rec.cmds = []
        build.build_side(side, verbose=False)
        assert rec.cmds == []
    build.build(verbose=False)
    objs = ["{ROOT}/protein_redesign_amd/csrc/" + s.replace(".hip", ".o") for s in build.SOURCES]
    assert len(build.SOURCES) == 9
    assert [c[-3:] for c in rec.cmds[:-1]] == [["{ROOT}/protein_redesign_amd/csrc/" + s, "-o", o] for s, o in zip(build.SOURCES, objs)]
    assert rec.cmds[-1][-len(objs) - 2:] == ["-o", "{ROOT}/protein_redesign_amd/libprd_hip.so"] + objs
    rec.cmds = []
    build.build(verbose=False)                  # and they are up to date again
    assert rec.cmds == []


# ---- the geometry: what the launch sites computed before prd_launch.h, restated --------------------------------------------------

def old_grid_for(tasks, per_wg, cap):
    g = (tasks + per_wg - 1) // per_wg
    if g > cap:
        g = cap
    if g < 1:
        g = 1
    return g


def old_rows_per_head(rows_total, H, xcd8=None):
    """xcd8 None: prd_tri_attn_core, its fused form, the heads kernels (forward and backward); True / False: prd_tri_attn_core_v2 with
    PRD_TUNE_TA2_NO_XCD8 clear / set (prd_tri_attn_pair: always True)"""
    cap = 256 // H
    per_head = cap if cap < rows_total else rows_total
    if per_head < 1:
        per_head = 1
    rounds = (rows_total + per_head - 1) // per_head
    per_head = (rows_total + rounds - 1) // rounds
    if xcd8 is None:
        return per_head
    if per_head >= 8 and xcd8:
        per_head = (per_head + 7) // 8 * 8
    if per_head > cap:
        per_head = cap
    return per_head


def old_rows_per_head_chunked(rows_total, H):
    """prd_tri_attn_core_chunked had no ``per_head < 1`` clamp (rows_total >= 1 there: the same values)"""
    cap = 256 // H
    per_head = cap if cap < rows_total else rows_total
    rounds = (rows_total + per_head - 1) // per_head
    return (rows_total + rounds - 1) // rounds


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_geometry_is_the_arithmetic_of_the_former_launch_sites(tmp_path):
    exe = str(tmp_path / "launch_geometry")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-std=c++17", "-Wall", "-Wno-unused-function",
                    os.path.join(ROOT, "tests", "native", "launch_geometry.hip"), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    g = [tuple(map(int, ln.split()[1:])) for ln in lines if ln.startswith("g ")]
    r = [tuple(map(int, ln.split()[1:])) for ln in lines if ln.startswith("r ")]
    # the (per_wg, cap) pairs of the sources: every grid_for call names them as literals or as a constexpr wave count of 8
    used = set()
    for text in denoiser_files().values():
        for per_wg, cap in re.findall(r"\bgrid_for\([^;]*?,\s*(\w+),\s*(\d+)\)", text):
            used.add((int(per_wg) if per_wg.isdigit() else 8, int(cap)))
    assert used == {(p, c) for _, p, c, _ in g} and len(used) == 8
    assert len(g) == 8 * (4201 + 7) and {t for t, _, _, _ in g} >= set(range(0, 4201)) | {2 ** 31 + 5}
    bad = [(t, p, c, v) for t, p, c, v in g if v != old_grid_for(t, p, c)]
    assert not bad, bad[:5]
    assert len(r) == 8 * 4200 and {(n, h) for n, h, _, _, _ in r} == {(n, h) for n in range(1, 4201) for h in range(1, 9)}
    bad = [row for row in r if row[2:] != (old_rows_per_head(row[0], row[1]), old_rows_per_head(row[0], row[1], True),
                                           old_rows_per_head(row[0], row[1], False))
           or row[2] != old_rows_per_head_chunked(row[0], row[1])]
    assert not bad, bad[:5]
    assert any(a != b for _, _, a, b, _ in r) and all(a == c for _, _, a, _, c in r)       # the rounding does something; switched off, nothing
