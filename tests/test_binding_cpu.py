"""CPU-only checks of what is derived from include/prd_hip.h: the ctypes binding (protein_redesign_amd._lib) against the frozen
snapshot tests/golden/binding_v101.json -- the hand-written tables, PRD_TUNE_* words and hipcc command lines that the derivation
replaced, recorded from them -- and the one compile routine of protein_redesign_amd.build.  An ABI change updates the snapshot
on purpose."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

from conftest import ROOT
from protein_redesign_amd import _lib, build, ops

TYPE_NAMES = {C.c_void_p: "c_void_p", C.c_int: "c_int", C.c_float: "c_float", C.c_size_t: "c_size_t", C.c_longlong: "c_longlong",
              C.c_char_p: "c_char_p", C.POINTER(_lib.PrdGemm): "POINTER(PrdGemm)"}


@pytest.fixture(scope="module")
def snap():
    with open(os.path.join(ROOT, "tests", "golden", "binding_v101.json")) as f:
        return json.load(f)


def header_text():
    with open(os.path.join(ROOT, "include", "prd_hip.h")) as f:
        return f.read()


def test_derived_binding_equals_the_frozen_tables(snap):
    assert _lib.ABI_VERSION == snap["abi_version"]
    assert len(_lib.ENTRIES) == 78 and set(_lib.SIGNATURES) == set(_lib.ENTRIES)
    assert {n: [TYPE_NAMES[t] for t in a] for n, a in _lib.SIGNATURES.items()} == snap["signatures"]

    def members(inject, before_stream):
        return sorted(n for n, e in _lib.ENTRIES.items() if e.inject == inject and (e.at == len(e.argtypes) - 2) == before_stream)
    assert members("arith", True) == snap["arith_before_stream"]
    assert members("arith", False) == snap["arith_last"]
    assert members("tune", True) == snap["tune_before_stream"]
    assert members("tune", False) == snap["tune_last"]
    assert sorted(n for n, e in _lib.ENTRIES.items() if e.inject is None) == sorted(
        set(snap["signatures"]) - set(snap["arith_before_stream"] + snap["arith_last"] + snap["tune_before_stream"] + snap["tune_last"]))
    assert sorted(n for n, e in _lib.ENTRIES.items() if e.restype is C.c_size_t) == snap["size_t_returns"]
    assert all(e.restype in (C.c_size_t, C.c_int) for e in _lib.ENTRIES.values())
    for n, e in _lib.ENTRIES.items():           # the injected slot is an int, and the one after it (if any) the stream
        if e.inject:
            assert e.argtypes[e.at] is C.c_int and e.argtypes[e.at + 1:] in ([], [C.c_void_p]), n


def exported(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("prd_")}


def test_built_library_exports_exactly_the_derived_names():
    have, want = exported(os.path.join(ROOT, "protein_redesign_amd", "libprd_hip.so")), set(_lib.ENTRIES)
    assert have - want == set(), "exported but not declared in include/prd_hip.h"
    assert want - have == set(), "declared in include/prd_hip.h but not exported"
    L = _lib.lib()                              # loading sets argtypes / restype on every one of them
    for n, e in _lib.ENTRIES.items():
        raw = getattr(L._cdll, n)
        assert list(raw.argtypes) == e.argtypes and raw.restype is e.restype, n


# ---- the parser on synthetic header text ---------------------------------------------------------------------------------------

def test_parser_refuses_a_misplaced_arith():
    with pytest.raises(ValueError, match="prd_bad_place"):
        _lib.parse_header("int prd_fine(int N, int arith);\nint prd_bad_place(float* x, int arith, int N, hipStream_t stream);\n")
    with pytest.raises(ValueError, match="prd_tune_early"):
        _lib.parse_header("int prd_tune_early(int tune, int N);\n")
    with pytest.raises(ValueError, match="prd_two"):
        _lib.parse_header("int prd_two(int tune, int arith);\n")
    with pytest.raises(ValueError, match="prd_not_stream"):       # last but one, and the last is not the stream
        _lib.parse_header("int prd_not_stream(float* x, int arith, int N);\n")


def test_parser_refuses_an_unknown_parameter_type():
    with pytest.raises(TypeError, match="prd_wide.*double"):
        _lib.parse_header("int prd_wide(float* x, double scale, hipStream_t stream);\n")
    with pytest.raises(TypeError, match="unsigned"):
        _lib.parse_header("int prd_u(unsigned n);\n")
    with pytest.raises(TypeError, match="struct PrdGemm"):
        _lib.parse_struct("typedef struct PrdGemm { int M; short K; } PrdGemm;", "PrdGemm")


def test_parser_reads_prototypes_over_several_lines_and_skips_comments():
    text = """
/* int prd_in_comment(float* x, int arith, int N);
 * int prd_in_comment2(int N); */
// int prd_in_line_comment(int N);
size_t prd_three_lines(const float* x,      /* a comment between the parameters */
                       const float* const* w, long long rows,
                       int tune, hipStream_t stream);
int prd_version(void);
int prd_name(const char* op, const PrdGemm *g, size_t bytes, float s, int arith);
void prd_other_return(int N);
"""
    e = _lib.parse_header(text)
    assert sorted(e) == ["prd_name", "prd_three_lines", "prd_version"]
    assert e["prd_three_lines"] == ([C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p], C.c_size_t, "tune", 3)
    assert e["prd_version"] == ([], C.c_int, None, None)
    assert e["prd_name"] == ([C.c_char_p, C.POINTER(_lib.PrdGemm), C.c_size_t, C.c_float, C.c_int], C.c_int, "arith", 4)


# ---- the injected word lands in the slot the header names ----------------------------------------------------------------------

def test_arithmetic_is_injected_into_its_slot():
    """prd_tri_attn_variant(N, P, arith) is a host-only query whose answer depends on the arithmetic alone (prd_hip.h: rows of 449
    positions are long rows on the fp32 kernel, 1, or on the split-operand kernel, 2)."""
    with _lib.arithmetic("fp32"):
        assert ops.tri_attn_variant(449, 64) == 1
    with _lib.arithmetic("split16"):
        assert ops.tri_attn_variant(449, 64) == 2


def test_tune_word_is_injected_into_its_slot():
    """prd_tri_attn_v2_form(N, P, tune): rows of 320 positions run the overlapped-phase core (2), with PRD_TUNE_TA2_NO_V3 the one
    with a barrier per phase (1)."""
    L = _lib.lib()
    before = L.prd_get_tune()
    try:
        assert L.prd_set_tune(0) == 0 and L.prd_tri_attn_v2_form(320, 64) == 2
        assert L.prd_set_tune(1 << 4) == 0 and L.prd_tri_attn_v2_form(320, 64) == 1          # PRD_TUNE_TA2_NO_V3
    finally:
        L.prd_set_tune(before)
    assert L.prd_get_tune() == before


# ---- PRD_TUNE_* words from the environment --------------------------------------------------------------------------------------

def test_tune_words_equal_the_recorded_ones(snap):
    cases = snap["tune_words"]
    seen = {k for c in cases for k in c["env"]}
    assert {name for name, _, _ in _lib._TUNE_ENV} | {"PRD_TA_VARIANT", "PRD_TA2_FLAGS", "PRD_TMS_DEPTH"} <= seen
    assert {c["env"].get("PRD_TA2_FLAGS") for c in cases} >= {"-1", "0", "9", "31", "63", ""}
    assert {(c["env"].get("PRD_TMS_NW"), c["env"].get("PRD_TMS_DEPTH")) for c in cases} >= {
        (nw, d) for nw in (None, "8", "12", "16") for d in (None, "2", "3")}
    for c in cases:
        assert _lib.tune_from_env(c["env"]) == c["word"], c
    assert all(0 <= c["word"] < (1 << 23) for c in cases)


def test_every_tune_switch_of_the_header_has_a_row():
    """a PRD_TUNE_* switch added to the header without an environment variable (or the other way round) is noticed"""
    defined = set(re.findall(r"#define\s+PRD_TUNE_(\w+)\s+\(", header_text()))
    used = {s for _, _, switches in _lib._TUNE_ENV for s in switches.values()} | {"TA2_FLAGS_SET", "TMS_DEPTH3"}
    assert used == defined and defined == set(_lib._TUNE) - {"TA_VARIANT_MASK"}
    assert _lib._TUNE_SHIFT == 8 and (_lib._FLAGS_MASK, _lib._FLAGS_SHIFT) == (31, 7)


# ---- PrdGemm ------------------------------------------------------------------------------------------------------------------------

def test_prdgemm_matches_the_header_struct_and_the_c_compiler(snap):
    body = re.search(r"typedef struct PrdGemm \{(.*?)\} PrdGemm;", re.sub(r"/\*.*?\*/", " ", header_text(), flags=re.S), flags=re.S).group(1)
    names = [re.search(r"(\w+)\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]
    assert [n for n, _ in _lib.PrdGemm._fields_] == names
    assert [[n, TYPE_NAMES[t]] for n, t in _lib.PrdGemm._fields_] == snap["prdgemm_fields"]
    assert C.sizeof(_lib.PrdGemm) == snap["prdgemm_sizeof"]
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    exe = build.build_asan(verbose=False)       # tests/native/host_abi_check.c prints the size the C compiler gives the struct
    out = subprocess.run([exe], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), capture_output=True, text=True, timeout=300).stdout
    assert int(re.search(r"sizeof\(PrdGemm\) = (\d+)", out).group(1)) == C.sizeof(_lib.PrdGemm)


# ---- build.py: one routine, four variants ------------------------------------------------------------------------------------------

class Recorder:
    """stands in for subprocess.run / check_call / call inside protein_redesign_amd.build"""

    def __init__(self, execute):
        self.execute, self.cmds = execute, []
        self.real = {k: getattr(subprocess, k) for k in ("run", "check_call", "call")}

    def install(self, monkeypatch):
        for k in self.real:
            monkeypatch.setattr(build.subprocess, k, lambda cmd, *a, _k=k, **kw: self(_k, cmd, *a, **kw))

    def __call__(self, kind, cmd, *a, **kw):
        if os.path.basename(cmd[0]) == "hipcc":
            self.cmds.append([t.replace(ROOT, "{ROOT}") for t in cmd])
        if self.execute:
            return self.real[kind](cmd, *a, **kw)
        return subprocess.CompletedProcess(cmd, 0, stdout="", stderr="") if kind == "run" else 0


@pytest.mark.parametrize("variant", ["shipped", "ab", "timing", "asan"])
def test_variants_issue_the_recorded_hipcc_commands(snap, monkeypatch, variant):
    """With everything stale and nothing executed, every variant starts hipcc with the recorded argument lists, token for token and
    in the recorded order -- the kernels are compiled as they were."""
    monkeypatch.delenv("HIPCC", raising=False)
    monkeypatch.setattr(build, "_stale", lambda out, deps: True)
    rec = Recorder(execute=False)
    rec.install(monkeypatch)
    {"shipped": build.build, "ab": build.build_ab, "timing": build.build_timing, "asan": build.build_asan}[variant](verbose=False)
    assert rec.cmds == snap["hipcc_argv"][variant]


def test_variant_table_names_the_documented_outputs():
    pkg = os.path.join(ROOT, "protein_redesign_amd")
    assert {k: (os.path.relpath(v.objdir, pkg), os.path.relpath(v.lib, pkg)) for k, v in build.VARIANTS.items()} == {
        "shipped": ("csrc", "libprd_hip.so"), "ab": ("csrc/ab", "libprd_hip_ab.so"),
        "timing": ("csrc/timing", "libprd_hip_timing.so"), "trace": ("csrc/trace", "libprd_hip_trace.so"),
        "asan": ("csrc/asan", "libprd_hip_asan.so")}
    # the trace variant differs from the shipped compile by its macro and by unoptimised device code, which none of its calls reaches
    assert build.VARIANTS["trace"].cflags == ["-DPRD_LAUNCH_TRACE", "-Xarch_device", "-O0"] and not build.VARIANTS["trace"].ldflags
    assert build.LIB == build.VARIANTS["shipped"].lib and build.RESOURCE_JSON == os.path.join(pkg, "csrc", "resource_usage.json")


def test_second_build_starts_no_compiler(monkeypatch):
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    build.build(verbose=False)
    build.build_asan(verbose=False)             # (built by tests/test_host_cpu.py as well; incremental like the shipped one)
    rec = Recorder(execute=True)
    rec.install(monkeypatch)
    assert build.build(verbose=False) == build.LIB
    build.build_asan(verbose=False)
    assert rec.cmds == []
