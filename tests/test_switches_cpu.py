"""CPU: the list of environment switches cannot drift.  Three sets are equal -- the PRD_* variables the package reads, the first
column of the README's switch table, the keys of tests/switch_cases.py -- and every registry entry names GPU tests that exist and
carry the gpu mark.  Where tests/golden/launch_trace.txt.xz holds a shape that a GPU case of tests/test_switches.py uses, the
recording shows that the launches under the switch differ from those under tune 0.  No device is touched."""
import glob
import importlib
import lzma
import os
import re

import pytest

import switch_cases as SC
from conftest import ROOT
from protein_redesign_amd import _lib

PACKAGE = os.path.join(ROOT, "protein_redesign_amd")


def variables_the_package_reads():
    names = set()
    for path in glob.glob(os.path.join(PACKAGE, "*.py")):
        with open(path) as f:
            names |= set(re.findall(r"""os\.environ\.get\(\s*f?["'](PRD_\w+)["']""", f.read()))
    return names | {name for name, _, _ in _lib._TUNE_ENV} | {"PRD_TA_VARIANT", "PRD_TA2_FLAGS", "PRD_TMS_DEPTH"}


def readme_table(text):
    """{variable: (default cell, effect cell)} of the table under "Environment switches": a row may name several variables"""
    rows = {}
    body = text[text.index("| variable | default | effect |"):]
    for ln in body.splitlines()[2:]:
        if not ln.startswith("|"):
            break
        cells = [c.strip() for c in re.split(r"(?<!\\)\|", ln)[1:-1]]
        for name in re.findall(r"`(PRD_\w+)`", cells[0]):
            assert name not in rows, f"README lists {name} twice"
            rows[name] = (cells[1], cells[2])
    return rows


def compare(read, readme, registry):
    """the three-way equality, with a message that says which set lacks what"""
    msgs = []
    for a, b, an, bn in ((read, readme, "read by the package", "in the README table"), (read, registry, "read by the package", "in tests/switch_cases.py"),
                         (readme, registry, "in the README table", "in tests/switch_cases.py")):
        if a - b:
            msgs.append(f"{an} but not {bn}: {sorted(a - b)}")
        if b - a:
            msgs.append(f"{bn} but not {an}: {sorted(b - a)}")
    return msgs


@pytest.fixture(scope="module")
def readme():
    with open(os.path.join(ROOT, "README.md")) as f:
        return readme_table(f.read())


def test_package_readme_and_registry_list_the_same_variables(readme):
    read = variables_the_package_reads()
    assert len(read) > 30 and {"PRD_LIB", "PRD_TA2_V3", "PRD_TASK_QUEUE", "PRD_TRAIN_FUSED_RESIDUAL"} <= read
    msgs = compare(read, set(readme), set(SC.REGISTRY))
    assert not msgs, "\n".join(msgs)


def test_the_comparison_notices_a_missing_row_and_a_new_variable(readme):
    """the check checks: a README row deleted, a registry entry deleted, a variable the package newly reads"""
    read, table, reg = variables_the_package_reads(), set(readme), set(SC.REGISTRY)
    assert compare(read, table - {"PRD_TA2_XCD8"}, reg) and compare(read, table, reg - {"PRD_HEAD_SLAB"}) and compare(read | {"PRD_NEW"}, table, reg)
    assert re.findall(r"""os\.environ\.get\(\s*f?["'](PRD_\w+)["']""", 'X = os.environ.get("PRD_NEW", "1") != "0"') == ["PRD_NEW"]
    text = "| variable | default | effect |\n|---|---|---|\n| `PRD_A`, `PRD_B` | `1` | a \\| b |\n| *the ones below* | | |\n\nafter | `PRD_C` |"
    assert readme_table(text) == {"PRD_A": ("`1`", "a \\| b"), "PRD_B": ("`1`", "a \\| b")}


def test_readme_rows_state_the_registry_values(readme):
    """the README row of a switch names the non-default value the registry sets; PRD_TA2_LONG says what the shipped library runs"""
    assert "PRD_TRAIN_FUSED_RESIDUAL" in readme
    assert "fp32" in readme["PRD_TA2_LONG"][1] and "PRD_FIRST_GEN" in readme["PRD_TA2_LONG"][1]
    for name, s in SC.REGISTRY.items():
        if s.how is None:
            assert s.reason.startswith("not a switch"), name
            continue
        assert re.search(r"`%s`:" % re.escape(s.value), readme[name][1]) or re.search(r"`%s`" % re.escape(s.value), readme[name][1]), \
            f"the README row of {name} does not describe the value {s.value}"
    assert {n for n, s in SC.REGISTRY.items() if s.how is None} == {"PRD_LIB", "PRD_GEMM_MODE", "PRD_BF16X3"}


def test_every_entry_can_be_set_the_way_it_says():
    tune_names = {name: (default, values) for name, default, values in _lib._TUNE_ENV}
    for arm_id, name, s in SC.arms("step") + SC.arms("train") + SC.arms("covered"):
        assert s.how in ("tune", "attr", "env"), arm_id
        if s.how == "tune":
            word = SC.bits(s.target, _lib._TUNE)
            assert 0 < word < (1 << 23), arm_id
            # the bits are what the binding makes of the variable at that value
            assert _lib.tune_from_env({name: s.value}) == word and _lib.tune_from_env({}) == 0, arm_id
            if name in tune_names:
                assert int(s.value) != tune_names[name][0] and tune_names[name][1][int(s.value)] == s.target, arm_id
        elif s.how == "attr":
            module, attr = s.target.split(".")
            mod = importlib.import_module("protein_redesign_amd." + module)
            assert isinstance(getattr(mod, attr), bool) and isinstance(s.attr_value, bool), arm_id
            with open(os.path.join(PACKAGE, module + ".py")) as f:      # the attribute is the variable, read at import
                m = re.search(r"^%s = os\.environ\.get\(\"%s\", \"([01])\"\) ([!=]=) \"([01])\"" % (re.escape(attr), name), f.read(), flags=re.M)
            assert m, arm_id
            default = (m.group(1) == m.group(3)) == (m.group(2) == "==")
            assert s.attr_value == (not default) and ((s.value == m.group(3)) == (m.group(2) == "==")) == s.attr_value, arm_id
        else:
            assert s.target == name, arm_id
    # the switches of the header, each in the registry
    targets = {s.target.split("=")[0] for _, _, s in SC.arms("step") + SC.arms("covered") if s.how == "tune"}
    assert targets | {"TMS_NW12", "TA_VARIANT_MASK", "TA2_FLAGS_SET", "TA_VARIANT", "TA2_FLAGS"} >= set(_lib._TUNE)


def _is_gpu_test(module, function):
    mod = importlib.import_module(module)
    fn = getattr(mod, function, None)
    if not callable(fn):
        return False
    marks = list(getattr(fn, "pytestmark", []))
    pm = getattr(mod, "pytestmark", [])
    marks += pm if isinstance(pm, (list, tuple)) else [pm]
    return any(m.name == "gpu" for m in marks)


def test_every_entry_names_gpu_tests_that_exist():
    for name, s in SC.REGISTRY.items():
        if s.how is None:
            assert not s.tests, name
            continue
        assert s.tests, f"{name}: no GPU test"
        for t in s.tests:
            module, function = t.split("::")
            assert _is_gpu_test(module, function), f"{name}: {t} is not a gpu-marked test function"
    assert not _is_gpu_test("test_switches_cpu", "test_every_entry_names_gpu_tests_that_exist")
    assert not _is_gpu_test("test_ab_build", "test_ab_library_exports_the_same_abi") and not _is_gpu_test("test_hip_parity", "no_such_test")
    # the parametrised tests take their arms from the registry: an entry of kind "step" / "train" is run by them
    import test_switches as TS
    assert [a[0] for a in SC.arms("step")] == TS.STEP_IDS and [a[0] for a in SC.arms("train")] == TS.TRAIN_IDS
    for arm_id, name, s in SC.arms("step"):
        assert SC.STEP in s.tests, arm_id
    for arm_id, name, s in SC.arms("train"):
        assert SC.TRAIN in s.tests, arm_id


# ---- the recorded launch trace: the switch changes what runs at shapes the GPU cases use -------------------------------------------
def _sections():
    with lzma.open(os.path.join(ROOT, "tests", "golden", "launch_trace.txt.xz"), "rt") as f:
        lines = f.read().split("\n")
    out, cur = {}, None
    for ln in lines:
        m = re.fullmatch(r"# switches b (\d+) N (\d+) P (\d+) tune (\d+)", ln)
        if m:
            cur = out.setdefault(tuple(map(int, m.groups())), [])
        elif ln.startswith("#"):
            cur = None
        elif cur is not None:
            cur.append(ln)
    return out


def _launches_of(section, call):
    """[(kernel, grid, block, lds)] of the L lines in front of ``C <call> = ...`` and the call's return value"""
    got = []
    for ln in section:
        if ln.startswith("L "):
            m = re.match(r"L (.*) grid (\d+ \d+ \d+) block (\d+ \d+ \d+) lds (\d+) args", ln)
            got.append(m.groups())
        elif ln.startswith("C "):
            if re.fullmatch(r"C %s = -?\d+" % re.escape(call), ln):
                return got, int(ln.rsplit(" = ", 1)[1])
            got = []
    raise AssertionError(f"no call {call} in the section")


def test_recorded_launches_differ_under_the_switch():
    import test_switches as TS
    sections = _sections()
    checked = 0
    for name, s in SC.REGISTRY.items():
        if s.trace is None:
            continue
        call, shapes = s.trace
        word = SC.bits(s.target, _lib._TUNE)
        for b, N, P in shapes:
            assert (b, N, P) in TS.TRACED_SHAPES[name], f"{name}: no GPU case of tests/test_switches.py at b {b} N {N} P {P}"
            base, code0 = _launches_of(sections[(b, N, P, 0)], call)
            got, code = _launches_of(sections[(b, N, P, word)], call)
            assert code0 == 0 and code == 0 and base and got, (name, b, N, P)
            assert got != base, f"{name}: the recorded launches of {call} at b {b} N {N} P {P} are the same under tune {word} and tune 0"
            checked += 1
    assert checked >= 6
    # what the GPU cases assert about the dispatch, from the recording: one barrier per phase; long rows off the second generation
    v3 = SC.bits("TA2_NO_V3", _lib._TUNE)
    assert _launches_of(sections[(1, 33, 32, v3)], "tri_attn_core_v2")[0][0][0].startswith("tri_attn_core_v2_kernel<32")
    nl = SC.bits("TA2_NO_LONG", _lib._TUNE)
    for N, kernel in ((385, "tri_attn_core_kernel<32"), (417, "tri_attn_core_kernel<32"), (449, "tri_attn_core_long_kernel<32")):
        assert "Q tri_attn_v2_form = 0" in sections[(1, N, 32, nl)]
        assert _launches_of(sections[(1, N, 32, nl)], "tri_attn")[0][0][0].startswith(kernel)           # the fp32 kernels of that length
        assert _launches_of(sections[(1, N, 32, 0)], "tri_attn")[0][0][0].startswith("tri_attn_core_v2l_kernel<32")
    x8 = SC.bits("TA2_NO_XCD8", _lib._TUNE)
    assert _launches_of(sections[(1, 449, 32, x8)], "tri_attn")[0][0][1] == "228 1 1" and _launches_of(sections[(1, 449, 32, 0)], "tri_attn")[0][0][1] == "256 1 1"
