"""CPU: the host decisions above every denoiser kernel launch -- which kernel, its grid, its block, its LDS bytes, its arguments -- and the
values of the host-only queries, held to a recording.  The trace build of the library (protein_redesign_amd/csrc/prd_launch.h under
-DPRD_LAUNCH_TRACE, build.py variant "trace") prints a line per launch instead of launching; tests/native/launch_trace.c walks the
entry points over a sweep of shapes, arithmetics, switches and head layouts.  tests/golden/launch_trace.txt.xz is that output for the
commit BEFORE the LDS sizes and the dispatch decisions were gathered into named host functions (only the trace #ifdef applied to it):
a refactor of the launch sites must reproduce it line for line.  The fixture is still that pre-refactor recording, with one kernel
renamed in it: tri_attn_core_kernel<P, 12, true, false> became <P, 12> when its two dead template parameters went.  No device is touched."""
import lzma
import os
import re
import subprocess

import pytest

from conftest import ROOT
from protein_redesign_amd import build

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_trace.txt.xz")

# kernels of the shipped library that no call of the driver can launch
NOT_TRACED = {
    # reachable only through prd_tri_attn_pair, which asks the device for its CU count and clears its barrier words: not a pure launch
    "tri_attn_pair_kernel<32, 12>", "tri_attn_pair_kernel<64, 12>",
    # instantiated by the two-way LayerNorm dispatch of launch_ring, never launched: prd_gemm takes <4, 4> for rows without LayerNorm only
    "gemm_ring_kernel<4, 4, true, false>",
}


@pytest.fixture(scope="module")
def recorded():
    with lzma.open(FIXTURE, "rt") as f:
        return f.read().split("\n")


@pytest.fixture(scope="module")
def traced():
    exe = build.build_trace(verbose=False)
    return subprocess.run([exe], capture_output=True, text=True, check=True, timeout=600).stdout.split("\n")


def test_fixture_is_small_and_covers_the_sweep(recorded):
    assert os.path.getsize(FIXTURE) < 300 * 1024
    text = "\n".join(recorded)
    for n in (1, 31, 32, 33, 63, 64, 65, 319, 320, 321, 384, 385, 416, 417, 449, 769, 960, 961, 1024, 1025, 1961, 4096):
        for b in (1, 2, 8):
            for p in (32, 64, 48):
                for a in (0, 1):
                    assert f"# pair track b {b} N {n} P {p} arith {a}\n" in text
    tunes = {int(m) for m in re.findall(r"^# switches b \d+ N \d+ P \d+ tune (\d+)$", text, flags=re.M)}
    with open(os.path.join(ROOT, "include", "prd_hip.h")) as f:
        header = f.read()
    for name, value, shift in re.findall(r"#define\s+(PRD_TUNE_\w+)\s+\((\d+) << (\d+)\)", header):
        assert int(value) << int(shift) in tunes, name                # every switch of the header alone
    assert {0, 1, 2, 3, 10} <= tunes
    assert {(int(h), int(c)) for h, c in re.findall(r"^# heads .* H (\d+) c (\d+)$", text, flags=re.M)} >= {(4, 16), (8, 8), (2, 32)}
    assert {int(s) for s in re.findall(r"^C outer_linear S (\d+) =", text, flags=re.M)} >= {128, 256, 384, 512, 2528}
    assert {int(d) for d in re.findall(r"^# pair head .* dd (\d+)$", text, flags=re.M)} >= {128, 136, 256, 624, 632}
    queries = set(re.findall(r"^Q (\w+)", text, flags=re.M))
    assert queries >= {"tri_attn_variant", "tri_attn_v2_form", "tri_attn_v2_supported", "tri_attn_stats_bytes", "workspace_bytes",
                       "pair_head_supported", "tri_mul_chain_supported", "tri_attn_core_fused_supported", "tri_attn_pair_supported",
                       "tri_attn_bwd_core_v2_supported", "pair_linear_supported", "spa_attn_core_supported", "tri_attn_heads_supported",
                       "tri_attn_bwd_heads_supported", "gemm_slab_ok", "single_fc1_folded_ok"}


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_every_shipped_kernel_is_in_the_recorded_trace(recorded):
    launched = {ln[2:ln.index(" grid ")] for ln in recorded if ln.startswith("L ")}
    shipped = set(build.resource_usage())
    assert NOT_TRACED <= shipped
    assert shipped - launched == NOT_TRACED
    assert launched <= shipped


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_trace_of_this_tree_equals_the_recorded_one(recorded, traced):
    assert len(traced) == len(recorded)
    bad = [(i, want, got) for i, (want, got) in enumerate(zip(recorded, traced)) if want != got]
    assert not bad, bad[:5]
