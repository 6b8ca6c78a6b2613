"""CPU: the host decisions above every denoiser kernel launch -- which kernel, its grid, its block, its LDS bytes, its arguments -- and the
values of the host-only queries, held to a recording.  The trace build of the library (protein_redesign_amd/csrc/prd_launch.h under
-DPRD_LAUNCH_TRACE, build.py variant "trace") prints a line per launch instead of launching; tests/native/launch_trace.c walks the
entry points over a sweep of shapes, arithmetics, switches and head layouts.  tests/golden/launch_trace.txt.xz is that output for the
commit BEFORE the LDS sizes and the dispatch decisions were gathered into named host functions (only the trace #ifdef applied to it):
a refactor of the launch sites must reproduce it line for line.  The fixture is still that pre-refactor recording, with kernels
renamed in it and nothing else: tri_attn_core_kernel<P, 12, true, false> became <P, 12> when its two dead template parameters went;
and when the fp32 and split-16 forms of four kernels became one body each, with the arithmetic as a template argument,
    pair_init_kernel<P> -> pair_init_kernel<P, false>                 pair_init_h2_kernel<P> -> pair_init_kernel<P, true>
    opm_pair_kernel<P> -> opm_pair_kernel<P, false>                   opm_pair_h2_kernel<P> -> opm_pair_kernel<P, true>
    outer_linear_res_kernel<P, 8> -> outer_linear_res_kernel<P, 8, false>
    outer_linear_res_h2_kernel<P, 8> -> outer_linear_res_kernel<P, 8, true>, whose lines gained the null `queue` pointer as first argument
    linear_wgrad_kernel<NBLK> -> linear_wgrad_kernel<NBLK, false>     linear_wgrad_h2_kernel<NBLK> -> linear_wgrad_kernel<NBLK, true>
No device is touched."""
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


# ---- the five side libraries: the same, by a driver and a recording of their own -------------------------------------------------
# tests/native/side_launch_trace.c walks every entry point of include/prd_{align,tmalign,quality,condition,sequence}.h over the shapes
# at which a host decision changes.  tests/golden/side_launch_trace.txt.xz is its output for the commit BEFORE the side libraries took
# the launch helper (their raw launches, attribute calls and memset made to print under a trace #ifdef, nothing else changed).
SIDE_FIXTURE = os.path.join(ROOT, "tests", "golden", "side_launch_trace.txt.xz")

# kernels of the side libraries that no call of the driver can launch
SIDE_NOT_TRACED = set()


@pytest.fixture(scope="module")
def side_recorded():
    with lzma.open(SIDE_FIXTURE, "rt") as f:
        return f.read().split("\n")


def launches(lines, kernel):
    """(grid, block, lds) of every launch of ``kernel``, in order"""
    out = []
    for ln in lines:
        m = re.match(r"L %s grid (\d+) (\d+) (\d+) block (\d+) (\d+) (\d+) lds (\d+) args" % re.escape(kernel), ln)
        if m:
            v = tuple(map(int, m.groups()))
            out.append((v[:3], v[3:6], v[6]))
    return out


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_side_trace_of_this_tree_equals_the_recorded_one(side_recorded):
    exe = build.build_trace_side(verbose=False)
    traced = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=600).stdout.split("\n")
    assert len(traced) == len(side_recorded)
    bad = [(i, want, got) for i, (want, got) in enumerate(zip(side_recorded, traced)) if want != got]
    assert not bad, bad[:5]


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_every_side_kernel_is_in_the_recorded_trace(side_recorded):
    launched = {ln[2:ln.index(" grid ")] for ln in side_recorded if ln.startswith("L ")}
    shipped = {k for s in build.SIDE_LIBS.values() if s.traced for k in build.resource_usage(sources=s.sources)}
    assert len(shipped) == 14 and SIDE_NOT_TRACED <= shipped
    assert shipped - launched == SIDE_NOT_TRACED
    assert launched <= shipped


def test_side_fixture_is_small_and_covers_the_sweep(side_recorded):
    assert os.path.getsize(SIDE_FIXTURE) < 64 * 1024
    text, KB48 = "\n".join(side_recorded), 48 * 1024

    def result(line):
        m = re.search(r"^%s = (-?\d+)$" % re.escape(line), text, flags=re.M)
        assert m, line
        return int(m.group(1))

    def after(marker):
        """the lines between ``marker`` and the next marker"""
        at = side_recorded.index(marker)
        end = next(i for i in range(at + 1, len(side_recorded)) if side_recorded[i].startswith("#") or not side_recorded[i])
        return side_recorded[at + 1:end]

    # align: 4 -> 8 waves at N = 1025, the search kernel's 24 N bytes of LDS on either side of 48 KiB, the limit and one above it
    for n in (1, 3, 1024, 1025, 2048, 2049, 4096, 4097):
        for s, r, pairs in ((1, 1, 0), (8, 1, 0), (1, 1, 1), (8, 8, 1)):
            for mode in (0, 1):
                for mirror in (0, 1):
                    got = after(f"# align N {n} S {s} R {r} pairs {pairs} mode {mode} mirror {mirror}")
                    assert got[-1] == f"C align_superimpose = {-3 if n > 4096 else 0}" and (got[0] == "Q align_workspace_bytes = 0") == (n > 4096)
                    search = launches(got, "align_search_kernel")
                    npairs = s * (s - 1) // 2 if pairs else s * r
                    assert len(launches(got, "align_compact_kernel")) == len(launches(got, "align_finalize_kernel")) == (n <= 4096)
                    assert len(search) == (n <= 4096 and npairs > 0)                 # S = R = 1 on itself: no pair, no search launch
                    if search:
                        assert search[0][0][0] == npairs * (2 if mirror else 1) and search[0][1][0] == (256 if n <= 1024 else 512) and search[0][2] == 24 * n
    assert {lds for _, _, lds in launches(side_recorded, "align_search_kernel")} >= {KB48, KB48 + 24}
    assert result("C align_superimpose ws exact") == 0
    assert result("C align_superimpose ws one byte short") == result("C align_superimpose ws misaligned") == -4
    assert result("C align_superimpose 2^31 pairs") == -3
    assert [(s, result(f"C align_apply S {s} N {n}")) for s in (65535, 65536) for n in (1, 256, 257)] == [(65535, 0)] * 3 + [(65536, -3)] * 3
    assert {g for g, _, _ in launches(side_recorded, "align_apply_kernel")} >= {(1, 1, 1), (1, 65535, 1), (2, 65535, 1)}

    # tmalign: ta_lds_bytes is 69 n + 27 (refine) and 32 n (search) at Nx = Ny = n, rounded up to 16: 48 KiB falls between 711 | 712
    # and between 1536 | 1537; the limit 2048 and one above it; 3 S R (mirror ? 2 : 1) problems within 2^20 and above
    for nx, ny in ((1, 1), (2, 1), (1, 2), (711, 711), (712, 712), (1536, 1536), (1537, 1537), (2048, 1), (1, 2048), (2048, 2048), (2049, 1), (1, 2049)):
        for s, r in ((1, 1), (3, 2)):
            for mirror in (0, 1):
                got = after(f"# tmalign Nx {nx} Ny {ny} S {s} R {r} mirror {mirror}")
                ok = max(nx, ny) <= 2048
                assert got[-1] == f"C tmalign_align = {0 if ok else -3}" and (got[0] == "Q tmalign_workspace_bytes = 0") == (not ok)
                kernels = [ln.split()[1] for ln in got if ln.startswith("L ")]
                assert kernels == (["tmalign_compact_kernel", "tmalign_refine_kernel", "tmalign_search_kernel", "tmalign_finalize_kernel"] if ok else [])
                if ok:
                    nm = 2 if mirror else 1
                    assert launches(got, "tmalign_compact_kernel")[0][0][0] == s + r and launches(got, "tmalign_finalize_kernel")[0][0][0] == s * r
                    assert launches(got, "tmalign_refine_kernel")[0][0][0] == 3 * s * r * nm and launches(got, "tmalign_search_kernel")[0][0][0] == s * r * nm
    up16 = lambda b: (b + 15) // 16 * 16
    assert up16(69 * 711 + 27) <= KB48 < up16(69 * 712 + 27) and 32 * 1536 <= KB48 < 32 * 1537
    assert {lds for _, _, lds in launches(side_recorded, "tmalign_refine_kernel")} >= {up16(69 * 711 + 27), up16(69 * 712 + 27), up16(69 * 2048 + 27)}
    assert {lds for _, _, lds in launches(side_recorded, "tmalign_search_kernel")} >= {32 * 1536, up16(32 * 1537), 32 * 2048}
    for s, r, mirror in ((349525, 1, 0), (349526, 1, 0), (174762, 1, 1), (174763, 1, 1)):
        got = after(f"# tmalign problems S {s} R {r} mirror {mirror}")
        assert got[-1] == f"C tmalign_align = {0 if 3 * s * r * (2 if mirror else 1) <= 2 ** 20 else -3}"
    assert 3 * 349525 <= 2 ** 20 < 3 * 349526 and 6 * 174762 <= 2 ** 20 < 6 * 174763
    assert result("C tmalign_align ws exact") == 0
    assert result("C tmalign_align ws one byte short") == result("C tmalign_align ws misaligned") == -4

    # quality: row tiles of 64, N and S at their limits and one above, exclude given and absent, the memset of S ints ahead of the census
    for n in (1, 64, 65, 32768, 32769):
        for s in (1, 65535, 65536):
            got, ok = after(f"# quality N {n} S {s}"), n <= 32768 and s <= 65535
            assert [ln.split(" = ")[1] for ln in got if ln.startswith("C ")] == [str(0 if ok else -3)] * 3
            tiles = (n + 63) // 64
            assert launches(got, "quality_lddt_kernel") == ([((tiles, s, 1), (256, 1, 1), 0)] if ok else [])
            assert launches(got, "quality_contacts_kernel") == ([((tiles, s, 1), (256, 1, 1), 0)] * 2 if ok else [])
            assert [ln.split()[2:] for ln in got if ln.startswith("M ")] == ([["0", str(4 * s)]] * 2 if ok else [])
            if ok:
                excluded = [ln.split(" args ")[1].split()[7] for ln in got if ln.startswith("L quality_contacts_kernel")]
                assert excluded[0] != excluded[1] and excluded[1] in ("(nil)", "0", "0x0")

    # condition: 3 N elements per sample without the sequence clamp and 24 N with it, on either side of a multiple of 256; b = 1 and 8
    for n in (1, 31, 32, 33, 85, 86, 255, 256, 257, 16777216):
        for b in (1, 8):
            for keep_z in (0, 1):
                for keep_seq in (0, 1):
                    line = f"C condition_rows N {n} b {b} keep_z {keep_z} keep_seq {keep_seq} = 0"
                    at = side_recorded.index(line)
                    if keep_z or keep_seq:
                        per = n * (24 if keep_seq else 3)
                        assert launches(side_recorded[at - 1:at], "condition_rows_kernel") == [(((per + 255) // 256, b, 1), (256, 1, 1), 0)]
                    else:
                        assert not side_recorded[at - 1].startswith("L ")                      # nothing kept: a successful no-op
    assert result("C condition_rows N 16777217 b 1 keep_z 1 keep_seq 1") == result("C condition_rows N 32 b 65536 keep_z 1 keep_seq 0") == -3
    assert result("C condition_rows N 32 b 65535 keep_z 1 keep_seq 1") == 0

    # sequence: row tiles of 8; the census grid is S (S + reference) pair blocks and ceil(21 N / 64) profile blocks
    for n in (1, 8, 9, 64, 65, 16777216, 16777217):
        for b in (1, 65535, 65536):
            got, ok = after(f"# sequence constrain N {n} b {b}"), n <= 16777216 and b <= 65535
            assert launches(got, "constrain_kernel") == ([(((n + 7) // 8, b, 1), (256, 1, 1), 0)] * 3 if ok else [])
            assert [ln.split(" = ")[1] for ln in got if ln.startswith("C ")] == [str(0 if ok else -3)] * 4      # (no rows: a no-op)
        for s in (1, 2, 4096, 4097):
            got, ok = after(f"# sequence decode, census N {n} S {s}"), n <= 16777216 and s <= 4096
            assert launches(got, "decode_kernel") == ([(((n + 7) // 8, s, 1), (256, 1, 1), 0)] * 3 if ok else [])
            profile = (21 * n + 63) // 64
            assert launches(got, "census_kernel") == ([((s * (s + 1) + profile, 1, 1), (64, 1, 1), 0), ((s * s + profile, 1, 1), (64, 1, 1), 0)] if ok else [])
            assert [ln.split(" = ")[1] for ln in got if ln.startswith("C ")] == [str(0 if ok else -3)] * 5
