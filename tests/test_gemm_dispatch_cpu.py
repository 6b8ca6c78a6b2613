"""CPU: which kernel of csrc/prd_gemm.hip a call lands on, for every case of tests/gemm_cases.py.  The trace build of the library prints a
line per launch instead of launching; tests/native/gemm_dispatch_trace.c makes ONE call per case with dummy addresses.  Held here:
every case runs the kernel(s) it states with the grid and block its shape implies; the table reaches every shipped kernel of the file
but the one never-launched form; the two (or more) cases beside a threshold land on different outcomes; the refusals return their
codes before any launch; and -- the float64 references alone, evaluated from the cases' seeds -- no row, column or tensor that
tests/test_gemm_edges.py measures lies under the floor of its measure, so the GPU test exempts nothing.  No device is touched."""
import os
import re
import subprocess

import pytest

import gemm_cases as T
import gemm_ref as R
from protein_redesign_amd import build

HAVE_HIPCC = os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
needs_hipcc = pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")

# what the issue of this table found reached by no operator-level GEMM test: each is the kernel of at least one GPU case here
ONCE_UNREACHED = {"ring_k576_many": T.ring(4, 1), "ring_k320": T.ring(8, 1), "ring_k448": T.ring(8, 1), "ring_k192": T.ring(4, 1),
                  "skinny8_k1024": T.SKINNY8, "tile64_t1089": T.TILE64, "slab_ragged_group": T.SLAB, "slab_sk1_odd": T.SLAB, "slab_sk2_odd": T.SLAB,
                  "slab_sk3": T.SLAB, "slab_sk5": T.SLAB, "slab_sk7": T.SLAB}


@pytest.fixture(scope="module")
def traced():
    """{case id: ([(kernel, grid, block, lds, args)], the C / Q line's value)}"""
    exe = build.build_gemm_dispatch(verbose=False)
    text = "\n".join(T.driver_line(c) for c in T.CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=600).stdout
    res, cur = {}, None
    for ln in out.split("\n"):
        if ln.startswith("# "):
            cur = res[ln[2:]] = [[], None]
        elif ln.startswith("L "):
            m = re.match(r"L (.*) grid (\d+) (\d+) (\d+) block (\d+) (\d+) (\d+) lds (\d+) args(.*)$", ln)
            v = tuple(map(int, m.groups()[1:8]))
            cur[0].append((m.group(1), v[:3], v[3:6], v[6], m.group(9).split()))
        elif ln.startswith(("C ", "Q ")):
            cur[1] = int(ln.split(" = ")[1])
    assert set(res) == {c.id for c in T.CASES}
    return res


def test_the_table_is_well_formed():
    assert len({c.id for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        assert c.entry in ("gemm", "ln_rows", "softmax_rows", "fc1_folded", "slab_ok", "fc1_folded_ok") and c.arith in ("fp32", "split16"), c.id
        assert c.gpu == (bool(c.kernels) and c.gpu), c.id                  # a refusal or a query is no GPU case
        assert (c.ret == 0) == bool(c.kernels) or c.entry.endswith("_ok"), c.id
        for off in (c.b_off, c.c_off) + ((c.a_off,) if c.entry == "gemm" else ()):
            assert off % 4 == 0, c.id
        if c.entry == "gemm":
            lda, ldb, ldc = T.dims(c)
            assert lda >= c.K and ldb >= (c.N if c.b_kn else c.K) and ldc >= c.N, c.id
            for name, v in (("act_from", T.act_from(c)), ("rowmask_cols", T.rowmask_cols(c)), ("n_split", T.n_split(c))):
                if v:                                                       # off every tile edge of the family (a multiple of 4 on the slab path)
                    assert 0 < v < c.N and v % 32 not in (0,), (c.id, name, v)
    for name, cases in T.pairs().items():
        assert len(cases) >= 2, name
    # the largest operand of a GPU case is 2560 x 1280, the largest output the 2112 x 2112 of the 1089-tile case
    for c in T.GPU_CASES:
        if c.entry == "gemm":
            G = c.G1 * c.G2
            assert max(G * c.M * c.K, G * c.N * c.K) <= 2560 * 1280 and G * c.M * c.N <= 2112 * 2112, c.id


@needs_hipcc
def test_every_case_runs_the_kernels_it_states_with_the_grid_its_shape_implies(traced):
    for c in T.CASES:
        launches, ret = traced[c.id]
        assert ret == c.ret, (c.id, ret)
        assert [(k, g, b) for k, g, b, _, _ in launches] == T.expected_launches(c), (c.id, launches)
        o = c.opts or {}
        for k, _, _, _, args in launches:
            if k == T.SLAB:             # A W ws M N K lda ldb tiles_m tiles_n nslab spw xmap wscale A2 lda2
                assert [int(a) for a in args[3:13]] == [c.M, c.N, c.K, *T.dims(c)[:2], T.ceil_div(c.M, 160), T.ceil_div(c.N, 64), o["nslab"], o["spw"], o["xmap"]], c.id
            elif k == T.SLAB_X:
                assert [int(a) for a in args[3:13]] == [c.M, c.N, c.K, c.K, c.K + 64, T.ceil_div(c.M, 160), T.ceil_div(c.N, 64), o["nslab"], o["spw"], o["xmap"]], c.id
            elif k == T.SLAB_REDUCE:
                assert int(args[-1]) == T.ceil_div(o["nslab"], o["spw"]), c.id
    ragged = T.BY_ID["slab_ragged_group"].opts
    assert ragged["nslab"] % ragged["spw"] != 0


@needs_hipcc
def test_refusals_return_their_codes_before_any_launch(traced):
    want = {"ring_ln_k1088_refused": T.ERR_UNSUPPORTED, "softmax_a_refused": T.ERR_UNSUPPORTED, "refuse_out_ln_no_ws": T.ERR_UNSUPPORTED,
            "epi_slab_out_ln_n516_refused": T.ERR_UNSUPPORTED, "refuse_lda": T.ERR_ALIGN, "refuse_ldb": T.ERR_ALIGN}
    for cid, code in want.items():
        assert traced[cid] == [[], code], cid
    for c in T.CASES:
        if c.ret < 0:
            assert traced[c.id] == [[], c.ret], c.id
    assert [traced[f"fc1_ok_m{m}"][1] for m in (95, 96, 640, 641)] == [0, 1, 1, 0]
    assert [traced[f"fc1_m{m}"][1] for m in (95, 96, 640, 641)] == [T.ERR_UNSUPPORTED, 0, 0, T.ERR_UNSUPPORTED]


@needs_hipcc
def test_the_table_reaches_every_shipped_kernel_but_the_never_launched_form(traced):
    shipped = set(build.resource_usage(sources=["prd_gemm.hip"]))
    assert T.NEVER_LAUNCHED <= shipped
    stated = {k for c in T.CASES for k in c.kernels}
    assert stated == shipped - T.NEVER_LAUNCHED
    on_gpu = {k for c in T.GPU_CASES for k in c.kernels}
    assert on_gpu == stated                                                # ... and each of them by a case that runs on the device
    for cid, kernel in ONCE_UNREACHED.items():
        assert T.BY_ID[cid].gpu and kernel in T.BY_ID[cid].kernels and kernel in [k for k, *_ in traced[cid][0]], cid
    assert len(traced["ring_k576_many"][0]) == 1 and traced["ring_k576_many"][0][0][1][0] > 1024 and T.BY_ID["ring_k576_many"].K > 512
    assert {T.BY_ID[i].opts["xmap"] for i in ("slab_sk1_odd", "slab_sk2_odd", "slab_sk3", "slab_sk5", "slab_sk7")} == {0}
    assert {T.BY_ID[i].opts["xmap"] for i in ("slab_sk8", "slab_sk1_even", "slab_sk2_even")} == {1, 2}


@needs_hipcc
def test_every_threshold_pair_lands_on_different_outcomes(traced):
    def outcome(c):
        launches, ret = traced[c.id]
        o = c.opts or {}
        return (tuple(k for k, *_ in launches), ret, o.get("xmap"), o.get("spw"))
    for name, cases in T.pairs().items():
        outs = [outcome(c) for c in cases]
        assert len(set(outs)) == len(outs), (name, outs)
    want = ("ring k512: 64 | 65", "ring k512: 192 | 193", "ring k256: 128 | 129", "ring chunks 1 | 2", "ring chunks 2 | 3", "ring chunks 4 | 5", "ring chunks 8 | 9",
            "ring chunks 16 | 17", "ring beyond 8 chunks: 1024 | 1025", "a_ln: K 1024 | 1088", "64 x 64 tiles 511 | 512", "h2: K 992 | 1024", "fp32 skinny: K 1020 | 1024",
            "fp32 skinny, K 1024: 512 | 513", "fp32: 64 x 64 tiles 511 | 512", "fp32: 64 x 64 tiles 1024 | 1025", "fp32, more than 1024 tiles: M 64 | 65",
            "slab: M 95 | 96", "slab: tiles x slabs 127 | 128", "slab: tiles x slabs 512 | 528", "slab: N % 4", "slab: K % 128", "slab: 4096 | 4097 tiles", "slab map, one slab group",
            "slab map, two slab groups", "slab map: 7 | 8", "out_ln: N 512 | 516", "fc1 folded: M 95 | 96", "fc1 folded: M 640 | 641", "ln_rows, C 64: rows 4095 | 4096",
            "ln_rows, C 64: ldx % 4", "ln_rows, C 64: x 16-byte aligned", "ln_rows, 4096 rows: C 63 | 64", "ln_rows, 4096 rows: C 64 | 65", "[K][N] ring: K 512 | 576")
    for prefix in want:
        assert any(name.startswith(prefix) for name in T.pairs()), prefix


@needs_hipcc
def test_slab_queries_agree_with_the_dispatch(traced):
    for c in T.CASES:
        if c.entry == "slab_ok":
            assert traced[c.id][1] == c.ret, c.id
    for c in T.CASES:
        if c.entry == "gemm" and c.slab and c.arith == "split16" and c.epi == T.E0 and not c.tile_hint:
            took = T.SLAB in c.kernels
            key = f"slab_ok_{c.M}x{c.N}x{c.K}"
            if key in traced:
                assert traced[key][1] == int(took), c.id


@pytest.mark.parametrize("case", T.GPU_CASES, ids=lambda c: c.id)
def test_no_measured_row_column_or_tensor_of_the_reference_lies_under_its_floor(case):
    want = R.reference(case, R.inputs(case))
    assert want
    for name, w in want.items():
        assert R.floors(w) == [], (case.id, name)
