"""GPU: every kernel-selection switch of the README table computes the right numbers.

tests/test_launch_trace_cpu.py pins WHICH kernel and grid the host picks under every PRD_TUNE_* bit; here the kernel or grid so
picked is held to float64, and the host-side switches (module attributes, the two variables read at call time) with them:
  1. the whole step the benchmark replays (N = 320, four blocks) under every inference switch of tests/switch_cases.py, each alone,
     in both arithmetics: against the stored oracle, bit-reproducible, and against the default arm;
  2. each selected kernel alone at the smallest shapes where it can go wrong -- rows that are no multiple of a tile, grids that are no
     multiple of 8, surplus workgroups, fewer tasks than waves, batches with a masked tail -- against float64 on the whole tensor;
  3. the training switches, each off alone, against the reference's and the oracle's gradients.
The switches act in split-16 arithmetic unless said; the operator-level cases therefore run in it.  No test leaves a switch set."""
import contextlib
import importlib
import math
import os

import pytest
import torch
import torch.nn.functional as F

import prd_oracle as O
import switch_cases as SC
import test_hip_parity as HP
from conftest import mismatch_report, rel_l2
from protein_redesign_amd import _lib, ops, torch_ref as TR, trunk
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.synthetic import NoiseSource, batch_to, synthetic_batch
from test_hip_parity import BLOCK_TOL, DEV, OP_TOL, cu, gemm_mode  # noqa: F401  (gemm_mode: the fixture)

pytestmark = pytest.mark.gpu
ARM_TOL = 2e-6          # against the default arm where both arms use the same arithmetic in another order
STEP_ARMS, TRAIN_ARMS = SC.arms("step"), SC.arms("train")
STEP_IDS, TRAIN_IDS = [a[0] for a in STEP_ARMS], [a[0] for a in TRAIN_ARMS]


def tune_bits(name):
    return SC.bits(name, _lib._TUNE)


@contextlib.contextmanager
def tuned(*names):
    """the PRD_TUNE_* bits ``names`` on top of the process's switch word; the word comes back on exit"""
    lib = _lib.lib()
    tune0 = lib.prd_get_tune()
    word = tune0
    for n in names:
        word |= tune_bits(n)
    try:
        assert lib.prd_set_tune(word) == 0
        yield
    finally:
        assert lib.prd_set_tune(tune0) == 0


@contextlib.contextmanager
def split16():
    lib = _lib.lib()
    prev = lib.prd_get_gemm_mode()
    try:
        assert lib.prd_set_gemm_mode(1) == 0
        yield
    finally:
        assert lib.prd_set_gemm_mode(prev) == 0


@contextlib.contextmanager
def switched(name, s, monkeypatch):
    """one registry entry in force, the way the entry says"""
    if s.how == "tune":
        with tuned(s.target):
            yield
    elif s.how == "attr":
        module, attr = s.target.split(".")
        with monkeypatch.context() as mp:
            mp.setattr(importlib.import_module("protein_redesign_amd." + module), attr, s.attr_value)
            yield
    else:
        assert s.how == "env"
        with monkeypatch.context() as mp:
            mp.setenv(name, s.value)
            yield


def row_errors(got, want):
    """rel-L2 of every row [b, i, :, :] (the expression of test_triangle_attention_long_rows_split_tail)"""
    return (got - want).flatten(2).norm(dim=2) / want.flatten(2).norm(dim=2).clamp_min(1e-30)


def randomised(mod, g):
    """``mod`` with every parameter drawn: matrices ~ 1 / sqrt(fan-in), vectors ~ 1 / 3 (the 'final' / 'gating' initialisers are zeros)"""
    sd = {k: torch.randn(v.shape, generator=g) / (math.sqrt(v.shape[-1]) if v.dim() == 2 else 3.0) for k, v in mod.state_dict().items()}
    mod.load_state_dict(sd)
    return mod.to(DEV), {k: v.double() for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------
# 1. the whole step under every switch
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def step_case():
    args, model, params, pb, z, seq_t, t = HP._full_size_case(64, 256, 4, seed=4)
    dpb = batch_to(pb, DEV)
    return dict(args=args, model=model, dpb=dpb, z=cu(z), seq_t=cu(seq_t), t=cu(t), want=HP._stored_oracle_step("n320_b4_s4"), default={})


def _step(model, c):
    with torch.inference_mode():
        out = model.sample_step(c["dpb"], c["z"], c["seq_t"], c["dpb"]["residue_and_atom_mask"], c["t"])
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _default_step(c, mode):
    """the default arm, once per arithmetic: no switch is in force while it runs"""
    if mode not in c["default"]:
        assert _lib.lib().prd_get_tune() == 0 and not os.environ.get("PRD_TASK_QUEUE") and os.environ.get("PRD_SIDE_STREAM", "0") != "1"
        base = _step(c["model"], c)
        for o, w in zip(base, c["want"]):
            assert rel_l2(o, w) < 2 * BLOCK_TOL
        c["default"][mode] = base
    return c["default"][mode]


@pytest.mark.parametrize("arm", STEP_ARMS, ids=STEP_IDS)
def test_whole_step_under_the_switch(arm, gemm_mode, step_case, monkeypatch):
    """model.sample_step at the shape bench.py replays, the switch alone: within the bound of the default arm against the stored oracle
    (2 * BLOCK_TOL on both outputs), finite, equal bits on two runs, and < 1e-5 from the default arm -- EQUAL BITS where the switch
    cannot apply: a split-16-only switch under fp32 arithmetic, and the switches whose forms only the -DPRD_AB library carries."""
    arm_id, name, s = arm
    c = step_case
    monkeypatch.delenv("PRD_TASK_QUEUE", raising=False)
    monkeypatch.delenv("PRD_SIDE_STREAM", raising=False)
    base = _default_step(c, gemm_mode)
    with switched(name, s, monkeypatch):
        model = c["model"]
        if name == "PRD_SIDE_STREAM":           # SideStream reads the variable when it is constructed: a model built under it
            model, _ = HP.build(c["args"], seed=4)
        runs = [_step(model, c) for _ in range(2)]
        if name == "PRD_SIDE_STREAM":
            assert model._side.enabled and model._side.stream is not None
        if name == "PRD_TASK_QUEUE":
            assert ops._QUEUES
            for q in ops._QUEUES.values():
                assert int(q.abs().sum()) == 0, "a task-queue counter is not back at zero after the step"
    assert _lib.lib().prd_get_tune() == 0
    # (a run of this file against the A/B library itself, through PRD_LIB, does carry the ab_only forms)
    exact = (s.ab_only and "libprd_hip_ab" not in _lib.LIB_PATH) or (s.split16_only and gemm_mode == "fp32")
    for k, what in enumerate(("noise_pred", "seq_pred")):
        got, again, dflt, want = runs[0][k], runs[1][k], base[k], c["want"][k]
        assert torch.isfinite(got).all(), (arm_id, what)
        err, arm_err = rel_l2(got, want), rel_l2(got, dflt)
        print(f"SWITCH step {arm_id} [{gemm_mode}] {what}: vs float64 {err:.3e} (default arm {rel_l2(dflt, want):.3e}), vs default arm {arm_err:.3e}")
        assert torch.equal(got, again), (arm_id, what, "two runs under the switch differ", rel_l2(again, got))
        assert err < 2 * BLOCK_TOL, (arm_id, what, mismatch_report(got, want))
        if exact:
            assert torch.equal(got, dflt), (arm_id, what, "the switch cannot apply here, yet the bits changed", mismatch_report(got, dflt))
        else:
            assert arm_err < 1e-5, (arm_id, what, mismatch_report(got, dflt))


def test_side_stream_inside_the_captured_graph(golden, monkeypatch):
    """PRD_SIDE_STREAM=1 through sample()'s captured step graph (small golden model, 8 steps: the first eager, the rest replayed; the
    forked launches are parallel branches of the graph): the default loop reproduces itself bit for bit, and the loop of a model built
    under the variable equals it bit for bit -- the same kernels on the same inputs, only their streams differ."""
    monkeypatch.delenv("PRD_SIDE_STREAM", raising=False)
    case, z, args, model, params = HP.golden_case(golden, "small64")
    assert model.use_hip_graph and args["num_steps"] == 8
    one = batch_to(synthetic_batch([tuple(case["traj_sample"])], esm_dim=args["esm_dim"], seed=case["batch_seed"] + 500), DEV)

    def loop(m):
        out = m.sample({k: (v.clone() if torch.is_tensor(v) else v) for k, v in one.items()}, sources=[NoiseSource(HP.NOISE_SEED, 0)])
        torch.cuda.synchronize()
        return [o.cpu() for o in out]

    first, second = loop(model), loop(model)
    assert not model._side.enabled
    assert all(torch.equal(a, b) for a, b in zip(first, second)), "the default loop does not reproduce itself"
    assert rel_l2(first[0], z["traj_pos"]) < HP.TRAJ_TOL and rel_l2(first[1], z["traj_logits"]) < HP.TRAJ_TOL
    monkeypatch.setenv("PRD_SIDE_STREAM", "1")
    side_model, _ = HP.build(args, case["weight_seed"], case.get("weight_style", "random"), case.get("weight_scales"))
    got = loop(side_model)
    assert side_model._side.enabled and side_model.use_hip_graph
    for a, b, what in zip(got, first, ("positions", "logits")):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), (what, mismatch_report(a, b))


# ---------------------------------------------------------------------------------------------------
# 2. each selected kernel alone, at the edges
# ---------------------------------------------------------------------------------------------------

def og_float64(pair, mask, wts, H, c, ending):
    """float64: the gated head outputs [b,N,N,H c] of a triangle attention BEFORE its output projection, in the orientation of the pair
    tensor (modules.py:185-225 over the rows of pair, or of its transpose); 64 rows at a time"""
    wq, wk, wv, wg, bg = [w.detach().cpu().double() for w in wts]
    x, mask = pair.double(), mask.double()
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    if ending:
        x, m2 = x.transpose(1, 2), m2.transpose(1, 2)
    b, N = mask.shape
    out = torch.empty(b, N, N, H * c, dtype=torch.float64)
    for r0 in range(0, N, 64):
        xn = F.layer_norm(x[:, r0:r0 + 64], x.shape[-1:], None, None, 1e-5)
        split = lambda t: t.reshape(b, -1, N, H, c).transpose(-2, -3)          # [b, rows, H, N, c]
        q, k, v = split(xn @ wq.t()), split(xn @ wk.t()), split(xn @ wv.t())
        gate = split(torch.sigmoid(xn @ wg.t() + bg))
        logits = (q / math.sqrt(c)) @ k.transpose(-1, -2)
        logits = logits.masked_fill(m2[:, r0:r0 + 64].unsqueeze(-2).unsqueeze(-2) < 0.5, -(2.0 ** 15))
        out[:, r0:r0 + 64] = (gate * (torch.softmax(logits, -1) @ v)).transpose(-2, -3).reshape(b, -1, N, H * c)
    return out.transpose(1, 2) if ending else out


def attention_case(P, b, N, valid, mode, seed):
    g = torch.Generator().manual_seed(seed)
    mod, sd = randomised(trunk.TriangleAttention(P, 16, 4, mode), g)
    pair = torch.randn(b, N, N, P, generator=g)
    mask = torch.ones(b, N)
    mask[-1, valid:] = 0
    return mod, pair, mask


def check_attention(got, want, ending, what, rerun=None):
    """OP_TOL on the whole tensor, 2 * OP_TOL on the worst attention row"""
    assert torch.isfinite(got).all(), (what, mismatch_report(got, want))
    err = rel_l2(got, want)
    g, w = (got.transpose(1, 2), want.transpose(1, 2)) if ending else (got, want)
    rows = row_errors(g.double(), w.double())
    print(f"SWITCH op {what}: vs float64 {err:.3e}, worst row {float(rows.max()):.3e}")
    assert err < OP_TOL, (what, mismatch_report(got, want, rerun))
    assert float(rows.max()) < 2 * OP_TOL, (what, "row", int(rows.argmax()), mismatch_report(got, want, rerun))
    return err


V2_SHAPES = [(1, 33, 33), (1, 97, 64), (3, 200, 200), (2, 288, 280), (1, 384, 384)]


@pytest.mark.parametrize("ending", [False, True], ids=["starting", "ending"])
@pytest.mark.parametrize("b,N,valid", V2_SHAPES)
@pytest.mark.parametrize("P", [32, 64])
def test_short_row_core_with_one_barrier_per_phase(P, b, N, valid, ending):
    """PRD_TA2_V3=0: tri_attn_core_v2_kernel at rows other than N = 352 (the only length that reaches it by default): more waves than
    query blocks (33), a padded last tile (97 with 64 valid), batches, the largest short row.  The whole og tensor against float64."""
    mod, pair, mask = attention_case(P, b, N, valid, "ending" if ending else "starting", 3000 + 7 * N + P + ending)
    wts = mod.attn.weights()[:5]
    want = og_float64(pair, mask, wts, 4, 16, ending)
    dp, dm = cu(pair), cu(mask)

    def run():
        og = torch.full((b, N, N, 64), float("nan"), device=DEV)
        return ops.tri_attn_core_v2(dp, dm, wts, 4, 16, ending=ending, og=og).cpu()
    dflt = run()
    with tuned("TA2_NO_V3"):
        assert _lib.lib().prd_tri_attn_v2_form(N, P) == 1
        got = run()
        check_attention(got, want, ending, f"TA2_NO_V3 P {P} b {b} N {N} {'ending' if ending else 'starting'}", run)
    arm = rel_l2(got, dflt)
    print(f"SWITCH op TA2_NO_V3 P {P} b {b} N {N}: vs default arm {arm:.3e}")
    assert arm < ARM_TOL, mismatch_report(got, dflt)


XCD8_SHAPES = [(1, 97, 97), (1, 130, 123), (2, 70, 61), (1, 449, 440)]


def _attention_update(mod, pair, mask):
    return mod.run(cu(pair), cu(mask), residual=False, out=torch.full(pair.shape, float("nan"), device=DEV)).cpu()


def _update_float64(mod, pair, mask, ending):
    return TR.triangle_attention(pair.double(), mask.double(), *[w.detach().cpu().double() for w in mod.attn.weights()], 4, 16, ending=ending)


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("b,N,valid", XCD8_SHAPES)
@pytest.mark.parametrize("P", [32, 64])
def test_rows_per_head_not_rounded_to_eight(P, b, N, valid, mode):
    """PRD_TA2_XCD8=0: 49, 44, 47 and 57 rows in flight per head instead of 56, 48, 48 and 64 -- grids of the overlapped-phase and the
    long-row core that are no multiple of 8, under a block -> (row, head) map written for multiples of 8.  Whole update against float64."""
    ending = mode == "ending"
    mod, pair, mask = attention_case(P, b, N, valid, mode, 4000 + 7 * N + P + ending)
    want = _update_float64(mod, pair, mask, ending)
    with split16():
        assert _lib.lib().prd_tri_attn_v2_form(N, P) == (3 if N > 384 else 2)
        dflt = _attention_update(mod, pair, mask)
        with tuned("TA2_NO_XCD8"):
            run = lambda: _attention_update(mod, pair, mask)
            got = run()
            check_attention(got, want, ending, f"TA2_NO_XCD8 P {P} b {b} N {N} {mode}", run)
    arm = rel_l2(got, dflt)
    print(f"SWITCH op TA2_NO_XCD8 P {P} b {b} N {N} {mode}: vs default arm {arm:.3e}")
    assert arm < ARM_TOL, mismatch_report(got, dflt)


NO_LONG_SHAPES = [(385, 385), (417, 416), (449, 449)]


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("N,valid", NO_LONG_SHAPES)
@pytest.mark.parametrize("P", [32, 64])
def test_long_rows_without_the_second_generation(P, N, valid, mode):
    """PRD_TA2_LONG=0, the first long rows: the second-generation core refuses them (form 0) and -- the first-generation split-16 cores
    being compiled out of the shipped library -- the fp32 kernels of that length serve them, as under fp32 arithmetic (README).  The
    arithmetic changes with the switch: float64 is the only yardstick."""
    ending = mode == "ending"
    mod, pair, mask = attention_case(P, 1, N, valid, mode, 5000 + 7 * N + P + ending)
    want = _update_float64(mod, pair, mask, ending)
    lib = _lib.lib()
    with split16():
        assert lib.prd_tri_attn_v2_form(N, P) == 3
        with tuned("TA2_NO_LONG"):
            assert lib.prd_tri_attn_v2_form(N, P) == 0 and not ops.tri_attn_v2_supported(N, P)
            variant = ops.tri_attn_variant(N, P)
            if "libprd_hip_ab" not in _lib.LIB_PATH:        # (the A/B library keeps the first-generation split-16 kernels)
                assert lib.prd_set_gemm_mode(0) == 0
                assert variant == ops.tri_attn_variant(N, P) == (1 if N >= 449 else 0)
                assert lib.prd_set_gemm_mode(1) == 0
            run = lambda: _attention_update(mod, pair, mask)
            check_attention(run(), want, ending, f"TA2_NO_LONG P {P} N {N} {mode}", run)


@pytest.mark.parametrize("S", [128, 256, 512])
@pytest.mark.parametrize("P", [32, 64])
def test_outer_linear_round_two_kernel(P, S):
    """PRD_OL_VARIANT=1 at the widths of the K-split kernel (S = 128 / 256 / 512 otherwise never reach outer_linear_res_kernel<P, 8, true>):
    b = 2, ragged N = 70 as in test_outer_linear_full_width, against float64."""
    g = torch.Generator().manual_seed(6000 + P + S)
    N = 70
    mod = trunk.OuterLinear(S, P)
    w, bvec = torch.randn(P, 2 * S, generator=g) / math.sqrt(2 * S), 0.1 * torch.randn(P, generator=g)
    mod.load_state_dict({"linear.weight": w, "linear.bias": bvec})
    mod = mod.to(DEV)
    single = torch.randn(2, N, S, generator=g) * 1.5 + 0.3
    want = O.outer_linear({"ol.linear.weight": w.double(), "ol.linear.bias": bvec.double()}, "ol", single.double())

    def run():
        out = torch.full((2, N, N, P), float("nan"), device=DEV)
        return mod.run(cu(single), out, residual=False, out=out).cpu()
    with split16():
        dflt = run()
        with tuned("OL_GEN2"):
            got = run()
    err, arm = rel_l2(got, want), rel_l2(got, dflt)
    print(f"SWITCH op OL_GEN2 P {P} S {S}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
    assert torch.isfinite(got).all() and err < OP_TOL, mismatch_report(got, want, run)
    assert arm < ARM_TOL, mismatch_report(got, dflt)


TMP_SHAPES = [(2, 45, 37), (1, 97, 97), (1, 190, 181)]


@pytest.mark.parametrize("form", ["outgoing", "incoming", "chain"])
@pytest.mark.parametrize("b,N,valid", TMP_SHAPES)
def test_triangle_multiplication_projection_on_16_waves(b, N, valid, form):
    """PRD_TMP_NW=16 (pair_dim 64 only): tri_mul_proj_kernel<64, 16, true> in prd_tri_mul, and in prd_tri_mul_chain, whose FIRST projection
    stage takes the bit too (its fused second one, tri_mul_out_proj_kernel, has no 16-wave form) -- a ragged ldn (45 -> 64), fewer tasks
    than waves, more than one round of tasks; masked tail.  Against float64."""
    P = 64
    g = torch.Generator().manual_seed(7000 + N)
    mods, params = {}, {}
    for m in ("outgoing", "incoming"):
        mods[m], sd = randomised(trunk.TriangleMultiplication(P, m), g)
        params.update({f"{m}.{k}": v for k, v in sd.items()})
    pair = torch.randn(b, N, N, P, generator=g)
    mask = torch.ones(b, N)
    mask[-1, valid:] = 0
    m2 = (mask.unsqueeze(-1) * mask.unsqueeze(-2)).double()
    if form == "chain":
        want = pair.double() + O.triangle_multiplication(params, "outgoing", pair.double(), m2, False)
        want = want + O.triangle_multiplication(params, "incoming", want, m2, True)
    else:
        want = O.triangle_multiplication(params, form, pair.double(), m2, form == "incoming")

    def run():
        if form == "chain":
            return ops.tri_mul_chain_(cu(pair).clone(), cu(mask), mods["outgoing"].weights(), mods["incoming"].weights()).cpu()
        return mods[form].run(cu(pair), cu(mask), residual=False, out=torch.full(pair.shape, float("nan"), device=DEV)).cpu()
    with split16():
        assert form != "chain" or ops.tri_mul_chain_supported(N, P)
        dflt = run()
        with tuned("TMP_NW16"):
            got = run()
    err, arm = rel_l2(got, want), rel_l2(got, dflt)
    print(f"SWITCH op TMP_NW16 {form} b {b} N {N}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
    assert torch.isfinite(got).all() and err < OP_TOL, mismatch_report(got, want, run)
    assert arm < ARM_TOL, mismatch_report(got, dflt)


@pytest.mark.parametrize("M,N,K,a_ln", [(320, 8192, 512, False), (385, 4740, 512, False), (385, 4740, 1024, False), (320, 8192, 512, True), (385, 4740, 512, True)])
def test_tile_gemm_with_the_xcd_column_map(M, N, K, a_ln):
    """PRD_GEMM_XCDCOLS=1: gemm_h2_kernel<1> and <4> under the XCD column map (tile_hint = -8), reachable in no other way.  The production
    projection (128 column tiles) and N = 4740: 75 column tiles, no multiple of 8 -- a grid of 560 workgroups for 525 tiles, so 35 surplus
    ones that must write nothing, and a ragged last column tile (4740 = 74 x 64 + 4) -- with the epilogue of the packed projections
    (column scale, bias, sigmoid from a column on), once more with the LayerNorm of the A rows fused.  Against float64."""
    g = torch.Generator().manual_seed(8000 + M + N + K)
    x = torch.randn(M, K, generator=g) * 1.5 + 0.7
    w, bias = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    cs = 0.5 + torch.rand(N, generator=g)
    act_from = 3 * (N // 4) + 1
    a = O.ln(x.double()) if a_ln else x.double()
    want = (a @ w.double().t()) * cs.double() + bias.double()
    want[:, act_from:] = torch.sigmoid(want[:, act_from:])

    def run():
        out = torch.full((M, N), float("nan"), device=DEV)
        return ops.gemm(cu(x), cu(w), out, M, N, K, K, K, N, bias=cu(bias), colscale=cu(cs), act=2, act_from=act_from, a_ln=a_ln).cpu()
    with split16():
        assert ops.split16_gemm_ok(M, N, K)
        dflt = run()
        with tuned("GEMM_XCD_COLS"):
            got = run()
    err, arm = rel_l2(got, want), rel_l2(got, dflt)
    print(f"SWITCH op GEMM_XCD_COLS M {M} N {N} K {K} a_ln {int(a_ln)}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
    assert torch.isfinite(got).all() and err < OP_TOL, mismatch_report(got, want, run)
    assert arm < ARM_TOL, mismatch_report(got, dflt)


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("M,N", [(320, 64), (77, 33), (50, 96), (320, 512), (90, 40)])
def test_ring_gemm_one_wave_group(M, N, K):
    """PRD_GEMM_KG=0 at the shapes of test_operand_ring_gemm_edges with K = 256 and 512: 6 to 160 tiles, where the default splits the chunk
    loop over two or four wave groups (<2, 2>, <2, 4>, <4, 2>) and the switch keeps one (<4, 1>, <8, 1>) -- epilogue (bias, ReLU, residual)
    and the fused LayerNorm with the normalised rows on the side.  Against float64."""
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x = torch.randn(M, K, generator=g) * 1.5 + 0.7
    w, bvec = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    want = torch.relu(x.double() @ w.double().t() + bvec.double()) + res.double()
    want_ln = O.ln(x.double()) @ w.double().t() + bvec.double()

    def run():
        out = ops.linear(cu(x), cu(w), cu(bvec), act=1, resid=cu(res), out=torch.full((M, N), float("nan"), device=DEV)).cpu()
        xn, o2 = torch.full((M, K), float("nan"), device=DEV), torch.full((M, N), float("nan"), device=DEV)
        ops.gemm(cu(x), cu(w), o2, M, N, K, K, K, N, bias=cu(bvec), a_ln=True, ln_out=xn)
        return out, xn.cpu(), o2.cpu()
    with split16():
        dflt = run()
        with tuned("GEMM_NO_KG"):
            got = run()
    for what, gt, wt, df in zip(("linear", "ln_out", "ln linear"), got, (want, O.ln(x.double()), want_ln), dflt):
        err, arm = rel_l2(gt, wt), rel_l2(gt, df)
        print(f"SWITCH op GEMM_NO_KG M {M} N {N} K {K} {what}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
        assert torch.isfinite(gt).all() and err < OP_TOL, (what, mismatch_report(gt, wt))
        assert arm < ARM_TOL, (what, mismatch_report(gt, df))


@pytest.mark.parametrize("Nk,c", [(128, 96), (192, 70)])
def test_batched_gemms_on_the_k_split_kernel(Nk, c):
    """PRD_GEMM_BRING=0 on the calls of test_ring_gemm_batched_and_kn: the per-head logits q k^T + bias (batch grid) and P V with the gate
    (B as [K][N]) on the fp32 K-split kernels; the row softmax inside the product (a_ln = 2) exists on the ring only and is REFUSED, which
    the caller takes as "softmax by its own launch".  The arithmetic changes with the switch: against float64 only."""
    g = torch.Generator().manual_seed(Nk + c)
    b, H, N = 2, 4, Nk
    L = 4 * H * c
    qkvg = torch.randn(b, N, L, generator=g) / math.sqrt(c) * 3
    bias = torch.randn(b, H, N, N, generator=g)
    q, k, v, gate = [t.view(b, N, H, c).double() for t in qkvg.split(H * c, dim=-1)]
    want_logits = torch.einsum("bihc,bjhc->bhij", q, k) + bias.double()
    P_ = torch.softmax(want_logits, -1)
    want_o = (torch.einsum("bhij,bjhc->bihc", P_, v) * gate).reshape(b, N, H * c)
    dq = cu(qkvg)
    pv = dict(b_off=2 * H * c, G1=b, G2=H, sa=(H * N * N, N * N), sb=(N * L, c), sc=(N * H * c, c), b_kn=True, mulmat=dq, mul_off=3 * H * c,
              smu=(N * L, c), ldmul=L, a_scale=1024.0)
    with split16(), tuned("GEMM_NO_BATCHED_RING"):
        logits = torch.full((b, H, N, N), float("nan"), device=DEV)
        ops.gemm(dq, dq, logits, N, N, c, L, L, N, b_off=H * c, G1=b, G2=H, sa=(N * L, c), sb=(N * L, c), sc=(H * N * N, N * N),
                 addmat=cu(bias), sad=(H * N * N, N * N), ldadd=N)
        o = torch.full((b, N, H * c), float("nan"), device=DEV)
        ops.gemm(cu(P_.float()), dq, o, N, c, N, N, L, H * c, **pv)
        o2 = torch.full((b, N, H * c), float("nan"), device=DEV)
        refused = ops.gemm(cu(want_logits.float()), dq, o2, N, c, N, N, L, H * c, a_ln=2, unsupported_ok=True, **pv)
        torch.cuda.synchronize()
    assert refused is None and bool(torch.isnan(o2).all()), "a_ln = 2 off the ring kernel must be refused before any launch"
    for what, gt, wt in (("logits", logits.cpu(), want_logits), ("P V", o.cpu(), want_o)):
        err = rel_l2(gt, wt)
        print(f"SWITCH op GEMM_NO_BATCHED_RING Nk {Nk} c {c} {what}: vs float64 {err:.3e}")
        assert torch.isfinite(gt).all() and err < OP_TOL, (what, mismatch_report(gt, wt))


@pytest.mark.parametrize("N", [97, 96])
def test_wide_head_attention_without_the_batched_ring(N, monkeypatch):
    """ops.gated_attention_single with wide heads (b = 2, H = 4, c = 128, key mask) in its three forms: prd_spa_attn_core; PRD_SPA_CORE=0 =
    logits GEMM + softmax + P V on the ring; and PRD_GEMM_BRING=0 on top, where a_ln = 2 is refused and the softmax runs as its own
    launch.  N = 97 (the issue's shape; its padded logits rows keep the softmax separate in either case) and N = 96, where the refusal
    is what selects the fallback.  Each against float64."""
    b, H, c, S = 2, 4, 128, 128
    g = torch.Generator().manual_seed(9000 + N)
    x = torch.randn(b, N, S, generator=g) * 1.5 + 0.4
    wq, wk, wv, wg = [torch.randn(H * c, S, generator=g) / math.sqrt(S) for _ in range(4)]
    wq = wq * 3.0                                                   # logits of a few units
    bg = torch.randn(H * c, generator=g) / 3
    wo, bo = torch.randn(S, H * c, generator=g) / math.sqrt(H * c), torch.randn(S, generator=g) / 3
    bias = torch.randn(b, H, N, N, generator=g)
    mask = torch.ones(b, N)
    mask[:, N - 7:] = 0
    mask[0, 3] = 0
    want = TR.gated_attention(x.double(), mask.double(), *[t.double() for t in (wq, wk, wv, wg, bg, wo, bo)], H, c, bias=bias.double())
    dw = [cu(t) for t in (wq, wk, wv, wg, bg)]
    packed = ops.pack_attention(*dw, 1.0 / math.sqrt(c))
    dwo, dbo, dx, dm, dbias = cu(wo), cu(bo), cu(x), cu(mask), cu(bias)

    def run():
        return ops.gated_attention_single(dx, dm, dbias, packed, dwo, dbo, H, c, key_mask=True, resid=None, ln_a=True, logits_fp32=False).cpu()
    outs = {}
    with split16():
        outs["spa core"] = run()
        monkeypatch.setattr(ops, "SPA_CORE", False)
        outs["SPA_CORE=0"] = run()
        with tuned("GEMM_NO_BATCHED_RING"):
            outs["SPA_CORE=0 GEMM_NO_BATCHED_RING"] = run()
    for what, got in outs.items():
        err = rel_l2(got, want)
        rows = (got.double() - want).norm(dim=-1) / want.norm(dim=-1).clamp_min(1e-30)
        print(f"SWITCH op attention N {N} {what}: vs float64 {err:.3e}, worst row {float(rows.max()):.3e}")
        assert torch.isfinite(got).all() and err < OP_TOL, (what, mismatch_report(got, want))
        assert float(rows.max()) < 2 * OP_TOL, (what, int(rows.argmax()))


@pytest.mark.parametrize("M,N,K", [(173, 516, 1024), (96, 2048, 512)])
def test_linears_without_the_k_slab_path(M, N, K):
    """PRD_GEMM_SLAB=0 on the calls of test_k_slab_gemm: prd_gemm_slab_ok turns 0, a linear that ASKS for the slab path (slab=True, with a
    workspace, with the row sums for the LayerNorm by linearity) runs on the ring kernels instead.  Against float64."""
    g = torch.Generator().manual_seed(M + 3 * N + K)
    x = torch.randn(M, K, generator=g) * 1.5 + 0.7
    w, bvec = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    xd, wd = x.double(), w.double()
    want = torch.relu(xd @ wd.t() + bvec.double()) + res.double()
    want2 = torch.relu(O.ln(xd) @ wd.t() + bvec.double())
    wsum = cu(wd.sum(1).float())

    def run():
        out = [ops.linear(cu(x), cu(w), cu(bvec), act=1, resid=cu(res), slab=True, out=torch.full((M, N), float("nan"), device=DEV)).cpu()]
        if K <= 512:
            out.append(ops.linear(cu(x), cu(w), cu(bvec), act=1, ln_a=True, slab=True, wsum=wsum, out=torch.full((M, N), float("nan"), device=DEV)).cpu())
        return out
    with split16():
        assert ops.slab_ok(M, N, K)
        dflt = run()
        with tuned("GEMM_NO_SLAB"):
            assert not ops.slab_ok(M, N, K) and _lib.lib().prd_gemm_slab_ok(M, N, K) == 0
            got = run()
    for what, gt, wt, df in zip(("linear", "ln linear"), got, (want, want2), dflt):
        err, arm = rel_l2(gt, wt), rel_l2(gt, df)
        print(f"SWITCH op GEMM_NO_SLAB M {M} N {N} K {K} {what}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
        assert torch.isfinite(gt).all() and err < OP_TOL, (what, mismatch_report(gt, wt))
        assert arm < ARM_TOL, (what, mismatch_report(gt, df))


@pytest.mark.parametrize("N,b", [(97, 1), (70, 2)])
def test_single_track_without_the_k_slab_path(N, b, monkeypatch):
    """PRD_GEMM_SLAB=0 through a folding block's single track at full width (attention, transition, the merged projection after it): the
    consumers of the slab path's by-products -- LN(result) from its reduce launch, the folded first layer -- must FALL BACK to their
    separate launches, not hand prd_gemm an out_ln it refuses.  Every output against float64 (tests/test_single_chain_folded.py)."""
    import test_single_chain_folded as SF
    blk, nxt = SF.make_block(31, DEV), SF.make_block(32, DEV)
    g = torch.Generator().manual_seed(1000 + 7 * N + b)
    single = (torch.randn(b, N, SF.S, generator=g) * 1.5 + 0.5 * torch.randn(b, N, 1, generator=g)).to(DEV)
    bias = torch.randn(b, SF.H, N, N, generator=g).to(DEV)
    mask = torch.ones(b, N)
    mask[b - 1, N - 9:] = 0.0
    mask = mask.to(DEV)

    def run():
        extra = {}
        s, x, u = blk.single_track_(single.clone(), mask, bias, next_block=nxt, qkvg=None, tail=None, extra=extra)
        torch.cuda.synchronize()
        return dict(single=s.cpu(), u=u.cpu(), qkvg=extra["qkvg"].cpu())
    with torch.no_grad(), split16():
        want = SF.reference(blk, nxt, None, single, mask, bias)
        assert ops.slab_ok(b * N, SF.S, SF.S * SF.TF)
        dflt = run()
        with tuned("GEMM_NO_SLAB"):
            assert not ops.slab_ok(b * N, SF.S, SF.S * SF.TF) and not ops.fc1_fold_ok(b * N, SF.S, SF.H * SF.C, SF.S * SF.TF)
            got = run()
    for name in ("single", "u", "qkvg"):
        wt = want[name].cpu()
        err, arm = rel_l2(got[name], wt), rel_l2(got[name], dflt[name])
        print(f"SWITCH op GEMM_NO_SLAB single track N {N} b {b} {name}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
        assert torch.isfinite(got[name]).all() and err < OP_TOL, (name, mismatch_report(got[name], wt))
        assert arm < ARM_TOL, (name, mismatch_report(got[name], dflt[name]))


@pytest.fixture(scope="module")
def head_model():
    args = make_args(single_dim=512, pair_dim=64, num_blocks=1, num_steps=1000, mask_prob=0.3)
    return HP.build(args, seed=41)


@pytest.mark.parametrize("N", [97, 320])
def test_trunk_head_projection_on_the_k_slab_kernel(N, head_model, monkeypatch):
    """PRD_HEAD_SLAB=1: the merged projection at the head of the trunk (OPM's a | b and SPAttention's q | k | v | gate of the SAME normalised
    rows, S = 512 -> 8448 columns) through gemm_slab_kernel and its reduce launch, which applies the LayerNorm by linearity and writes two
    outputs and the normalised rows: a | b (masked), q | k | v | gate and LN(single) against float64."""
    model, params = head_model
    den = model.Denoiser
    g = torch.Generator().manual_seed(4100 + N)
    single = torch.randn(1, N, 512, generator=g) * 1.5 + 0.5 * torch.randn(1, N, 1, generator=g)
    mask = torch.ones(1, N)
    mask[0, N - 5:] = 0
    p = {k: v.double() for k, v in params.items() if k.startswith(("Denoiser.opm.", "Denoiser.SPAAttnBlock."))}
    xd = single.double()
    xo = O.ln(xd, p["Denoiser.opm.layer_norm.weight"], p["Denoiser.opm.layer_norm.bias"])
    want_ab = torch.cat([O.lin(p, "Denoiser.opm.linear_1", xo), O.lin(p, "Denoiser.opm.linear_2", xo)], -1) * mask.double().unsqueeze(-1)
    m = O.ln(xd, p["Denoiser.SPAAttnBlock.layer_norm_m.weight"], p["Denoiser.SPAAttnBlock.layer_norm_m.bias"])
    a = "Denoiser.SPAAttnBlock.mha."
    want_qkvg = torch.cat([O.lin(p, a + "linear_q", m) / math.sqrt(512), O.lin(p, a + "linear_k", m), O.lin(p, a + "linear_v", m),
                           torch.sigmoid(O.lin(p, a + "linear_g", m))], -1)
    want = dict(ab=want_ab, xhat=O.ln(xd), qkvg=want_qkvg)

    def run():
        with torch.inference_mode():
            ab, xhat, qkvg, merged = den.project_single(cu(single), cu(mask))
        torch.cuda.synchronize()
        assert merged
        return dict(ab=ab.cpu(), xhat=xhat.cpu(), qkvg=qkvg.cpu())
    with split16():
        assert ops.slab_ok(N, 256 + 4 * 2048, 512)
        dflt = run()
        monkeypatch.setattr(trunk, "_HEAD_SLAB", True)
        got = run()
    for name in ("ab", "xhat", "qkvg"):
        err, arm = rel_l2(got[name], want[name]), rel_l2(got[name], dflt[name])
        print(f"SWITCH op _HEAD_SLAB N {N} {name}: vs float64 {err:.3e}, vs default arm {arm:.3e}")
        assert torch.isfinite(got[name]).all() and err < OP_TOL, (name, mismatch_report(got[name], want[name]))
        assert arm < ARM_TOL, (name, mismatch_report(got[name], dflt[name]))


# (b, N, pair_dim) of the cases above, per switch: tests/test_switches_cpu.py looks the recorded launch trace up at them
TRACED_SHAPES = {
    "PRD_TA2_V3": {(b, N, P) for b, N, _ in V2_SHAPES for P in (32, 64)},
    "PRD_TA2_LONG": {(1, N, P) for N, _ in NO_LONG_SHAPES for P in (32, 64)},
    "PRD_TA2_XCD8": {(b, N, P) for b, N, _ in XCD8_SHAPES for P in (32, 64)},
}


# ---------------------------------------------------------------------------------------------------
# 3. the training switches, each off alone
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def train_cases(golden):
    """name -> the inputs of one optimisation step and the oracle's gradients, built once at first use.  "cfg1": the golden case (pair_dim
    32, b = 1, N = 140), with the imported reference's fingerprints; "n70": b = 2, N = 70 on the small64 widths (pair_dim 64, the width the
    row kernels of PRD_PAIR_LINEAR and the fused heads' backward of PRD_HEADS_BWD are built for)."""
    from test_training_cpu import case_inputs, oracle_grads
    from protein_redesign_amd.synthetic import deterministic_state_dict
    from protein_redesign_amd.weights import spec_tensors
    built = {}

    def get(name):
        if name in built:
            return built[name]
        if name == "cfg1":
            case, z, args, params, pb = case_inputs(golden, "cfg1")
            t = torch.from_numpy(z["train_t"])
            nz, ns = torch.from_numpy(z["train_noise_z"]), torch.from_numpy(z["train_noise_seq"])
        else:
            z = None
            args = make_args(**golden("small64")[0]["args"])
            params = deterministic_state_dict(spec_tensors(args), seed=75, style="random")
            sizes = [(6, 64), (5, 58)]
            batch = synthetic_batch(sizes, esm_dim=args["esm_dim"], seed=76, n_total=70)
            pb = O.prepare_batch(batch, args["mask_prob"], [NoiseSource(HP.NOISE_SEED, 100 + k).randperm(n) for k, (_, n) in enumerate(sizes)])
            g = torch.Generator().manual_seed(77)
            t = torch.tensor([5, 2])
            nz = O.remove_mean(torch.randn(2, 70, 3, generator=g), pb["residue_and_atom_mask"])
            ns = O.remove_mean(torch.randn(2, 70, 21, generator=g), pb["residue_mask"])
        want_loss, want = oracle_grads(args, params, pb, t, nz, ns)
        built[name] = dict(z=z, args=args, params=params, pb=pb, t=t, nz=nz, ns=ns, want_loss=want_loss, want=want, default={})
        return built[name]
    return get


def _train_step(c):
    from test_training_gpu import hip_model
    model = hip_model(c["args"], c["params"])
    dpb = batch_to(c["pb"], DEV)
    mask = dpb["residue_and_atom_mask"]
    diff = model.diffusion_loss(dpb, dpb["x"], mask, c["t"].to(DEV), c["nz"].to(DEV), c["ns"].to(DEV))
    loss = torch.mean(diff / (mask > 0.5).sum(-1))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {k: p.grad.detach().cpu().double().reshape(-1) for k, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("case", ["cfg1", "n70"])
@pytest.mark.parametrize("arm", TRAIN_ARMS, ids=TRAIN_IDS)
def test_training_switch_off_alone(arm, case, gemm_mode, train_cases, monkeypatch):
    """One optimisation step's loss and gradients with ONE training switch off, on the cfg1 golden case (b = 1, N = 140, pair_dim 32) and
    on b = 2, N = 70 at pair_dim 64 -- 19600 and 9800 pair positions, above the ops.WGRAD_MIN_ROWS = 8192 from which the library backward
    runs at all; pair_dim 64 because PRD_PAIR_LINEAR's row kernel and PRD_HEADS_BWD's fused backward serve no other width, so that on
    cfg1 alone those two would have nothing to switch.  Every gradient within GRAD_TOL of the oracle's autograd (cfg1: and of the imported
    reference's fingerprints, as in test_training_step_gradients_vs_reference_and_oracle); the loss within 1e-6 of the default arm's."""
    import json

    import numpy as np

    from test_training_cpu import FINGERPRINT_TOL, GRAD_PROJECTIONS
    from test_training_gpu import GRAD_TOL
    arm_id, name, s = arm
    c = train_cases(case)
    z = c["z"]
    b, N = c["pb"]["atom_mask"].shape
    assert b * N * N >= ops.WGRAD_MIN_ROWS, "the case is too small for the library backward: the switch would have nothing to switch"
    if gemm_mode not in c["default"]:
        c["default"][gemm_mode] = _train_step(c)
    loss0, grads0 = c["default"][gemm_mode]
    with switched(name, s, monkeypatch):
        loss, got = _train_step(c)
    assert abs(loss - loss0) <= 1e-6 * abs(loss0), (arm_id, loss, loss0)
    assert abs(loss - c["want_loss"]) < GRAD_TOL * abs(c["want_loss"])
    names = sorted(c["want"])
    assert sorted(got) == names
    scale = float(torch.stack([v.double().norm() for v in c["want"].values()]).norm())
    worst = 0.0
    for k in names:
        err = float((got[k] - c["want"][k].double().reshape(-1)).norm())
        ref = float(c["want"][k].double().norm())
        assert err < GRAD_TOL * ref + 1e-6 * scale, (arm_id, k, err, ref)
        worst = max(worst, err / max(ref, 1e-3 * scale))
    if z is not None:                   # the imported reference's training_step: loss, and norm and seeded projections of every gradient
        assert abs(loss - float(z["train_loss"])) < GRAD_TOL * abs(float(z["train_loss"]))
        ref_names = json.loads(str(z["train_grad_names"]))
        assert sorted(ref_names) == names
        rscale = float(np.linalg.norm(z["train_grad_norm"]))
        for i, k in enumerate(ref_names):
            gk, n_ref = got[k], float(z["train_grad_norm"][i])
            assert abs(float(gk.norm()) - n_ref) < FINGERPRINT_TOL * n_ref + 1e-6 * rscale, (arm_id, k, float(gk.norm()), n_ref)
            for j in range(GRAD_PROJECTIONS):
                gen = torch.Generator().manual_seed(4242 + 16 * i + j)
                proj = float(torch.dot(gk, torch.randn(gk.numel(), generator=gen, dtype=torch.float64)))
                assert abs(proj - float(z["train_grad_proj"][i, j])) < FINGERPRINT_TOL * n_ref + 1e-6 * rscale, (arm_id, k, j)
    moved = max(float((got[k] - grads0[k]).norm()) / max(float(grads0[k].norm()), 1e-3 * scale) for k in names)
    print(f"SWITCH train {arm_id} {case} [{gemm_mode}]: loss vs default arm {abs(loss - loss0) / abs(loss0):.3e}, worst gradient vs the oracle's autograd "
          f"{worst:.3e}, vs default arm {moved:.3e}")
