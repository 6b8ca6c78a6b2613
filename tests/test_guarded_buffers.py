"""GPU: the denoiser operators inside guarded, poisoned device buffers (tests/guarded_alloc.py).

Every case runs inside ``guarded(poison)``: each buffer the package allocates, and each test input (``put``), sits between two
4096-byte guard bands inside a larger buffer pre-filled with a poison byte.  After ``torch.cuda.synchronize()`` a case asserts, in
this order,
  (a) ``intact()``: no byte outside any buffer was touched (an overrun of an output, a scratch or a ``prd_*_workspace*`` result);
  (b) every returned tensor is finite and free of the 0x7F pattern value (an element the kernel never wrote; a read of memory nobody
      wrote, which returns NaN under 0xFF and 3.4e38 under 0x7F -- the second because ``v_max_f32`` / ``fmaxf`` drop a NaN operand);
  (c) parity with the oracle call and the tolerance tests/test_hip_parity.py (and the backward tests) use for that operator.
Oracles are computed once per shape and shared by the poison patterns and the arithmetic modes.

Row lengths (``SHAPES``): 33 = one over a 32-block, and below the 97 positions under which helper waves of the triangle-attention
cores have no tiles; 70 with b = 2 and the second sample masked from 61; 97 = first over 96; 130 = two over 128 with 123 valid.
"""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prd_oracle as O
from conftest import rel_l2
from guarded_alloc import HUGE, check_written, guarded
from protein_redesign_amd import _lib, masking, ops
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch, synthetic_batch
from test_head_layouts import PFX, attn_params
from test_head_layouts_backward import TA_NAMES, check_grads, float64_grads
from test_hip_parity import BLOCK_TOL, CFG, NOISE_SEED, OP_TOL, TRAJ_TOL, build, gemm_mode, golden_case  # noqa: F401 (gemm_mode: fixture)
from test_single_chain_folded import make_block, reference as single_chain_reference
from test_training_cpu import FINGERPRINT_TOL, GRAD_PROJECTIONS, case_inputs, oracle_grads
from test_training_gpu import GRAD_TOL, hip_model
from test_training_masks import seeded_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, sizes = (atoms, residues) per sample): see the module docstring
SHAPES = {33: [(5, 28)], 70: [(8, 62), (7, 54)], 97: [(9, 88)], 130: [(11, 112)], 190: [(12, 169)]}
VALID = {33: 33, 70: 61, 97: 97, 130: 123, 190: 181}
LENGTHS = (33, 70, 97, 130)                             # every operator; 190: the row kernels (test_forward_operator_cooperative_leftover)


@pytest.fixture(params=["nan", "huge"])
def poison(request):
    return request.param


# ---------------------------------------------------------------------------------------------------
# shared inputs and oracles
# ---------------------------------------------------------------------------------------------------
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def model_for(P, S=64):
    def make():
        args = make_args(**{**CFG[P], "single_dim": S})
        model, params = build(args, seed=10 + P + S)
        return args, model, params
    return cached(("model", P, S), make)


class Case:
    """Seeded inputs of one (P, S, N): the prepared batch, trunk inputs and step inputs, all on the CPU."""

    def __init__(self, P, S, N):
        self.P, self.S, self.N = P, S, N
        self.args, self.model, self.params = model_for(P, S)
        sizes = SHAPES[N]
        batch = synthetic_batch(sizes, esm_dim=self.args["esm_dim"], seed=20 + P + N, n_total=N)
        perms = [NoiseSource(NOISE_SEED, 100 + k).randperm(n) for k, (_, n) in enumerate(sizes)]
        self.pb = O.prepare_batch(batch, self.args["mask_prob"], perms)
        self.mask = self.pb["residue_and_atom_mask"]
        self.b = self.mask.shape[0]
        assert self.mask.shape == (len(sizes), N) and int(self.mask[-1].sum()) == VALID[N]
        g = torch.Generator().manual_seed(99 + P + N + S)
        self.single = torch.randn(self.b, N, S, generator=g)
        self.pair = torch.randn(self.b, N, N, P, generator=g)
        self.z = torch.randn(self.b, N, 3, generator=g)
        self.seq_t = torch.randn(self.b, N, 21, generator=g)
        self.t = torch.tensor([5, 2][:self.b])
        self.m2 = self.mask.unsqueeze(-1) * self.mask.unsqueeze(-2)
        self.H, self.c = self.args["num_heads"], self.args["head_dim"]

    def want(self, name, make):
        """The oracle's value of ``name`` for this case, computed once."""
        def run():
            with torch.inference_mode():
                return make()
        return cached(("want", name, self.P, self.S, self.N), run)


def case(P, S, N):
    return cached(("case", P, S, N), lambda: Case(P, S, N))


class Put:
    """What a case gets: ``put(t)`` = a test input in a guarded device buffer of its own; ``put.empty(*shape)`` = a poisoned, guarded
    fp32 output buffer for an operator that takes ``out``."""

    def __init__(self, g):
        self.g = g

    def __call__(self, t):
        return self.g.put(t, DEV)

    def empty(self, *shape):
        return self.g.empty(*shape, device=DEV)


def run_guarded(poison, fn, modules=()):
    """``fn(put)`` inside the manager -> its outputs (a dict name -> tensor) after (a) and (b)."""
    with guarded(poison, modules=modules) as g:
        outs = fn(Put(g))
        torch.cuda.synchronize()
        assert g.intact(), g.report()
        for name, t in outs.items():
            check_written(name, t)
        outs = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in outs.items()}
    return outs


def check_parity(got, want, tol):
    for name in want:
        assert got[name].shape == want[name].shape, name
        err = rel_l2(got[name], want[name])
        assert err < tol, f"{name}: rel-L2 {err:.3e} (bound {tol:g})"


# ---------------------------------------------------------------------------------------------------
# the harness on the device
# ---------------------------------------------------------------------------------------------------
def test_a_write_past_a_carved_interior_is_reported(poison):
    """Teeth: one element past the end of a buffer the package allocated, written with torch indexing (no kernel of the project)."""
    x = torch.randn(5, 7, device=DEV)
    with guarded(poison) as g:
        y = ops.layer_norm(x)                           # allocates its output through ops' torch.empty_like
        torch.cuda.synchronize()
        assert g.intact(), g.report()
        assert len(g.records) == 1 and g.records[0][1] == y.numel() * 4
        flat = y.as_strided((y.numel() + 1,), (1,))     # the interior and the first element after it
        flat[y.numel()] = 0.0
        torch.cuda.synchronize()
        assert not g.intact()
        assert "allocation #0 [5, 7] torch.float32" in g.report() and "after the tensor" in g.report() and "offset +0 " in g.report()
        assert "layer_norm" in g.report()
    assert ops.torch is torch


def test_unwritten_elements_and_caches_on_the_device(poison):
    with guarded(poison) as g:
        buf = ops.gemm_workspace(DEV, 1000)             # the cached K-slab scratch is re-made guarded
        assert len(g.records) == 1 and g.records[0][1] == 1000 and list(ops._GEMM_WS.values())[0] is buf
        bad = ~torch.isfinite(buf) | (buf == HUGE)
        assert bool(bad.all())
        with pytest.raises(AssertionError):
            check_written("buf", buf)
        z = ops.tri_attn_pair_bar(DEV)
        assert int(z.abs().sum()) == 0 and len(g.records) == 2
        assert g.intact()
    assert all(v is not buf for v in ops._GEMM_WS.values()) and all(v is not z for v in ops._PAIR_BARS.values())


# ---------------------------------------------------------------------------------------------------
# forward operators
# ---------------------------------------------------------------------------------------------------
def fb0(c):
    return c.model.Denoiser.folding_blocks[0]


B0 = "Denoiser.folding_blocks.0"


def op_pair_bias(c, put):
    fb = fb0(c)
    got = {"bias": ops.pair_bias(put(c.pair), fb.attn_bias[1].weight, fb.attn_bias[1].bias)}
    return got, {"bias": c.want("pair_bias", lambda: O.pair_bias(c.params, B0 + ".attn_bias", c.pair))}, OP_TOL


def spa_bias(c, pair):
    p = c.params
    z = O.ln(pair, p["Denoiser.SPAAttnBlock.linear_z.0.weight"], p["Denoiser.SPAAttnBlock.linear_z.0.bias"])
    return F.linear(z, p["Denoiser.SPAAttnBlock.linear_z.1.weight"]).permute(0, 3, 1, 2)


def op_pair_bias2(c, put):
    spa, ab0 = c.model.Denoiser.SPAAttnBlock, fb0(c).attn_bias[1]
    oa, ob = ops.pair_bias2(put(c.pair), (spa.linear_z[1].weight, None, spa.linear_z[0].weight, spa.linear_z[0].bias),
                            (ab0.weight, ab0.bias, None, None))
    want = {"spa_bias": c.want("spa_bias", lambda: spa_bias(c, c.pair)),
            "bias": c.want("pair_bias", lambda: O.pair_bias(c.params, B0 + ".attn_bias", c.pair))}
    return {"spa_bias": oa, "bias": ob}, want, OP_TOL


def op_single_attention(c, put):
    bias = c.want("pair_bias", lambda: O.pair_bias(c.params, B0 + ".attn_bias", c.pair))
    got = {"single": fb0(c).single_attn(put(c.single), put(c.mask), attn_bias=put(bias))}
    want = c.want("single_attn", lambda: O.gated_attention(c.params, B0 + ".single_attn", c.single, c.mask, c.H, c.c, bias=bias))
    return got, {"single": want}, OP_TOL


def op_single_pair_attention(c, put):
    """SPAttention as the sampler runs it (no autograd): in split-16 arithmetic prd_spa_attn_core with its workspace
    (prd_spa_attn_core_workspace), in fp32 arithmetic the GEMM-path form (logits, softmax, P V)."""
    if _lib.lib().prd_get_gemm_mode() == 1:
        assert _lib.lib().prd_spa_attn_core_supported(c.N, c.S) == 1
    with torch.no_grad():
        got = {"single": c.model.Denoiser.SPAAttnBlock(put(c.single), put(c.pair), put(c.mask))}
    want = c.want("spa", lambda: O.single_pair_attention(c.params, "Denoiser.SPAAttnBlock", c.single, c.pair, c.H))
    return got, {"single": want}, OP_TOL


def op_single_transition(c, put):
    fc = fb0(c).single_fc
    got = {"single": ops.transition_single(put(c.single), fc[1].weight, fc[1].bias, fc[3].weight, fc[3].bias, residual=False)}
    return got, {"single": c.want("single_fc", lambda: O.transition(c.params, B0 + ".single_fc", c.single))}, OP_TOL


def op_single_transition_slab(c, put):
    """The transition with the row sums of W1 (FoldingBlock.single_track_'s call): at single_dim 512 both layers take the K-slab
    path where prd_gemm_slab_ok says so (gemm_slab_kernel + its reduce launch, scratch from prd_gemm_slab_workspace), and the
    second one writes LN(result) on the side."""
    fc = fb0(c).single_fc
    wsum1 = fc[1].weight.double().sum(1).float().contiguous()
    out, xhat = ops.transition_single(put(c.single), fc[1].weight, fc[1].bias, fc[3].weight, fc[3].bias, residual=True, wsum1=wsum1,
                                      want_ln=True)
    want = {"single": c.want("single_fc_res", lambda: c.single + O.transition(c.params, B0 + ".single_fc", c.single))}
    got = {"single": out}
    if xhat is not None:
        got["xhat"], want["xhat"] = xhat, c.want("single_fc_res_ln", lambda: O.ln(want["single"]))
    return got, want, OP_TOL


def op_outer_linear(c, put):
    got = {"pair": fb0(c).outer_linear(put(c.single))}
    return got, {"pair": c.want("outer_linear", lambda: O.outer_linear(c.params, B0 + ".outer_linear", c.single))}, OP_TOL


def op_outer_product_update(c, put):
    got = {"pair": c.model.Denoiser.opm(put(c.single), put(c.mask))}
    return got, {"pair": c.want("opm", lambda: O.outer_product_update(c.params, "Denoiser.opm", c.single, c.mask))}, OP_TOL


def op_input_stage(c, put):
    """static_pair, atom_embed, single_init, time_embed, pair_init (the separate launches of the input stage)."""
    m, pb = c.model, c.pb
    dbatch = {k: (put(v) if torch.is_tensor(v) else v) for k, v in pb.items()}
    st = m._static_inputs(dbatch)
    gs = ops.single_init(st["single"], put(c.seq_t), dbatch["residue_mask"], m.embed_residue_type[1].weight)
    eb = ops.time_embed(put(c.t), m.embed_beta[0].weight, m.embed_beta[1].weight, c.args["num_steps"])
    gp = ops.pair_init(st["pair"], put(c.z), put(c.mask), m.embed_dist[0].center, m.embed_dist[1].weight, eb)
    emb = c.want("embed", lambda: O.embed_inputs(c.params, c.args, pb, c.z, c.seq_t, c.mask, c.t))
    return {"single": gs, "pair": gp, "static_pair": st["pair"], "static_single": st["single"], "ebeta": eb}, {"single": emb[0], "pair": emb[1]}, OP_TOL


def op_pair_head(c, put):
    """The head of the pair track as Denoiser.run_ runs it: prd_pair_head (pair_init + outer-product tail + the two first bias
    heads in one row pass) where the library has that form -- split-16 arithmetic, single_dim 512 -- else its three launches."""
    m, den, pb = c.model, c.model.Denoiser, c.pb
    dbatch = {k: (put(v) if torch.is_tensor(v) else v) for k, v in pb.items()}
    st = m._static_inputs(dbatch)
    eb = ops.time_embed(put(c.t), m.embed_beta[0].weight, m.embed_beta[1].weight, c.args["num_steps"])
    opm, spa, ab0 = den.opm, den.SPAAttnBlock, den.folding_blocks[0].attn_bias[1]
    single = c.want("embed", lambda: O.embed_inputs(c.params, c.args, pb, c.z, c.seq_t, c.mask, c.t))[0]
    dsingle, dmask = put(single), put(c.mask)
    ab = opm.project(dsingle, dmask)
    sets = dict(set_a=(spa.linear_z[1].weight, None, spa.linear_z[0].weight, spa.linear_z[0].bias), set_b=(ab0.weight, ab0.bias, None, None))
    if c.S == 512 and _lib.lib().prd_get_gemm_mode() == 1:
        assert ops.pair_head_supported(c.P, m.embed_dist[1].weight.shape[1], opm.c_hidden)
    if ops.pair_head_supported(c.P, m.embed_dist[1].weight.shape[1], opm.c_hidden):
        pair, ba, bb = ops.pair_head(st["pair"], put(c.z), dmask, m.embed_dist[0].center, m.embed_dist[1].weight, eb, ab,
                                     opm.linear_out.weight, opm.linear_out.bias, apply_mask=True, **sets)
    else:
        pair = ops.pair_init(st["pair"], put(c.z), dmask, m.embed_dist[0].center, m.embed_dist[1].weight, eb)
        opm.run(dsingle, pair, dmask, residual=True, apply_mask=True, out=pair, ab=ab)
        ba, bb = ops.pair_bias2(pair, sets["set_a"], sets["set_b"])

    def make():
        s, p0, _, m2 = O.embed_inputs(c.params, c.args, pb, c.z, c.seq_t, c.mask, c.t)
        p1 = p0 + m2.unsqueeze(-1) * O.outer_product_update(c.params, "Denoiser.opm", s, c.mask)
        return {"pair": p1, "spa_bias": spa_bias(c, p1), "bias": O.pair_bias(c.params, B0 + ".attn_bias", p1)}
    return {"pair": pair, "spa_bias": ba, "bias": bb}, c.want("pair_head", make), OP_TOL


def tri_mul_op(mode):
    def op(c, put):
        mod = getattr(fb0(c), f"pair_mul_{mode}")
        got = {"pair": mod(put(c.pair), put(c.m2))}
        want = c.want(f"tri_mul_{mode}", lambda: O.triangle_multiplication(c.params, f"{B0}.pair_mul_{mode}", c.pair, c.m2, mode == "incoming"))
        return got, {"pair": want}, OP_TOL
    return op


def op_tri_mul_chain(c, put):
    """pair += outgoing(pair); pair += incoming(pair) as FoldingBlock.run_ does it: prd_tri_mul_chain in split-16 arithmetic, two
    prd_tri_mul calls in fp32 arithmetic -- both on one workspace of workspace_bytes("tri_mul")."""
    fb = fb0(c)
    pair, mask = put(c.pair), put(c.mask)
    ws = put.empty(ops.workspace_bytes("tri_mul", c.b, c.N, 0, c.P) // 4)
    if ops.tri_mul_chain_supported(c.N, c.P):
        ops.tri_mul_chain_(pair, mask, fb.pair_mul_outgoing.weights(), fb.pair_mul_incoming.weights(), ws=ws)
    else:
        assert _lib.lib().prd_get_gemm_mode() == 0
        fb.pair_mul_outgoing.run(pair, mask, residual=True, out=pair, ws=ws)
        fb.pair_mul_incoming.run(pair, mask, residual=True, out=pair, ws=ws)

    def make():
        w = c.pair + O.triangle_multiplication(c.params, B0 + ".pair_mul_outgoing", c.pair, c.m2, False)
        return w + O.triangle_multiplication(c.params, B0 + ".pair_mul_incoming", w, c.m2, True)
    return {"pair": pair}, {"pair": c.want("tri_mul_chain", make)}, OP_TOL


def want_tri_attn(c, mode):
    return c.want(f"tri_attn_{mode}", lambda: O.triangle_attention(c.params, f"{B0}.pair_attn_{mode}", c.pair, c.m2, c.H, c.c, mode == "ending"))


def tri_attn_op(mode):
    def op(c, put):
        mod = getattr(fb0(c), f"pair_attn_{mode}")
        return {"pair": mod(put(c.pair), put(c.m2))}, {"pair": want_tri_attn(c, mode)}, OP_TOL
    return op


def tri_attn_core_v2_op(mode):
    def op(c, put):
        """prd_tri_attn_core_v2 called directly (rows shorter than 97 positions: helper waves without tiles); og is projected
        with the oracle's output weights on the host."""
        mod = getattr(fb0(c), f"pair_attn_{mode}")
        assert ops.tri_attn_v2_supported(c.N, c.P)
        og = ops.tri_attn_core_v2(put(c.pair), put(c.mask), mod.attn.weights()[:5], c.H, c.c, ending=mode == "ending")
        pfx = f"{B0}.pair_attn_{mode}.attn.out_proj."
        proj = og.cpu() @ c.params[pfx + "weight"].T + c.params[pfx + "bias"]
        return {"og": og, "pair": proj}, {"pair": want_tri_attn(c, mode)}, OP_TOL
    return op


def heads_op(H, c_, mode):
    def op(c, put):
        """The general heads core (prd_tri_attn_core_heads + prd_tri_attn_heads_workspace_bytes) through ops.tri_attn."""
        assert ops.tri_attn_heads_supported(c.N, c.P, H, c_)
        p, w = attn_params(H, c_, c.P, seed=100 * H + c_ + c.P)
        got = {"pair": ops.tri_attn(put(c.pair), put(c.mask), w, H, c_, ending=mode == "ending", residual=False)}
        want = c.want(f"heads_{H}x{c_}_{mode}", lambda: O.triangle_attention(p, PFX, c.pair, c.m2, H, c_, mode == "ending"))
        return got, {"pair": want}, OP_TOL
    return op


def op_pair_transition(c, put):
    pf = fb0(c).pair_fc
    got = {"pair": ops.pair_transition(put(c.pair), pf[1].weight, pf[1].bias, pf[3].weight, pf[3].bias, residual=False)}
    return got, {"pair": c.want("pair_fc", lambda: O.transition(c.params, B0 + ".pair_fc", c.pair))}, OP_TOL


def op_block_tail(c, put):
    blk, nxt = c.model.Denoiser.folding_blocks[0], c.model.Denoiser.folding_blocks[1]
    ta, pf = blk.pair_attn_ending.attn, blk.pair_fc
    pair, mask = put(c.pair), put(c.mask)
    og = ops.tri_attn_core(pair, mask, ta.weights()[:5], c.H, c.c, ending=True)
    bias = ops.block_tail_(pair, og, ta.out_proj.weight, ta.out_proj.bias, pf[1].weight, pf[1].bias, pf[3].weight, pf[3].bias,
                           nxt.attn_bias[1].weight, nxt.attn_bias[1].bias)

    def make():
        w = c.pair + want_tri_attn(c, "ending")
        w = w + O.transition(c.params, B0 + ".pair_fc", w)
        return {"pair": w, "bias": O.pair_bias(c.params, "Denoiser.folding_blocks.1.attn_bias", w)}
    return {"pair": pair, "bias": bias, "og": og}, c.want("block_tail", make), BLOCK_TOL


def op_coord_head(c, put):
    wr = c.model.weight_radial
    mask = put(c.mask)
    raw = ops.coord_head(put(c.pair), put(c.z), mask, wr[1].weight, wr[1].bias, wr[3].weight)
    eps = ops.remove_mean(raw, mask)

    def make():
        zij = c.z.unsqueeze(-2) - c.z.unsqueeze(-3)
        return O.heads(c.params, c.single, 0.5 * (c.pair + c.pair.transpose(1, 2)), zij, c.m2, c.mask)[0]
    return {"raw": raw, "eps": eps}, {"eps": c.want("coord_head", make)}, OP_TOL


def op_remove_mean(c, put):
    got = {"z": ops.remove_mean(put(c.z), put(c.mask)), "seq": ops.remove_mean(put(c.seq_t), put(c.pb["residue_mask"]))}
    want = {"z": c.want("rm_z", lambda: O.remove_mean(c.z, c.mask)), "seq": c.want("rm_seq", lambda: O.remove_mean(c.seq_t, c.pb["residue_mask"]))}
    return got, want, OP_TOL


def op_folding_block(c, put):
    got = dict(zip(("single", "pair"), fb0(c)(put(c.single), put(c.pair), put(c.mask))))
    want = c.want("folding_block", lambda: dict(zip(("single", "pair"), O.folding_block(c.params, B0, c.single, c.pair, c.mask, c.H, c.c))))
    return got, want, BLOCK_TOL


def op_denoiser(c, put):
    den = c.model.Denoiser
    gs, gp, _ = den({k: (put(v) if torch.is_tensor(v) else v) for k, v in c.pb.items()}, None, None, put(c.single), put(c.pair), None)
    want = c.want("denoiser", lambda: dict(zip(("single", "pair"), O.denoiser(c.params, c.args, c.single, c.pair, c.mask))))
    return {"single": gs, "pair": gp}, want, BLOCK_TOL


FORWARD = {
    "pair_bias": op_pair_bias, "pair_bias2": op_pair_bias2, "single_attention": op_single_attention,
    "single_pair_attention": op_single_pair_attention, "single_transition": op_single_transition,
    "single_transition_slab": op_single_transition_slab, "outer_linear": op_outer_linear,
    "outer_product_update": op_outer_product_update, "input_stage": op_input_stage, "pair_head": op_pair_head,
    "tri_mul_outgoing": tri_mul_op("outgoing"), "tri_mul_incoming": tri_mul_op("incoming"), "tri_mul_chain": op_tri_mul_chain,
    "tri_attn_starting": tri_attn_op("starting"), "tri_attn_ending": tri_attn_op("ending"),
    "tri_attn_core_v2_starting": tri_attn_core_v2_op("starting"), "tri_attn_core_v2_ending": tri_attn_core_v2_op("ending"),
    "heads_8x32_starting": heads_op(8, 32, "starting"), "heads_8x32_ending": heads_op(8, 32, "ending"),
    "heads_3x20_starting": heads_op(3, 20, "starting"), "heads_3x20_ending": heads_op(3, 20, "ending"),
    "pair_transition": op_pair_transition, "block_tail": op_block_tail, "coord_head": op_coord_head, "remove_mean": op_remove_mean,
    "folding_block": op_folding_block, "denoiser": op_denoiser,
}
# single_dim 512: where a different kernel runs at full width (OuterLinear's K-split kernel, the fp16 x 2 OuterProductUpdate,
# the K-slab / folded single transition, prd_pair_head, prd_spa_attn_core at c = 512)
WIDE = ("outer_linear", "outer_product_update", "single_transition_slab", "single_pair_attention", "pair_head", "folding_block")


def run_forward(name, P, S, N, poison):
    c = case(P, S, N)
    box = {}

    def fn(put):
        got, box["want"], box["tol"] = FORWARD[name](c, put)
        return got
    got = run_guarded(poison, fn, modules=[c.model])
    check_parity(got, box["want"], box["tol"])


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("name", sorted(FORWARD))
def test_forward_operator(name, P, N, poison, gemm_mode):
    run_forward(name, P, 64, N, poison)


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("name", WIDE)
def test_forward_operator_full_width(name, P, N, poison, gemm_mode):
    run_forward(name, P, 512, N, poison)


ROW_KERNELS = ("pair_bias", "pair_bias2", "outer_linear", "outer_product_update", "tri_mul_outgoing", "tri_mul_incoming", "tri_mul_chain",
               "tri_attn_starting", "tri_attn_ending", "pair_transition", "block_tail", "folding_block")


@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("name", ROW_KERNELS)
def test_forward_operator_cooperative_leftover(name, P, poison, gemm_mode):
    """N = 190 (181 valid), an edge the four lengths miss.  The 8-wave row kernels of csrc/prd_pair.hip and csrc/prd_tri.hip deal
    tasks of 32 pair positions in rounds of ``slots = 4 * gridDim.x`` (at most 256 workgroups) and compute what is left after the
    whole rounds with the four SIMDs of a workgroup together when ``left <= 2 * gridDim.x`` (``coop``): only reached beyond 1024
    tasks, i.e. from N = 182 on.  190 x 190 positions = 1128 whole tasks + one of 4 positions: a leftover round of 105 tasks whose
    last task is ragged (tests/test_hip_parity.py has N = 192 = exactly 1152 tasks)."""
    assert 1024 < -(-190 * 190 // 32) <= 1024 + 512 and (190 * 190) % 32 != 0
    run_forward(name, P, 64, 190, poison)


@pytest.mark.parametrize("ending", [False, True])
@pytest.mark.parametrize("P,b,N", [(64, 2, 40), (32, 1, 70), (64, 1, 130), (32, 1, 33), (64, 1, 97)])
def test_triangle_attention_core_with_fused_previous_update(P, b, N, ending, poison):
    """prd_tri_attn_core_fused under guards: pair_out and og against prd_tri_attn_out followed by prd_tri_attn_core, as
    tests/test_hip_parity.py::test_triangle_attention_core_with_fused_previous_update holds them (its shapes, plus N = 33 and 97).
    The kernel is a first-generation core: compiled only into the -DPRD_AB library, where the test below runs this one."""
    L = _lib.lib()
    prev = L.prd_get_gemm_mode()
    assert L.prd_set_gemm_mode(1) == 0
    try:
        if not ops.tri_attn_core_fused_supported(N, P):
            assert "libprd_hip_ab" not in _lib.LIB_PATH, "the -DPRD_AB library must have the fused first-generation core"
            pytest.skip("first-generation attention cores live in the -DPRD_AB build: test_fused_previous_update_core_in_the_ab_library "
                        "runs this test there")
        g = torch.Generator().manual_seed(7 * N + P)
        pair, og_in = torch.randn(b, N, N, P, generator=g), torch.randn(b, N, N, 64, generator=g)
        mask = torch.ones(b, N)
        mask[b - 1, N - 6:] = 0
        wo, bo = torch.randn(P, 64, generator=g) / 8.0, torch.randn(P, generator=g) / 4.0
        wts = [torch.randn(64, P, generator=g) / math.sqrt(P) for _ in range(4)] + [torch.randn(64, generator=g) / 4.0]
        d = [t.to(DEV) for t in (pair, og_in, wo, bo, mask, *wts)]
        want_pair = ops.tri_attn_out(d[0], d[1], d[2], d[3], residual=True)
        want_og = ops.tri_attn_core(want_pair, d[4], d[5:], 4, 16, ending=ending)

        def fn(put):
            pair_out = put.empty(b, N, N, P)
            og = ops.tri_attn_core_fused(put(pair), put(og_in), put(wo), put(bo), put(mask), [put(w) for w in wts], 4, 16, ending=ending,
                                         pair_out=pair_out)
            return {"pair_out": pair_out, "og": og}
        got = run_guarded(poison, fn)
        check_parity(got, {"pair_out": want_pair.cpu()}, 1e-6)
        check_parity(got, {"og": want_og.cpu()}, 2e-6)
    finally:
        assert L.prd_set_gemm_mode(prev) == 0


def test_fused_previous_update_core_in_the_ab_library():
    """The cases above in a child process that loads libprd_hip_ab.so through PRD_LIB (as tests/test_ab_build.py runs the parity
    test of the same kernel): all of them pass there, none skips."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from protein_redesign_amd import build as build_mod
    lib = build_mod.build_ab(verbose=False)
    env = dict(os.environ, PRD_LIB=lib, PRD_TA_VARIANT="10")
    env.pop("PRD_LDS_POISON", None)
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "core_with_fused_previous_update",
           "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "20 passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], tail


@pytest.mark.parametrize("N,b,variant", [(97, 1, "next"), (70, 2, "tail"), (130, 1, "next"), (33, 1, "next"), (320, 2, "next"), (130, 5, "tail")])
def test_single_track_full_width(N, b, variant, poison, gemm_mode):
    """FoldingBlock.single_track_ at single_dim 512 against the float64 evaluation of tests/test_single_chain_folded.py, every
    output at OP_TOL: b N = 97, 140, 130 and 640 rows take prd_single_fc1_folded in split-16 arithmetic (its range is 96..640 rows:
    fc1_fold_plan in csrc/prd_gemm.hip), 33 rows (below it) and 650 rows (above it) the separate launches; fp32 arithmetic the
    separate launches throughout.  The K-slab second layer writes LN(single) for the merged projection, whose column blocks are
    the outputs u and qkvg / tail."""
    S, H, C = 512, 4, 16
    blk, nxt = cached("single_track_blocks", lambda: (make_block(11, DEV), make_block(12, DEV)))
    if _lib.lib().prd_get_gemm_mode() == 1:
        assert ops.fc1_fold_ok(b * N, S, H * C, 4 * S) == (96 <= b * N <= 640)

    def make():
        g = torch.Generator().manual_seed(1000 + 7 * N + b)
        single = torch.randn(b, N, S, generator=g) * 1.5 + 0.5 * torch.randn(b, N, 1, generator=g)
        bias = torch.randn(b, H, N, N, generator=g)
        mask = torch.ones(b, N)
        mask[b - 1, N - max(1, N // 9):] = 0.0
        tail = (torch.randn(S, S, generator=g) / math.sqrt(S), 0.1 * torch.randn(S, generator=g)) if variant == "tail" else None
        with torch.no_grad():               # (make_block seeds every parameter of the single track: the CPU twins hold the same weights)
            want = single_chain_reference(make_block(11), make_block(12) if tail is None else None, tail, single, mask, bias)
        return single, bias, mask, tail, want
    single, bias, mask, tail, want = cached(("single_track", N, b, variant), make)

    def fn(put):
        extra = {}
        dtail = tuple(put(t) for t in tail) if tail is not None else None
        with torch.no_grad():
            s, x, u = blk.single_track_(put(single), put(mask), put(bias), next_block=nxt if tail is None else None, qkvg=None, tail=dtail,
                                        extra=extra)
        return {"single": s, "u": u, "x": x, **extra}
    got = run_guarded(poison, fn, modules=[blk, nxt])
    assert set(want) <= set(got)
    check_parity(got, {k: v.float() for k, v in want.items()}, OP_TOL)


@pytest.mark.parametrize("M,N,K,G,slab", [(37, 64, 64, 1, False), (70, 21, 512, 1, False), (7, 5, 64, 1, False), (173, 516, 1024, 1, True),
                                          (140, 140, 16, 8, False)])
def test_linear_and_gemm_edge_shapes(M, N, K, G, slab, poison, gemm_mode):
    """ops.linear / ops.gemm at the edge shapes of tests/test_hip_parity.py (test_gemm_nt, test_k_slab_gemm, and the smallest shape
    of test_linear_with_fused_layer_norm, whose fused form is the next test) against a float64 matmul at their bound, 2e-6: ragged M / N tiles, N = 21 and 5 (rows that are no multiple
    of a float4), the K-slab path with its workspace query (M = 173, N = 516), a batch of 8."""
    def make():
        g = torch.Generator().manual_seed(M * 7 + N)
        A, B = torch.randn(G, M, K, generator=g), torch.randn(G, N, K, generator=g) / math.sqrt(K)
        bias, res = torch.randn(N, generator=g), torch.randn(G, M, N, generator=g)
        want = torch.relu(0.5 * torch.matmul(A.double(), B.double().transpose(1, 2)) + bias.double()) + res.double()
        return A, B, bias, res, want
    A, B, bias, res, want = cached(("gemm", M, N, K, G), make)
    if slab and gemm_mode == "split16":
        assert ops.slab_ok(M, N, K)

    def fn(put):
        if G == 1:
            return {"out": ops.linear(put(A[0]), put(B[0]), put(bias), act=1, alpha=0.5, resid=put(res[0]), slab=slab).unsqueeze(0)}
        out = put.empty(G, M, N)
        ops.gemm(put(A), put(B), out, M, N, K, K, K, N, G1=G, sa=(M * K, 0), sb=(N * K, 0), sc=(M * N, 0), alpha=0.5, bias=put(bias), act=1,
                 resid=put(res), sr=(M * N, 0), ldr=N)
        return {"out": out}
    got = run_guarded(poison, fn)
    check_parity(got, {"out": want}, 2e-6)


@pytest.mark.parametrize("M,N,K", [(7, 5, 64), (45, 2048, 512)])
def test_linear_with_fused_layer_norm(M, N, K, poison, gemm_mode):
    """PrdGemm.a_ln (the LayerNorm of the A rows inside the GEMM) at the smallest and a ragged-M shape of
    tests/test_hip_parity.py::test_linear_with_fused_layer_norm, on its inputs (rows with |mean| several times the spread),
    against LayerNorm + float64 matmul at its bound, 5e-6."""
    def make():
        g = torch.Generator().manual_seed(M + N + K)
        x = torch.randn(M, K, generator=g) * 2.0
        x[::3] = x[::3] * 0.25 + 4.0
        w, b = torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g)
        return x, w, b, torch.relu(O.ln(x).double() @ w.double().t() + b.double())
    x, w, b, want = cached(("gemm_ln", M, N, K), make)
    got = run_guarded(poison, lambda put: {"out": ops.linear(put(x), put(w), put(b), act=1, ln_a=True)})
    check_parity(got, {"out": want}, 5e-6)


# ---------------------------------------------------------------------------------------------------
# long rows: the long-row core, its ragged key tail, the key-chunked form with its statistics workspace
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("N,valid", [(385, 380), (417, 416), (961, 950)])
@pytest.mark.parametrize("P", [32, 64])
def test_triangle_attention_long_rows(P, N, valid, mode, poison, gemm_mode):
    """N = 385 / 417: tri_attn_core_v2l in split-16 arithmetic (a last key tile of one key: 385 = 12 x 32 + 1, 417 = 13 x 32 + 1,
    with 417 = 6 x 64 + 33 rows not split over idle workgroups); N = 961: past the 960 positions up to which K / V of a row stay in
    the LDS of the fp32 kernels -- key-chunked there (P = 64), with the softmax statistics workspace of prd_tri_attn_stats_bytes.
    The oracle is consulted on the row subset of tests/test_hip_parity.py::test_triangle_attention_long_rows; (a) and (b) cover
    every other row."""
    args, model, params = model_for(P)
    H, c = args["num_heads"], args["head_dim"]
    pfx = f"{B0}.pair_attn_{mode}"

    def make_pair():
        pair = torch.randn(1, N, N, P, generator=torch.Generator().manual_seed(N))
        mask = torch.ones(1, N)
        mask[0, valid:] = 0
        return pair, mask
    pair, mask = cached(("long_pair", P, N), make_pair)

    def make():
        g = torch.Generator().manual_seed(N + (mode == "ending"))
        rows = sorted({0, 1, 31, 32, 63, 64, N // 2, valid - 1, min(valid, N - 1), N - 1} | set(torch.randint(0, N, (6,), generator=g).tolist()))
        m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
        with torch.inference_mode():
            if mode == "starting":
                sub, msub = pair[:, rows], m2[:, rows]
            else:
                sub, msub = pair[:, :, rows].transpose(1, 2), m2[:, :, rows].transpose(1, 2)
            want = O.gated_attention(params, pfx + ".attn", sub, msub, H, c)
        return rows, want
    rows, want = cached(("long", P, N, mode), make)
    if N > 960 and P == 64 and gemm_mode == "fp32":
        assert ops.tri_attn_variant(N, P) == 3 and ops.tri_attn_stats_floats(1, N, P, H) > 0
    mod = getattr(model.Denoiser.folding_blocks[0], f"pair_attn_{mode}")

    def fn(put):
        full = mod.run(put(pair), put(mask), residual=False)
        return {"pair": full, "rows": (full[:, rows] if mode == "starting" else full[:, :, rows].transpose(1, 2)).contiguous()}
    with guarded(poison, modules=[model]) as g:
        outs = fn(Put(g))
        torch.cuda.synchronize()
        assert g.intact(), g.report()
        check_written("pair", outs["pair"])
        got = outs["rows"].cpu()
    assert rel_l2(got, want) < OP_TOL
    for k in range(len(rows)):
        assert rel_l2(got[:, k], want[:, k]) < 2 * OP_TOL, rows[k]


# ---------------------------------------------------------------------------------------------------
# mask_lowest_k, the reverse update and the step boundary
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["random", "spatial", "nearest", "within"])
@pytest.mark.parametrize("b,N", [(1, 33), (2, 70), (3, 130), (2, 2049)])
def test_mask_lowest_k(b, N, mode, poison):
    """prd_mask_lowest_k in its three modes (random key, spatial, the two ligand forms) against masking.restate_lowest_k, exactly;
    N = 2049 is one position over the kernel's LDS tile of 2048 keys."""
    rm, am, key, ap, rap, tokens = seeded_inputs(b, N, 31 * N + b, False)
    ca = rap[:, :, 1].contiguous()
    if mode == "random":
        p, kw = torch.full((b,), 0.37), dict(key=key)
    elif mode == "spatial":
        # ONE k = int(p x the lower median of the counts): the first k from 0.37 of the median on at which no sample has two keys
        # within 1e-3 (relative) of each other at the boundary -- fp32 rounding in another summation order cannot move a residue
        kw = dict(atom_pos=ap, atom_mask=am, ca_pos=ca)
        d = masking.spatial_keys(ap.double(), am.double(), ca.double())
        med = float((rm > 0.5).sum(-1).float().median())
        sorted_keys = [torch.sort(d[s][rm[s] > 0.5]).values for s in range(b)]
        k = next(k for k in range(int(0.37 * med), int(med)) if all(k >= ds.numel() or float(ds[k] - ds[k - 1]) >= 1e-3 * float(ds[k])
                                                                       for ds in sorted_keys))
        p = torch.full((b,), (k + 0.5) / med)
    else:
        kw = dict(atom_pos=ap, atom_mask=am, ca_pos=ca, ligand=mode)
        keys = masking.ligand_keys(ap, am, ca)
        # "within": a radius halfway between two neighbouring keys of sample 0, so that no key sits on the boundary
        ks = torch.sort(keys[rm > 0.5]).values
        p = torch.full((b,), 0.37) if mode == "nearest" else torch.full((b,), float(0.5 * (ks[ks.numel() // 3] + ks[ks.numel() // 3 + 1])))
    want = masking.restate_lowest_k(rm, p, tokens=tokens, **kw)
    if mode == "spatial":
        assert int(want[1][0].sum()) == min(k, int((rm[0] > 0.5).sum()))

    def fn(put):
        tok = put(tokens)
        dkw = {k: (put(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
        extra, inv = ops.mask_lowest_k(put(rm), put(p), tokens=tok, **dkw)
        return {"extra": extra, "inv": inv, "tokens": tok}
    got = run_guarded(poison, fn)
    for name, w in zip(("extra", "inv", "tokens"), want):
        assert torch.equal(got[name], w), (name, int((got[name] != w).sum()))


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("P", [32, 64])
def test_reverse_update_and_step_boundary(P, fused, poison, gemm_mode, monkeypatch):
    """The reverse loop launch by launch (no graph): prd_step_boundary (reverse update + the next step's single / time-embedding
    inputs + the sequence head's last layer), and with PRD_FUSED_BOUNDARY=0 prd_reverse_update, against the oracle's loop at the
    trajectory tolerance; N = 45, b = 2, ragged."""
    args, model, params = model_for(P)
    monkeypatch.setenv("PRD_FUSED_BOUNDARY", "1" if fused else "0")
    monkeypatch.setattr(model, "use_hip_graph", False)
    sizes = [(6, 39), (5, 33)]
    batch = synthetic_batch(sizes, esm_dim=args["esm_dim"], seed=300 + P)
    want = cached(("loop", P), lambda: O.sample(params, args, clone_batch(batch), [NoiseSource(5, k) for k in range(2)]))

    def fn(put):
        pos, logits = model.sample({k: (put(v) if torch.is_tensor(v) else v) for k, v in clone_batch(batch).items()},
                                   sources=[NoiseSource(5, k) for k in range(2)])
        return {"pos": pos, "logits": logits}
    got = run_guarded(poison, fn, modules=[model])
    # a non-finite loop must not be rescued by the fp32 repeat of nonfinite_policy = "fp32" (which would also pin the shared model)
    assert model.arith_fallbacks == 0 and model.arithmetic is None
    check_parity(got, {"pos": want[0], "logits": want[1]}, TRAJ_TOL)


# ---------------------------------------------------------------------------------------------------
# the whole step, the sampler with its captured graph
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [45, 130])
@pytest.mark.parametrize("P", [32, 64])
def test_sample_step(P, N, poison, gemm_mode):
    """model.sample_step against the oracle's step at BLOCK_TOL: N = 45 with b = 2 (ragged: 45 and 38 valid), N = 130 (123 valid)."""
    args, model, params = model_for(P)
    sizes = [(6, 39), (5, 33)] if N == 45 else SHAPES[130]

    def make():
        batch = synthetic_batch(sizes, esm_dim=args["esm_dim"], seed=40 + P + N, n_total=N)
        perms = [NoiseSource(NOISE_SEED, 100 + k).randperm(n) for k, (_, n) in enumerate(sizes)]
        pb = O.prepare_batch(batch, args["mask_prob"], perms)
        g = torch.Generator().manual_seed(N + P)
        b = len(sizes)
        z, seq_t, t = torch.randn(b, N, 3, generator=g), torch.randn(b, N, 21, generator=g), torch.tensor([5, 2][:b])
        with torch.inference_mode():
            want = O.network_step(params, args, pb, z, seq_t, pb["residue_and_atom_mask"], t)
        return pb, z, seq_t, t, want
    pb, z, seq_t, t, want = cached(("step", P, N), make)

    def fn(put):
        d = {k: (put(v) if torch.is_tensor(v) else v) for k, v in pb.items()}
        with torch.inference_mode():
            eps, logits = model.sample_step(d, put(z), put(seq_t), d["residue_and_atom_mask"], put(t))
        return {"eps": eps, "logits": logits}
    got = run_guarded(poison, fn, modules=[model])
    check_parity(got, {"eps": want[0], "logits": want[1]}, BLOCK_TOL)


@pytest.mark.parametrize("name", ["small32", "small64"])
def test_sample_with_its_captured_graph(golden, name, poison, gemm_mode):
    """model.sample() as it is -- first step eager, the second captured, the rest replayed -- with every buffer of the eager steps
    and of the graph's pool guarded: guards checked after the last replay, the trajectory against the golden vectors at TRAJ_TOL,
    and bit-equal to the same call outside the manager (the result does not depend on surrounding memory).  The guarded graph is not
    the shipped graph of 73 launches: the poison fill of every carved buffer is captured with it, so each replay also re-poisons
    interiors and guards before the step's kernels run."""
    case_, z, args, model, params = cached(("golden_model", name), lambda: golden_case(golden, name))
    one = synthetic_batch([tuple(case_["traj_sample"])], esm_dim=args["esm_dim"], seed=case_["batch_seed"] + 500)
    assert model.use_hip_graph
    plain = model.sample(batch_to(clone_batch(one), DEV), sources=[NoiseSource(NOISE_SEED, 0)])
    plain = [t.cpu() for t in plain]

    def fn(put):
        pos, logits = model.sample({k: (put(v) if torch.is_tensor(v) else v) for k, v in clone_batch(one).items()},
                                   sources=[NoiseSource(NOISE_SEED, 0)])
        return {"pos": pos, "logits": logits}
    got = run_guarded(poison, fn, modules=[model])
    assert model.arith_fallbacks == 0 and model.arithmetic is None      # (as above: no fp32 repeat behind the result)
    check_parity(got, {"pos": torch.from_numpy(z["traj_pos"]), "logits": torch.from_numpy(z["traj_logits"])}, TRAJ_TOL)
    assert torch.equal(got["pos"], plain[0]) and torch.equal(got["logits"], plain[1])


# ---------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small32", "small64"])
def test_training_step_gradients(golden, name, poison, gemm_mode, monkeypatch):
    """The loss and every gradient of the training step against the reference's fingerprints and the oracle's autograd, as
    tests/test_training_gpu.py holds them (GRAD_TOL, FINGERPRINT_TOL)."""
    case_, z, args, params, pb = cached(("train_inputs", name), lambda: case_inputs(golden, name))
    if name != "small32":
        monkeypatch.setattr(ops, "WGRAD_MIN_ROWS", 1)
    t = torch.from_numpy(z["train_t"])
    nz, ns = torch.from_numpy(z["train_noise_z"]), torch.from_numpy(z["train_noise_seq"])
    want_loss, want = cached(("train_want", name), lambda: oracle_grads(args, params, pb, t, nz, ns))
    model = hip_model(args, params)
    names = json.loads(str(z["train_grad_names"]))

    def fn(put):
        dpb = {k: (put(v) if torch.is_tensor(v) else v) for k, v in pb.items()}
        mask = dpb["residue_and_atom_mask"]
        diff = model.diffusion_loss(dpb, dpb["x"], mask, put(t), put(nz), put(ns))
        loss = torch.mean(diff / (mask > 0.5).sum(-1))
        loss.backward()
        return {"loss": loss, **{k: p.grad for k, p in model.named_parameters() if p.requires_grad}}
    got = run_guarded(poison, fn, modules=[model])
    loss = float(got.pop("loss"))
    assert abs(loss - float(z["train_loss"])) < GRAD_TOL * abs(float(z["train_loss"])) and abs(loss - want_loss) < GRAD_TOL * abs(want_loss)
    assert sorted(got) == sorted(names) and all(g is not None for g in got.values())
    scale = float(np.linalg.norm(z["train_grad_norm"]))
    for i, k in enumerate(names):
        g = got[k].double().reshape(-1)
        err, ref = float((g - want[k].double().reshape(-1)).norm()), float(want[k].double().norm())
        assert err < GRAD_TOL * ref + 1e-6 * scale, (k, err, ref)
        n_ref = float(z["train_grad_norm"][i])
        assert abs(float(g.norm()) - n_ref) < FINGERPRINT_TOL * n_ref + 1e-6 * scale, (k, float(g.norm()), n_ref)
        for j in range(GRAD_PROJECTIONS):
            gen = torch.Generator().manual_seed(4242 + 16 * i + j)
            proj = float(torch.dot(g, torch.randn(g.numel(), generator=gen, dtype=torch.float64)))
            assert abs(proj - float(z["train_grad_proj"][i, j])) < FINGERPRINT_TOL * n_ref + 1e-6 * scale, (k, j)


TM_NAMES = ["ab_proj.weight", "ab_proj.bias", "ab_gate.weight", "ab_gate.bias", "out_proj.weight", "out_proj.bias", "out_gate.weight", "out_gate.bias"]
TA4_NAMES = ["attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight", "attn.gate_proj.weight", "attn.gate_proj.bias",
             "attn.out_proj.weight", "attn.out_proj.bias"]


def ragged(b, N):
    mask = torch.ones(b, N)
    mask[b - 1, N - 7:] = 0
    return mask


@pytest.mark.parametrize("mode", ["outgoing", "incoming"])
@pytest.mark.parametrize("P,b,N", [(64, 2, 45), (32, 1, 97)])
def test_tri_mul_backward(P, b, N, mode, poison, gemm_mode):
    """ops.tri_mul_backward (forward recompute into its own workspace, the ldn = round_up(N, 32) strided operands, the stacked
    contraction, the weight gradients) against the oracle's autograd at the bound of tests/test_training_gpu.py, 1e-5."""
    def make():
        g = torch.Generator().manual_seed(70 + P + N)
        pair, mask = torch.randn(b, N, N, P, generator=g), ragged(b, N)
        shapes = [(2 * P, P), (2 * P,), (2 * P, P), (2 * P,), (P, P), (P,), (P, P), (P,)]
        wts = [torch.randn(s, generator=g) / (math.sqrt(P) if len(s) == 2 else 4.0) for s in shapes]
        dy = torch.randn(b, N, N, P, generator=g)
        pl = pair.clone().requires_grad_(True)
        leaf = {"tm." + n: w.clone().requires_grad_(True) for n, w in zip(TM_NAMES, wts)}
        O.triangle_multiplication(leaf, "tm", pl, mask.unsqueeze(-1) * mask.unsqueeze(-2), mode == "incoming").backward(dy)
        return pair, mask, wts, dy, {"pair": pl.grad, **{n: leaf["tm." + n].grad for n in TM_NAMES}}
    pair, mask, wts, dy, want = cached(("tm_bwd", P, b, N, mode), make)

    def fn(put):
        dpair, grads = ops.tri_mul_backward(put(dy), put(pair), put(mask), [put(w) for w in wts], incoming=mode == "incoming")
        return {"pair": dpair, **dict(zip(TM_NAMES, grads))}
    check_parity(run_guarded(poison, fn), want, 1e-5)


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("P,b,N", [(64, 2, 45), (64, 1, 97)])
def test_tri_attn_backward(P, b, N, mode, poison, gemm_mode):
    """ops.tri_attn_backward at 4 x 16 (forward recompute with kept statistics where the arithmetic has them, the tuned backward
    cores, prd_ln_rows_bwd, the weight gradients) against the oracle's autograd at 1e-5 (tests/test_training_gpu.py)."""
    H, c = 4, 16

    def make():
        g = torch.Generator().manual_seed(80 + P + N)
        pair, mask = torch.randn(b, N, N, P, generator=g), ragged(b, N)
        shapes = [(64, P), (64, P), (64, P), (64, P), (64,), (P, 64), (P,)]
        wts = [torch.randn(s, generator=g) / (math.sqrt(s[-1]) if len(s) == 2 else 4.0) for s in shapes]
        dy = torch.randn(b, N, N, P, generator=g)
        pl = pair.clone().requires_grad_(True)
        leaf = {"ta." + n: w.clone().requires_grad_(True) for n, w in zip(TA4_NAMES, wts)}
        O.triangle_attention(leaf, "ta", pl, mask.unsqueeze(-1) * mask.unsqueeze(-2), H, c, mode == "ending").backward(dy)
        return pair, mask, wts, dy, {"pair": pl.grad, **{n: leaf["ta." + n].grad for n in TA4_NAMES}}
    pair, mask, wts, dy, want = cached(("ta_bwd", P, b, N, mode), make)

    def fn(put):
        dpair, grads = ops.tri_attn_backward(put(dy), put(pair), put(mask), [put(w) for w in wts], H, c, ending=mode == "ending")
        return {"pair": dpair, **dict(zip(TA4_NAMES, grads))}
    check_parity(run_guarded(poison, fn), want, 1e-5)


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("N", [30, 97])
def test_tri_attn_bwd_core_heads(N, mode, poison, gemm_mode):
    """prd_tri_attn_bwd_core_heads at 8 x 32 (with prd_tri_attn_core_heads_lse's statistics and both workspace queries) through
    ops.tri_attn_backward, against float64 autograd under the criteria of tests/test_head_layouts_backward.py (check_grads)."""
    H, c, P, b = 8, 32, 64, 2
    ending = mode == "ending"

    def make():
        g = torch.Generator().manual_seed(9000 + 131 * H + 7 * c + N + b + P)
        pair, mask = torch.randn(b, N, N, P, generator=g), ragged(b, N)
        HC = H * c
        shapes = [(HC, P), (HC, P), (HC, P), (HC, P), (HC,), (P, HC), (P,)]
        wts = [torch.randn(*s, generator=g) * (1 / math.sqrt(s[-1]) if len(s) == 2 else 0.25) for s in shapes]
        dy = torch.randn(b, N, N, P, generator=g)
        want = float64_grads(pair.to(DEV), mask.to(DEV), [w.to(DEV) for w in wts], dy.to(DEV), H, c, ending)
        return pair, mask, wts, dy, [w.cpu() for w in want]
    pair, mask, wts, dy, want = cached(("heads_bwd", N, mode), make)

    def fn(put):
        dpair, grads = ops.tri_attn_backward(put(dy), put(pair), put(mask), [put(w) for w in wts], H, c, ending=ending)
        return {"pair": dpair, **dict(zip(TA_NAMES, grads))}
    got = run_guarded(poison, fn)
    check_grads(["pair", *TA_NAMES], [got[n] for n in ["pair", *TA_NAMES]], want, 1.0, tag=f"guarded 8x32 {mode} N={N} [{gemm_mode}]")


def test_weight_gradient_reductions(poison, gemm_mode):
    """The slab reductions with a workspace query of their own, at a row count that is no multiple of any slab (9001), and the
    outer-linear backward's reductions at R = 301: prd_linear_wgrad (through a strided column slice, with the bias gradient),
    prd_embed_wgrad, prd_embed_wgrad_multi, prd_outer_linear_bwd_reduce -- against float64 at the bounds of
    tests/test_training_gpu.py (2e-6; 1e-6 for the outer-linear reductions)."""
    rows = 9001
    assert rows >= ops.WGRAD_MIN_ROWS

    def make():
        g = torch.Generator().manual_seed(rows)
        wide, x = torch.randn(rows, 128 + 64, generator=g), torch.randn(rows, 128, generator=g)
        cards = [5, 6, 2, 8, 65]
        dy = torch.randn(rows, 32, generator=g)
        idxs = [torch.randint(0, k, (rows,), generator=g) for k in cards]
        idxs[1][:7] = -1
        scales = [torch.rand(rows, generator=g), None, torch.rand(rows, generator=g), None, (torch.rand(rows, generator=g) > 0.3).float()]
        T, w1, xs = torch.randn(301, 64, 130, generator=g), torch.randn(64, 260, generator=g), torch.randn(301, 130, generator=g)
        want = {"dw": wide[:, 64:].double().t() @ x.double(), "db": wide[:, 64:].double().sum(0)}
        for k, card in enumerate(cards):
            v = dy.double() * (scales[k].double().unsqueeze(1) if scales[k] is not None else 1.0)
            ok = idxs[k] >= 0
            want[f"table{k}"] = torch.zeros(card, 32, dtype=torch.float64).index_add_(0, idxs[k][ok], v[ok])
        want["table_one"] = torch.zeros(65, 32, dtype=torch.float64).index_add_(0, idxs[4], dy.double())
        want["dx"] = (T.double() * w1[:, :130].double()).sum(1)
        want["dw1"] = (T.double() * xs.double().unsqueeze(1)).sum(0)
        return wide, x, cards, dy, idxs, scales, T, w1, xs, want
    wide, x, cards, dy, idxs, scales, T, w1, xs, want = cached("wgrad", make)

    def fn(put):
        dw, db = ops.linear_wgrad(put(wide)[:, 64:], put(x), bias=True)
        ddy, didx = put(dy), [put(i) for i in idxs]
        tabs = ops.embed_wgrad_multi(didx, ddy, cards, [put(s) if s is not None else None for s in scales])
        one = ops.embed_wgrad(didx[4], ddy, 65)
        dx, dw1 = ops.outer_linear_bwd_reduce(put(T), put(w1)[:, :130], put(xs))
        return {"dw": dw, "db": db, **{f"table{k}": t for k, t in enumerate(tabs)}, "table_one": one, "dx": dx, "dw1": dw1}
    got = run_guarded(poison, fn)
    check_parity({k: got[k] for k in ("dx", "dw1")}, {k: want[k] for k in ("dx", "dw1")}, 1e-6)
    check_parity(got, {k: v for k, v in want.items() if k not in ("dx", "dw1")}, 2e-6)
