"""The issue / commit staging of the row kernels' prologues (csrc/prd_common.h: StageH2 ...), on the GPU, in split-16 arithmetic.

The staging can only go wrong where piece counts, optional operands or runtime sizes change, so the shapes are the smallest that
exercise those: N = 33 (one full 32-row tile and a ragged one), b in {1, 2}, pair_dim in {32, 64} (one / several pieces per thread,
threads without a piece), every optional operand present and absent, 1 / 4 / 8 bias-head rows, and the distance / outer-product
widths around the in-flight budget of the fused head.  References are the float64 forms of the oracle the corresponding tests of
tests/test_hip_parity.py use, at those tests' tolerances.  Every case runs twice and must give the same bits: a piece left unwritten
would otherwise hide behind whatever the LDS still held (run the file under PRD_LDS_POISON=1 as well)."""
import math

import pytest
import torch

import prd_oracle as O
from conftest import rel_l2
from protein_redesign_amd import _lib, ops
from test_hip_parity import BLOCK_TOL, OP_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 33


def cu(x):
    return x.to(DEV).contiguous()


@pytest.fixture(autouse=True)
def split16():
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(1) == 0
    yield
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


def twice(fn):
    """fn() -> tensor or tuple of tensors, run twice; the results of the first run, after checking the second has the same bits"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    ta = a if isinstance(a, (tuple, list)) else (a,)
    tb = b if isinstance(b, (tuple, list)) else (b,)
    for x, y in zip(ta, tb):
        assert torch.isfinite(x).all()
        assert torch.equal(x, y)
    return a


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def w_(g, o, i):
    return rnd(g, o, i, scale=1.0 / math.sqrt(i))


def f32(t):
    return cu(t.float())


def masked(b):
    mask = torch.ones(b, N, dtype=torch.float64)
    mask[b - 1, N - 4:] = 0
    return mask


# ---- pair_tail_h2_kernel: prd_block_tail (og given) and prd_pair_transition (og absent) -----------------------------------------
@pytest.mark.parametrize("H", [0, 1, 4, 8])
@pytest.mark.parametrize("P,b", [(32, 1), (64, 1), (64, 2)])
def test_block_tail(P, b, H):
    g = torch.Generator().manual_seed(11 * P + b + H)
    pair, og = rnd(g, b, N, N, P), rnd(g, b, N, N, 64)
    p = {"o.weight": w_(g, P, 64), "o.bias": rnd(g, P, scale=0.3), "fc.1.weight": w_(g, 4 * P, P), "fc.1.bias": rnd(g, 4 * P, scale=0.3),
         "fc.3.weight": w_(g, P, 4 * P), "fc.3.bias": rnd(g, P, scale=0.3), "ab.1.weight": w_(g, max(H, 1), P), "ab.1.bias": rnd(g, max(H, 1), scale=0.3)}
    want = pair + O.lin(p, "o", og)
    want = want + O.transition(p, "fc", want)
    d = {k: f32(v) for k, v in p.items()}

    def run():
        x = f32(pair)
        bias = ops.block_tail_(x, f32(og), d["o.weight"], d["o.bias"], d["fc.1.weight"], d["fc.1.bias"], d["fc.3.weight"], d["fc.3.bias"],
                               d["ab.1.weight"] if H else None, d["ab.1.bias"] if H else None)
        return (x, bias) if H else (x,)
    got = twice(run)
    assert rel_l2(got[0].cpu(), want) < BLOCK_TOL
    if H:
        assert rel_l2(got[1].cpu(), O.pair_bias(p, "ab", want)) < BLOCK_TOL


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("P,b", [(32, 1), (64, 2)])
def test_pair_transition_without_attention_output(P, b, residual):
    g = torch.Generator().manual_seed(13 * P + b)
    pair = rnd(g, b, N, N, P)
    p = {"fc.1.weight": w_(g, 4 * P, P), "fc.1.bias": rnd(g, 4 * P, scale=0.3), "fc.3.weight": w_(g, P, 4 * P), "fc.3.bias": rnd(g, P, scale=0.3)}
    want = O.transition(p, "fc", pair) + (pair if residual else 0)
    d = {k: f32(v) for k, v in p.items()}
    got = twice(lambda: ops.pair_transition(f32(pair), d["fc.1.weight"], d["fc.1.bias"], d["fc.3.weight"], d["fc.3.bias"], residual=residual))
    assert rel_l2(got.cpu(), want) < OP_TOL


# ---- pair_head_h2_kernel ------------------------------------------------------------------------------------------------------
# dist_dim: the widths the launch trace sweeps (128, 136, 256, 632), and 384 and 640.  128 and 256 are one chunk of the staging; 384
# (pair_dim 64) and 640 (pair_dim 32) exceed the in-flight budget of 4 pieces x 512 threads and run the chunk loop (640 also a second
# chunk of centers).  136 and 632 are not multiples of 128, for which the natural-order image does not exist, and 640 x 64 does not
# fit the LDS: the library must say so (the model then runs the three separate launches).
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("Ha,Hb", [(1, 8), (8, 1)])
@pytest.mark.parametrize("DK", [128, 136, 256, 384, 632, 640])
@pytest.mark.parametrize("P,b", [(32, 1), (64, 2)])
def test_pair_head(P, b, DK, Ha, Hb, affine):
    C = 128
    g = torch.Generator().manual_seed(17 * P + DK + Ha)
    sp, z, mask = f32(rnd(g, b, N, N, P)), f32(rnd(g, b, N, 3, scale=3.0)), f32(masked(b))
    centers, w_dist, eb = f32(torch.linspace(0, 2, DK, dtype=torch.float64)), f32(w_(g, P, DK)), f32(rnd(g, b, P))
    ab, w_out, b_out = f32(rnd(g, b, N, 2 * C)), f32(w_(g, P, C)), f32(rnd(g, P, scale=0.3))

    def head_set(H, with_affine):
        return (f32(w_(g, H, P)), f32(rnd(g, H, scale=0.3)), f32(1 + rnd(g, P, scale=0.1)) if with_affine else None,
                f32(rnd(g, P, scale=0.1)) if with_affine else None)
    set_a, set_b = head_set(Ha, True), head_set(Hb, affine)         # (one set always with the LayerNorm affine pair, as in the model)
    if not affine:
        set_a, set_b = set_b, set_a
    lds = 4 * P * DK + 4 * P * C + (DK + 21 * P) * 4                # the image of the fused head (pair_head_lds_bytes)
    assert ops.pair_head_supported(P, DK, C) == (DK % 128 == 0 and lds <= 160 * 1024)
    if not ops.pair_head_supported(P, DK, C):
        with pytest.raises(Exception):
            ops.pair_head(sp, z, mask, centers, w_dist, eb, ab, w_out, b_out, apply_mask=True, set_a=set_a, set_b=set_b)
        return
    # reference: the three separate launches it fuses (their kernels keep the loop staging), as in
    # test_fused_launches_equal_their_separate_forms, at its tolerance
    want = ops.pair_init(sp, z, mask, centers, w_dist, eb)
    want = ops.opm_pair(want, ab, mask, w_out, b_out, residual=True, apply_mask=True)
    want_a, want_b = ops.pair_bias2(want, set_a, set_b)
    got = twice(lambda: ops.pair_head(sp, z, mask, centers, w_dist, eb, ab, w_out, b_out, apply_mask=True, set_a=set_a, set_b=set_b))
    for x, y in zip(got, (want, want_a, want_b)):
        assert rel_l2(x.cpu(), y.cpu()) < OP_TOL


# ---- the triangle multiplication's row kernels and tri_attn_out -----------------------------------------------------------------
def tri_mul_params(g, P, prefix):
    return {f"{prefix}.ab_proj.weight": w_(g, 2 * P, P), f"{prefix}.ab_proj.bias": rnd(g, 2 * P, scale=0.3),
            f"{prefix}.ab_gate.weight": w_(g, 2 * P, P), f"{prefix}.ab_gate.bias": rnd(g, 2 * P, scale=0.3),
            f"{prefix}.out_proj.weight": w_(g, P, P), f"{prefix}.out_proj.bias": rnd(g, P, scale=0.3),
            f"{prefix}.out_gate.weight": w_(g, P, P), f"{prefix}.out_gate.bias": rnd(g, P, scale=0.3)}


def tri_mul_wts(p, prefix):
    return [f32(p[f"{prefix}.{n}.{k}"]) for n in ("ab_proj", "ab_gate", "out_proj", "out_gate") for k in ("weight", "bias")]


@pytest.mark.parametrize("P,b", [(32, 1), (64, 1), (64, 2)])
def test_tri_mul_chain(P, b):
    assert ops.tri_mul_chain_supported(N, P)
    g = torch.Generator().manual_seed(19 * P + b)
    p = {**tri_mul_params(g, P, "outgoing"), **tri_mul_params(g, P, "incoming")}
    pair, mask = rnd(g, b, N, N, P), masked(b)
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    want = pair + O.triangle_multiplication(p, "outgoing", pair, m2, False)
    want = want + O.triangle_multiplication(p, "incoming", want, m2, True)
    got = twice(lambda: ops.tri_mul_chain_(f32(pair), f32(mask), tri_mul_wts(p, "outgoing"), tri_mul_wts(p, "incoming")))
    assert rel_l2(got.cpu(), want) < OP_TOL


@pytest.mark.parametrize("incoming", [False, True])
@pytest.mark.parametrize("P,b", [(32, 1), (64, 1), (64, 2)])
def test_tri_mul_plain(P, b, incoming):
    g = torch.Generator().manual_seed(23 * P + b + incoming)
    p = tri_mul_params(g, P, "m")
    pair, mask = rnd(g, b, N, N, P), masked(b)
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    want = O.triangle_multiplication(p, "m", pair, m2, incoming)
    got = twice(lambda: ops.tri_mul(f32(pair), f32(mask), tri_mul_wts(p, "m"), incoming=incoming, residual=False))
    assert rel_l2(got.cpu(), want) < OP_TOL


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("P,b", [(32, 1), (64, 1), (64, 2)])
def test_tri_attn_out(P, b, residual):
    g = torch.Generator().manual_seed(29 * P + b)
    pair, og = rnd(g, b, N, N, P), rnd(g, b, N, N, 64)
    p = {"o.weight": w_(g, P, 64), "o.bias": rnd(g, P, scale=0.3)}
    want = O.lin(p, "o", og) + (pair if residual else 0)
    got = twice(lambda: ops.tri_attn_out(f32(pair), f32(og), f32(p["o.weight"]), f32(p["o.bias"]), residual=residual))
    assert rel_l2(got.cpu(), want) < OP_TOL


# ---- coordinate head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,b", [(32, 1), (64, 1), (64, 2)])
def test_coord_head(P, b):
    g = torch.Generator().manual_seed(31 * P + b)
    pair, z, mask = rnd(g, b, N, N, P), rnd(g, b, N, 3, scale=3.0), masked(b)
    p = {"weight_radial.1.weight": w_(g, P, P), "weight_radial.1.bias": rnd(g, P, scale=0.3), "weight_radial.3.weight": w_(g, 1, P)}
    # O.heads without its mean removal and sequence half: the kernel symmetrises the pair itself
    sym = 0.5 * (pair + pair.transpose(1, 2))
    w = torch.nn.functional.linear(torch.relu(O.lin(p, "weight_radial.1", O.ln(sym))), p["weight_radial.3.weight"])
    zij = z.unsqueeze(2) - z.unsqueeze(1)
    r = zij * torch.rsqrt(torch.sum(torch.square(zij), -1, keepdim=True) + 1e-4)
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    want = (m2.unsqueeze(-1) * w * r).sum(dim=2)
    got = twice(lambda: ops.coord_head(f32(pair), f32(z), f32(mask), f32(p["weight_radial.1.weight"]), f32(p["weight_radial.1.bias"]),
                                       f32(p["weight_radial.3.weight"])))
    assert rel_l2(got.cpu(), want) < OP_TOL


# ---- the triangle-attention cores' weight image -------------------------------------------------------------------------------
# N = 33 and 320: the short-row cores (v3 at 320, the bench shape); N = 449: the long-row core (v2l).
@pytest.mark.parametrize("ending", [False, True])
@pytest.mark.parametrize("P,n", [(32, 33), (64, 33), (64, 320), (64, 449)])
def test_tri_attn_core(P, n, ending):
    H, c = 4, 16
    assert ops.tri_attn_v2_supported(n, P)
    g = torch.Generator().manual_seed(37 * P + n)
    pair = rnd(g, 1, n, n, P)
    mask = torch.ones(1, n, dtype=torch.float64)
    mask[0, n - 5:] = 0
    p = {f"a.{k}_proj.weight": w_(g, H * c, P) for k in ("q", "k", "v", "gate")}
    p["a.gate_proj.bias"] = rnd(g, H * c, scale=0.3)
    p["a.out_proj.weight"] = torch.eye(H * c, dtype=torch.float64)          # the core's output is what the projection receives
    wts = [f32(p[f"a.{k}_proj.weight"]) for k in ("q", "k", "v", "gate")] + [f32(p["a.gate_proj.bias"])]
    dpair, dmask = f32(pair), f32(mask)
    got = twice(lambda: ops.tri_attn_core_v2(dpair, dmask, wts, H, c, ending=ending)).cpu()
    # whole tensor against the fp32-MFMA core (another kernel, which keeps the loop staging), rows against the oracle in float64:
    # the two references of test_triangle_attention_core_v2
    assert _lib.lib().prd_set_gemm_mode(0) == 0
    ref = ops.tri_attn_core(dpair, dmask, wts, H, c, ending=ending)
    assert _lib.lib().prd_set_gemm_mode(1) == 0
    assert rel_l2(got, ref.cpu()) < OP_TOL
    rows = sorted({0, n // 2, n - 6, n - 1} | set(torch.randint(0, n, (3,), generator=g).tolist()))
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    if not ending:
        sub, msub, gsub = pair[:, rows], m2[:, rows], got[:, rows]
    else:
        sub, msub, gsub = pair[:, :, rows].transpose(1, 2), m2[:, :, rows].transpose(1, 2), got[:, :, rows].transpose(1, 2)
    want = O.gated_attention(p, "a", sub, msub, H, c)
    assert rel_l2(gsub, want) < OP_TOL
