"""GPU: the hand-written backward kernels at the shapes and gradient scales of training (BASELINE configs[3] per GPU: 2 complexes,
N = 320..384, pair_dim 64) against float64 autograd of the oracle's restatement of each operator.

Every case holds every returned gradient (input and weights) to rel-L2 < OP_TOL, and the pair gradient's worst 64 x 64 block of
positions (i, j) to BLOCK_TOL, so that one bad tile, a ragged edge or the row padding cannot hide in the whole-tensor norm.  The
incoming gradient ``dy`` is drawn at several scales: gradients are linear in it, so the relative error must not depend on its
scale.  Training feeds the backward gradients of rms ~1e-2 and below; the split-16 arithmetic (fp16 hi + lo operands) loses
them to the fp16 subnormal range unless the split operand is scaled.

The float64 references run on the device (plain torch ops, not project kernels), from dy at scale 1, and are cached across the
two arithmetic modes and the dy scales."""
import math
from types import SimpleNamespace

import pytest
import torch

import prd_oracle as O
from protein_redesign_amd import _lib, ops, training

pytestmark = pytest.mark.gpu
DEV = "cuda"
OP_TOL = 1e-5           # the operator bar of the suite
BLOCK_TOL = 4e-5        # worst 64 x 64 block of pair positions


@pytest.fixture(params=["fp32", "split16"])
def gemm_mode(request):
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(_lib.GEMM_MODES[request.param]) == 0
    yield request.param
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


# key -> inputs and float64 reference gradients for dy at scale 1, on the device, shared by both arithmetic modes (pytest runs every
# fp32 case before the split-16 ones): about 4 GB for the whole file
_WANT = {}


def cached(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def ragged_mask(b, N):
    mask = torch.ones(b, N)
    mask[b - 1, N - 9:] = 0                     # the last complex is shorter than the padded length
    return mask.to(DEV)


def rel(got, want):
    want = want.double()
    return float((got.double() - want).norm() / want.norm().clamp_min(1e-300))


def worst_block(got, want, blk=64):
    """Largest ||got - want|| / ||want|| over the 64 x 64 blocks of pair positions (i, j) of a [b, N, N, C] gradient.  A block whose
    reference is tiny against the average block (exact zeros of masked positions) is measured against 1e-3 of that average."""
    b, N = want.shape[:2]
    T = (N + blk - 1) // blk
    d = torch.zeros(b, T * blk, T * blk, device=want.device, dtype=torch.float64)
    w = torch.zeros_like(d)
    d[:, :N, :N] = (got.double() - want.double()).pow(2).flatten(3).sum(-1)
    w[:, :N, :N] = want.double().pow(2).flatten(3).sum(-1)
    e = d.view(b, T, blk, T, blk).sum(dim=(2, 4)).sqrt()
    r = w.view(b, T, blk, T, blk).sum(dim=(2, 4)).sqrt()
    floor = 1e-3 * float(r.mean())
    worst = e / r.clamp_min(floor)
    k = int(worst.argmax())
    return float(worst.max()), (k // (T * T), (k // T) % T * blk, k % T * blk)


def check_grads(names, got, want, scale, pair_grads=("pair",), tag=""):
    """got[k] against scale * want[k], whole tensor and (for the pair gradients) by block; one message with every figure."""
    errs, fails = {}, []
    for n, a, w in zip(names, got, want):
        assert a is not None, n
        assert torch.isfinite(a).all(), f"{tag} {n}: non-finite gradient"
        ws = w * scale
        errs[n] = rel(a, ws)
        if errs[n] >= OP_TOL:
            fails.append(f"{n} rel-L2 {errs[n]:.2e}")
        if n in pair_grads:
            wb, at = worst_block(a, ws)
            errs[n + "[block]"] = wb
            if wb >= BLOCK_TOL:
                fails.append(f"{n} worst 64x64 block {wb:.2e} at (b, i0, j0) = {at}")
    print(f"\n{tag} dy x {scale:g}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert not fails, f"{tag} dy x {scale:g}: " + "; ".join(fails)


# ---------------------------------------------------------------------------------------------------
# A. TriangleMultiplication: TriMulFn (forward workspace reused) and ops.tri_mul_backward(ws=None)
# ---------------------------------------------------------------------------------------------------

TM_NAMES = ["ab_proj.weight", "ab_proj.bias", "ab_gate.weight", "ab_gate.bias", "out_proj.weight", "out_proj.bias", "out_gate.weight",
            "out_gate.bias"]


def tri_mul_case(P, b, N, incoming):
    def make():
        g = torch.Generator().manual_seed(7000 + 10 * N + P + b)
        pair = randn(g, b, N, N, P)
        mask = ragged_mask(b, N)
        shapes = [(2 * P, P), (2 * P,), (2 * P, P), (2 * P,), (P, P), (P,), (P, P), (P,)]
        wts = [randn(g, *s, scale=1 / math.sqrt(P) if len(s) == 2 else 0.25) for s in shapes]
        dy = randn(g, b, N, N, P)
        leaves = [t.double().requires_grad_(True) for t in (pair, *wts)]
        m2 = (mask.unsqueeze(-1) * mask.unsqueeze(-2)).double()
        out = O.triangle_multiplication({"tm." + n: w for n, w in zip(TM_NAMES, leaves[1:])}, "tm", leaves[0], m2, incoming)
        want = [x.detach() for x in torch.autograd.grad(out, leaves, dy.double())]
        return pair, mask, wts, dy, want
    return cached(("tri_mul", P, b, N, incoming), make)


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e-6])
@pytest.mark.parametrize("path", ["fn", "fn_residual", "ws_none"])
@pytest.mark.parametrize("mode", ["outgoing", "incoming"])
@pytest.mark.parametrize("P,b,N", [(64, 2, 320), (64, 1, 384), (64, 2, 200), (64, 1, 97), (32, 1, 161)])
def test_tri_mul_backward(P, b, N, mode, path, scale, gemm_mode):
    """(64, 2, 320): several 160 x 160 contraction tiles per channel and off-diagonal transpose tiles, ragged second complex;
    384 = 2 x 160 + 64: a ragged last contraction tile; 200, 97, 161: N % 32 != 0, the row padding ldn > N."""
    incoming = mode == "incoming"
    pair, mask, wts, dy0, want = tri_mul_case(P, b, N, incoming)
    dy = dy0 * scale
    if path == "ws_none":
        dpair, grads = ops.tri_mul_backward(dy, pair, mask, wts, incoming=incoming, ws=None)
        got = [dpair, *grads]
    else:
        residual = path == "fn_residual"
        leaves = [t.clone().requires_grad_(True) for t in (pair, *wts)]
        out = training.TriMulFn.apply(leaves[0], mask, incoming, residual, *leaves[1:])
        got = list(torch.autograd.grad(out, leaves, dy))
        if residual:
            want = [want[0] + dy0.double(), *want[1:]]
    check_grads(["pair", *TM_NAMES], got, want, scale, tag=f"tri_mul {mode} {path} P={P} b={b} N={N} [{gemm_mode}]")


# ---------------------------------------------------------------------------------------------------
# B. the stacked gradient contraction dA | dB = [dO | dO^T] x [B^T | A^T] on prd_tri_mul_contract (2P = 128 channels)
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dscale", [1e-3, 1e-6])
@pytest.mark.parametrize("N", [161, 320, 384, 200])
def test_stacked_gradient_contraction(N, dscale, gemm_mode):
    """O[c, m, n] = sum_k A[c, m, k] B[c, n, k] for 128 channels per complex, as the backward runs it (prd_tri_mul_contract_scaled):
    the first operand (the gradient dO | dO^T) small, with its max |.| per complex as the backward's output stage leaves it, the
    second (the forward operands B^T | A^T) O(1); against float64 to the tolerance of test_triangle_multiplication_contraction_direct.
    (The unscaled split, prd_tri_mul_contract, gave 1.7e-5 at dO x 1e-3 and 1.7e-2 at 1e-6.)"""
    from protein_redesign_amd._lib import check, dptr, stream
    C, b = 128, 2
    ldn = (N + 31) // 32 * 32
    g = torch.Generator().manual_seed(9000 + N)
    ab = torch.zeros(b, 2 * C, N, ldn, device=DEV)
    ab[..., :N] = randn(g, b, 2 * C, N, N)
    ab[:, :C] *= dscale
    want = torch.einsum("bpmk,bpnk->bpmn", ab[:, :C, :, :N].double(), ab[:, C:, :, :N].double())
    amax = ab[:, :C].abs().amax(dim=(1, 2, 3)).contiguous().view(torch.int32)        # float bits of max |dO| per complex
    o = torch.full((b, C, N, ldn), float("nan"), device=DEV)
    check(_lib.lib().prd_tri_mul_contract_scaled(dptr(o), dptr(ab), dptr(amax, torch.int32), b, N, C, stream()),
          "prd_tri_mul_contract_scaled")
    got = o[..., :N]
    assert torch.isfinite(got).all()
    err = rel(got, want)
    print(f"\ncontract 2P=128 N={N} dO x {dscale:g} [{gemm_mode}]: rel-L2 {err:.2e}")
    assert err < 2e-6


# ---------------------------------------------------------------------------------------------------
# C. OuterLinearFn: the split-16 tile GEMM branch (N % 32 == 0, >= 512 tiles) and the batched-GEMM branch
# ---------------------------------------------------------------------------------------------------

def outer_linear_fwd(x, w, c, pair_in=None):
    """The HIP forward of the outer-linear update as training.folding_block runs it."""
    bsz, n, S = x.shape
    P = w.shape[0]
    out = torch.empty(bsz, n, n, P, device=x.device, dtype=torch.float32)
    xn = ops.layer_norm(x.contiguous())
    u = torch.empty(bsz, n, P, device=x.device, dtype=torch.float32)
    ops.gemm(xn, w, u, bsz * n, P, S, S, 2 * S, P, b_off=S)
    if pair_in is not None:
        return ops.outer_linear_pair(pair_in, xn, u, w, c, residual=True, out=out)
    return ops.outer_linear_pair(out, xn, u, w, c, residual=False, out=out)


@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("b,N,S,P", [(2, 320, 512, 64), (1, 384, 512, 64), (2, 140, 512, 64)])
def test_outer_linear_backward(b, N, S, P, residual, scale, gemm_mode):
    def make():
        g = torch.Generator().manual_seed(8000 + N + b)
        single = randn(g, b, N, S)
        w = randn(g, P, 2 * S, scale=1 / math.sqrt(2 * S))
        c = randn(g, P, scale=0.25)
        pair = randn(g, b, N, N, P)
        dy = randn(g, b, N, N, P)
        leaves = [t.double().requires_grad_(True) for t in (single, w, c)]
        out = O.outer_linear({"ol.linear.weight": leaves[1], "ol.linear.bias": leaves[2]}, "ol", leaves[0])
        want = [x.detach() for x in torch.autograd.grad(out, leaves, dy.double())]
        return single, w, c, pair, dy, want
    single, w, c, pair, dy0, want = cached(("outer_linear", b, N, S, P), make)
    if gemm_mode == "split16" and N % 32 == 0:
        assert ops.split16_gemm_ok(N * P, S, N)         # the tile-GEMM branch of OuterLinearFn.backward runs
    else:
        assert not ops.split16_gemm_ok(N * P, S, N)
    leaves = [t.clone().requires_grad_(True) for t in (single, w, c)]
    names = ["single", "weight", "bias"]
    if residual:
        pl = pair.clone().requires_grad_(True)
        out = training.OuterLinearFn.apply(*leaves, outer_linear_fwd, pl)
        got = torch.autograd.grad(out, leaves + [pl], dy0 * scale)
        names, want = names + ["pair"], want + [dy0.double()]
    else:
        out = training.OuterLinearFn.apply(*leaves, outer_linear_fwd)
        got = torch.autograd.grad(out, leaves, dy0 * scale)
    check_grads(names, got, want, scale, tag=f"outer_linear residual={residual} b={b} N={N} [{gemm_mode}]")


# ---------------------------------------------------------------------------------------------------
# D. TriangleAttention: TriAttnFn (the forward's og / lse handed to the backward), the fp32 core past v2's N <= 384, and the
#    HipOp recompute past training.TRI_ATTN_BWD_MAX_N
# ---------------------------------------------------------------------------------------------------

TA_NAMES = ["attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight", "attn.gate_proj.weight", "attn.gate_proj.bias",
            "attn.out_proj.weight", "attn.out_proj.bias"]


def tri_attn_case(P, b, N, ending):
    def make():
        H, c = 4, 16
        g = torch.Generator().manual_seed(6000 + N + b)
        pair = randn(g, b, N, N, P)
        mask = ragged_mask(b, N)
        shapes = [(64, P), (64, P), (64, P), (64, P), (64,), (P, 64), (P,)]
        wts = [randn(g, *s, scale=1 / math.sqrt(s[-1]) if len(s) == 2 else 0.25) for s in shapes]
        dy = randn(g, b, N, N, P)
        leaves = [t.double().requires_grad_(True) for t in (pair, *wts)]
        m2 = (mask.unsqueeze(-1) * mask.unsqueeze(-2)).double()
        out = O.triangle_attention({"ta." + n: w for n, w in zip(TA_NAMES, leaves[1:])}, "ta", leaves[0], m2, H, c, ending)
        want = [x.detach() for x in torch.autograd.grad(out, leaves, dy.double())]
        del out, leaves
        return pair, mask, wts, dy, want
    return cached(("tri_attn", P, b, N, ending), make)


@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("P,b,N", [(64, 2, 320), (64, 1, 384), (64, 1, 400), (64, 1, 416), (64, 1, 417)])
def test_tri_attn_backward(P, b, N, mode, residual, scale, gemm_mode):
    """N <= 384: the v2 backward core in split-16 mode; 400, 416: the fp32 core (v2 holds rows up to 384); 417: past
    training.TRI_ATTN_BWD_MAX_N, training.tri_attn_update's recompute through torch_ref (HipOp)."""
    ending = mode == "ending"
    pair, mask, wts, dy0, want = tri_attn_case(P, b, N, ending)
    leaves = [t.clone().requires_grad_(True) for t in (pair, *wts)]
    if N > training.TRI_ATTN_BWD_MAX_N:
        ta = SimpleNamespace(attn=SimpleNamespace(num_heads=4, head_dim=16, weights=lambda: leaves[1:]), mode=mode)
        out = training.tri_attn_update(ta, leaves[0], mask, residual=residual)
    else:
        out = training.TriAttnFn.apply(leaves[0], mask, ending, 4, 16, residual, *leaves[1:])
    got = torch.autograd.grad(out, leaves, dy0 * scale)
    if residual:
        want = [want[0] + dy0.double(), *want[1:]]
    check_grads(["pair", *TA_NAMES], got, want, scale, tag=f"tri_attn {mode} residual={residual} b={b} N={N} [{gemm_mode}]")


# ---------------------------------------------------------------------------------------------------
# E. the other pair-track backwards at b = 2, N = 320, P = 64
# ---------------------------------------------------------------------------------------------------

E_B, E_N, E_P = 2, 320, 64


@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("residual", [False, True])
def test_pair_transition_backward(residual, scale, gemm_mode):
    def make():
        g = torch.Generator().manual_seed(5001)
        HID = 4 * E_P
        w = [randn(g, HID, E_P, scale=1 / math.sqrt(E_P)), randn(g, HID, scale=0.25), randn(g, E_P, HID, scale=1 / math.sqrt(HID)),
             randn(g, E_P, scale=0.25)]
        x = randn(g, E_B, E_N, E_N, E_P)
        # The ReLU has no derivative at 0: a hidden unit whose pre-activation lies within rounding of 0 takes the other branch in
        # fp32 than in the float64 reference (one unit at 7e-8 of the rms put its 64 x 64 block at 1e-4).  Such rows are drawn again.
        for _ in range(8):
            pre = O.ln(x.double()) @ w[0].double().t() + w[1].double()
            near = (pre.abs() < 1e-5 * pre.std()).any(-1)
            del pre
            if not near.any():
                break
            x[near] = randn(g, int(near.sum()), E_P)
        assert not near.any()
        dy = randn(g, E_B, E_N, E_N, E_P)
        leaves = [t.double().requires_grad_(True) for t in (x, *w)]
        p = dict(zip(["pf.1.weight", "pf.1.bias", "pf.3.weight", "pf.3.bias"], leaves[1:]))
        want = [t.detach() for t in torch.autograd.grad(O.transition(p, "pf", leaves[0]), leaves, dy.double())]
        return x, w, dy, want
    x, w, dy0, want = cached(("pair_transition",), make)
    leaves = [t.clone().requires_grad_(True) for t in (x, *w)]
    out = training.PairTransitionFn.apply(*leaves, residual)
    got = torch.autograd.grad(out, leaves, dy0 * scale)
    if residual:
        want = [want[0] + dy0.double(), *want[1:]]
    check_grads(["pair", "w1", "b1", "w2", "b2"], got, want, scale, tag=f"pair_transition residual={residual} [{gemm_mode}]")


@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("form", ["folding_block", "spa_affine"])
def test_pair_bias_backward(form, scale, gemm_mode):
    """The folding block's attention bias (H = 4, bias c) and SPAttention's affine-LayerNorm pair bias (H = 8, no c)."""
    affine = form == "spa_affine"
    H = 8 if affine else 4

    def make():
        g = torch.Generator().manual_seed(5100 + H)
        pair = randn(g, E_B, E_N, E_N, E_P, scale=1.7) + 0.3
        w = randn(g, H, E_P, scale=1 / 8)
        extra = [1 + randn(g, E_P, scale=0.2), randn(g, E_P, scale=0.1)] if affine else [randn(g, H)]
        dy = randn(g, E_B, H, E_N, E_N)
        leaves = [t.double().requires_grad_(True) for t in (pair, w, *extra)]
        if affine:
            bias = F_linear_bias(O.ln(leaves[0], leaves[2], leaves[3]), leaves[1], None)
        else:
            bias = O.pair_bias({"ab.1.weight": leaves[1], "ab.1.bias": leaves[2]}, "ab", leaves[0])
        want = [t.detach() for t in torch.autograd.grad(bias, leaves, dy.double())]
        return pair, w, extra, dy, want
    pair, w, extra, dy0, want = cached(("pair_bias", form), make)
    leaves = [t.clone().requires_grad_(True) for t in (pair, w, *extra)]
    if affine:
        out = training.PairBiasFn.apply(leaves[0], leaves[1], None, leaves[2], leaves[3])
        names = ["pair", "weight", "gamma", "beta"]
    else:
        out = training.PairBiasFn.apply(leaves[0], leaves[1], leaves[2])
        names = ["pair", "weight", "bias"]
    got = torch.autograd.grad(out, leaves, dy0 * scale)
    check_grads(names, got, want, scale, tag=f"pair_bias {form} [{gemm_mode}]")


def F_linear_bias(x, w, c):
    """bias[b, h, i, j] = (x W^T + c)[b, i, j, h]"""
    return torch.nn.functional.linear(x, w, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize("scale", [1.0, 1e-6])
def test_coordinate_head_backward(scale, gemm_mode):
    """HeadsFn's hand-written coordinate-head backward (gradient of the noise prediction with respect to the pair and the three
    weight_radial tensors) against float64 autograd of O.heads on the symmetrised pair."""
    S = 64

    def make():
        g = torch.Generator().manual_seed(5200)
        pair = randn(g, E_B, E_N, E_N, E_P)
        single = randn(g, E_B, E_N, S)
        z = randn(g, E_B, E_N, 3, scale=3.0)
        mask = ragged_mask(E_B, E_N)
        w = [randn(g, E_P, E_P, scale=1 / math.sqrt(E_P)), randn(g, E_P, scale=0.25), randn(g, 1, E_P, scale=1 / math.sqrt(E_P)),
             randn(g, S, S, scale=1 / math.sqrt(S)), randn(g, S, scale=0.25), randn(g, 21, S, scale=1 / math.sqrt(S))]
        deps = randn(g, E_B, E_N, 3)
        leaves = [t.double().requires_grad_(True) for t in (pair, *w[:3])]
        p = {"weight_radial.1.weight": leaves[1], "weight_radial.1.bias": leaves[2], "weight_radial.3.weight": leaves[3],
             "seq_mlp.1.weight": w[3].double(), "seq_mlp.1.bias": w[4].double(), "seq_mlp.3.weight": w[5].double()}
        m = mask.double()
        z64 = z.double()
        zij = z64.unsqueeze(-2) - z64.unsqueeze(-3)
        psym = 0.5 * (leaves[0] + leaves[0].transpose(1, 2))
        eps, _ = O.heads(p, single.double(), psym, zij, m.unsqueeze(-1) * m.unsqueeze(-2), m)
        want = [t.detach() for t in torch.autograd.grad(eps, leaves, deps.double())]
        return pair, single, z, mask, w, deps, want
    pair, single, z, mask, w, deps0, want = cached(("heads",), make)

    def heads_hip(s_, p_, *w_):                     # as training.network runs the heads
        eps_raw = ops.coord_head(p_.contiguous(), z.contiguous(), mask, w_[0], w_[1], w_[2])
        eps = ops.remove_mean(eps_raw, mask)
        h = ops.linear(s_.contiguous(), w_[3], w_[4], act=1, ln_a=True)
        return eps, ops.linear(h, w_[5])

    leaves = [t.clone().requires_grad_(True) for t in (pair, *w[:3])]
    eps, _ = training.HeadsFn.apply(heads_hip, z, mask, single, leaves[0], *leaves[1:], *w[3:])
    got = torch.autograd.grad(eps, leaves, deps0 * scale)
    check_grads(["pair", "weight_radial.1.weight", "weight_radial.1.bias", "weight_radial.3.weight"], got, want, scale,
                tag=f"heads [{gemm_mode}]")
