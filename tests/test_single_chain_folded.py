"""The single track of a folding block with the attention's output projection folded into the transition's first layer
(FoldingBlock.single_track_, prd_single_fc1_folded) against a float64 evaluation of the UNFOLDED formulas (modules.py:185-225,
306-311; torch_ref in float64), on every element of every output: single, the outer-linear term u, the next block's q|k|v|gate or
the tail ReLU layer.

Tolerance: none invented.  The separate-launch path (PRD_FOLD_OUT_PROJ=0, what the tree ran before the fold) is measured against
the same float64 reference on the same inputs in the same test, and the folded path must stay within 2x of that error in both
relative L2 and max |error| / rms -- 2x because the reassociation (W1 Wo formed once, og split next to single) changes which products
round together.  Where the fold does not apply (fp32 arithmetic, fewer than 96 or more than 640 rows) both paths are the same launches and the
figures coincide.

Measured on MI355X, split-16 arithmetic, separate -> folded (every case and output: profiles/r07_fold_errors.txt):
    N=320 b=1  single  rel-L2 1.121e-07 -> 1.142e-07   max/rms 6.468e-07 -> 7.509e-07
               u       rel-L2 1.901e-07 -> 1.913e-07   max/rms 9.711e-07 -> 9.283e-07
               qkvg    rel-L2 1.787e-07 -> 1.795e-07   max/rms 1.109e-06 -> 1.135e-06
               tail    rel-L2 1.886e-07 -> 1.905e-07   max/rms 1.234e-06 -> 1.269e-06
    N=320 b=2 masked   single 1.116e-07 -> 1.144e-07 (max 6.174e-07 -> 6.669e-07), u 2.074e-07 -> 2.084e-07 (1.038e-06 -> 1.052e-06)
    N=110 b=3 masked   single 1.138e-07 -> 1.156e-07 (max 5.922e-07 -> 5.926e-07), u 1.925e-07 -> 1.927e-07 (8.609e-07 -> 9.088e-07)
    N=64  b=2          single 1.144e-07 -> 1.166e-07 (max 5.250e-07 -> 5.947e-07), u 1.936e-07 -> 1.922e-07 (8.305e-07 -> 7.909e-07)
worst ratio over all cases and outputs: rel-L2 1.03x, max/rms 1.25x (u at N=320 b=2: 1.038e-06 -> 1.294e-06).  fp32 arithmetic,
N = 33 and (N = 64, b = 1) run the separate launches in both arms (identical figures, 1.3e-07 .. 2.6e-07).
"""
import math

import pytest
import torch

from protein_redesign_amd import ops, torch_ref as TR, trunk

S, P, H, C, TF = 512, 64, 4, 16, 4


def make_block(seed, device="cpu"):
    """A FoldingBlock whose single-track parameters are all non-trivial (the 'final' / 'gating' initialisers are zeros)."""
    blk = trunk.FoldingBlock(S, P, C, H, TF)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if not name.startswith(("single_attn", "single_fc", "outer_linear")):
                continue
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1]))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    return blk.to(device).eval()


# ---------------------------------------------------------------------------------------------------
# pack-time products (CPU)
# ---------------------------------------------------------------------------------------------------

def test_packed_products_match_float64():
    blk = make_block(1)
    sa, fc = blk.single_attn, blk.single_fc
    wo, bo, w1 = sa.out_proj.weight, sa.out_proj.bias, fc[1].weight
    w1cat, woT, wsum1, w1bo = ops.pack_fc1_fold(wo, bo, w1)
    assert w1cat.shape == (S * TF, S + H * C) and w1cat.dtype == torch.float32
    assert torch.equal(w1cat[:, :S], w1.detach())
    assert torch.equal(woT, wo.detach().t())
    prod = w1.detach().double() @ wo.detach().double()
    # rounded ONCE from the float64 product: half an ulp of fp32 per element (2^-24 relative), not the ~sqrt(512) ulps of an fp32 GEMM
    err = (w1cat[:, S:].double() - prod).abs()
    assert bool((err <= prod.abs() * 2.0 ** -24 + 1e-45).all()), float((err / prod.abs().clamp_min(1e-30)).max())
    for got, want in ((wsum1, w1.detach().double().sum(1)), (w1bo, w1.detach().double() @ bo.detach().double())):
        e = (got.double() - want).abs()
        assert bool((e <= want.abs() * 2.0 ** -24 + 1e-45).all())


def test_pack_is_rebuilt_when_any_source_changes_in_place():
    blk = make_block(2)
    sa, fc = blk.single_attn, blk.single_fc
    srcs = (sa.out_proj.weight, sa.out_proj.bias, fc[1].weight)
    calls = []

    def get():
        return ops.cached_pack(blk, "fc1_fold", srcs, lambda: calls.append(1) or ops.pack_fc1_fold(*srcs))
    first = get()
    assert get() is first and len(calls) == 1
    for k, p in enumerate(srcs):
        with torch.no_grad():
            p.mul_(1.5)
        again = get()
        assert len(calls) == 2 + k, f"source {k} changed in place without a rebuild"
        want = ops.pack_fc1_fold(*srcs)
        assert all(torch.equal(a, w) for a, w in zip(again, want))


# ---------------------------------------------------------------------------------------------------
# the chain on the GPU
# ---------------------------------------------------------------------------------------------------

def reference(blk, nxt, tail, single, mask, bias):
    """float64, unfolded: out-projection as its own linear, then the transition, then the consumers of LN(single_out)."""
    d = lambda t: t.detach().double()
    sa, fc = blk.single_attn, blk.single_fc
    single, mask, bias = d(single), d(mask), d(bias)
    wq, wk, wv, wg, bg, wo, bo = [d(w) for w in sa.weights()]
    s1 = single + TR.gated_attention(single, mask, wq, wk, wv, wg, bg, wo, bo, H, C, bias=bias)
    s2 = s1 + TR.transition(s1, d(fc[1].weight), d(fc[1].bias), d(fc[3].weight), d(fc[3].bias))
    x = TR.ln(s2)
    out = {"single": s2, "u": x @ d(blk.outer_linear.linear.weight)[:, S:].t()}
    if nxt is not None:
        nq, nk, nv, ng, nbg = [d(w) for w in nxt.single_attn.weights()[:5]]
        out["qkvg"] = torch.cat([(x @ nq.t()) / math.sqrt(C), x @ nk.t(), x @ nv.t(), torch.sigmoid(x @ ng.t() + nbg)], dim=-1)
    else:
        out["tail"] = torch.relu(x @ d(tail[0]).t() + d(tail[1]))
    return out


def run_chain(blk, nxt, tail, single, mask, bias, fold, monkeypatch):
    monkeypatch.setattr(trunk, "_FOLD_OUT_PROJ", fold)
    extra = {}
    s, x, u = blk.single_track_(single.clone(), mask, bias, next_block=nxt, qkvg=None, tail=tail, extra=extra)
    torch.cuda.synchronize()
    out = {"single": s, "u": u}
    out.update(extra)
    return out


def errors(got, want):
    d = (got.double() - want).abs()
    return float(d.pow(2).sum().sqrt() / want.norm()), float(d.max() / want.pow(2).mean().sqrt())


CASES = [(N, b, False, "next") for N in (320, 33, 64) for b in (1, 2)] + [(320, 2, True, "next"), (320, 1, False, "tail"), (64, 2, True, "tail"),
                                                                               (110, 3, True, "next"), (50, 2, False, "tail")]   # M = 330, 100: ragged row tiles


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split16", "fp32"])
@pytest.mark.parametrize("N,b,masked,variant", CASES)
def test_folded_chain_within_2x_of_separate_launches(N, b, masked, variant, mode, monkeypatch):
    from protein_redesign_amd import _lib
    L = _lib.lib()
    prev = L.prd_get_gemm_mode()
    assert L.prd_set_gemm_mode(1 if mode == "split16" else 0) == 0
    try:
        dev = "cuda"
        blk, nxt = make_block(11, dev), make_block(12, dev)
        g = torch.Generator().manual_seed(1000 + 7 * N + b)
        single = (torch.randn(b, N, S, generator=g) * 1.5 + 0.5 * torch.randn(b, N, 1, generator=g)).to(dev)
        bias = torch.randn(b, H, N, N, generator=g).to(dev)
        mask = torch.ones(b, N)
        if masked:
            mask[b - 1, N - max(1, N // 9):] = 0.0          # a padded tail in the last batch entry
        mask = mask.to(dev)
        tail = None
        if variant == "tail":
            tail = ((torch.randn(S, S, generator=g) / math.sqrt(S)).to(dev), (0.1 * torch.randn(S, generator=g)).to(dev))
            nxt = None
        with torch.no_grad():
            want = reference(blk, nxt, tail, single, mask, bias)
            sep = run_chain(blk, nxt, tail, single, mask, bias, False, monkeypatch)
            fold = run_chain(blk, nxt, tail, single, mask, bias, True, monkeypatch)
        folded_here = mode == "split16" and ops.fc1_fold_ok(b * N, S, H * C, S * TF)
        assert folded_here == (mode == "split16" and 96 <= b * N <= 640)
        assert set(fold) == set(want) == set(sep)
        fails = []
        for name in sorted(want):
            assert fold[name].shape == want[name].shape and bool(torch.isfinite(fold[name]).all())
            (l2_s, mx_s), (l2_f, mx_f) = errors(sep[name], want[name]), errors(fold[name], want[name])
            print(f"FOLD N={N} b={b} masked={int(masked)} {variant} {mode} folded={int(folded_here)} {name}: "
                  f"rel-L2 {l2_s:.3e} -> {l2_f:.3e}   max/rms {mx_s:.3e} -> {mx_f:.3e}")
            if not (l2_f <= 2.0 * l2_s and mx_f <= 2.0 * mx_s):
                fails.append((name, l2_s, l2_f, mx_s, mx_f))
        assert not fails, fails
    finally:
        assert L.prd_set_gemm_mode(prev) == 0


@pytest.mark.gpu
def test_changed_weight_reaches_the_folded_launch(monkeypatch):
    """out_proj's bias and weight change in place between two calls: the second call must compute with the new values."""
    dev = "cuda"
    blk, nxt = make_block(21, dev), make_block(22, dev)
    g = torch.Generator().manual_seed(5)
    b, N = 1, 320
    single, bias, mask = torch.randn(b, N, S, generator=g).to(dev), torch.randn(b, H, N, N, generator=g).to(dev), torch.ones(b, N, device=dev)
    assert ops.fc1_fold_ok(b * N, S, H * C, S * TF)
    with torch.no_grad():
        first = run_chain(blk, nxt, None, single, mask, bias, True, monkeypatch)
        blk.single_attn.out_proj.bias.add_(0.5)
        blk.single_attn.out_proj.weight.mul_(-2.0)
        want = reference(blk, nxt, None, single, mask, bias)
        second = run_chain(blk, nxt, None, single, mask, bias, True, monkeypatch)
        sep = run_chain(blk, nxt, None, single, mask, bias, False, monkeypatch)
    assert errors(first["single"], want["single"])[0] > 1e-2          # the change is visible at all
    for name in want:
        (l2_f, mx_f), (l2_s, mx_s) = errors(second[name], want[name]), errors(sep[name], want[name])
        assert l2_f <= 2.0 * l2_s and mx_f <= 2.0 * mx_s, (name, l2_s, l2_f, mx_s, mx_f)
