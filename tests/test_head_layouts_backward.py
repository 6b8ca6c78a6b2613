"""GPU: the general triangle-attention backward core (prd_tri_attn_bwd_core_heads, csrc/prd_tri_heads_bwd.hip) through
ops.tri_attn_backward / training.TriAttnFn, for every head layout the forward serves and rows of any length.

Bars and method are those of section D of test_backward_training_shapes.py, restated here: every returned gradient to rel-L2 <
OP_TOL and the pair gradient's worst 64 x 64 block of positions to BLOCK_TOL, against float64 autograd of
prd_oracle.triangle_attention evaluated on the device.  Gradients are linear in ``dy`` and fp32 MFMA has no operand range, so the
same bar holds at dy x 1 and dy x 1e-6.  The float64 references are cached across the arithmetic modes and scales (about 3 GB)."""
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
GRAD_TOL = 1e-4         # whole-model gradients (test_head_layouts.py)
LAYOUTS = [(1, 32), (2, 32), (8, 8), (8, 32), (4, 64), (3, 20), (5, 12), (4, 16)]
TA_NAMES = ["attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight", "attn.gate_proj.weight", "attn.gate_proj.bias",
            "attn.out_proj.weight", "attn.out_proj.bias"]


@pytest.fixture(params=["fp32", "split16"])
def gemm_mode(request):
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(_lib.GEMM_MODES[request.param]) == 0
    yield request.param
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


@pytest.fixture
def general_core_for_4x16(monkeypatch):
    """4 x 16 keeps its tuned cores up to 416 positions; with their limit at 0 ops.tri_attn_backward hands 4 x 16 to the general core."""
    monkeypatch.setattr(ops, "TRI_ATTN_BWD_TUNED_MAX_N", 0)


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
    """Largest ||got - want|| / ||want|| over the 64 x 64 blocks of pair positions (i, j) of a [b, R, N, C] gradient (R = N, or a
    subset of rows).  A block whose reference is tiny against the average block (exact zeros of masked positions) is measured
    against 1e-3 of that average."""
    b, R, N = want.shape[:3]
    TR, T = (R + blk - 1) // blk, (N + blk - 1) // blk
    d = torch.zeros(b, TR * blk, T * blk, device=want.device, dtype=torch.float64)
    w = torch.zeros_like(d)
    d[:, :R, :N] = (got.double() - want.double()).pow(2).flatten(3).sum(-1)
    w[:, :R, :N] = want.double().pow(2).flatten(3).sum(-1)
    e = d.view(b, TR, blk, T, blk).sum(dim=(2, 4)).sqrt()
    r = w.view(b, TR, blk, T, blk).sum(dim=(2, 4)).sqrt()
    floor = 1e-3 * float(r.mean())
    worst = e / r.clamp_min(floor)
    k = int(worst.argmax())
    return float(worst.max()), (k // (TR * T), (k // T) % TR * blk, k % T * blk)


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


def make_weights(g, H, c, P):
    HC = H * c
    shapes = [(HC, P), (HC, P), (HC, P), (HC, P), (HC,), (P, HC), (P,)]
    return [randn(g, *s, scale=1 / math.sqrt(s[-1]) if len(s) == 2 else 0.25) for s in shapes]


def float64_grads(pair, mask, wts, dy, H, c, ending):
    leaves = [t.double().requires_grad_(True) for t in (pair, *wts)]
    m2 = (mask.unsqueeze(-1) * mask.unsqueeze(-2)).double()
    out = O.triangle_attention({"ta." + n: w for n, w in zip(TA_NAMES, leaves[1:])}, "ta", leaves[0], m2, H, c, ending)
    want = [x.detach() for x in torch.autograd.grad(out, leaves, dy.double())]
    del out, leaves
    return want


def tri_attn_case(H, c, P, b, N, ending, mask=None, dy_fn=None, tag="std"):
    def make():
        g = torch.Generator().manual_seed(9000 + 131 * H + 7 * c + N + b + P)
        pair = randn(g, b, N, N, P)
        m = ragged_mask(b, N) if mask is None else mask.to(DEV)
        wts = make_weights(g, H, c, P)
        dy = randn(g, b, N, N, P)
        if dy_fn is not None:
            dy = dy_fn(dy)
        return pair, m, wts, dy, float64_grads(pair, m, wts, dy, H, c, ending)
    return cached((tag, H, c, P, b, N, ending), make)


def fn_grads(H, c, pair, mask, wts, dy, mode, residual):
    """Through training.tri_attn_update -> TriAttnFn (forward keeps og and, for the general layouts, the statistics)."""
    leaves = [t.clone().requires_grad_(True) for t in (pair, *wts)]
    ta = SimpleNamespace(attn=SimpleNamespace(num_heads=H, head_dim=c, weights=lambda: leaves[1:]), mode=mode)
    out = training.tri_attn_update(ta, leaves[0], mask, residual=residual)
    return list(torch.autograd.grad(out, leaves, dy))


# ---------------------------------------------------------------------------------------------------
# 1. the core against float64
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("P,b,N", [(32, 2, 30), (64, 2, 30), (32, 2, 97), (64, 2, 97), (32, 1, 320), (64, 1, 320)])
@pytest.mark.parametrize("H,c", LAYOUTS)
def test_core_vs_float64(H, c, P, b, N, mode, residual, scale, gemm_mode, general_core_for_4x16):
    """Every layout through TriAttnFn (kept og and statistics); 4 x 16 through ops.tri_attn_backward with the tuned cores' limit at 0:
    its forward recompute is the tuned core without statistics, i.e. the lse == NULL form of the new entry.  (8, 32): 4 H c = 1024 is
    beyond prd_pair_linear, so the projections' activation-gradient GEMM goes through ops.linear."""
    ending = mode == "ending"
    pair, mask, wts, dy0, want = tri_attn_case(H, c, P, b, N, ending)
    if (H, c) == (8, 32) and N >= 97:
        assert ops.pair_linear(torch.zeros(8192, 4 * H * c, device=DEV), torch.cat(wts[:4]).t()) is None
    if (H, c) == (4, 16):
        dpair, grads = ops.tri_attn_backward(dy0 * scale, pair, mask, wts, H, c, ending=ending, residual=residual)
        got = [dpair, *grads]
    else:
        got = fn_grads(H, c, pair, mask, wts, dy0 * scale, mode, residual)
    if residual:
        want = [want[0] + dy0.double(), *want[1:]]
    check_grads(["pair", *TA_NAMES], got, want, scale, tag=f"tri_attn ({H}, {c}) {mode} residual={residual} P={P} b={b} N={N} [{gemm_mode}]")


# ---------------------------------------------------------------------------------------------------
# 2. rows of any length: a row subset against the float64 attention of those rows
# ---------------------------------------------------------------------------------------------------

def long_row_case(H, c, N, ending):
    def make():
        P = 64
        g = torch.Generator().manual_seed(500 + N + H + ending)
        pair = randn(g, 1, N, N, P)
        mask = torch.ones(1, N)
        valid = N - 17
        mask[0, valid:] = 0
        mask = mask.to(DEV)
        rows = sorted({0, 63, 64, 256, N // 2, valid - 1, valid, N - 1} | set(torch.randint(0, N, (8,), generator=g).tolist()))
        wts = make_weights(g, H, c, P)
        dy = torch.zeros(1, N, N, P, device=DEV)
        dr = randn(g, 1, len(rows), N, P)
        if ending:
            dy[:, :, rows] = dr.transpose(1, 2)
        else:
            dy[:, rows] = dr
        leaves = [t.double().requires_grad_(True) for t in (pair, *wts)]
        src = leaves[0].transpose(1, 2) if ending else leaves[0]
        m2 = (mask.unsqueeze(-1) * mask.unsqueeze(-2)).double()
        p = {"ta." + n: w for n, w in zip(TA_NAMES, leaves[1:])}
        out = O.gated_attention(p, "ta.attn", src[:, rows], m2[:, rows], H, c)
        want = [x.detach() for x in torch.autograd.grad(out, leaves, dr.double())]
        del out, leaves
        return pair, mask, wts, dy, want, rows
    return cached(("long", H, c, N, ending), make)


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("N", [449, 769])
@pytest.mark.parametrize("H,c", [(8, 32), (4, 16)])
def test_long_rows(H, c, N, mode, gemm_mode):
    """(8, 32) keeps the statistics of its forward; 4 x 16 beyond 416 positions runs the tuned long-row forward, which keeps none:
    the lse == NULL form (the path that recomputed through torch before).  dy is zero outside 16 rows (first, last valid, masked,
    scattered), so whole-tensor float64 autograd (29 GB per saved tensor at 769) is replaced by the attention of those rows."""
    ending = mode == "ending"
    pair, mask, wts, dy, want, rows = long_row_case(H, c, N, ending)
    assert N > training.TRI_ATTN_BWD_MAX_N
    got = fn_grads(H, c, pair, mask, wts, dy, mode, False)
    sel = (lambda t: t.transpose(1, 2)[:, rows]) if ending else (lambda t: t[:, rows])
    other = torch.ones(N, dtype=torch.bool, device=DEV)
    other[rows] = False
    assert float(sel_other(got[0], other, ending).abs().max()) == 0.0            # rows without dy receive exactly nothing
    check_grads(["pair", *TA_NAMES], [sel(got[0]), *got[1:]], [sel(want[0]), *want[1:]], 1.0,
                tag=f"tri_attn long rows ({H}, {c}) {mode} N={N} [{gemm_mode}]")


def sel_other(t, other, ending):
    return t.transpose(1, 2)[:, other] if ending else t[:, other]


# ---------------------------------------------------------------------------------------------------
# 3. edge rows
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("H,c", [(8, 32), (3, 20), (4, 16)])
def test_edge_rows(H, c, mode, gemm_mode, general_core_for_4x16):
    """b = 2, N = 97: complex 0 has an interior masked position (its row: every key masked) and a masked tail; complex 1 has ONE valid
    position (every valid row has one valid key)."""
    P, b, N = 64, 2, 97
    mask = torch.ones(b, N)
    mask[0, 31] = 0
    mask[0, N - 9:] = 0
    mask[1, :] = 0
    mask[1, 5] = 1
    ending = mode == "ending"
    pair, m, wts, dy0, want = tri_attn_case(H, c, P, b, N, ending, mask=mask, tag="edge")
    if (H, c) == (4, 16):
        dpair, grads = ops.tri_attn_backward(dy0, pair, m, wts, H, c, ending=ending)
        got = [dpair, *grads]
    else:
        got = fn_grads(H, c, pair, m, wts, dy0, mode, False)
    check_grads(["pair", *TA_NAMES], got, want, 1.0, tag=f"tri_attn edge rows ({H}, {c}) {mode} [{gemm_mode}]")


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("H,c", [(8, 32), (4, 16)])
def test_single_position_dy_and_zero_dy(H, c, mode, gemm_mode, general_core_for_4x16):
    P, b, N = 64, 2, 97
    ending = mode == "ending"

    def one(dy):
        z = torch.zeros_like(dy)
        z[1, 40, 17] = dy[1, 40, 17]
        return z
    pair, m, wts, dy0, want = tri_attn_case(H, c, P, b, N, ending, dy_fn=one, tag="one")

    def run(dy):
        if (H, c) == (4, 16):
            dpair, grads = ops.tri_attn_backward(dy, pair, m, wts, H, c, ending=ending)
            return [dpair, *grads]
        return fn_grads(H, c, pair, m, wts, dy, mode, False)
    # the out-projection bias gradient is dy's column sum; every other gradient is compared as usual
    check_grads(["pair", *TA_NAMES], run(dy0), want, 1.0, tag=f"tri_attn one-position dy ({H}, {c}) {mode} [{gemm_mode}]")
    for gz in run(torch.zeros_like(dy0)):
        assert bool((gz == 0).all())


# ---------------------------------------------------------------------------------------------------
# 4. the statistics of the forward
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("H,c,P,N", [(8, 32, 64, 97), (3, 20, 32, 97), (4, 16, 64, 320), (5, 12, 64, 30)])
def test_forward_statistics(H, c, P, N, mode):
    b = 2 if N < 320 else 1
    ending = mode == "ending"
    g = torch.Generator().manual_seed(77 + H + N)
    pair = randn(g, b, N, N, P)
    mask = ragged_mask(b, N)
    mask[0, N // 3] = 0                          # a fully masked row
    wts = make_weights(g, H, c, P)
    og0 = ops.tri_attn_core_heads(pair, mask, wts[:5], H, c, ending=ending).clone()
    lse = torch.full((b * N, H, N, 2), float("nan"), device=DEV)
    og1 = ops.tri_attn_core_heads(pair, mask, wts[:5], H, c, ending=ending, lse=lse)
    assert torch.equal(og0, og1)
    assert torch.isfinite(lse).all()
    x = O.ln((pair.transpose(1, 2) if ending else pair).double())
    q = (x @ wts[0].double().t()).view(b, N, N, H, c).transpose(2, 3) / math.sqrt(c)
    k = (x @ wts[1].double().t()).view(b, N, N, H, c).transpose(2, 3)
    logits = q @ k.transpose(-1, -2)                                            # [b, row, H, query, key]
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)                                # [b, row, key]
    logits = logits.masked_fill(m2[:, :, None, None, :] < 0.5, -(2.0 ** 15))
    want = torch.logsumexp(logits, dim=-1) * math.log2(math.e)
    got = (lse[..., 0].double() + lse[..., 1].double()).view(b, N, H, N)
    err = rel(got, want)
    print(f"\nm + log2 l ({H}, {c}) P={P} N={N} {mode}: rel-L2 {err:.1e}")
    assert err < OP_TOL


@pytest.mark.parametrize("kept", [True, False])
@pytest.mark.parametrize("H,c,P,b,N,mode", [(8, 32, 64, 2, 97, "starting"), (3, 20, 32, 2, 30, "ending"), (2, 32, 64, 1, 320, "ending")])
def test_kept_and_recomputed_statistics(H, c, P, b, N, mode, kept, gemm_mode):
    """The backward with the forward's statistics and with lse == NULL, at the bars of (1); the first case has a fully masked row."""
    ending = mode == "ending"
    if N == 97:
        mask = ragged_mask(b, N).cpu()
        mask[0, 31] = 0
        pair, m, wts, dy0, want = tri_attn_case(H, c, P, b, N, ending, mask=mask, tag="stats")
    else:
        pair, m, wts, dy0, want = tri_attn_case(H, c, P, b, N, ending)
    lse = torch.empty(b * N, H, N, 2, device=DEV) if kept else None
    og = ops.tri_attn_core_heads(pair, m, wts[:5], H, c, ending=ending, lse=lse)
    dpair, grads = ops.tri_attn_backward(dy0, pair, m, wts, H, c, ending=ending, og=og, lse=lse)
    check_grads(["pair", *TA_NAMES], [dpair, *grads], want, 1.0, tag=f"tri_attn ({H}, {c}) {mode} N={N} kept={kept} [{gemm_mode}]")


# ---------------------------------------------------------------------------------------------------
# 5. reproducibility
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kept", [True, False])
@pytest.mark.parametrize("H,c,P,b,N", [(8, 32, 64, 2, 97), (5, 12, 32, 2, 30), (4, 16, 64, 1, 449)])
def test_core_is_reproducible_and_writes_everything(H, c, P, b, N, kept):
    g = torch.Generator().manual_seed(31 + N)
    pair = randn(g, b, N, N, P)
    mask = ragged_mask(b, N)
    mask[0, N // 2] = 0
    wts = make_weights(g, H, c, P)
    dog = randn(g, b, N, N, H * c)
    lse = torch.empty(b * N, H, N, 2, device=DEV) if kept else None
    og = ops.tri_attn_core_heads(pair, mask, wts[:5], H, c, ending=True, lse=lse).clone()
    nws = int(_lib.lib().prd_tri_attn_bwd_heads_workspace_bytes(b, N, P, H, c)) // 4
    outs = []
    for _ in range(2):
        dqkvg = torch.full((b, N, N, 4, H * c), float("nan"), device=DEV)
        x = torch.full_like(pair, float("nan"))
        ws = torch.full((nws,), float("nan"), device=DEV)
        ops.tri_attn_bwd_core_heads(dog, og, pair, mask, wts[:5], H, c, ending=True, lse=lse, x_out=x, dqkvg=dqkvg, ws=ws)
        assert torch.isfinite(dqkvg).all() and torch.isfinite(x).all()
        outs.append((dqkvg, x))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert rel(outs[0][1], O.ln(pair.double())) < OP_TOL


# ---------------------------------------------------------------------------------------------------
# 6. the memory claim
# ---------------------------------------------------------------------------------------------------

def test_training_backward_memory_is_below_one_logits_tensor():
    """training.tri_attn_update at (8, 8), P = 64, N = 320, b = 1, forward + autograd.grad: the peak above the inputs stays below
    b H N^3 * 4 B = 1.05 GB, the size of ONE logits tensor -- a bound the recompute through autograd cannot meet (it keeps the
    probabilities of every row chunk), derived, not measured.  By the list of ops.tri_attn_backward's allocations (og, dog, out, dxn,
    dpair, x: 64 floats per position each; dqkvg: 256; lse: 16; the workspace: 22 MB) the hand-written path comes to ~0.3 GB; measured on an MI355X: 0.282 GB."""
    H, c, P, b, N = 8, 8, 64, 1, 320
    g = torch.Generator().manual_seed(3)
    pair = randn(g, b, N, N, P)
    mask = ragged_mask(b, N)
    wts = make_weights(g, H, c, P)
    dy = randn(g, b, N, N, P)
    leaves = [t.clone().requires_grad_(True) for t in (pair, *wts)]
    ta = SimpleNamespace(attn=SimpleNamespace(num_heads=H, head_dim=c, weights=lambda: leaves[1:]), mode="starting")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = training.tri_attn_update(ta, leaves[0], mask, residual=False)
    grads = torch.autograd.grad(out, leaves, dy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    bound = b * H * N ** 3 * 4
    print(f"\ntri_attn_update (8, 8) N=320 forward + backward: peak {peak / 1e9:.3f} GB above the inputs, bound {bound / 1e9:.3f} GB")
    assert all(torch.isfinite(x).all() for x in grads)
    assert peak < bound


# ---------------------------------------------------------------------------------------------------
# 7. the whole model
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("process_mode,train_variant", [("fp32", "plain"), ("split16", "plain"), ("fp32", "checkpoint"),
                                                        ("split16", "checkpoint"), ("split16", "fp32_pinned")])
@pytest.mark.parametrize("H,c", [(8, 32), (2, 32)])
def test_training_step_gradients_vs_oracle(H, c, process_mode, train_variant, monkeypatch, golden):
    """training_step gradients of an (8, 32) and a (2, 32) model against the oracle's autograd at GRAD_TOL, on the inputs of the
    "heads" fixture as test_head_layouts.py does ((2, 32): the same case with its attention layout changed); also with per-block
    checkpointing (og = None in the backward: the forward recompute with statistics) and with the model pinned to fp32 under a
    split-16 process default."""
    from test_training_cpu import case_inputs, oracle_grads
    from protein_redesign_amd.diffusion_model import ProteinReDiffModel
    from protein_redesign_amd.synthetic import batch_to, deterministic_state_dict
    from protein_redesign_amd.weights import spec_tensors
    monkeypatch.setattr(_lib.lib(), "_mode", _lib.GEMM_MODES[process_mode])
    if train_variant == "checkpoint":
        monkeypatch.setattr(training, "USE_CHECKPOINT", True)
    case, z, args, params, pb = case_inputs(golden, "heads")
    if (H, c) != (args["num_heads"], args["head_dim"]):
        args = dict(args, num_heads=H, head_dim=c)
        params = deterministic_state_dict(spec_tensors(args), seed=case["weight_seed"], style=case.get("weight_style", "random"),
                                          scales=case.get("weight_scales"))
    t = torch.from_numpy(z["train_t"])
    nz, ns = torch.from_numpy(z["train_noise_z"]), torch.from_numpy(z["train_noise_seq"])
    want_loss, want = cached(("model", H, c), lambda: oracle_grads(args, params, pb, t, nz, ns))
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    model = model.to(DEV).train()
    model.run_setup_schedule()
    model.setup_schedule = True
    if train_variant == "fp32_pinned":
        model.arithmetic = "fp32"
    dpb = batch_to(pb, DEV)
    mask = dpb["residue_and_atom_mask"]
    diff = model.diffusion_loss(dpb, dpb["x"], mask, t.to(DEV), nz.to(DEV), ns.to(DEV))
    loss = torch.mean(diff / (mask > 0.5).sum(-1))
    loss.backward()
    assert abs(float(loss) - want_loss) < GRAD_TOL * abs(want_loss)
    got = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    scale = math.sqrt(sum(float(w.double().norm()) ** 2 for w in want.values()))
    for k, gk in got.items():
        assert gk is not None, k
        err = float((gk.detach().cpu().double().reshape(-1) - want[k].double().reshape(-1)).norm())
        ref = float(want[k].double().norm())
        assert err < GRAD_TOL * ref + 1e-6 * scale, (k, err, ref)


# ---------------------------------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------------------------------

def _raw_call(L, dqkvg, dog, og, pair, mask, w, lse, x, b, N, P, H, c, ws, ws_bytes):
    p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    return L.prd_tri_attn_bwd_core_heads(p(dqkvg), p(dog), p(og), p(pair), p(mask), *[p(w)] * 5, p(lse), p(x), 0, b, N, P, H, c,
                                         p(ws), ws_bytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("H,c,P", [(9, 16, 64), (4, 18, 64), (4, 128, 64), (2, 32, 48)])
def test_c_entry_refuses_unsupported_without_launching(H, c, P):
    L = _lib.lib()
    b, N = 1, 8
    HC = H * c
    pair = torch.randn(b, N, N, P, device=DEV)
    mask = torch.ones(b, N, device=DEV)
    w = torch.randn(HC * P, device=DEV)
    dog = torch.randn(b, N, N, HC, device=DEV)
    dqkvg = torch.full((b, N, N, 4, HC), 7.0, device=DEV)
    x = torch.full((b, N, N, P), 7.0, device=DEV)
    ws = torch.full((1 << 18,), 7.0, device=DEV)
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, w, None, x, b, N, P, H, c, ws, ws.numel() * 4) == -3        # PRD_ERR_UNSUPPORTED
    assert L.prd_tri_attn_bwd_heads_workspace_bytes(b, N, P, H, c) == 0
    torch.cuda.synchronize()
    assert bool((dqkvg == 7.0).all()) and bool((x == 7.0).all()) and bool((ws == 7.0).all())


def test_c_entry_refuses_bad_arguments_without_launching():
    L = _lib.lib()
    b, N, P, H, c = 1, 8, 64, 8, 32
    HC = H * c
    pair = torch.randn(b, N, N, P, device=DEV)
    mask = torch.ones(b, N, device=DEV)
    w = torch.randn(HC * P, device=DEV)
    dog = torch.randn(b, N, N, HC, device=DEV)
    buf = torch.full((b * N * N * 4 * HC + 4,), 7.0, device=DEV)
    dqkvg = buf[:-4]
    x = torch.full((b, N, N, P), 7.0, device=DEV)
    need = int(L.prd_tri_attn_bwd_heads_workspace_bytes(b, N, P, H, c))
    assert need > 0
    ws = torch.full((need // 4,), 7.0, device=DEV)
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, w, None, x, b, N, P, H, c, ws, need - 4) == -4              # PRD_ERR_WORKSPACE
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, w, None, x, b, N, P, H, c, None, need) == -1                # PRD_ERR_ARG
    assert _raw_call(L, None, dog, dog, pair, mask, w, None, x, b, N, P, H, c, ws, need) == -1
    assert _raw_call(L, dqkvg, None, dog, pair, mask, w, None, x, b, N, P, H, c, ws, need) == -1
    assert _raw_call(L, dqkvg, dog, None, pair, mask, w, None, x, b, N, P, H, c, ws, need) == -1
    assert _raw_call(L, dqkvg, dog, dog, pair, None, w, None, x, b, N, P, H, c, ws, need) == -1
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, None, None, x, b, N, P, H, c, ws, need) == -1
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, w, None, x, 0, N, P, H, c, ws, need) == -1
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, w, None, x, b, 0, P, H, c, ws, need) == -1
    assert _raw_call(L, buf.data_ptr() + 4, dog, dog, pair, mask, w, None, x, b, N, P, H, c, ws, need) == -2     # PRD_ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()) and bool((x == 7.0).all()) and bool((ws == 7.0).all())
    # and the same arguments are accepted once they are right (lse and x_out may be NULL)
    assert _raw_call(L, dqkvg, dog, dog, pair, mask, w, None, None, b, N, P, H, c, ws, need) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dqkvg).all() and not bool((dqkvg == 7.0).all())
