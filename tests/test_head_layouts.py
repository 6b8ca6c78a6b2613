"""GPU: attention head layouts other than 4 heads x 16 channels (``--num_heads`` / ``--head_dim`` of the reference, model.py:146-147).

The general triangle-attention core (prd_tri_attn_core_heads, csrc/prd_tri_heads.hip) + its output projection against the oracle for
a spread of (H, c) -- widths padded inside the kernel (c = 12, 20), H*c from 32 to 256 -- both orientations, pair_dim 32 / 64, rows
with a masked tail and fully masked rows, rows far beyond any LDS row limit; the same kernel at 4 x 16 against the tuned cores; whole
network steps against the oracle; a network step, a hipGraph-replayed trajectory and a training step against fixtures captured from
the imported reference with --num_heads 8 --head_dim 32 (tests/golden/heads.npz, tools/gen_golden_heads.py); and the refusals."""
import json

import numpy as np
import pytest
import torch

import prd_oracle as O
from conftest import mismatch_report, rel_l2
from protein_redesign_amd import _lib, ops, training
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.diffusion_model import ProteinReDiffModel
from protein_redesign_amd.synthetic import NoiseSource, batch_to, deterministic_state_dict, synthetic_batch
from protein_redesign_amd.weights import spec_tensors

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOISE_SEED = 7
OP_TOL, BLOCK_TOL, TRAJ_TOL, GRAD_TOL = 1e-5, 2e-5, 1e-4, 1e-4
PFX = "blk.pair_attn"
LAYOUTS = [(1, 32), (2, 32), (8, 8), (8, 32), (4, 64), (3, 20), (5, 12)]


@pytest.fixture(params=["fp32", "split16"])
def gemm_mode(request):
    """Both arithmetic modes (the core runs fp32 MFMA in both; the output projection and the rest of the network do not)."""
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(1 if request.param == "split16" else 0) == 0
    yield request.param
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


def cu(x):
    return x.to(DEV).contiguous()


def attn_params(H, c, P, seed):
    g = torch.Generator().manual_seed(seed)
    HC = H * c
    p = {f"{PFX}.attn.q_proj.weight": torch.randn(HC, P, generator=g) / P ** 0.5,
         f"{PFX}.attn.k_proj.weight": torch.randn(HC, P, generator=g) / P ** 0.5,
         f"{PFX}.attn.v_proj.weight": torch.randn(HC, P, generator=g) / P ** 0.5,
         f"{PFX}.attn.gate_proj.weight": torch.randn(HC, P, generator=g) / P ** 0.5,
         f"{PFX}.attn.gate_proj.bias": torch.randn(HC, generator=g),
         f"{PFX}.attn.out_proj.weight": torch.randn(P, HC, generator=g) / HC ** 0.5,
         f"{PFX}.attn.out_proj.bias": torch.randn(P, generator=g)}
    names = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "gate_proj.weight", "gate_proj.bias", "out_proj.weight", "out_proj.bias")
    return p, [cu(p[f"{PFX}.attn.{n}"]) for n in names]


def inputs(b, N, P, seed):
    """pair, and a node mask with a masked tail and one masked interior position (their rows have every key masked)."""
    g = torch.Generator().manual_seed(seed)
    pair = torch.randn(b, N, N, P, generator=g)
    mask = torch.ones(b, N)
    mask[0, N - max(1, N // 10):] = 0
    mask[0, N // 3] = 0
    if b > 1:
        mask[1, N - 3:] = 0
    return pair, mask


_WANT = {}


def oracle_attention(p, pair, mask, H, c, ending, key):
    """O.triangle_attention, cached across the two arithmetic modes (the oracle does not depend on them)."""
    if key not in _WANT:
        m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
        with torch.inference_mode():
            _WANT[key] = O.triangle_attention(p, PFX, pair, m2, H, c, ending)
    return _WANT[key]


# ---------------------------------------------------------------------------------------------------
# 1-3: the operator
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [30, 97, 320])
@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("H,c", LAYOUTS)
def test_operator_vs_oracle(H, c, P, mode, N, gemm_mode):
    assert ops.tri_attn_heads_supported(N, P, H, c)
    b = 2 if N < 320 else 1
    p, w = attn_params(H, c, P, seed=100 * H + c + P)
    pair, mask = inputs(b, N, P, seed=N + P)
    ending = mode == "ending"
    want = oracle_attention(p, pair, mask, H, c, ending, (H, c, P, mode, N))

    def evaluate():
        return ops.tri_attn(cu(pair), cu(mask), w, H, c, ending=ending, residual=False).cpu()
    got = evaluate()
    assert rel_l2(got, want) < OP_TOL, mismatch_report(got, want, evaluate)
    # every row on its own, the fully masked ones included
    rows = got.transpose(1, 2) if ending else got
    wrows = want.transpose(1, 2) if ending else want
    row_err = (rows - wrows).flatten(2).norm(dim=2) / wrows.flatten(2).norm(dim=2).clamp_min(1e-30)
    assert float(row_err.max()) < 4 * OP_TOL, int(row_err.argmax())


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("P", [32, 64])
def test_residual_form(P, mode, gemm_mode):
    """residual=True, in place (out = pair): pair + update."""
    H, c, N = 8, 32, 61
    p, w = attn_params(H, c, P, seed=7)
    pair, mask = inputs(1, N, P, seed=8)
    want = pair + oracle_attention(p, pair, mask, H, c, mode == "ending", (H, c, P, mode, N, "res"))
    d = cu(pair)
    ops.tri_attn(d, cu(mask), w, H, c, ending=mode == "ending", residual=True, out=d)
    assert rel_l2(d.cpu(), want) < OP_TOL


@pytest.mark.parametrize("N", [30, 97, 320])
@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("P", [32, 64])
def test_general_core_at_4x16(P, mode, N, gemm_mode):
    """The general kernel also serves 4 x 16 (the model keeps the tuned kernels there): same contract as ops.tri_attn_core."""
    H, c = 4, 16
    p, w = attn_params(H, c, P, seed=41 + P)
    pair, mask = inputs(2, N, P, seed=3 * N + P)
    ending = mode == "ending"
    dp, dm = cu(pair), cu(mask)
    og = ops.tri_attn_core_heads(dp, dm, w[:5], H, c, ending=ending)
    og_tuned = ops.tri_attn_core(dp, dm, w[:5], H, c, ending=ending)
    assert og.shape == og_tuned.shape == (2, N, N, 64)
    assert rel_l2(og.cpu(), og_tuned.cpu()) < OP_TOL
    got = ops.linear(og, w[5], w[6]).cpu()
    want = oracle_attention(p, pair, mask, H, c, ending, (H, c, P, mode, N, "4x16"))
    assert rel_l2(got, want) < OP_TOL


@pytest.mark.parametrize("mode", ["starting", "ending"])
@pytest.mark.parametrize("N", [449, 769, 1100])
def test_long_rows(N, mode, gemm_mode):
    """(8, 32), P = 64: rows the LDS could never hold (keys stream through it in chunks of 64 with an online softmax).  N = 449:
    the whole tensor; 769 and 1100: a subset of rows (first, last valid, masked, scattered) -- row i of the update depends on row
    i of the (transposed) pair only.  At 1100, b N N H c = 3.1e8 floats: 64-bit offsets."""
    H, c, P = 8, 32, 64
    p, w = attn_params(H, c, P, seed=N)
    g = torch.Generator().manual_seed(N + (mode == "ending"))
    pair = torch.randn(1, N, N, P, generator=g)
    mask = torch.ones(1, N)
    valid = N - 17
    mask[0, valid:] = 0
    ending = mode == "ending"
    got = ops.tri_attn(cu(pair), cu(mask), w, H, c, ending=ending, residual=False).cpu()
    if ending:
        got = got.transpose(1, 2)
    src = pair.transpose(1, 2) if ending else pair
    m2 = mask.unsqueeze(-1) * mask.unsqueeze(-2)
    if N == 449:
        rows = list(range(N))
    else:
        rows = sorted({0, 1, 63, 64, 255, 256, N // 2, valid - 1, valid, N - 1} | set(torch.randint(0, N, (6,), generator=g).tolist()))
    want = torch.empty(1, len(rows), N, P)
    with torch.inference_mode():
        for r0 in range(0, len(rows), 32):
            rr = rows[r0:r0 + 32]
            want[:, r0:r0 + len(rr)] = O.gated_attention(p, PFX + ".attn", src[:, rr].contiguous(), m2[:, rr].contiguous(), H, c)
    sub = got[:, rows]
    assert rel_l2(sub, want) < OP_TOL
    row_err = (sub - want).flatten(2).norm(dim=2) / want.flatten(2).norm(dim=2).clamp_min(1e-30)
    assert float(row_err.max()) < 4 * OP_TOL, rows[int(row_err.argmax())]


# ---------------------------------------------------------------------------------------------------
# 4: whole network steps against the oracle
# ---------------------------------------------------------------------------------------------------

def build_model(args, seed, style="random"):
    params = deterministic_state_dict(spec_tensors(args), seed=seed, style=style)
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    return model.to(DEV).eval(), params


_STEP_WANT = {}


def network_step_case(args, sizes, n_total, seed):
    model, params = build_model(args, seed)
    batch = synthetic_batch(sizes, esm_dim=args["esm_dim"], seed=seed + 1, n_total=n_total)
    perms = [NoiseSource(NOISE_SEED, 100 + k).randperm(n) for k, (_, n) in enumerate(sizes)]
    pb = O.prepare_batch(batch, args["mask_prob"], perms)
    b, N = pb["atom_mask"].shape
    g = torch.Generator().manual_seed(seed + 2)
    z, seq_t = torch.randn(b, N, 3, generator=g), torch.randn(b, N, 21, generator=g)
    t = torch.tensor([5, 2][:b])
    key = json.dumps([args, sizes, n_total, seed], sort_keys=True)
    if key not in _STEP_WANT:
        with torch.inference_mode():
            _STEP_WANT[key] = O.network_step(params, args, pb, z, seq_t, pb["residue_and_atom_mask"], t)
    d = batch_to(pb, DEV)
    with torch.inference_mode():
        got = model.sample_step(d, cu(z), cu(seq_t), d["residue_and_atom_mask"], cu(t))
    torch.cuda.synchronize()
    return got, _STEP_WANT[key]


@pytest.mark.parametrize("P", [32, 64])
@pytest.mark.parametrize("H,c", [(8, 32), (4, 8), (2, 32)])
def test_network_step_vs_oracle(H, c, P, gemm_mode):
    """(2, 32): H c = 64 with c != 16 -- the ending attention's projection rides in the fused block tail; (4, 8): H c = 32 --
    output projection, pair transition and the next block's bias heads as separate launches."""
    args = make_args(single_dim=64, pair_dim=P, head_dim=c, num_heads=H, num_blocks=2, esm_dim=32, num_steps=8, mask_prob=0.3)
    got, want = network_step_case(args, [(6, 30), (3, 22)], 40, seed=H * 100 + c + P)
    for a, b_ in zip(got, want):
        assert rel_l2(a.cpu(), b_) < BLOCK_TOL * 2


def test_network_step_full_width(gemm_mode):
    """N = 320, single_dim 512, pair_dim 64, (8, 32), 4 blocks."""
    args = make_args(single_dim=512, pair_dim=64, head_dim=32, num_heads=8, num_blocks=4, esm_dim=64, num_steps=8, mask_prob=0.3)
    got, want = network_step_case(args, [(20, 300)], None, seed=3)
    assert got[0].shape[1] == 320
    for a, b_ in zip(got, want):
        assert rel_l2(a.cpu(), b_) < BLOCK_TOL * 2


# ---------------------------------------------------------------------------------------------------
# 5-6: against the imported reference (--num_heads 8 --head_dim 32)
# ---------------------------------------------------------------------------------------------------

def golden_model(golden):
    case, z = golden("heads")
    args = make_args(**case["args"])
    assert (args["num_heads"], args["head_dim"]) == (8, 32)
    model, params = build_model(args, case["weight_seed"], case.get("weight_style", "random"))
    return case, z, args, model, params


def test_network_step_vs_reference_golden(golden, gemm_mode):
    case, z, args, model, params = golden_model(golden)
    sizes = [tuple(s) for s in case["sizes"]]
    batch = synthetic_batch(sizes, esm_dim=args["esm_dim"], seed=case["batch_seed"], n_total=case["n_total"])
    perms = [NoiseSource(NOISE_SEED, 100 + k).randperm(n) for k, (_, n) in enumerate(sizes)]
    pb = batch_to(O.prepare_batch(batch, args["mask_prob"], perms), DEV)
    with torch.inference_mode():
        eps, logits = model.sample_step(pb, cu(torch.from_numpy(z["step_z"])), cu(torch.from_numpy(z["step_seq_t"])),
                                        pb["residue_and_atom_mask"], cu(torch.from_numpy(z["step_t"])))
    assert rel_l2(eps.cpu(), z["step_noise_pred"]) < BLOCK_TOL * 2
    assert rel_l2(logits.cpu(), z["step_seq_pred"]) < BLOCK_TOL * 2


def test_trajectory_vs_reference_golden(golden, gemm_mode):
    """sample(): first step eager, the rest one captured hipGraph replayed, T = 8."""
    case, z, args, model, params = golden_model(golden)
    assert model.use_hip_graph
    one = batch_to(synthetic_batch([tuple(case["traj_sample"])], esm_dim=args["esm_dim"], seed=case["batch_seed"] + 500), DEV)
    pos, logits = model.sample(one, sources=[NoiseSource(NOISE_SEED, 0)])
    assert rel_l2(pos.cpu(), z["traj_pos"]) < TRAJ_TOL
    assert rel_l2(logits.cpu(), z["traj_logits"]) < TRAJ_TOL


def test_training_step_gradients_vs_reference_and_oracle(golden, gemm_mode):
    from test_training_cpu import FINGERPRINT_TOL, GRAD_PROJECTIONS, case_inputs, oracle_grads
    case, z, args, params, pb = case_inputs(golden, "heads")
    t = torch.from_numpy(z["train_t"])
    nz, ns = torch.from_numpy(z["train_noise_z"]), torch.from_numpy(z["train_noise_seq"])
    want_loss, want = oracle_grads(args, params, pb, t, nz, ns)
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    model = model.to(DEV).train()
    model.run_setup_schedule()
    model.setup_schedule = True
    dpb = batch_to(pb, DEV)
    mask = dpb["residue_and_atom_mask"]
    diff = model.diffusion_loss(dpb, dpb["x"], mask, t.to(DEV), nz.to(DEV), ns.to(DEV))
    loss = torch.mean(diff / (mask > 0.5).sum(-1))
    loss.backward()
    assert abs(float(loss) - float(z["train_loss"])) < GRAD_TOL * abs(float(z["train_loss"]))
    assert abs(float(loss) - want_loss) < GRAD_TOL * abs(want_loss)
    got = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    names = json.loads(str(z["train_grad_names"]))
    assert sorted(got) == sorted(names) and all(g is not None for g in got.values())
    scale = float(np.linalg.norm(z["train_grad_norm"]))
    for i, k in enumerate(names):
        g = got[k].detach().cpu().double().reshape(-1)
        err = float((g - want[k].double().reshape(-1)).norm())
        ref = float(want[k].double().norm())
        assert err < GRAD_TOL * ref + 1e-6 * scale, (k, err, ref)
        n_ref = float(z["train_grad_norm"][i])
        assert abs(float(g.norm()) - n_ref) < FINGERPRINT_TOL * n_ref + 1e-6 * scale, (k, float(g.norm()), n_ref)
        for j in range(GRAD_PROJECTIONS):
            gen = torch.Generator().manual_seed(4242 + 16 * i + j)
            proj = float(torch.dot(g, torch.randn(g.numel(), generator=gen, dtype=torch.float64)))
            assert abs(proj - float(z["train_grad_proj"][i, j])) < FINGERPRINT_TOL * n_ref + 1e-6 * scale, (k, j)


def test_training_step_and_optimizer_step():
    """training_step + the optimiser step (Adam + LinearLR + EMA) end to end for an (8, 32) model: finite loss, parameters move."""
    args = make_args(single_dim=64, pair_dim=64, head_dim=32, num_heads=8, num_blocks=2, esm_dim=16, num_steps=50, mask_prob=0.3,
                     learning_rate=1e-3, warmup_steps=2)
    params = deterministic_state_dict(spec_tensors(args), seed=5, style="near_init")
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    model = model.to(DEV).train()
    model.run_setup_schedule()
    model.setup_schedule = True
    cfg = model.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    batch = batch_to(synthetic_batch([(4, 18), (3, 14)], esm_dim=16, seed=6, n_total=24), DEV)
    w0 = model.Denoiser.folding_blocks[0].pair_attn_starting.attn.q_proj.weight.detach().clone()
    losses = []
    for step in range(2):
        losses.append(float(training.fit_step(model, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}, step,
                                              opt, sched, sources=[NoiseSource(1, k) for k in range(2)])))
    assert all(np.isfinite(losses))
    assert not torch.equal(model.Denoiser.folding_blocks[0].pair_attn_starting.attn.q_proj.weight.detach(), w0)


# ---------------------------------------------------------------------------------------------------
# 7: refusals
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,c", [(4, 18), (4, 128), (9, 16)])
def test_unsupported_layout_raises_with_the_supported_set(H, c):
    args = make_args(single_dim=64, pair_dim=64, head_dim=c, num_heads=H, num_blocks=1, esm_dim=16, num_steps=4, mask_prob=0.3)
    model, _ = build_model(args, seed=1)
    batch = batch_to(synthetic_batch([(3, 12)], esm_dim=16, seed=2), DEV)
    pb = model.prepare_batch(batch, sources=[NoiseSource(1, 0)])
    N = pb["atom_mask"].shape[1]
    z, seq_t = torch.zeros(1, N, 3, device=DEV), torch.zeros(1, N, 21, device=DEV)
    with pytest.raises(ValueError, match=r"num_heads 1\.\.8, head_dim a multiple of 4 up to 64, pair_dim 32/64"):
        with torch.inference_mode():
            model.sample_step(pb, z, seq_t, pb["residue_and_atom_mask"], torch.tensor([1], device=DEV))
    with pytest.raises(ValueError, match=r"num_heads 1\.\.8"):
        model.sample(batch_to(synthetic_batch([(3, 12)], esm_dim=16, seed=2), DEV), sources=[NoiseSource(1, 0)])


@pytest.mark.parametrize("H,c,P", [(9, 16, 64), (4, 18, 64), (4, 128, 64), (4, 0, 64), (2, 32, 48)])
def test_c_entry_refuses_without_launching(H, c, P):
    L = _lib.lib()
    b, N = 1, 8
    pair = torch.randn(b, N, N, P, device=DEV)
    mask = torch.ones(b, N, device=DEV)
    w = torch.randn(max(1, H * c) * P, device=DEV)
    og = torch.full((b * N * N * max(1, H * c),), 7.0, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    torch.cuda.synchronize()
    code = L.prd_tri_attn_core_heads(og.data_ptr(), pair.data_ptr(), mask.data_ptr(), *[w.data_ptr()] * 5, 0, b, N, P, H, c,
                                     ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    assert code == -3                                   # PRD_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((og == 7.0).all())
    # and the other refusals: short workspace, NULL pointer, empty shapes
    ok = (8, 32, 64)
    H, c, P = ok
    pair = torch.randn(b, N, N, P, device=DEV)
    w = torch.randn(H * c * P, device=DEV)
    og = torch.full((b * N * N * H * c,), 7.0, device=DEV)
    need = int(L.prd_tri_attn_heads_workspace_bytes(b, N, P, H, c))
    st = torch.cuda.current_stream().cuda_stream
    args = (og.data_ptr(), pair.data_ptr(), mask.data_ptr(), *[w.data_ptr()] * 5, 0)
    assert L.prd_tri_attn_core_heads(*args, b, N, P, H, c, ws.data_ptr(), need - 4, st) == -4
    assert L.prd_tri_attn_core_heads(*args, b, N, P, H, c, None, need, st) == -1
    assert L.prd_tri_attn_core_heads(*args, 0, N, P, H, c, ws.data_ptr(), need, st) == -1
    assert L.prd_tri_attn_core_heads(*args, b, 0, P, H, c, ws.data_ptr(), need, st) == -1
    torch.cuda.synchronize()
    assert bool((og == 7.0).all())
