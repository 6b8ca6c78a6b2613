"""GPU: a model whose weights CHANGED between calls computes with the new weights.

Every other GPU test builds a model, loads it once and uses it once.  The forward keeps derived copies of weights
(``ops.cached_pack``: qkvg, ab, bo_beta, head_proj, after_transition_next / _tail, fc1_fold / fc1_rowsum), so the optimisation loop
-- train, validate, sample, swap the EMA in and out, reload -- is correct only if every such copy follows every way the
parameters change.  The fused Adam of ``configure_optimizers`` changes them without moving ``p._version``.

Has the state gone stale?  A FRESH model loaded with a clone of M's current state_dict has never run and holds no pack; the
kernels are deterministic by construction, so M and the fresh model are compared with ``torch.equal``, after the control that two
fresh models of the same weights agree bit for bit.
Is it right at all?  The oracle at M's current weights, at the project's own bars: loss 1e-4 relative (GRAD_TOL), gradients
``err < GRAD_TOL * ref + 1e-6 * scale`` (test_training_gpu), a network step 2e-5 relative L2 (BLOCK_TOL, test_hip_parity).

Under the earlier cache key, (data_ptr, _version) alone, on MI355X: every scenario that trains with the fused Adam failed in both
arithmetic modes and both configurations (1, 2, 3, 4 and 7: the loss after ONE step 56.27 against a fresh model's 57.35 at
single_dim 512, samples after three steps 3e-3 .. 5e-2 in the positions and 0.17 .. 0.40 in the logits off a fresh model's);
reload (5), the arithmetic switch (6) and the update arithmetic (8) passed.  The gradient check of scenarios 1 and 7 then found the
split-16 fallback GEMMs of ``ops.tri_attn_backward`` below ``ops.WGRAD_MIN_ROWS`` rows ("Packed weights").
"""
import functools
import math
from types import SimpleNamespace

import pytest
import torch

import prd_oracle as O
from conftest import rel_l2
from protein_redesign_amd import _lib, ops, training
from protein_redesign_amd.constants import BOND_FEATURE_CARDS, make_args
from protein_redesign_amd.diffusion_model import ProteinReDiffModel
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch, deterministic_state_dict, synthetic_batch
from protein_redesign_amd.weights import spec_tensors
from test_hip_parity import BLOCK_TOL
from test_training_cpu import oracle_grads, oracle_training_loss
from test_training_gpu import GRAD_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
MASK_SEED, SAMPLE_SEED = 1, 2
COMMON = dict(esm_dim=16, num_steps=8, mask_prob=0.3, learning_rate=1e-3, warmup_steps=2)
CONFIGS = {
    # the batch of test_training_step_api_and_optimizer_step: b N = 48 rows, the transition's unfolded first layer (fc1_rowsum)
    "A": dict(args=dict(single_dim=64, pair_dim=32, num_blocks=2, **COMMON), sizes=[(4, 18), (3, 14)], n_total=24),
    # b N = 96 rows at single_dim 512: split-16 inference folds the attention's out-projection into the transition (fc1_fold)
    "B": dict(args=dict(single_dim=512, pair_dim=32, head_dim=16, num_heads=4, num_blocks=2, **COMMON), sizes=[(6, 40), (5, 31)], n_total=48),
}
ALWAYS_PACKED = {"qkvg", "ab", "bo_beta", "after_transition_next", "after_transition_tail", "head_proj"}


@pytest.fixture(params=["fp32", "split16"])
def gemm_mode(request):
    prev = _lib.lib().prd_get_gemm_mode()
    assert _lib.lib().prd_set_gemm_mode(_lib.GEMM_MODES[request.param]) == 0
    yield request.param
    assert _lib.lib().prd_set_gemm_mode(prev) == 0


@functools.lru_cache(maxsize=None)
def setup(cfg):
    """Fixed inputs of a configuration, built once and never written: weights, batch, the oracle's prepared batch, t, noises."""
    c = CONFIGS[cfg]
    args = make_args(**c["args"])
    params = deterministic_state_dict(spec_tensors(args), seed=5, style="near_init")
    other = deterministic_state_dict(spec_tensors(args), seed=6, style="near_init")
    batch = synthetic_batch(c["sizes"], esm_dim=args["esm_dim"], seed=6, n_total=c["n_total"])
    b, N = batch["atom_mask"].shape
    # synthetic_batch bonds 5 % of the atom pairs: among these few atoms none, and the bond tables would get a gradient of exactly
    # zero (Adam then leaves them where they are).  A chain of bonds along the ligand atoms, every feature class in turn.
    for k, (na, _) in enumerate(c["sizes"]):
        for i in range(na - 1):
            batch["bond_mask"][k, i, i + 1] = batch["bond_mask"][k, i + 1, i] = 1.0
            for f, card in enumerate(BOND_FEATURE_CARDS):
                batch["bond_feats"][k, i, i + 1, f] = batch["bond_feats"][k, i + 1, i, f] = (i + f) % card
    pb = O.prepare_batch(batch, args["mask_prob"], [NoiseSource(MASK_SEED, k).randperm(nr) for k, (_, nr) in enumerate(c["sizes"])])
    g = torch.Generator().manual_seed(3)
    nz = O.remove_mean(torch.randn(b, N, 3, generator=g), pb["residue_and_atom_mask"])
    ns = O.remove_mean(torch.randn(b, N, 21, generator=g), pb["residue_mask"])
    z = O.remove_mean(torch.randn(b, N, 3, generator=g), pb["residue_and_atom_mask"])
    seq_t = torch.randn(b, N, 21, generator=g)
    t = torch.tensor([5, 2])
    return SimpleNamespace(cfg=cfg, args=args, params=params, other=other, batch=batch, b=b, N=N, pb=pb, t=t, nz=nz, ns=ns, z=z, seq_t=seq_t,
                           dbatch=batch_to(batch, DEV), dpb=batch_to(pb, DEV), dt=t.to(DEV), dnz=nz.to(DEV), dns=ns.to(DEV))


def new_model(S, state, like=None):
    """A model that has never run: constructed, loaded with clones, moved to the GPU."""
    model = ProteinReDiffModel(S.args)
    model.load_state_dict({k: v.clone() for k, v in state.items()})
    model = model.to(DEV).train()
    model.run_setup_schedule()
    model.setup_schedule = True
    if like is not None:
        model.arithmetic, model.sample_seed = like.arithmetic, like.sample_seed
    return model


def snapshot(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def fresh_like(model, S):
    return new_model(S, snapshot(model), like=model)


def loss_of(model, S, grad=True):
    """training_step's loss on the fixed inputs; ``grad``: the training forward (training.network), else the no_grad one (validation)."""
    mask = S.dpb["residue_and_atom_mask"]
    with torch.enable_grad() if grad else torch.no_grad(), _lib.arithmetic(model.arithmetic):
        diff = model.diffusion_loss(dict(S.dpb), S.dpb["x"], mask, S.dt, S.dnz, S.dns)
        return torch.mean(diff / (mask > 0.5).sum(-1))


def sample_of(model, S):
    assert model.use_hip_graph
    pos, logits = model.sample(clone_batch(S.dbatch), sources=[NoiseSource(SAMPLE_SEED, k) for k in range(S.b)])
    return pos.clone(), logits.clone()


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def fit_steps(model, S, opt, sched, steps):
    for step in steps:
        training.fit_step(model, clone_batch(S.dbatch), step, opt, sched, t=S.dt, noise_z=S.dnz, noise_seq=S.dns,
                          sources=[NoiseSource(MASK_SEED, k) for k in range(S.b)])


def pack_names(model):
    return {name for m in model.modules() for name in m.__dict__.get("_prd_pack_cache", {})}


def warm(model, S, gemm_mode):
    """One training forward and one sampling loop: every pack the two paths use now exists (a vacuous pass is ruled out here)."""
    loss_of(model, S)
    out = sample_of(model, S)
    folded = S.cfg == "B" and gemm_mode == "split16"
    want = ALWAYS_PACKED | {"fc1_fold" if folded else "fc1_rowsum"}
    assert want <= pack_names(model), (sorted(want - pack_names(model)), sorted(pack_names(model)))
    return out


def assert_every_trainable_tensor_moved(model, S, since=None):
    since = S.params if since is None else since
    still = [k for k, p in model.named_parameters() if p.requires_grad and torch.equal(p.detach().cpu(), since[k])]
    assert not still, f"unchanged after the optimiser steps: {still}"


def check_loss(model, S, what):
    """M's loss == a fresh model's, bit for bit, in the training and in the no_grad forward; and == the oracle's at GRAD_TOL."""
    state = snapshot(model)
    fresh = new_model(S, state, like=model)
    lm, lf = loss_of(model, S), loss_of(fresh, S)
    assert torch.equal(lm.detach(), lf.detach()), f"{what}: training forward {float(lm):.9g}, a fresh model of the same weights {float(lf):.9g}"
    vm, vf = loss_of(model, S, grad=False), loss_of(fresh, S, grad=False)
    assert torch.equal(vm, vf), f"{what}: no_grad forward {float(vm):.9g}, a fresh model of the same weights {float(vf):.9g}"
    with torch.no_grad():
        want = float(oracle_training_loss(state, S.args, S.pb, S.t, S.nz, S.ns))
    print(f"{what}: loss {float(lm):.9g}, oracle {want:.9g}, rel {abs(float(lm) - want) / abs(want):.2e}")
    assert abs(float(lm) - want) < GRAD_TOL * abs(want), what
    assert abs(float(vm) - want) < GRAD_TOL * abs(want), what
    return lm, state


def check_grads(model, S, loss, state, what):
    model.zero_grad(set_to_none=True)
    loss.backward()
    _, want = oracle_grads(S.args, state, S.pb, S.t, S.nz, S.ns)
    got = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    assert sorted(got) == sorted(want) and all(g is not None for g in got.values())
    scale = float(torch.cat([g.reshape(-1) for g in want.values()]).double().norm())
    worst = 0.0
    for k in want:
        err = float((got[k].detach().cpu().double() - want[k].double()).norm())
        ref = float(want[k].double().norm())
        worst = max(worst, err / max(ref, 1e-3 * scale))
        assert err < GRAD_TOL * ref + 1e-6 * scale, (what, k, err, ref)
    print(f"{what}: {len(want)} gradients, worst rel-L2 vs oracle autograd {worst:.2e}")


def check_sample(model, fresh, S, what):
    got, want = sample_of(model, S), sample_of(fresh, S)
    assert all(bool(torch.isfinite(x).all()) for x in got)
    assert same(got, want), (f"{what}: positions rel-L2 {rel_l2(got[0].cpu(), want[0].cpu()):.3e}, logits rel-L2 "
                             f"{rel_l2(got[1].cpu(), want[1].cpu()):.3e} against a fresh model of the same weights")
    return got


def check_network_step(model, S, what):
    """One eager network step of M against the oracle at M's current weights."""
    state = snapshot(model)
    with torch.inference_mode():
        want = O.network_step(state, S.args, S.pb, S.z, S.seq_t, S.pb["residue_and_atom_mask"], S.t)
        with _lib.arithmetic(model.arithmetic):
            got = model.sample_step(S.dpb, S.z.to(DEV), S.seq_t.to(DEV), S.dpb["residue_and_atom_mask"], S.dt)
    errs = [rel_l2(g.cpu(), w) for g, w in zip(got, want)]
    print(f"{what}: network step vs oracle rel-L2 noise {errs[0]:.3e} logits {errs[1]:.3e}")
    assert errs[0] < BLOCK_TOL and errs[1] < BLOCK_TOL, (what, errs)


def control(S, state, fn):
    """Two fresh models of the same weights agree bit for bit on ``fn`` (a determinism finding if not; never a reason for a tolerance)."""
    a, b = fn(new_model(S, state), S), fn(new_model(S, state), S)
    a, b = (a, b) if isinstance(a, tuple) else ((a.detach(),), (b.detach(),))
    assert same(a, b), "control: two fresh models of the same weights differ"


def trained(S, gemm_mode, steps=3):
    """M warmed at the initial weights (every pack built from them), then ``steps`` optimisation steps through fit_step."""
    model = new_model(S, S.params)
    cfg = model.configure_optimizers()
    before = warm(model, S, gemm_mode)
    fit_steps(model, S, cfg["optimizer"], cfg["lr_scheduler"]["scheduler"], range(steps))
    assert_every_trainable_tensor_moved(model, S)
    return model, before


# ---------------------------------------------------------------------------------------------------
# 1. train -> train
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["A", "B"])
def test_train_then_train(cfg, gemm_mode):
    S = setup(cfg)
    control(S, S.params, loss_of)
    model = new_model(S, S.params)
    conf = model.configure_optimizers()
    warm(model, S, gemm_mode)
    first = float(loss_of(model, S).detach())
    for step in range(3):
        fit_steps(model, S, conf["optimizer"], conf["lr_scheduler"]["scheduler"], [step])
        loss, state = check_loss(model, S, f"{cfg} [{gemm_mode}] after optimisation step {step}")
    assert_every_trainable_tensor_moved(model, S)
    assert float(loss) != first
    if cfg == "A":
        check_grads(model, S, loss, state, f"{cfg} [{gemm_mode}] after 3 steps")


# ---------------------------------------------------------------------------------------------------
# 2. train -> sample      3. sample -> train -> sample
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["A", "B"])
def test_train_then_sample(cfg, gemm_mode):
    S = setup(cfg)
    control(S, S.params, sample_of)
    model, before = trained(S, gemm_mode)
    got = check_sample(model, fresh_like(model, S), S, f"{cfg} [{gemm_mode}] sample after 3 steps")
    assert not same(got, before)
    check_network_step(model, S, f"{cfg} [{gemm_mode}] after 3 steps")


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_sample_then_train_then_sample(cfg, gemm_mode):
    """M samples FIRST: every pack of the inference path is built under inference_mode and is an inference tensor; the training
    forward that follows must take or rebuild them without raising."""
    S = setup(cfg)
    control(S, S.params, sample_of)
    model = new_model(S, S.params)
    conf = model.configure_optimizers()
    before = sample_of(model, S)
    assert {"qkvg", "head_proj", "bo_beta"} <= pack_names(model)
    fit_steps(model, S, conf["optimizer"], conf["lr_scheduler"]["scheduler"], range(2))
    assert_every_trainable_tensor_moved(model, S)
    got = check_sample(model, fresh_like(model, S), S, f"{cfg} [{gemm_mode}] sample, 2 steps, sample")
    assert not same(got, before)
    check_loss(model, S, f"{cfg} [{gemm_mode}] sample, 2 steps, sample, loss")


# ---------------------------------------------------------------------------------------------------
# 4. EMA swap
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["A", "B"])
def test_ema_swap_in_and_out(cfg, gemm_mode):
    S = setup(cfg)
    control(S, S.params, sample_of)
    model, _ = trained(S, gemm_mode)
    model.sample_seed = 7
    live = snapshot(model)
    shadow = dict(live)
    for (k, _), s in zip(model.named_parameters(), model.ema.shadow):
        shadow[k] = s.detach().cpu().clone()
    assert any(not torch.equal(shadow[k], live[k]) for k in live)
    outside = check_sample(model, new_model(S, live, like=model), S, f"{cfg} [{gemm_mode}] before the swap")
    with model.ema.average_parameters(model.parameters()):
        inside = check_sample(model, new_model(S, shadow, like=model), S, f"{cfg} [{gemm_mode}] inside average_parameters")
    assert not same(inside, outside)
    again = check_sample(model, new_model(S, live, like=model), S, f"{cfg} [{gemm_mode}] after leaving average_parameters")
    assert same(again, outside)
    # predict_step swaps by itself
    got = model.predict_step(clone_batch(S.dbatch), 0)
    want = new_model(S, shadow, like=model).sample(clone_batch(S.dbatch), batch_idx=0)
    assert same(got, want), f"predict_step: positions rel-L2 {rel_l2(got[0].cpu(), want[0].cpu()):.3e} against the shadow-weights model"
    check_loss(model, S, f"{cfg} [{gemm_mode}] after predict_step")


# ---------------------------------------------------------------------------------------------------
# 5. reload into a warmed model      6. arithmetic switch on a warmed model
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", ["A", "B"])
def test_reload_into_a_warmed_model(cfg, gemm_mode):
    S = setup(cfg)
    control(S, S.other, sample_of)
    model = new_model(S, S.params)
    before = warm(model, S, gemm_mode)
    model.load_state_dict({k: v.clone() for k, v in S.other.items()})
    got = check_sample(model, new_model(S, S.other), S, f"{cfg} [{gemm_mode}] after load_state_dict")
    assert not same(got, before)
    check_loss(model, S, f"{cfg} [{gemm_mode}] after load_state_dict")


@pytest.mark.parametrize("cfg", ["A", "B"])
def test_arithmetic_switch_on_a_warmed_model(cfg):
    S = setup(cfg)

    def fp32_sample(model, S_):
        model.arithmetic = "fp32"
        return sample_of(model, S_)
    control(S, S.params, fp32_sample)
    model = new_model(S, S.params)
    model.arithmetic = "split16"
    warm(model, S, "split16")
    model.arithmetic = "fp32"
    fresh = new_model(S, S.params, like=model)
    check_sample(model, fresh, S, f"{cfg} split16 -> fp32")
    lm, lf = loss_of(model, S), loss_of(fresh, S)
    assert torch.equal(lm.detach(), lf.detach())


# ---------------------------------------------------------------------------------------------------
# 7. the optimiser stepped directly, outside Fitter
# ---------------------------------------------------------------------------------------------------

def test_optimizer_stepped_outside_fitter(gemm_mode):
    S = setup("A")
    control(S, S.params, loss_of)
    model = new_model(S, S.params)
    conf = model.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    before = warm(model, S, gemm_mode)
    first = float(loss_of(model, S).detach())
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        loss_of(model, S).backward()
        opt.step()
        sched.step()
        loss, state = check_loss(model, S, f"A [{gemm_mode}] direct optimiser step {step}")
    assert_every_trainable_tensor_moved(model, S)
    assert float(loss) != first
    check_grads(model, S, loss, state, f"A [{gemm_mode}] after 3 direct steps")
    got = check_sample(model, fresh_like(model, S), S, f"A [{gemm_mode}] sample after 3 direct steps")
    assert not same(got, before)


# ---------------------------------------------------------------------------------------------------
# 8. the update arithmetic, teacher-forced
# ---------------------------------------------------------------------------------------------------

def ulp32(x64):
    """The fp32 spacing at |x|, elementwise."""
    a = x64.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def test_update_arithmetic_teacher_forced(gemm_mode):
    """Adam + LinearLR + EMA as finish_accumulation applies them: from host copies of the parameters, gradients, Adam state and
    shadow taken just before the step, every parameter equals the float64 Adam update and every shadow tensor the float64 EMA
    update, element by element.  Bound: 4 fp32 ulps of the largest operand (a handful of fp32 roundings, half an ulp each), plus for
    the parameters 1e-5 * lr: the Adam quotient m^ / (sqrt(v^) + eps) is at most ~1 in magnitude and is formed from a few fp32
    operations (relative 6e-8 each), times lr.  Derived, not measured."""
    S = setup("A")
    model = new_model(S, S.params)
    conf = model.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    fitter = training.Fitter(model, opt, sched, accumulate_grad_batches=2)
    b1, b2 = opt.defaults["betas"]
    eps, base = opt.defaults["eps"], S.args["learning_rate"]
    assert opt.defaults["weight_decay"] == 0 and not opt.defaults["amsgrad"] and opt.defaults["fused"]
    start, iters = 1.0 / S.args["warmup_steps"], S.args["warmup_steps"] - 1
    d64 = lambda x: x.detach().cpu().double().clone()
    params = list(model.parameters())
    for step in range(3):
        fitter.step(clone_batch(S.dbatch), 2 * step, t=S.dt, noise_z=S.dnz, noise_seq=S.dns,
                    sources=[NoiseSource(MASK_SEED, k) for k in range(S.b)])
        assert fitter.micro == 1 and fitter.optimizer_steps == step
        old = [d64(p) for p in params]
        grads = [None if p.grad is None else d64(p.grad) for p in params]
        states = [{k: d64(v) for k, v in opt.state[p].items()} if p in opt.state and opt.state[p] else None for p in params]
        shadow = [d64(s) for s in model.ema.shadow]
        n = model.ema.num_updates + 1
        fitter.finish_accumulation()
        lr = base * (start + (1.0 - start) * min(step, iters) / iters)
        decay = min(S.args["ema_decay"], (1 + n) / (10 + n))
        worst_p = worst_s = 0.0
        for (name, p), p0, g, st, s0, s in zip(model.named_parameters(), old, grads, states, shadow, model.ema.shadow):
            p1, s1 = d64(p), d64(s)
            if not p.requires_grad:
                assert g is None and torch.equal(p1, p0) and torch.equal(s1, s0), name
                continue
            assert (st is None) == (step == 0)
            m0, v0, k = (st["exp_avg"], st["exp_avg_sq"], float(st["step"])) if st else (torch.zeros_like(g), torch.zeros_like(g), 0.0)
            assert k == step
            m = b1 * m0 + (1 - b1) * g
            v = b2 * v0 + (1 - b2) * g * g
            want = p0 - lr / (1 - b1 ** (k + 1)) * m / (v.sqrt() / math.sqrt(1 - b2 ** (k + 1)) + eps)
            tol = 4 * ulp32(torch.maximum(torch.maximum(p0.abs(), p1.abs()), want.abs())) + 1e-5 * lr
            over = ((p1 - want).abs() / tol).max()
            worst_p = max(worst_p, float(over))
            assert over <= 1.0, (name, step, "Adam", float(over))
            want_s = s0 - (1.0 - decay) * (s0 - p1)
            tol_s = 4 * ulp32(torch.maximum(torch.maximum(s0.abs(), p1.abs()), want_s.abs()))
            over = ((s1 - want_s).abs() / tol_s).max()
            worst_s = max(worst_s, float(over))
            assert over <= 1.0, (name, step, "EMA", float(over))
        print(f"step {step}: lr {lr:.3e}, EMA decay {decay:.4f}; worst error / bound: Adam {worst_p:.3f}, EMA {worst_s:.3f}")
        assert abs(opt.param_groups[0]["lr"] - base * (start + (1.0 - start) * min(step + 1, iters) / iters)) < 1e-12 * base
    assert model.ema.num_updates == 3 and fitter.optimizer_steps == 3
