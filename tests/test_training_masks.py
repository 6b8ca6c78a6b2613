"""GPU: the training-mode masks (reference model.py:442-458, mask_utils.py) selected on the device.

1. prd_mask_lowest_k against the reference's fixtures (tests/golden/training_masks.npz, exact) and against its torch restatement
   (masking.restate_lowest_k, exact) on seeded inputs: row lengths at and across the LDS tile, ties, bit-reproducibility, and
   outputs that come back fully written.
2. ``training_step`` with ``training_mode=True`` and injected draws: the loss against the imported reference's, loss and every
   gradient against the oracle's autograd -- with the tolerances tests/test_training_gpu.py applies to the eval branch.
3. ``sample()`` with ``training_mode=True`` against the oracle's loop on the same masks, at the trajectory tolerance.
4. The training-mode ``prepare_batch`` performs no host synchronisation.
"""
import numpy as np
import pytest
import torch

import prd_oracle as O
from conftest import rel_l2
from no_host_sync import run_without_host_sync
from protein_redesign_amd import masking, ops
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.diffusion_model import ProteinReDiffModel
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch, deterministic_state_dict, synthetic_batch, synthetic_esm_tokens
from protein_redesign_amd.weights import spec_tensors
from test_hip_parity import TRAJ_TOL
from test_training_cpu import oracle_grads
from test_training_gpu import GRAD_TOL, gemm_mode, hip_model  # noqa: F401  (gemm_mode: fixture)
from test_training_masks_cpu import case_batch, load_fixture, recorded_draws

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_CASES = ["random_b1", "spatial_b1", "none_b1", "spatial_b2", "spatial_b3", "random_below", "random_at"]


def launch(rm, p, *, key=None, geom=None, tokens=None):
    """ops.mask_lowest_k on CPU inputs -> CPU outputs (tokens: the masked copy)."""
    b = rm.shape[0]
    pd = torch.as_tensor(p, dtype=torch.float32).reshape(-1).expand(b).contiguous().to(DEV)
    tok = tokens.clone().to(DEV) if tokens is not None else None
    if key is not None:
        extra, inv = ops.mask_lowest_k(rm.to(DEV), pd, key=key.to(DEV), tokens=tok)
    else:
        ap, am, rap = geom
        extra, inv = ops.mask_lowest_k(rm.to(DEV), pd, atom_pos=ap.to(DEV), atom_mask=am.to(DEV), ca_pos=rap.to(DEV)[:, :, 1], tokens=tok)
    return extra.cpu(), inv.cpu(), (tok.cpu() if tok is not None else None)


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_kernel_reproduces_the_reference_masks_exactly(name):
    meta, z = load_fixture()
    case = meta["cases"][name]
    batch = case_batch(meta, case)
    b, N = batch["residue_mask"].shape
    d = recorded_draws(case, z, name, batch).draw(b, N, meta["args"]["mask_prob"])
    tokens = batch["residue_esm_tokens"]
    if d.branch == "spatial":
        extra, inv, tok = launch(batch["residue_mask"], d.fraction, geom=(batch["atom_pos"], batch["atom_mask"], batch["residue_atom_pos"]),
                                 tokens=tokens)
    else:
        extra, inv, tok = launch(batch["residue_mask"], d.fraction, key=d.keys if d.keys is not None else batch["residue_mask"],
                                 tokens=tokens if d.branch != "none" else None)
    assert torch.equal(extra, torch.from_numpy(z[f"{name}_extra"])), name
    assert torch.equal(inv, torch.from_numpy(z[f"{name}_inv"])), name
    assert torch.equal(tok if tok is not None else tokens, torch.from_numpy(z[f"{name}_tokens"])), name


def seeded_inputs(b, N, seed, ties):
    """A ragged batch: per sample a block of atoms, then a block of residues with a few holes, then padding."""
    g = torch.Generator().manual_seed(seed)
    rm, am = torch.zeros(b, N), torch.zeros(b, N)
    for s in range(b):
        na = max(1, N // 8)
        nr = N - na - (s * N) // 7
        am[s, :na] = 1
        rm[s, na:na + nr] = (torch.rand(nr, generator=g) > 0.05).float()
        rm[s, na] = 1
    key = torch.rand(b, N, generator=g)
    if ties:                                            # deliberate ties: a handful of distinct values, the lower index wins
        key = torch.randint(0, 5, (b, N), generator=g).float()
    ap = am.unsqueeze(-1) * 5.0 * torch.randn(b, N, 3, generator=g)
    rap = rm[:, :, None, None] * 10.0 * torch.randn(b, N, 37, 3, generator=g)
    tokens = torch.randint(4, 24, (b, N), generator=g)
    return rm, am, key, ap, rap, tokens


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("N", [37, 320, 769, 1961, 2048, 4500])
def test_kernel_equals_the_restatement_on_seeded_inputs(N, b):
    """N in {37, 320, 769, 1961} as the issue sets them, plus 2048 (exactly one LDS tile) and 4500 (three tiles); k in
    {0, 1, count - 1, count} (fractions chosen per sample from its own count, random mode), distinct keys and tied keys."""
    for ties in (False, True):
        rm, am, key, ap, rap, tokens = seeded_inputs(b, N, 100 * N + b, ties)
        counts = rm.sum(-1)
        for which in ("0", "1", "count-1", "count"):
            k = {"0": torch.zeros(b), "1": torch.ones(b), "count-1": counts - 1, "count": counts}[which]
            p = ((k + 0.5) / counts).float()            # int(count * p) = k: the half keeps the product clear of an integer
            want = masking.restate_lowest_k(rm, p, key=key, tokens=tokens)
            assert want[1].sum(-1).tolist() == k.tolist(), (which, k, want[1].sum(-1))
            got = launch(rm, p, key=key, tokens=tokens)
            for name, a, w in zip(("extra", "inv", "tokens"), got, want):
                assert torch.equal(a, w), (N, b, ties, which, name, int((a != w).sum()))


@pytest.mark.parametrize("b,N", [(1, 37), (3, 320), (2, 1961), (3, 2500)])
def test_spatial_kernel_equals_the_restatement(b, N):
    """Spatial mode forms the key in the launch: the selected SET equals the restatement's wherever fp32 rounding in another
    summation order cannot move a residue across the boundary -- the inputs are asserted to keep the k-th and (k+1)-th distance
    1e-4 apart (relative), the condition the fixtures are generated under."""
    rm, am, _, ap, rap, tokens = seeded_inputs(b, N, 7 * N + b, False)
    for frac in (0.0, 0.013, 0.37, 0.5):
        want = masking.restate_lowest_k(rm, frac, atom_pos=ap, atom_mask=am, ca_pos=rap[:, :, 1], tokens=tokens)
        k = int(want[1][0].sum())
        assert k <= int(rm.sum(-1).min())
        d = masking.spatial_keys(ap.double(), am.double(), rap[:, :, 1].double())
        for s in range(b):
            ds = torch.sort(d[s][rm[s] > 0.5]).values
            if 0 < k < ds.numel():
                assert float(ds[k] - ds[k - 1]) >= 1e-4 * float(ds[k]), "seeded input too close to a tie: pick another seed"
        got = launch(rm, frac, geom=(ap, am, rap), tokens=tokens)
        for name, a, w in zip(("extra", "inv", "tokens"), got, want):
            assert torch.equal(a, w), (N, b, frac, name, int((a != w).sum()))


def test_two_launches_are_equal_and_outputs_come_back_fully_written():
    b, N = 3, 1961
    rm, am, key, ap, rap, tokens = seeded_inputs(b, N, 5, True)
    p = torch.full((b,), 0.3).to(DEV)
    rmd, keyd, apd, amd, rapd = rm.to(DEV), key.to(DEV), ap.to(DEV), am.to(DEV), rap.to(DEV)
    first = None
    for _ in range(2):
        r = ops.mask_lowest_k(rmd, p, key=keyd) + ops.mask_lowest_k(rmd, p, atom_pos=apd, atom_mask=amd, ca_pos=rapd[:, :, 1])
        if first is None:
            first = [t.clone() for t in r]
        assert all(torch.equal(a, f) for a, f in zip(r, first))
    # outputs pre-filled with NaN come back fully written (also when nothing is selected: k = 0 skips the ranking)
    for mode in ("random", "spatial", "zero"):
        out = tuple(torch.full((b, N), float("nan"), device=DEV) for _ in range(2))
        if mode == "spatial":
            extra, inv = ops.mask_lowest_k(rmd, p, atom_pos=apd, atom_mask=amd, ca_pos=rapd[:, :, 1], out=out)
        else:
            extra, inv = ops.mask_lowest_k(rmd, p * (0.0 if mode == "zero" else 1.0), key=keyd, out=out)
        assert extra is out[0] and inv is out[1]
        assert torch.isfinite(extra).all() and torch.isfinite(inv).all()
        assert torch.equal(extra + inv, rmd) and set(inv.unique().tolist()) <= {0.0, 1.0}


def test_operator_refuses_what_it_does_not_serve():
    rm = torch.ones(257, 8, device=DEV)
    with pytest.raises(RuntimeError, match="PRD_ERR_UNSUPPORTED"):
        ops.mask_lowest_k(rm, torch.zeros(257, device=DEV), key=rm)
    with pytest.raises(ValueError):
        ops.mask_lowest_k(rm[:2], torch.zeros(2, device=DEV))


# ---------------------------------------------------------------------------------------------------
# 2. loss and gradients of the optimisation step
# ---------------------------------------------------------------------------------------------------
_oracle_prepare_batch = O.prepare_batch        # bound early: the sample() test below replaces the module attribute


def oracle_batch(batch, extra, inv):
    """The oracle's prepared batch (prd_oracle.prepare_batch) carrying the given masks."""
    pb = _oracle_prepare_batch({k: v for k, v in batch.items() if k != "residue_esm_tokens"}, 0.0,
                         [torch.arange(int(n)) for n in batch["residue_mask"].sum(-1)])
    one_hot = torch.nn.functional.one_hot(batch["residue_type"], num_classes=21) * 2.0 - 1.0
    pb["residue_esm"] = batch["residue_esm"] * extra.unsqueeze(-1)
    pb["residue_type_masked"] = (batch["residue_type"] * extra).long()
    pb["residue_one_hot"] = one_hot * extra.unsqueeze(-1)
    pb["residue_extra_mask"], pb["residue_inv_extra_mask"] = extra, inv
    return pb


@pytest.mark.parametrize("name", ["random_b1", "spatial_b1", "none_b1"])
def test_training_step_loss_and_gradients(name, gemm_mode):
    meta, z = load_fixture()
    case = meta["cases"][name]
    args = make_args(**meta["args"])
    assert args["training_mode"]
    params = deterministic_state_dict(spec_tensors(args), seed=meta["weight_seed"])
    batch = case_batch(meta, case)
    t = torch.from_numpy(z[f"{name}_train_t"])
    nz, ns = torch.from_numpy(z[f"{name}_train_noise_z"]), torch.from_numpy(z[f"{name}_train_noise_seq"])
    extra, inv = torch.from_numpy(z[f"{name}_extra"]), torch.from_numpy(z[f"{name}_inv"])
    want_loss, want = oracle_grads(args, params, oracle_batch(batch, extra, inv), t, nz, ns)
    model = hip_model(args, params)
    assert model.training_mode
    dbatch = batch_to(clone_batch(batch), DEV)
    loss = model.training_step(dbatch, 0, t=t.to(DEV), noise_z=nz.to(DEV), noise_seq=ns.to(DEV),
                               mask_draws=recorded_draws(case, z, name, batch))
    loss.backward()
    ref_loss = float(z[f"{name}_train_loss"])
    print(f"\n{name} [{gemm_mode}]: loss {float(loss):.6f}, reference {ref_loss:.6f}, oracle {want_loss:.6f}")
    assert torch.equal(dbatch["residue_extra_mask"].cpu(), extra) and torch.equal(dbatch["residue_inv_extra_mask"].cpu(), inv)
    assert torch.equal(dbatch["residue_esm_tokens"].cpu(), torch.from_numpy(z[f"{name}_tokens"]))
    assert abs(float(loss) - ref_loss) < GRAD_TOL * abs(ref_loss)
    assert abs(float(loss) - want_loss) < GRAD_TOL * abs(want_loss)
    got = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    assert sorted(got) == sorted(want) and all(g is not None for g in got.values())
    scale = float(np.linalg.norm([float(w.double().norm()) for w in want.values()]))
    worst = 0.0
    for k in want:
        g = got[k].detach().cpu().double().reshape(-1)
        err = float((g - want[k].double().reshape(-1)).norm())
        ref = float(want[k].double().norm())
        worst = max(worst, err / max(ref, 1e-3 * scale))
        assert err < GRAD_TOL * ref + 1e-6 * scale, (k, err, ref)
    print(f"{name} [{gemm_mode}]: {len(want)} gradients, worst rel-L2 vs oracle autograd {worst:.2e}")


def test_free_running_training_steps_draw_fresh_masks():
    """Without injected draws: a scalar loss with a graph, with or without residue_esm_tokens, and over a few dozen prepared
    batches all three branches occur (keyed on the running count: the masks differ from step to step)."""
    meta, _ = load_fixture()
    args = make_args(**meta["args"])
    model = hip_model(args, deterministic_state_dict(spec_tensors(args), seed=meta["weight_seed"], style="near_init"))
    batch = synthetic_batch([(4, 18), (3, 14)], esm_dim=args["esm_dim"], seed=6, n_total=24)
    for with_tokens in (False, True):
        d = batch_to(clone_batch(batch), DEV)
        if with_tokens:
            d["residue_esm_tokens"] = synthetic_esm_tokens(batch, seed=1).to(DEV)
        loss = model.training_step(d, 0)
        assert loss.dim() == 0 and loss.requires_grad and bool(torch.isfinite(loss))
    torch.manual_seed(0)
    masked = []
    for _ in range(40):
        pb = model.prepare_batch(batch_to(clone_batch(batch), DEV))
        assert torch.equal(pb["residue_extra_mask"] + pb["residue_inv_extra_mask"], pb["residue_mask"])
        masked.append(tuple(int(v) for v in pb["residue_inv_extra_mask"].sum(-1)))
    assert masked.count((0, 0)) >= 10 and len(set(masked)) >= 3, masked
    with torch.no_grad():
        assert bool(torch.isfinite(model.validation_step(batch_to(clone_batch(batch), DEV), 0)))


# ---------------------------------------------------------------------------------------------------
# 3. sample()
# ---------------------------------------------------------------------------------------------------
class _NoPermutation:
    """The oracle's sample() draws a mask permutation first; under training_mode the model does not.  Same normals, no permutation."""

    def __init__(self, src):
        self.src = src

    def randperm(self, n):
        return torch.arange(n)

    def randn(self, *shape):
        return self.src.randn(*shape)


@pytest.mark.parametrize("name", ["random_b1", "spatial_b1", "none_b1", "spatial_b3"])
def test_sample_under_training_mode_matches_the_oracle(name, monkeypatch):
    meta, z = load_fixture()
    case = meta["cases"][name]
    args = make_args(**meta["args"])
    params = deterministic_state_dict(spec_tensors(args), seed=meta["weight_seed"])
    batch = case_batch(meta, case)
    b = batch["residue_mask"].shape[0]
    extra, inv = torch.from_numpy(z[f"{name}_extra"]), torch.from_numpy(z[f"{name}_inv"])
    monkeypatch.setattr(O, "prepare_batch", lambda bt, mask_prob, perms: oracle_batch(bt, extra, inv))
    want_pos, want_logits = O.sample(params, args, {k: v for k, v in batch.items() if torch.is_tensor(v)},
                                     [_NoPermutation(NoiseSource(9, k)) for k in range(b)])
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    model = model.to(DEV).eval()
    assert model.training_mode
    pos, logits = model.sample(batch_to(clone_batch(batch), DEV), sources=[NoiseSource(9, k) for k in range(b)],
                               mask_draws=recorded_draws(case, z, name, batch))
    e_pos, e_log = rel_l2(pos.cpu(), want_pos), rel_l2(logits.cpu(), want_logits)
    print(f"\n{name}: sample() vs oracle: positions {e_pos:.2e}, logits {e_log:.2e}")
    assert e_pos < TRAJ_TOL and e_log < TRAJ_TOL
    pos2, _ = model.predict_step(batch_to(clone_batch(batch), DEV), 0)      # default draws: runs, finite
    assert bool(torch.isfinite(pos2).all())


# ---------------------------------------------------------------------------------------------------
# 4. no host synchronisation
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [0.1, 0.4, 0.9])
def test_training_mode_prepare_batch_does_not_synchronise(rt):
    """Mechanism: ``torch.cuda.set_sync_debug_mode("error")`` where this torch build honours it on ROCm (probed with an
    ``.item()``, which must raise); otherwise the call is captured into a graph on a side stream, where a synchronisation fails
    the capture.  Which one ran is printed.  (The eval branch is not held to this: it selects its mask on the host.)"""
    meta, _ = load_fixture()
    args = make_args(**meta["args"])
    model = ProteinReDiffModel(args).to(DEV)
    batch = synthetic_batch([(4, 18), (3, 14)], esm_dim=args["esm_dim"], seed=6, n_total=24)
    batch["residue_esm_tokens"] = synthetic_esm_tokens(batch, seed=1)
    rec = dict(rt=rt, u=0.3, scale=0.6, idx=700, keys=torch.stack([torch.randperm(24).float() for _ in range(2)]))
    want = model.prepare_batch(batch_to(clone_batch(batch), DEV), mask_draws=masking.MaskDraws(recorded=rec))     # warm: library, allocators
    want = {k: v.clone() for k, v in want.items() if torch.is_tensor(v)}
    d = batch_to(clone_batch(batch), DEV)
    draws = masking.MaskDraws(recorded=rec)
    got = run_without_host_sync(lambda: model.prepare_batch(d, mask_draws=draws))
    for k in ("residue_extra_mask", "residue_inv_extra_mask", "residue_type_masked", "residue_one_hot", "x", "residue_esm_tokens"):
        assert torch.equal(got[k], want[k]), k
    assert int(got["residue_inv_extra_mask"].sum()) == (0 if rt >= 0.5 else int(want["residue_inv_extra_mask"].sum()))
