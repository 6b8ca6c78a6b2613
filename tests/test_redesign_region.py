"""GPU: the design regions of inference (masking.Redesign) selected on the device.

1. prd_mask_lowest_k in its two ligand modes (PRD_MASK_LIGAND_NEAREST / _WITHIN) against the torch restatement
   (masking.restate_lowest_k(ligand=...)), exact for extra, inv and tokens, on the boundary-gapped fixtures and the exactly
   representable ties of tests/test_redesign_region_cpu.py (which holds the restatement against a float64 brute force):
   rows of 5 .. 2049 positions (257 crosses the 256-owner pass, 2049 the key tile: the long-row key store), 1 .. 300 ligand atoms
   (300 crosses MASK_ATOMS = 256, the atom tile of csrc/prd_mask.hip), C-alpha pitches 3 and 111, a sample without ligand atoms and
   one without valid residues; bit-reproducibility; the refusals.
2. ``prepare_batch`` under every kind of spec: equal to the batch built from the restatement, without a host synchronisation.
3. ``sample()``: a pocket spec against the same mask given as explicit positions (bit-identical), explicit positions against the
   oracle's loop on the same mask (trajectory tolerance).
4. Without a spec ``prepare_batch`` is the host-side permutation branch it was.
"""
import ctypes

import numpy as np
import pytest
import torch

import prd_oracle as O
from conftest import rel_l2
from no_host_sync import run_without_host_sync
from protein_redesign_amd import _lib, masking, ops
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.diffusion_model import ProteinReDiffModel
from protein_redesign_amd.masking import Redesign
from protein_redesign_amd.synthetic import NoiseSource, batch_to, clone_batch, deterministic_state_dict, synthetic_batch
from protein_redesign_amd.weights import spec_tensors
from test_hip_parity import TRAJ_TOL
from test_redesign_region_cpu import (CASES, GAP, SPECIAL_CASE, boundary_gaps, brute_force_keys, case_id, case_requests, fixture,
                                      tie_fixture, tie_requests)
from test_training_masks import _NoPermutation, oracle_batch
from test_training_masks_cpu import case_batch, load_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"
MASK_ATOMS = 256            # csrc/prd_mask.hip: positions staged per atom tile; the 300-atom fixtures cross it
MASK_LIGAND_MAX_N = 16384   # include/prd_hip.h: the row limit of PRD_MASK_LIGAND_NEAREST (64 verdict bits x 256 threads)


def launch(rm, p, mode, ap, am, rap, tokens=None, ld_ca=111):
    """ops.mask_lowest_k(ligand=mode) on CPU inputs -> CPU outputs (tokens: the masked copy).  ``ld_ca`` = 111: the C-alpha view of
    the [b,N,37,3] tensor as it lies; 3: a packed [b,N,3] copy."""
    b = rm.shape[0]
    pd = torch.as_tensor(p, dtype=torch.float32).reshape(-1).expand(b).contiguous().to(DEV)
    ca = rap.to(DEV)[:, :, 1] if ld_ca == 111 else rap[:, :, 1].contiguous().to(DEV)
    assert ca.stride(1) == ld_ca
    tok = tokens.clone().to(DEV) if tokens is not None else None
    extra, inv = ops.mask_lowest_k(rm.to(DEV), pd, atom_pos=ap.to(DEV), atom_mask=am.to(DEV), ca_pos=ca, tokens=tok, ligand=mode)
    return extra.cpu(), inv.cpu(), (tok.cpu() if tok is not None else None)


# ---------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [SPECIAL_CASE], ids=case_id)
def test_kernel_equals_the_restatement(case):
    """Per case: NEAREST with k in {0, 1, a third, count - 1, count}, WITHIN with radius 0, a radius through the residues, one
    beyond every key and NaN.  The C-alpha pitch and the presence of tokens alternate from case to case."""
    n = (CASES + [SPECIAL_CASE]).index(case)
    assert (300 > MASK_ATOMS) and any(c[2] == 300 for c in CASES)
    rm, am, ap, rap, tokens = fixture(*case)
    ld_ca = (111, 3)[n % 2]
    for r, (mode, p, k, label) in enumerate(case_requests(rm, case[0])):
        tk = tokens if (n + r) % 3 else None
        want = masking.restate_lowest_k(rm, p, atom_pos=ap, atom_mask=am, ca_pos=rap[:, :, 1], tokens=tk, ligand=mode)
        got = launch(rm, p, mode, ap, am, rap, tokens=tk, ld_ca=ld_ca)
        for name, a, w in zip(("extra", "inv", "tokens"), got, want):
            assert (a is None and w is None) or torch.equal(a, w), (case_id(case), mode, label, name, int((a != w).sum()))
    if len(case) > 4:       # sample 1 has no ligand atom, sample 2 no valid residue: nothing selected there, whatever is asked
        for mode, p in (("nearest", 1.0), ("within", 1e4)):
            extra, inv, _ = launch(rm, p, mode, ap, am, rap)
            assert torch.equal(inv[0], rm[0]) and float(inv[1:].sum()) == 0 and torch.equal(extra[1:], rm[1:])


@pytest.mark.parametrize("ld_ca", [3, 111])
def test_kernel_on_exactly_representable_ties(ld_ca):
    rm, am, ap, rap, tokens = tie_fixture()
    for mode, p, sel in tie_requests():
        extra, inv, tok = launch(rm, p, mode, ap, am, rap, tokens=tokens, ld_ca=ld_ca)
        assert sorted(torch.nonzero(inv[0]).flatten().tolist()) == sorted(sel), (mode, p)
        want = masking.restate_lowest_k(rm, p, atom_pos=ap, atom_mask=am, ca_pos=rap[:, :, 1], tokens=tokens, ligand=mode)
        assert torch.equal(extra, want[0]) and torch.equal(inv, want[1]) and torch.equal(tok, want[2])


def test_two_launches_are_bit_identical_and_outputs_come_back_fully_written():
    rm, am, ap, rap, _ = fixture(*CASES[-2])            # b = 3, N = 2049, 300 atoms: the long-row key store lies in `extra`
    b, N = rm.shape
    rmd, apd, amd, rapd = rm.to(DEV), ap.to(DEV), am.to(DEV), rap.to(DEV)
    for mode, p in (("nearest", 0.3), ("nearest", 0.0), ("within", 14.0), ("within", float("nan"))):
        pd = torch.full((b,), p, device=DEV)
        first = None
        for _ in range(2):
            out = tuple(torch.full((b, N), float("nan"), device=DEV) for _ in range(2))
            extra, inv = ops.mask_lowest_k(rmd, pd, atom_pos=apd, atom_mask=amd, ca_pos=rapd[:, :, 1], ligand=mode, out=out)
            assert extra is out[0] and inv is out[1]
            assert torch.isfinite(extra).all() and torch.isfinite(inv).all()
            assert torch.equal(extra + inv, rmd) and set(inv.unique().tolist()) <= {0.0, 1.0}
            if first is None:
                first = (extra.clone(), inv.clone())
            assert torch.equal(extra, first[0]) and torch.equal(inv, first[1])


def test_entry_refuses_before_any_launch():
    """Beyond the row limit of the verdict bitmask NEAREST returns PRD_ERR_UNSUPPORTED; a NULL atom_pos is PRD_ERR_ARG in both
    modes; WITHIN has no row limit (it compares every key in place)."""
    N = MASK_LIGAND_MAX_N + 1
    rm = torch.zeros(1, N, device=DEV)
    rm[0, 1:] = 1
    am = torch.zeros(1, N, device=DEV)
    am[0, 0] = 1
    ap = torch.zeros(1, N, 3, device=DEV)
    ca = torch.zeros(1, N, 3, device=DEV)
    ca[0, :, 0] = torch.arange(N, device=DEV)           # residue i lies i Angstrom from the one ligand atom
    p = torch.full((1,), 0.5, device=DEV)
    with pytest.raises(RuntimeError, match="PRD_ERR_UNSUPPORTED"):
        ops.mask_lowest_k(rm, p, atom_pos=ap, atom_mask=am, ca_pos=ca, ligand="nearest")
    out = tuple(torch.full((1, N), 7.0, device=DEV) for _ in range(2))
    f = _lib.lib().prd_mask_lowest_k
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for mode, n, a_pos, want in ((ops.MASK_LIGAND_NEAREST, N, ap, -3), (ops.MASK_LIGAND_NEAREST, 64, None, -1),
                                 (ops.MASK_LIGAND_WITHIN, 64, None, -1)):
        code = f(ptr(out[0]), ptr(out[1]), None, ptr(rm), None, ptr(a_pos) if a_pos is not None else None, ptr(am), ptr(ca), 3, ptr(p),
                 mode, 1, n, None)
        assert code == want, (mode, n, code)
    torch.cuda.synchronize()
    assert float(out[0].min()) == 7.0 and float(out[1].max()) == 7.0       # nothing was launched
    extra, inv = ops.mask_lowest_k(rm, torch.full((1,), 100.0, device=DEV), atom_pos=ap, atom_mask=am, ca_pos=ca, ligand="within")
    assert inv[0].nonzero().flatten().tolist() == list(range(1, 101)) and torch.equal(extra + inv, rm)
    with pytest.raises(ValueError):
        ops.mask_lowest_k(rm, p, atom_pos=ap, atom_mask=am, ca_pos=ca, ligand="pocket")
    with pytest.raises(ValueError):
        ops.mask_lowest_k(rm, p, key=rm, ligand="within")


# ---------------------------------------------------------------------------------------------------
# 2. prepare_batch
# ---------------------------------------------------------------------------------------------------
def restated_spec_masks(batch, kind, value):
    """(extra, inv) of a spec on a CPU batch through the restatement; the pocket kinds assert the fixture's boundary gap."""
    rm = batch["residue_mask"]
    if kind == "positions":
        return rm * (1 - value), rm * value
    geom = dict(atom_pos=batch["atom_pos"], atom_mask=batch["atom_mask"], ca_pos=batch["residue_atom_pos"][:, :, 1])
    keys = brute_force_keys(rm, batch["atom_mask"], batch["atom_pos"], batch["residue_atom_pos"][:, :, 1])
    b = rm.shape[0]
    counts = (rm > 0.5).sum(-1)
    ks = [(counts.double() * float(np.float32(value))).long()] if kind == "nearest" else []
    radii = [np.full(b, value)] if kind == "within" else []
    assert boundary_gaps(rm, keys, ks, radii) >= GAP, "fixture too close to a decision boundary: pick another seed or value"
    extra, inv, _ = masking.restate_lowest_k(rm, value, ligand=kind, **geom)
    return extra, inv


def spec_of(kind, value):
    return {"within": Redesign.within, "nearest": Redesign.nearest, "positions": Redesign.positions}[kind](value)


def positions_value(N):
    m = torch.zeros(N)
    m[[1, 5, 6, 9, N - 1]] = 1             # a ligand atom, residues of both samples, padding
    return m


@pytest.mark.parametrize("kind,value", [("within", 12.0), ("nearest", 0.3), ("positions", None)])
def test_prepare_batch_with_a_spec_equals_the_restatement_and_does_not_synchronise(kind, value):
    """Mechanism: ``torch.cuda.set_sync_debug_mode("error")`` where this torch build honours it on ROCm (probed with an
    ``.item()``, which must raise); otherwise the call is captured into a graph on a side stream, where a synchronisation fails
    the capture.  Which one ran is printed."""
    meta, _ = load_fixture()
    args = make_args(**dict(meta["args"], training_mode=False))
    model = ProteinReDiffModel(args).to(DEV)
    batch = synthetic_batch([(4, 18), (3, 14)], esm_dim=args["esm_dim"], seed=6, n_total=24)
    if kind == "positions":
        value = positions_value(24)
    extra, inv = restated_spec_masks(batch, kind, value)
    assert 0 < int(inv.sum()) < int(batch["residue_mask"].sum())
    want = oracle_batch(batch, extra, inv)
    spec = spec_of(kind, value).to(DEV)
    model.prepare_batch(batch_to(clone_batch(batch), DEV), redesign=spec)      # warm: library, allocators
    d = batch_to(clone_batch(batch), DEV)
    counter = model._sample_counter
    got = run_without_host_sync(lambda: model.prepare_batch(d, redesign=spec))
    assert model._sample_counter == counter == 0        # the noise sources are not consulted for the mask
    for k in ("residue_extra_mask", "residue_inv_extra_mask", "residue_type_masked", "residue_one_hot", "residue_esm", "x",
              "residue_and_atom_mask"):
        assert torch.equal(got[k].cpu(), want[k]), k
    model.redesign = spec                               # the attribute serves where no keyword is given
    again = model.prepare_batch(batch_to(clone_batch(batch), DEV))
    assert torch.equal(again["residue_inv_extra_mask"].cpu(), inv)


# ---------------------------------------------------------------------------------------------------
# 3. sample()
# ---------------------------------------------------------------------------------------------------
def sample_setup(num_steps=4):
    """The smallest fixture and model of test_training_masks.py's sample comparison (spatial_b1: 5 atoms + 20 residues in 27
    positions), as an inference model with a short T."""
    meta, _ = load_fixture()
    args = make_args(**dict(meta["args"], training_mode=False, num_steps=num_steps))
    params = deterministic_state_dict(spec_tensors(args), seed=meta["weight_seed"])
    batch = case_batch(meta, meta["cases"]["spatial_b1"])
    batch.pop("residue_esm_tokens")
    model = ProteinReDiffModel(args)
    model.load_state_dict(params)
    return args, params, batch, model.to(DEV).eval()


def test_sample_with_a_pocket_equals_sample_with_its_positions():
    args, params, batch, model = sample_setup()
    radius = 12.0
    extra, inv = restated_spec_masks(batch, "within", radius)
    assert 0 < int(inv.sum()) < int(batch["residue_mask"].sum())
    a = model.sample(batch_to(clone_batch(batch), DEV), sources=[NoiseSource(9, 0)], redesign=Redesign.within(radius))
    d = batch_to(clone_batch(batch), DEV)
    b = model.sample(d, sources=[NoiseSource(9, 0)], redesign=Redesign.positions(inv[0]))
    assert torch.equal(d["residue_inv_extra_mask"].cpu(), inv) and torch.equal(d["residue_extra_mask"].cpu(), extra)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    k = int(inv.sum())                                  # ... and the nearest k residues are the same set once more
    c = model.sample(batch_to(clone_batch(batch), DEV), sources=[NoiseSource(9, 0)],
                     redesign=Redesign.nearest((k + 0.5) / int(batch["residue_mask"].sum())))
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_sample_with_positions_matches_the_oracle(monkeypatch):
    args, params, batch, model = sample_setup()
    extra, inv = restated_spec_masks(batch, "within", 12.0)
    monkeypatch.setattr(O, "prepare_batch", lambda bt, mask_prob, perms: oracle_batch(bt, extra, inv))
    want_pos, want_logits = O.sample(params, args, {k: v for k, v in batch.items() if torch.is_tensor(v)}, [_NoPermutation(NoiseSource(9, 0))])
    pos, logits = model.sample(batch_to(clone_batch(batch), DEV), sources=[NoiseSource(9, 0)], redesign=Redesign.positions(inv))
    e_pos, e_log = rel_l2(pos.cpu(), want_pos), rel_l2(logits.cpu(), want_logits)
    print(f"\nsample(redesign=positions) vs oracle: positions {e_pos:.2e}, logits {e_log:.2e}")
    assert e_pos < TRAJ_TOL and e_log < TRAJ_TOL
    model.redesign = Redesign.positions(inv)
    d = batch_to(clone_batch(batch), DEV)
    pos2, _ = model.predict_step(d, 0)                  # the attribute serves where no keyword is given
    assert bool(torch.isfinite(pos2).all()) and torch.equal(d["residue_inv_extra_mask"].cpu(), inv)


# ---------------------------------------------------------------------------------------------------
# 4. the default path
# ---------------------------------------------------------------------------------------------------
def test_prepare_batch_without_a_spec_is_the_permutation_branch():
    """Expected values from the host restatement of the permutation branch (prd_oracle.prepare_batch with the permutations the keyed
    sources draw), not from a recorded run."""
    meta, _ = load_fixture()
    args = make_args(**dict(meta["args"], training_mode=False))
    model = ProteinReDiffModel(args).to(DEV)
    assert model.redesign is None
    batch = synthetic_batch([(4, 18), (3, 14)], esm_dim=args["esm_dim"], seed=6, n_total=24)
    counts = [int(n) for n in batch["residue_mask"].sum(-1)]
    want = O.prepare_batch(batch, args["mask_prob"], [NoiseSource(9, k).randperm(n) for k, n in enumerate(counts)])
    got = model.prepare_batch(batch_to(clone_batch(batch), DEV), sources=[NoiseSource(9, k) for k in range(2)])
    assert int(want["residue_inv_extra_mask"].sum()) == sum(int(n * args["mask_prob"]) for n in counts) > 0
    for k in ("residue_extra_mask", "residue_inv_extra_mask", "residue_type_masked", "residue_one_hot", "residue_esm", "x",
              "residue_and_atom_mask"):
        assert torch.equal(got[k].cpu(), want[k]), k
