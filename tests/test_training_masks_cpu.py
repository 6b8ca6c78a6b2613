"""CPU checks of the training-mode masks (reference model.py:442-458, mask_utils.py) without a GPU:

* the torch restatement of the device selection (masking.restate_lowest_k: what prd_mask_lowest_k computes, include/prd_hip.h), fed
  with the draws ``masking.MaskDraws`` hands to the device, reproduces every mask of tests/golden/training_masks.npz EXACTLY --
  the masks the imported reference drew with the same values pinned (tools/gen_golden_training_masks.py).  This pins the
  branching, the fractions, the median rule and the token masking against the reference;
* ``prepare_batch`` with ``training_mode=True`` reaches the HIP operator (which refuses CPU tensors) instead of raising
  NotImplementedError, and the draws are keyed and memoised as documented.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from protein_redesign_amd import masking
from protein_redesign_amd.constants import make_args
from protein_redesign_amd.diffusion_model import ProteinReDiffModel
from protein_redesign_amd.synthetic import synthetic_batch, synthetic_esm_tokens


def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "training_masks.npz"), allow_pickle=False)
    return json.loads(str(z["case"])), z


def case_batch(meta, case):
    sizes = [tuple(s) for s in case["sizes"]]
    batch = synthetic_batch(sizes, esm_dim=meta["args"]["esm_dim"], seed=case["batch_seed"], n_total=case["n_total"])
    batch["residue_esm_tokens"] = synthetic_esm_tokens(batch, seed=case["batch_seed"])
    return batch


def recorded_draws(case, z, name, batch):
    """The values the reference was given, as a MaskDraws source: in the random branch the pinned torch.randperm becomes the key
    vector that selects the same residues (batch size 1)."""
    rec = dict(rt=case["rt"], u=case["u"], scale=case.get("scale"), idx=case.get("idx"))
    if case["rt"] < 0.3:
        rec["keys"] = masking.keys_from_permutation(batch["residue_mask"][0], torch.from_numpy(z[f"{name}_perm"])).unsqueeze(0)
    return masking.MaskDraws(recorded=rec)


def restated_masks(meta, case, z, name):
    """(extra, inv, tokens, type_masked) of a fixture case through MaskDraws + the restatement of the device selection."""
    batch = case_batch(meta, case)
    b, N = batch["residue_mask"].shape
    d = recorded_draws(case, z, name, batch).draw(b, N, meta["args"]["mask_prob"])
    tokens = batch["residue_esm_tokens"]
    if d.branch == "spatial":
        extra, inv, tok = masking.restate_lowest_k(batch["residue_mask"], d.fraction, atom_pos=batch["atom_pos"], atom_mask=batch["atom_mask"],
                                                   ca_pos=batch["residue_atom_pos"][:, :, 1], tokens=tokens)
    else:
        keys = d.keys if d.keys is not None else batch["residue_mask"]
        extra, inv, tok = masking.restate_lowest_k(batch["residue_mask"], d.fraction, key=keys, tokens=tokens)
    if d.branch == "none":
        tok = tokens                                    # model.py:455: the tokens are left alone
    return d, extra, inv, tok, (batch["residue_type"] * extra).long()


def test_fixture_covers_the_cases_of_the_issue():
    meta, z = load_fixture()
    cases = meta["cases"]
    branch = {n: ("random" if c["rt"] < 0.3 else "spatial" if c["rt"] < 0.5 else "none") for n, c in cases.items()}
    for want in ("random", "spatial", "none"):
        assert any(branch[n] == want and len(c["sizes"]) == 1 and c.get("loss") for n, c in cases.items()), want
    for b in (2, 3):
        assert any(branch[n] == "spatial" and len(c["sizes"]) == b and len({s[1] for s in c["sizes"]}) == b for n, c in cases.items()), b
    assert int(z["random_below_inv"].sum()) + 1 == int(z["random_at_inv"].sum()) == 5      # p * count just below / at an integer


@pytest.mark.parametrize("name", ["random_b1", "spatial_b1", "none_b1", "spatial_b2", "spatial_b3", "random_below", "random_at"])
def test_restatement_reproduces_the_reference_masks_exactly(name):
    meta, z = load_fixture()
    d, extra, inv, tok, type_masked = restated_masks(meta, meta["cases"][name], z, name)
    assert torch.equal(extra, torch.from_numpy(z[f"{name}_extra"])), (name, d)
    assert torch.equal(inv, torch.from_numpy(z[f"{name}_inv"])), (name, d)
    assert torch.equal(tok, torch.from_numpy(z[f"{name}_tokens"])), (name, d)
    assert torch.equal(type_masked, torch.from_numpy(z[f"{name}_type_masked"])), (name, d)
    if d.branch == "spatial":                           # ONE k for the batch, from the lower median of the counts
        assert inv.sum(-1).tolist() == [float(z[f"{name}_k"])] * inv.shape[0]


def test_restatement_rules():
    """The rules of include/prd_hip.h on hand-made inputs: ties go to the lower index, invalid positions are never selected, k is
    clipped to the sample's own count, the lower median, and the fp32 product of the spatial k."""
    rm = torch.tensor([[0, 1, 1, 1, 1, 0], [1, 1, 0, 0, 0, 0]], dtype=torch.float32)
    key = torch.tensor([[0, 5, 2, 2, 2, 0], [3, 3, 0, 0, 0, 0]], dtype=torch.float32)
    extra, inv, _ = masking.restate_lowest_k(rm, torch.tensor([0.5, 1.0]), key=key)
    assert inv.tolist() == [[0, 0, 1, 1, 0, 0], [1, 1, 0, 0, 0, 0]] and torch.equal(extra, rm - inv)
    extra, inv, _ = masking.restate_lowest_k(rm, 7.0, key=key)                     # k far above the count: clipped
    assert torch.equal(inv, rm) and float(extra.sum()) == 0
    # spatial: counts 4 and 2 -> lower median 2 -> k = int(0.99f * 2) = 1 in both samples
    ap = torch.zeros(2, 6, 3)
    am = torch.zeros(2, 6)
    ca = torch.arange(36, dtype=torch.float32).reshape(2, 6, 3)
    extra, inv, tok = masking.restate_lowest_k(rm, 0.99, atom_pos=ap, atom_mask=am + torch.tensor([1.0, 0, 0, 0, 0, 0]), ca_pos=ca,
                                               tokens=torch.full((2, 6), 7))
    assert inv.tolist() == [[0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0]]
    assert tok.tolist() == [[1, 32, 7, 7, 7, 1], [32, 7, 1, 1, 1, 1]]
    # the fraction is rounded to fp32 and multiplied in fp32 (mask_utils.py:44-49: numpy double x 0-dim fp32 tensor)
    frac, med = float(np.linspace(0, 0.3, 1000)[666]), 10.0
    assert int(np.float32(frac) * np.float32(med)) == 2 and int(frac * med) == 1
    rm10 = torch.ones(1, 10)
    _, inv, _ = masking.restate_lowest_k(rm10, frac, atom_pos=torch.zeros(1, 10, 3), atom_mask=torch.ones(1, 10),
                                         ca_pos=torch.arange(30, dtype=torch.float32).reshape(1, 10, 3))
    assert int(inv.sum()) == 2
    meta, z = load_fixture()                            # ... and a fixture case sits on such a fraction
    c = meta["cases"]["spatial_b1"]
    assert int(np.linspace(0, c["u"], 1000)[c["idx"]] * 20.0) + 1 == int(z["spatial_b1_k"]) == int(z["spatial_b1_inv"].sum())


def test_mask_draws_are_keyed_memoised_and_branch_like_the_reference():
    a, b_, c = masking.MaskDraws(3, 0), masking.MaskDraws(3, 0), masking.MaskDraws(3, 1)
    da, db, dc = a.draw(2, 9, 0.15), b_.draw(2, 9, 0.15), c.draw(2, 9, 0.15)
    assert (da.rt, da.u, da.fraction) == (db.rt, db.u, db.fraction) and (da.rt, da.u) != (dc.rt, dc.u)
    assert a.draw(2, 9, 0.15) is da                     # memoised: a repeated prepare_batch sees the same mask
    seen = set()
    for i in range(200):
        d = masking.MaskDraws(11, i).draw(2, 9, 0.15)
        assert 0.0 <= d.rt < 1.0 and 0.1 <= d.u <= 0.15
        assert d.branch == ("random" if d.rt < 0.3 else "spatial" if d.rt < 0.5 else "none")
        if d.branch == "random":
            assert 0.0 <= d.scale < 1.0 and d.fraction == d.scale * d.u
            assert d.keys.shape == (2, 9) and all(sorted(r.tolist()) == list(range(9)) for r in d.keys)     # distinct keys
        elif d.branch == "spatial":
            assert d.fraction == float(np.linspace(0, d.u, 1000)[d.idx]) and d.keys is None
        else:
            assert d.fraction == 0.0
        seen.add(d.branch)
    assert seen == {"random", "spatial", "none"}


def test_training_mode_prepare_batch_reaches_the_hip_operator():
    """``training_mode=True`` no longer raises NotImplementedError: on a CPU batch the call gets as far as the HIP operator, which
    refuses CPU tensors like every operator of the package (there is no CPU fallback)."""
    args = make_args(single_dim=32, pair_dim=32, head_dim=16, num_heads=4, num_blocks=1, esm_dim=16, num_steps=6, mask_prob=0.15,
                     training_mode=True)
    m = ProteinReDiffModel(args)
    for rt in (0.1, 0.4, 0.9):                          # all three branches, with and without the optional tokens
        for with_tokens in (False, True):
            batch = synthetic_batch([(3, 9), (2, 6)], esm_dim=16, seed=5, n_total=14)
            if with_tokens:
                batch["residue_esm_tokens"] = synthetic_esm_tokens(batch, seed=1)
            rec = dict(rt=rt, u=0.12, scale=0.5, idx=500, keys=torch.zeros(2, 14))
            with pytest.raises(RuntimeError, match="GPU only"):
                m.prepare_batch(batch, mask_draws=masking.MaskDraws(recorded=rec))
    with pytest.raises(RuntimeError, match="GPU only"):
        m.prepare_batch(synthetic_batch([(3, 9)], esm_dim=16, seed=5))          # default draws: keyed on a running count
    assert m._mask_draw_counter == 1


def test_selection_kernel_compiles_without_scratch():
    """The compiler's figures for csrc/prd_mask.hip under the committed flags (protein_redesign_amd.build --resources; no GPU needed)."""
    from protein_redesign_amd import build
    u = build.resource_usage()["mask_lowest_k_kernel"]
    assert u["scratch"] == 0 and u["lds"] <= 16 * 1024, u
