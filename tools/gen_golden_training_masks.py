"""Generate tests/golden/training_masks.npz: the masks the IMPORTED reference's ``prepare_batch`` draws under
``training_mode=True`` (model.py:442-458, mask_utils.py), with its draws pinned, and the loss of its ``training_step`` for one case
per branch.  Build machine only, like oracle/gen_golden.py, whose import_reference / build_reference / _Sequence it reuses
unchanged:

    python tools/gen_golden_training_masks.py

The draws are pinned by patching torch.rand / np.random.uniform / np.random.rand / np.random.choice / torch.randperm (and
torch.randint, torch.randn_like for the loss) around the reference's own code.  Per case the fixture holds the batch seed and
sizes, the injected draws and the reference's residue_extra_mask, residue_inv_extra_mask, masked residue_esm_tokens and
residue_type_masked.  Two conditions on the chosen inputs are ASSERTED so that an exact comparison of the masks is fair:
  1. the spatial k does not exceed any sample's residue count (beyond it the reference picks among padded positions whose keys are
     all 1e10 in fp32: which ones is undefined, and the project clips k instead);
  2. in every spatial case the k-th and (k+1)-th smallest distance are at least 1e-4 of the distance apart, so that fp32 rounding
     in another summation order cannot change the selected SET (the set is what is compared, never the order).
It also asserts, for all 1000 fractions of a linspace, which arithmetic the reference's ``numpy double * 0-dim fp32 tensor``
(mask_utils.py:44-49) is: one fp32 product of the fraction rounded to fp32.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden  # noqa: E402

from protein_redesign_amd.synthetic import NoiseSource, clone_batch, synthetic_batch, synthetic_esm_tokens  # noqa: E402

MODEL = dict(
    args=dict(single_dim=64, pair_dim=32, head_dim=16, num_heads=4, num_blocks=2, esm_dim=32, num_steps=8, mask_prob=0.5,
              training_mode=True),
    weight_seed=2)
PERM_SEED = 7
CASES = {
    # all three branches at batch size 1 (with the training_step loss)
    "random_b1": dict(sizes=[(5, 20)], n_total=27, batch_seed=21, rt=0.1, u=0.25, scale=0.7, loss=True),
    # idx 666: linspace(0, 0.3, 1000)[666] = 0.19999999999999998, times 20 residues: 4 as an fp32 product, 3 in float64
    "spatial_b1": dict(sizes=[(5, 20)], n_total=27, batch_seed=22, rt=0.4, u=0.3, idx=666, loss=True),
    "none_b1": dict(sizes=[(5, 20)], n_total=27, batch_seed=23, rt=0.7, u=0.3, loss=True),
    # the spatial branch with unequal residue counts: ONE k for the batch, from the lower median of the counts
    "spatial_b2": dict(sizes=[(4, 18), (3, 12)], n_total=24, batch_seed=24, rt=0.3, u=0.3, idx=999),
    "spatial_b3": dict(sizes=[(4, 18), (3, 12), (5, 15)], n_total=24, batch_seed=25, rt=0.45, u=0.45, idx=640),
    # the random branch with p * count just below and just at an integer (20 residues, p = 1/4 - 2^-21 and 1/4)
    "random_below": dict(sizes=[(5, 20)], n_total=None, batch_seed=26, rt=0.2, u=0.5, scale=0.5 - 2.0 ** -20),
    "random_at": dict(sizes=[(5, 20)], n_total=None, batch_seed=26, rt=0.2, u=0.5, scale=0.5),
}


class _PinnedDraws:
    """The reference's global RNG calls inside prepare_batch return the case's values."""

    def __init__(self, case, perm):
        self.case, self.perm = case, perm
        self.used = []

    def __enter__(self):
        self._saved = (torch.rand, torch.randperm, np.random.uniform, np.random.rand, np.random.choice)
        c, used = self.case, self.used

        def rand(*shape, **kw):
            used.append("rt")
            return torch.full(shape if shape else (1,), c["rt"])

        def randperm(n, **kw):
            used.append("perm")
            assert n == self.perm.numel(), (n, self.perm.numel())
            return self.perm

        def uniform(low, high):
            used.append("u")
            assert low <= c["u"] <= high
            return np.float64(c["u"])

        def np_rand():
            used.append("scale")
            return np.float64(c.get("scale", 0.5))        # the "none" branch draws it too, times max_p = 0

        def choice(arr):
            used.append("idx")
            return arr[c["idx"]]

        torch.rand, torch.randperm = rand, randperm
        np.random.uniform, np.random.rand, np.random.choice = uniform, np_rand, choice
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randperm, np.random.uniform, np.random.rand, np.random.choice = self._saved


def check_scalar_product_arithmetic():
    """mask_utils.py:44-49: (numpy double) * (0-dim fp32 tensor) -> which rounding?  Must be fp32(frac) * fp32(median) in fp32."""
    n_f32 = n_f64 = 0
    for median in (12.0, 15.0, 20.0, 137.0, 256.0, 301.0):
        m = torch.tensor([median, median]).median()                # a 0-dim fp32 tensor, as residue_mask.sum(-1).median()
        for u in (0.1, 0.3, 0.45, 0.15):
            for frac in np.linspace(0, u, 1000):
                ref = (frac * m).int().item()
                as_f32 = int(np.float32(frac) * np.float32(median))
                as_f64 = int(frac * median)
                assert ref == as_f32, (median, u, frac, ref, as_f32, as_f64)
                n_f32 += 1
                n_f64 += ref != as_f64
    print(f"scalar product: {n_f32} fractions equal the fp32 product; {n_f64} of them differ from the float64 product")


def spatial_conditions(batch, frac):
    """(k, assertion of conditions 1 and 2) in float64."""
    rm, am = batch["residue_mask"].double(), batch["atom_mask"].double()
    counts = rm.sum(-1)
    k = int(np.float32(frac) * np.float32(float(batch["residue_mask"].sum(-1).median())))
    assert k <= int(counts.min()), ("condition 1", k, counts.tolist())
    cen = (am.unsqueeze(-1) * batch["atom_pos"].double()).sum(1) / am.sum(-1, keepdim=True)
    d = (cen.unsqueeze(1) - batch["residue_atom_pos"][:, :, 1].double()).norm(dim=-1)
    for s in range(rm.shape[0]):
        ds = torch.sort(d[s][rm[s] > 0.5]).values
        if 0 < k < ds.numel():
            gap = float(ds[k] - ds[k - 1])
            assert gap >= 1e-4 * float(ds[k]), ("condition 2", s, k, gap, float(ds[k]))
    return k


def run_case(name, case, model, args):
    batch = synthetic_batch(case["sizes"], esm_dim=args["esm_dim"], seed=case["batch_seed"], n_total=case["n_total"])
    batch["residue_esm_tokens"] = synthetic_esm_tokens(batch, seed=case["batch_seed"])
    b, N = batch["atom_mask"].shape
    n_res = int(batch["residue_mask"].sum())
    perm = NoiseSource(PERM_SEED, case["batch_seed"]).randperm(n_res)
    branch = "random" if case["rt"] < 0.3 else "spatial" if case["rt"] < 0.5 else "none"
    out = {}
    if branch == "spatial":
        frac = np.linspace(0, case["u"], 1000)[case["idx"]]
        out[f"{name}_k"] = np.array(spatial_conditions(batch, frac))
    if branch == "random":
        assert b == 1, "the reference flattens the batch in the random branch: fixtures at batch size 1 only"
    model.mask_prob = args["mask_prob"]
    work = clone_batch(batch)
    with _PinnedDraws(case, perm) as pin:
        pb = model.prepare_batch(work)
    expect = {"random": ["rt", "u", "scale", "perm"], "spatial": ["rt", "u", "idx"], "none": ["rt", "u", "scale", "perm"]}[branch]
    assert pin.used == expect, (name, pin.used)
    out.update({
        f"{name}_perm": perm.numpy(),
        f"{name}_extra": pb["residue_extra_mask"].numpy(), f"{name}_inv": pb["residue_inv_extra_mask"].numpy(),
        f"{name}_tokens": pb["residue_esm_tokens"].numpy(), f"{name}_type_masked": pb["residue_type_masked"].numpy()})
    nsel = int(pb["residue_inv_extra_mask"].sum())
    if case.get("loss"):
        mask = batch["atom_mask"] + batch["residue_mask"]
        g = torch.Generator().manual_seed(3000 + case["batch_seed"])
        t = torch.tensor([(3 + 2 * k) % args["num_steps"] for k in range(b)], dtype=torch.long)
        nz = gen_golden.O_remove_mean(torch.randn(b, N, 3, generator=g), mask)
        ns = gen_golden.O_remove_mean(torch.randn(b, N, 21, generator=g), batch["residue_mask"])
        randint = torch.randint
        torch.randint = lambda *a, **kw: t.clone()
        try:
            with _PinnedDraws(case, perm), gen_golden._Sequence([nz, ns]):
                loss = model.training_step(clone_batch(batch), 0)                 # model.py:528-549, prepare_batch included
        finally:
            torch.randint = randint
        out.update({f"{name}_train_t": t.numpy(), f"{name}_train_noise_z": nz.numpy(), f"{name}_train_noise_seq": ns.numpy(),
                    f"{name}_train_loss": np.array(float(loss.detach()))})
    print(f"{name}: {branch}, {nsel} residues masked" + (f", loss {float(out[name + '_train_loss']):.6f}" if case.get("loss") else ""))
    return out


def main():
    ref_model, _ = gen_golden.import_reference()
    check_scalar_product_arithmetic()
    model, args = gen_golden.build_reference(ref_model, MODEL)
    assert model.training_mode
    model.train()
    res = {"case": np.array(json.dumps(dict(MODEL, cases=CASES, perm_seed=PERM_SEED)))}
    for name, case in CASES.items():
        torch.manual_seed(0)
        res.update(run_case(name, case, model, args))
    assert int(res["random_below_inv"].sum()) == 4 and int(res["random_at_inv"].sum()) == 5
    assert int(res["spatial_b1_k"]) == 4 and int(np.linspace(0, 0.3, 1000)[666] * 20.0) == 3
    path = os.path.join(ROOT, "tests", "golden", "training_masks.npz")
    np.savez_compressed(path, **res)
    print("training_masks ->", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
