"""Generate tests/golden/heads.npz: a network step, a T = 8 trajectory and the gradient fingerprints of one training step,
captured from the IMPORTED reference with ``--num_heads 8 --head_dim 32`` (single_dim 64, pair_dim 64, 2 blocks) -- the head
layout the tuned 4 x 16 triangle-attention kernels do not serve (csrc/prd_tri_heads.hip).  Build machine only, like
oracle/gen_golden.py, whose import_reference / run_case / run_grad_case it reuses unchanged:

    python tools/gen_golden_heads.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden  # noqa: E402

CASE = dict(
    args=dict(single_dim=64, pair_dim=64, head_dim=32, num_heads=8, num_blocks=2, esm_dim=32, num_steps=8, mask_prob=0.3),
    sizes=[(6, 30), (3, 22)], n_total=37, batch_seed=14, weight_seed=4, leaves=False, traj_sample=(6, 30))


def main():
    ref_model, _ = gen_golden.import_reference()
    torch.manual_seed(0)
    res = gen_golden.run_case("heads", CASE, ref_model)
    torch.manual_seed(0)
    res.update(gen_golden.run_grad_case("heads", CASE, ref_model))
    path = os.path.join(ROOT, "tests", "golden", "heads.npz")
    np.savez_compressed(path, **res)
    print("heads ->", path, f"{os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
