"""Float64 restatements for the few-step sampling tests (a helper module, imported by tests/test_solver_cpu.py and tests/test_solver.py).

Nothing here imports protein_redesign_amd.solver: the levels, the coefficients and the loop are written again from the formulas, in
python floats / float64 tensors, so that the package's tables are held against something that is not themselves."""
import math

import torch

import prd_oracle as O


def levels(K, top):
    """[tau_0 .. tau_{K-1}]: K levels over [0, top], round half up, in exact integer arithmetic"""
    if K == 1:
        return [top]
    return [(2 * j * top + (K - 1)) // (2 * (K - 1)) for j in range(K)]


def abar(T, schedule="linear"):
    """float64 cumulative product of 1 - betas, the betas being the oracle's fp32 ones"""
    return torch.cumprod(1.0 - O.get_betas(T, schedule).double(), 0).tolist()


def coefficients(lv, ab, kind, eta=0.0, variance="beta"):
    """rows (w, a, c, r, q) per counter k for the ascending levels ``lv``, python floats"""
    rows = []
    for k, t in enumerate(lv):
        at = ab[t]
        as_ = ab[lv[k - 1]] if k > 0 else 1.0
        a = math.sqrt(as_ / at)
        if kind == "ancestral":
            bp = 1.0 - at / as_
            w = bp / math.sqrt(1.0 - at)
            c = math.sqrt(bp) if variance == "beta" else math.sqrt(bp * (1.0 - as_) / (1.0 - at))
        else:
            c = eta * math.sqrt((1.0 - as_) / (1.0 - at)) * math.sqrt(1.0 - at / as_)
            w = -(math.sqrt(max(1.0 - as_ - c * c, 0.0)) - a * math.sqrt(1.0 - at)) / a
        rows.append((w, a, c if k > 0 else 0.0, math.sqrt(1.0 - at), 1.0 / math.sqrt(at)))
    return rows


def ddim_true_noise_loop(x0, e, lv, ab):
    """The deterministic loop in float64 fed the TRUE noise of z_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) e at every level: returns
    what it ends at, which is x0"""
    co = coefficients(lv, ab, "ddim")
    top = lv[-1]
    z = math.sqrt(ab[top]) * x0 + math.sqrt(1.0 - ab[top]) * e
    for k in range(len(lv) - 1, -1, -1):
        w, a, _, _, _ = co[k]
        eps = (z - math.sqrt(ab[lv[k]]) * x0) / math.sqrt(1.0 - ab[lv[k]])          # the noise this z carries
        z = a * (z - w * eps)
    return z


def cast(tree, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in tree.items()}


@torch.inference_mode()
def oracle_loop(params, args, batch, source, lv, kind, eta=0.0, variance="beta", dtype=torch.float64):
    """One sample of the solver loop over the oracle's network in ``dtype``: (positions in Angstrom, masked logits, x0 of the last
    step).  ``source`` is consumed as ReverseDiffusion consumes it: the mask permutation, z_T, seq_T, then K - 1 update tensors iff any
    c is non-zero.  The coefficients are the float64 ones, rounded once to fp32 as the device table is, then used in ``dtype``."""
    cfg = args if isinstance(args, dict) else vars(args)
    T, K = cfg["num_steps"], len(lv)
    co = torch.tensor(coefficients(lv, abar(T, cfg.get("diffusion_schedule", "linear")), kind, eta, variance), dtype=torch.float64)
    co = co.to(torch.float32).to(dtype)
    N = batch["atom_mask"].shape[1]
    n_res = int(batch["residue_mask"].sum())
    pb = O.prepare_batch(batch, cfg["mask_prob"], [source.randperm(n_res)])
    z = source.randn(N, 3)[None]
    seq_t = source.randn(N, 21)[None]
    stochastic = bool((co[:, 2] != 0).any())
    draws = [source.randn(N, 3)[None] for _ in range(K - 1)] if stochastic else []
    pb, p = cast(pb, dtype), cast(params, dtype)
    mask, rm = pb["residue_and_atom_mask"], pb["residue_mask"]
    z = O.remove_mean(z.to(dtype), mask)
    seq_t = O.remove_mean(seq_t.to(dtype), rm)
    seq_t = pb["residue_extra_mask"].unsqueeze(-1) * pb["residue_one_hot"] + pb["residue_inv_extra_mask"].unsqueeze(-1) * seq_t
    x0 = None
    for k in range(K - 1, -1, -1):
        t = torch.full((1,), lv[k], dtype=torch.long if dtype == torch.float32 else dtype)
        eps, seq_pred = O.network_step(p, cfg, pb, z, seq_t, mask, t)
        w, a, c, r, q = co[k]
        x0 = q * (z - r * eps)
        z = a * (z - w * eps)
        if k > 0 and stochastic:
            z = z + c * O.remove_mean(draws[K - 1 - k].to(dtype), mask)
        seq_t = torch.softmax(seq_pred, dim=-1) * 2 - 1
    return 10.0 * z, rm.unsqueeze(-1) * seq_pred, x0


# the loops of the issue: name -> (levels over T = 16, kind, eta, variance) and how the package spells them
def cases(T=16):
    return {
        "ddim4": (levels(4, T - 1), "ddim", 0.0, "beta"),
        "ddim5_eta05": (levels(5, T - 1), "ddim", 0.5, "beta"),
        "ancestral4": (levels(4, T - 1), "ancestral", 0.0, "beta"),
        "ancestral4_posterior": (levels(4, T - 1), "ancestral", 0.0, "posterior"),
        "ddim_15_9_2": ([2, 9, 15], "ddim", 0.0, "beta"),
    }


def package_solver(name):
    from protein_redesign_amd.solver import Solver
    return {"ddim4": lambda: Solver.ddim(4), "ddim5_eta05": lambda: Solver.ddim(5, eta=0.5), "ancestral4": lambda: Solver.ancestral(4),
            "ancestral4_posterior": lambda: Solver.ancestral(4, variance="posterior"),
            "ddim_15_9_2": lambda: Solver(timesteps=[15, 9, 2], kind="ddim")}[name]()


SMOKE = dict(single_dim=128, pair_dim=64, num_blocks=2, esm_dim=64, num_steps=16, mask_prob=0.3)
LOOP_SEED = 3          # tests/test_solver_cpu.py holds the oracle's own fp32 run of every case within a third of the bound for this seed


def smoke_setup():
    """(args, params, CPU batch) of the smoke configuration: 8 atoms + 40 residues in 48 positions, T = 16"""
    from protein_redesign_amd.constants import make_args
    from protein_redesign_amd.synthetic import deterministic_state_dict, synthetic_batch
    from protein_redesign_amd.weights import spec_tensors
    args = make_args(**SMOKE)
    params = deterministic_state_dict(spec_tensors(args), seed=1)
    batch = synthetic_batch([(8, 40)], esm_dim=64, seed=0)
    return args, params, {k: v for k, v in batch.items() if torch.is_tensor(v)}


_REFERENCE = {}


def reference(name):
    """the float64 loop of case ``name`` on the smoke configuration, computed once per process"""
    from protein_redesign_amd.synthetic import NoiseSource
    if name not in _REFERENCE:
        args, params, batch = smoke_setup()
        lv, kind, eta, variance = cases()[name]
        _REFERENCE[name] = oracle_loop(params, args, batch, NoiseSource(LOOP_SEED, 0), lv, kind, eta, variance)
    return _REFERENCE[name]
