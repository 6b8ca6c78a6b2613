"""Shared helpers of the guided-sampling tests (a helper module, imported by tests/test_guidance_cpu.py and tests/test_guidance.py):
the inputs of the kernel comparison, the tolerance rule, and the float64 loop over the oracle's network with the restatement of the
guidance launch inserted between the network and the update -- tests/solver_ref.py's loop, extended.

The tables of the float64 loop are written again from the formulas (solver_ref.abar, solver_ref.coefficients), not taken from
``Guidance.tables``; the energy and its gradient are ``guidance.restate_guide``, which tests/test_guidance_cpu.py holds against
autograd."""
import torch

import prd_oracle as O
import solver_ref as R
from protein_redesign_amd import guidance as GD
from protein_redesign_amd.guidance import Guidance, Restraint

T = 16
FLOORS = torch.tensor([0.30, 0.25, 0.20])          # nm: the defaults of Guidance(clash=True)
WEIGHTS = torch.tensor([1.0, 0.7, 1.3])            # the kernel takes a weight per class; the spec gives all three the same
LONG_ROW = 70                                      # restraints of the one row that carries any: longer than a wave


def rel(a, b):
    """relative L2 of a against b; 0 when both vanish"""
    a, b = a.double(), b.double()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float(a.norm())


def table16(scale=0.8, cap=0.05):
    """[16,4] fp32 {q, r, lam, cap} of the linear schedule at T = 16, lam = scale q r, written from the formulas"""
    ab = torch.tensor(R.abar(T), dtype=torch.float64)
    q, r = 1.0 / ab.sqrt(), (1.0 - ab).sqrt()
    return torch.stack([q, r, scale * q * r, torch.full_like(q, cap)], dim=1).float()


def kernel_case(N, seed, b=3):
    """Inputs of one kernel comparison at b = 3: positions drawn so that a good share of the pairs sit inside their floors (a cloud of
    standard deviation 0.25 nm N^(1/3) / 4: the density of the cloud does not fall with N; two points: 0.05 nm), classes mixed over
    {0, 1, 2}, sample 1 padded
    with mask = 0 at its tail, a symmetric exclusion matrix, and ONE row (row N // 2 of every sample) carrying min(70, N - 1)
    restraints, every other row none of its own."""
    g = torch.Generator().manual_seed(seed)
    sigma = 0.25 * max(N, 8) ** (1.0 / 3.0) / 4.0 if N > 2 else 0.05      # two points: close enough to clash
    z = sigma * torch.randn(b, N, 3, generator=g)
    eps = 0.3 * torch.randn(b, N, 3, generator=g)
    mask = torch.ones(b, N)
    if N > 2:
        mask[1, N - max(N // 5, 1):] = 0.0
    cls = torch.randint(0, 3, (b, N), generator=g, dtype=torch.int32)
    cls[:, :2] = torch.tensor([1, 2], dtype=torch.int32)[:N]                # both classes occur, also at N = 1, 2
    upper = (torch.rand(b, N, N, generator=g) < 0.2).triu(1)
    exclude = (upper | upper.transpose(1, 2)).to(torch.uint8)
    csr = None
    if N > 1:
        own = N // 2
        others = [j for j in range(N) if j != own]
        n = min(LONG_ROW, len(others))
        pick = [others[int(k)] for k in torch.randperm(len(others), generator=g)[:n]]
        # Angstrom; a lower bound alone, an upper bound alone, a window -- in turn
        spec = Guidance(restraints=[Restraint(own, j, lo=((30.0 if k % 3 == 0 else 10.0) * sigma) if k % 3 != 1 else None,
                                              hi=(12.0 * sigma) if k % 3 else None,
                                              weight=0.5 + 0.01 * k) for k, j in enumerate(pick)], clash=False)
        csr = spec.csr({"atom_mask": torch.zeros(b, N)})
    return dict(z=z, eps_raw=eps, mask=mask, cls=cls, exclude=exclude, csr=csr, floors=FLOORS.clone(), wclash=WEIGHTS.clone())


def restate(c, counter, table, exclude=True, dtype=torch.float64):
    return GD.restate_guide(c["z"], c["eps_raw"], c["mask"], torch.tensor(counter), table, c["cls"], c["floors"], c["wclash"],
                            c["exclude"] if exclude else None, c["csr"], dtype=dtype)


def tolerances(c, counter, table, exclude=True):
    """(want in float64, tolerance of the added term, tolerance of e_out): 4 x the error of the restatement evaluated in fp32 against
    its float64 self, as relative L2 over the live samples -- a different summation order over up to N terms is legitimate."""
    want, f32 = restate(c, counter, table, exclude), restate(c, counter, table, exclude, dtype=torch.float32)
    live = want["live"]
    e_add = rel((f32["eps_out"] - c["eps_raw"])[live], (want["eps_out"] - c["eps_raw"].double())[live])
    e_en = rel(f32["e_out"][live], want["e_out"][live])
    return want, 4.0 * e_add, 4.0 * e_en, (e_add, e_en)


# ---- the float64 loop -----------------------------------------------------------------------------------------------------------------
def loop_spec(from_level=8, scale=0.5):
    """the guided loop of the tests on the smoke complex (8 atoms + 40 residues): the clash term plus three restraints -- a ligand atom
    near a residue, two residues held apart, two ligand atoms in a window --, guided from the middle of the schedule down"""
    return Guidance(restraints=[Restraint(3, 8 + 12, hi=6.0), Restraint(8 + 2, 8 + 30, lo=25.0, weight=0.5), Restraint(0, 5, lo=1.2, hi=1.6)],
                    clash=True, scale=scale, cap=0.2, from_level=from_level)


def guide_table(spec, lv, schedule="linear"):
    """[K,4] {q, r, lam, cap} at the ascending levels ``lv``: float64 from the formulas, rounded once to fp32"""
    ab = torch.tensor(R.abar(T, schedule), dtype=torch.float64)[lv]
    q, r = 1.0 / ab.sqrt(), (1.0 - ab).sqrt()
    lam = spec.scale * q * r if spec.schedule == "sigma" else torch.full_like(q, spec.scale)
    if spec.from_level is not None:
        lam = torch.where(torch.tensor(lv) > spec.from_level, torch.zeros_like(lam), lam)
    return torch.stack([q, r, lam, torch.full_like(q, spec.cap)], dim=1).float()


@torch.inference_mode()
def oracle_loop(params, args, batch, source, spec=None, solver=None, dtype=torch.float64):
    """One sample of the loop over the oracle's network in ``dtype``: (positions in Angstrom, masked logits, e_out [N,2] of the last
    step or None).  ``solver``: None -- every level, the (w, a, c) rows of the one-level-at-a-time loop (the package's fp32 table, as
    the device uses it), T - 1 update draws -- or ("ddim", K).  ``spec``: the guidance, whose launch is restated between the network
    and the update; None: the unguided loop of the same configuration."""
    from protein_redesign_amd.schedule import reverse_coefficients, schedule_tables
    cfg = args if isinstance(args, dict) else vars(args)
    N = batch["atom_mask"].shape[1]
    if solver is None:
        lv = list(range(T))
        co = reverse_coefficients(schedule_tables(T, "linear"))[:, :3].to(dtype)
        stochastic = True
    else:
        lv = R.levels(solver[1], T - 1)
        co = torch.tensor(R.coefficients(lv, R.abar(T), solver[0]), dtype=torch.float64).to(torch.float32).to(dtype)
        stochastic = False
    K = len(lv)
    n_res = int(batch["residue_mask"].sum())
    pb = O.prepare_batch(batch, cfg["mask_prob"], [source.randperm(n_res)])
    z = source.randn(N, 3)[None]
    seq_t = source.randn(N, 21)[None]
    draws = [source.randn(N, 3)[None] for _ in range(K - 1)] if stochastic else []
    terms = table = None
    if spec is not None:
        terms, table = spec.terms(pb), guide_table(spec, lv)
    pb, p = R.cast(pb, dtype), R.cast(params, dtype)
    mask, rm = pb["residue_and_atom_mask"], pb["residue_mask"]
    z = O.remove_mean(z.to(dtype), mask)
    seq_t = O.remove_mean(seq_t.to(dtype), rm)
    seq_t = pb["residue_extra_mask"].unsqueeze(-1) * pb["residue_one_hot"] + pb["residue_inv_extra_mask"].unsqueeze(-1) * seq_t
    e_out = None
    for k in range(K - 1, -1, -1):
        t = torch.full((1,), lv[k], dtype=torch.long if dtype == torch.float32 else dtype)
        eps, seq_pred = O.network_step(p, cfg, pb, z, seq_t, mask, t)
        if spec is not None:
            res = GD.restate_guide(z, eps, mask, None, table[k:k + 1], terms["cls"], terms["floors"], terms["wclash"], terms["exclude"],
                                   terms["csr"], dtype=dtype)
            eps, e_out = O.remove_mean(res["eps_out"], mask), res["e_out"][0]
        w, a, c = co[k, :3]
        z = a * (z - w * eps)
        if k > 0 and stochastic:
            z = z + c * O.remove_mean(draws[K - 1 - k].to(dtype), mask)
        seq_t = torch.softmax(seq_pred, dim=-1) * 2 - 1
    return 10.0 * z, rm.unsqueeze(-1) * seq_pred, e_out


_REFERENCE = {}


def reference(guided, solver):
    """the float64 loop on the smoke configuration (solver_ref.smoke_setup, seed solver_ref.LOOP_SEED), computed once per process"""
    from protein_redesign_amd.synthetic import NoiseSource
    key = (guided, solver)
    if key not in _REFERENCE:
        args, params, batch = R.smoke_setup()
        _REFERENCE[key] = oracle_loop(params, args, batch, NoiseSource(R.LOOP_SEED, 0), loop_spec() if guided else None, solver)
    return _REFERENCE[key]
