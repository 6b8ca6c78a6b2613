"""Float64 restatements for the multistep few-step sampling tests (a helper module, imported by tests/test_multistep_cpu.py and
tests/test_multistep.py).

Nothing here imports protein_redesign_amd.solver: the log-SNR levels, ``lam``, the gains and the corrected loop are written again, in
python floats / float64 tensors.  The gains are NOT the closed forms of the package: the integrals ``int_0^h e^u u^p du`` are Gauss-
Legendre quadratures, so that a wrong closed form or a badly placed series shows."""
import math

import numpy as np
import torch

import prd_oracle as O
import solver_ref as R

NODES = 32          # Gauss-Legendre nodes: e^u u^2 over [0, h], h <= 10, is integrated to below 1e-15 relative


def lam(T, schedule="linear"):
    """half the log signal-to-noise ratio per level, python floats"""
    return [0.5 * (math.log(a) - math.log1p(-a)) for a in R.abar(T, schedule)]


def levels(K, top, T, schedule="linear"):
    """[tau_0 .. tau_{K-1}] spaced evenly in lam over [0, top]: nearest level by exhaustive search (ties to the lower level), a forward
    pass, the top pinned, a backward pass"""
    if K == 1:
        return [top]
    lm = lam(T, schedule)
    tau = []
    for j in range(K):
        target = lm[0] + j * (lm[top] - lm[0]) / (K - 1)
        best = 0
        for t in range(1, top + 1):
            if abs(lm[t] - target) < abs(lm[best] - target):
                best = t
        tau.append(best)
    for j in range(1, K):
        tau[j] = max(tau[j], tau[j - 1] + 1)
    tau[K - 1] = top
    for j in range(K - 2, -1, -1):
        tau[j] = min(tau[j], tau[j + 1] - 1)
    return tau


def moment(h, p):
    """int_0^h e^(u - h) u^p du by Gauss-Legendre quadrature"""
    x, w = np.polynomial.legendre.leggauss(NODES)
    u = 0.5 * h * (x + 1.0)
    return float(0.5 * h * np.sum(w * np.exp(u - h) * u ** p))


def gains(lv, T, schedule="linear", order=2, form="exact"):
    """rows {g | one entry, g1 | two entries, g2 | two entries} per counter for the ascending levels ``lv``, python floats"""
    lm, ab = lam(T, schedule), R.abar(T, schedule)
    K = len(lv)
    rows = [[0.0, 0.0, 0.0] for _ in range(K)]
    if order == 1:
        return rows
    for k in range(1, K - 1):
        lt, ls = lm[lv[k]], lm[lv[k - 1]]
        h, alpha_s = ls - lt, math.sqrt(ab[lv[k - 1]])
        i1, i2 = alpha_s * moment(h, 1), alpha_s * moment(h, 2)
        u1 = lm[lv[k + 1]] - lt
        rows[k][0] = alpha_s * (1.0 - math.exp(-h)) * h / (2.0 * -u1) if form == "midpoint" else i1 / -u1
        if k + 2 <= K - 1:
            if order == 2:
                rows[k][1] = rows[k][0]
            else:
                u2 = lm[lv[k + 2]] - lt
                rows[k][1] = -(i2 - u2 * i1) / (u1 * (u1 - u2))
                rows[k][2] = -(i2 - u1 * i1) / (u2 * (u2 - u1))
    return rows


def flow_integral(poly, lam_t, lam_s, sigma_s):
    """sigma_s int_{lam_t}^{lam_s} e^lam x0(lam) dlam for x0(lam) = poly[0] + poly[1] lam + poly[2] lam^2, by quadrature"""
    x, w = np.polynomial.legendre.leggauss(NODES)
    u = lam_t + 0.5 * (lam_s - lam_t) * (x + 1.0)
    return float(sigma_s * 0.5 * (lam_s - lam_t) * np.sum(w * np.exp(u) * (poly[0] + poly[1] * u + poly[2] * u * u)))


# ---- the Gaussian toy problem: data N(mu, s^2 I), whose probability flow is known in closed form ------------------------------------
MU, S, START = (0.7, -0.3, 1.1), 0.5, (1.3, 0.2, -2.0)


def toy_noise(z, ab_t, mu=MU, s=S):
    """the true noise prediction at z: sigma_t (z - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2)"""
    al, sg = math.sqrt(ab_t), math.sqrt(1.0 - ab_t)
    return [sg * (zi - al * m) / (ab_t * s * s + sg * sg) for zi, m in zip(z, mu)]


def toy_flow(z_t, ab_t, ab_u, mu=MU, s=S):
    """the exact probability-flow solution at level u from z_t at level t"""
    f = math.sqrt((ab_u * s * s + 1.0 - ab_u) / (ab_t * s * s + 1.0 - ab_t))
    return [math.sqrt(ab_u) * m + f * (zi - math.sqrt(ab_t) * m) for zi, m in zip(z_t, mu)]


def toy_error(lv, ab, coef, gain):
    """Run the loop from ``START`` at the top level down to level ``lv[0]`` (the steps of the counters K - 1 .. 1) on the true noise,
    with the tables handed in (``coef`` rows (w, a, c, r, q), ``gain`` rows of three: anything indexable, float64), and return the
    largest deviation from the exact flow there."""
    K = len(lv)
    z, hist = list(START), []
    for k in range(K - 1, 0, -1):
        w, a, _, r, q = (float(x) for x in coef[k][:5])
        eps = toy_noise(z, ab[lv[k]])
        x0 = [q * (zi - r * e) for zi, e in zip(z, eps)]
        z = [a * (zi - w * e) for zi, e in zip(z, eps)]
        g = [float(x) for x in gain[k][:3]]
        if len(hist) == 1:
            z = [zi + g[0] * (x - p) for zi, x, p in zip(z, x0, hist[0])]
        elif len(hist) >= 2:
            z = [zi + g[1] * (x - p) + g[2] * (x - pp) for zi, x, p, pp in zip(z, x0, hist[0], hist[1])]
        hist = [x0] + hist[:1]
    want = toy_flow(list(START), ab[lv[-1]], ab[lv[0]])
    return max(abs(a - b) for a, b in zip(z, want))


# ---- the corrected loop over the oracle's network ------------------------------------------------------------------------------------
@torch.inference_mode()
def oracle_loop(params, args, batch, source, lv, order=2, form="exact", drop_at=None, guidance=None, dtype=torch.float64):
    """One sample of the multistep loop over the oracle's network in ``dtype``: (positions in Angstrom, masked logits, x0 of the last
    step).  solver_ref.oracle_loop's shape (the deterministic ddim rows, no update draws) plus the history of estimates; rows and gains
    are the float64 ones rounded once to fp32, as the device tables are, then used in ``dtype``.  ``drop_at``: the number of the step
    (0 = the first) before which the history is dropped, as ReverseDiffusion.restart(step, ...) drops it.  ``guidance``: a
    guidance.Guidance, whose launch is restated between the network and the update as tests/guidance_ref.py restates it."""
    cfg = args if isinstance(args, dict) else vars(args)
    T, K = cfg["num_steps"], len(lv)
    schedule = cfg.get("diffusion_schedule", "linear")
    co = torch.tensor(R.coefficients(lv, R.abar(T, schedule), "ddim"), dtype=torch.float64).to(torch.float32).to(dtype)
    gn = torch.tensor(gains(lv, T, schedule, order, form), dtype=torch.float64).to(torch.float32).to(dtype)
    N = batch["atom_mask"].shape[1]
    n_res = int(batch["residue_mask"].sum())
    pb = O.prepare_batch(batch, cfg["mask_prob"], [source.randperm(n_res)])
    z = source.randn(N, 3)[None]
    seq_t = source.randn(N, 21)[None]
    terms = table = None
    if guidance is not None:
        import guidance_ref as GR
        from protein_redesign_amd import guidance as GD
        terms, table = guidance.terms(pb), GR.guide_table(guidance, lv, schedule)
    pb, p = R.cast(pb, dtype), R.cast(params, dtype)
    mask, rm = pb["residue_and_atom_mask"], pb["residue_mask"]
    z = O.remove_mean(z.to(dtype), mask)
    seq_t = O.remove_mean(seq_t.to(dtype), rm)
    seq_t = pb["residue_extra_mask"].unsqueeze(-1) * pb["residue_one_hot"] + pb["residue_inv_extra_mask"].unsqueeze(-1) * seq_t
    x0, hist = None, []
    for k in range(K - 1, -1, -1):
        if drop_at is not None and K - 1 - k == drop_at:
            hist = []
        t = torch.full((1,), lv[k], dtype=torch.long if dtype == torch.float32 else dtype)
        eps, seq_pred = O.network_step(p, cfg, pb, z, seq_t, mask, t)
        if guidance is not None:
            res = GD.restate_guide(z, eps, mask, None, table[k:k + 1], terms["cls"], terms["floors"], terms["wclash"], terms["exclude"],
                                   terms["csr"], dtype=dtype)
            eps = O.remove_mean(res["eps_out"], mask)
        w, a, _, r, q = co[k]
        x0 = q * (z - r * eps)
        z = a * (z - w * eps)
        if k >= 1 and len(hist) == 1:
            z = z + gn[k, 0] * (x0 - hist[0])
        elif k >= 1 and len(hist) == 2:
            z = z + (gn[k, 1] * (x0 - hist[0]) + gn[k, 2] * (x0 - hist[1]))
        hist = [x0] + hist[:1]
        seq_t = torch.softmax(seq_pred, dim=-1) * 2 - 1
    return 10.0 * z, rm.unsqueeze(-1) * seq_pred, x0


# the loops of the GPU test: name -> (levels over T = 16, order, form) and how the package spells them
def cases(T=16):
    return {
        "multistep6_order2": (levels(6, T - 1, T), 2, "exact"),
        "multistep6_order3": (levels(6, T - 1, T), 3, "exact"),
        "dpmpp_2m_5": (levels(5, T - 1, T), 2, "midpoint"),
        "explicit_order3": ([0, 2, 6, 11, 15], 3, "exact"),
        "multistep16_order3": (levels(16, T - 1, T), 3, "exact"),
    }


def package_solver(name):
    from protein_redesign_amd.solver import Solver
    return {"multistep6_order2": lambda: Solver.multistep(6, order=2), "multistep6_order3": lambda: Solver.multistep(6, order=3),
            "dpmpp_2m_5": lambda: Solver.dpmpp_2m(5), "explicit_order3": lambda: Solver(timesteps=[15, 11, 6, 2, 0], kind="multistep", order=3),
            "multistep16_order3": lambda: Solver.multistep(16, order=3)}[name]()


_REFERENCE = {}


def reference(name, **kw):
    """the float64 loop of case ``name`` on the smoke configuration (solver_ref.smoke_setup, seed solver_ref.LOOP_SEED), computed once
    per process and keyword set; ``order=`` overrides the case's"""
    from protein_redesign_amd.synthetic import NoiseSource
    key = (name,) + tuple(sorted(kw.items(), key=lambda x: x[0]))
    if key not in _REFERENCE:
        args, params, batch = R.smoke_setup()
        lv, order, form = cases()[name]
        order = kw.pop("order", order)
        _REFERENCE[key] = oracle_loop(params, args, batch, NoiseSource(R.LOOP_SEED, 0), lv, order, form, **kw)
    return _REFERENCE[key]
