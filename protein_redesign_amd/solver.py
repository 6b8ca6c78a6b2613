"""Few-step sampling: which levels of the schedule a reverse-diffusion loop visits and how it moves between them (``Solver``), the
ctypes binding of libprd_solver.so (include/prd_solver.h) whose one kernel is the step boundary of such a loop, and a torch restatement
of what that launch computes.

A solver visits K levels ``tau_{K-1} > ... > tau_0`` of ``range(T)``; a counter ``k`` runs from K - 1 down to 0, one network evaluation
per counter.  Every update has the form the kernel evaluates, ``z <- a (z - w eps) + c noise``, and the clean-structure estimate of a
step is ``x0 = q (z - r eps)``.  With ``abar`` the float64 cumulative product of ``1 - get_betas(T, schedule)``, ``t = tau_k``,
``s = tau_{k-1}`` and ``abar_s = 1`` at ``k = 0``:

* ancestral (strided DDPM): ``beta' = 1 - abar_t / abar_s``, ``w = beta' / sqrt(1 - abar_t)``, ``a = sqrt(abar_s / abar_t)``,
  ``c = sqrt(beta')`` (``variance="beta"``, the reference's choice, model.py:419) or ``sqrt(beta' (1 - abar_s) / (1 - abar_t))``
  (``variance="posterior"``);
* ddim: ``sigma = eta sqrt((1 - abar_s) / (1 - abar_t)) sqrt(1 - abar_t / abar_s)``, ``a = sqrt(abar_s / abar_t)``,
  ``w = -(sqrt(1 - abar_s - sigma^2) - a sqrt(1 - abar_t)) / a``, ``c = sigma``;
* ``c = 0`` at ``k = 0`` for every kind; ``q = 1 / sqrt(abar_t)``, ``r = sqrt(1 - abar_t)``.

The coefficients are computed on the host in float64 and rounded ONCE to fp32.  THE FULL-LENGTH SPECIAL CASE: when the levels are all
of ``range(T)``, the kind is ancestral and the variance is "beta", the ``(w, a, c)`` rows are the rows of the one-level-at-a-time loop
themselves (``schedule.reverse_coefficients``: the model's ``_coef``, fp32 arithmetic as the reference does it), taken without any
arithmetic -- so ``Solver.ancestral(T)`` is the loop as it was, bit for bit.  (Row 0 of that table holds ``sqrt(beta_0)`` in its ``c``
column; no loop adds noise at the last counter, so the entry is never used.)

The loop itself is ``diffusion_model.ReverseDiffusion(..., solver=...)``; this module holds the spec, the tables, the launcher and the
restatement.  ``restate_boundary`` says in torch what the launch computes: the tests hold the kernel against it; the model never
calls it (there is no CPU fallback).  Nothing here says how good a sample is at a given number of steps."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from ._lib import SideLibrary, dptr, stream
from .schedule import get_betas, reverse_coefficients, schedule_tables

_BINDING = SideLibrary("solver", 100, "sequence rows of {N_CLS} classes (PRD_SOLVER_N_CLS), an even time_dim of at most {MAX_TIME_DIM} "
                       "(PRD_SOLVER_MAX_TIME_DIM), at most {MAX_B} samples per call (PRD_SOLVER_MAX_B) of {MAX_N} positions "
                       "(PRD_SOLVER_MAX_N), {MAX_K} visited levels (PRD_SOLVER_MAX_K), single_dim {MAX_S} (PRD_SOLVER_MAX_S), pair_dim "
                       "{MAX_P} (PRD_SOLVER_MAX_P)")
ENTRIES, _DEFINES, ABI_VERSION = _BINDING.entries, _BINDING.defines, _BINDING.version    # 100: include/prd_solver.h PRD_SOLVER_VERSION
lib, _check = _BINDING.lib, _BINDING.check
MAX_TIME_DIM, COEF_STRIDE = _DEFINES["MAX_TIME_DIM"], _DEFINES["COEF_STRIDE"]
KINDS, VARIANCES = ("ancestral", "ddim"), ("beta", "posterior")


def spaced_levels(steps: int, top: int) -> List[int]:
    """The K = ``steps`` levels ``tau_0 < ... < tau_{K-1} = top`` spread evenly over ``[0, top]`` in integer arithmetic:
    ``tau_j = (2 j top + (K - 1)) // (2 (K - 1))`` (round half up); ``K = 1`` gives ``[top]``; ``K > top + 1`` is a ValueError."""
    K = steps
    if K > top + 1:
        raise ValueError(f"Solver: {K} steps do not fit the {top + 1} levels 0 .. {top}")
    if K == 1:
        return [top]
    return [(2 * j * top + (K - 1)) // (2 * (K - 1)) for j in range(K)]


def alphas_cumprod64(T: int, schedule: str) -> torch.Tensor:
    """abar [T] float64: the float64 cumulative product of ``1 - get_betas(T, schedule)``"""
    return torch.cumprod(1.0 - get_betas(T, schedule).to(torch.float64), 0)


@dataclass(frozen=True, eq=False)
class Solver:
    """Which levels ``sample()`` visits and the update between them.  Immutable and deterministic, validated on construction
    (ValueError), keyword only: there is no model attribute.

    * ``Solver.ancestral(steps, variance="beta")``: strided ancestral (DDPM) sampling over ``steps`` evenly spaced levels;
    * ``Solver.ddim(steps, eta=0.0)``: DDIM; ``eta = 0`` is deterministic, ``eta = 1`` is ancestral with the posterior variance;
    * ``Solver(timesteps=[...], kind="ancestral" | "ddim", eta=..., variance=...)``: explicit levels, strictly decreasing, within
      ``[0, T - 1]``; with ``Scaffold(start=L)`` the first must be L.

    ``stochastic`` is False exactly when every ``c`` is 0 (ddim with ``eta = 0``, or a single step): such a loop draws no per-step noise
    and uploads no noise table.  Otherwise the table is ``[K-1, b, N, 3]``, drawn where the T - 1 draws of the full loop sit."""
    timesteps: Optional[Tuple[int, ...]] = None
    kind: str = "ancestral"
    eta: float = 0.0
    variance: str = "beta"
    steps: Optional[int] = None             # set by ``ancestral`` / ``ddim``: evenly spaced levels

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"Solver: kind must be one of {KINDS}, got {self.kind!r}")
        if self.variance not in VARIANCES:
            raise ValueError(f"Solver: variance must be one of {VARIANCES}, got {self.variance!r}")
        try:
            eta = float(self.eta)
        except (TypeError, ValueError):
            eta = float("nan")
        if not (eta >= 0.0 and math.isfinite(eta)):
            raise ValueError(f"Solver: eta must be a non-negative, finite number, got {self.eta!r}")
        if self.kind == "ancestral" and eta != 0.0:
            raise ValueError("Solver: eta belongs to kind='ddim' (ancestral sampling chooses its noise with variance=)")
        if self.kind == "ddim" and self.variance != "beta":
            raise ValueError("Solver: variance belongs to kind='ancestral' (ddim chooses its noise with eta=)")
        object.__setattr__(self, "eta", eta)
        if (self.timesteps is None) == (self.steps is None):
            raise ValueError("Solver: give the number of steps (Solver.ancestral / Solver.ddim) or explicit timesteps, not both or neither")
        if self.steps is not None:
            if isinstance(self.steps, bool) or not isinstance(self.steps, int) or self.steps < 1:
                raise ValueError(f"Solver: steps must be a positive integer, got {self.steps!r}")
        else:
            ts = list(self.timesteps.tolist() if torch.is_tensor(self.timesteps) else self.timesteps)
            if not ts or any(isinstance(x, bool) or int(x) != x for x in ts):
                raise ValueError(f"Solver: timesteps must be a non-empty sequence of integer levels, got {self.timesteps!r}")
            ts = tuple(int(x) for x in ts)
            if any(x < 0 for x in ts) or any(a <= b for a, b in zip(ts, ts[1:])):
                raise ValueError(f"Solver: timesteps must be strictly decreasing levels >= 0, got {list(ts)}")
            object.__setattr__(self, "timesteps", ts)

    @classmethod
    def ancestral(cls, steps: int, variance: str = "beta") -> "Solver":
        return cls(None, "ancestral", 0.0, variance, steps)

    @classmethod
    def ddim(cls, steps: int, eta: float = 0.0) -> "Solver":
        return cls(None, "ddim", eta, "beta", steps)

    @property
    def K(self) -> int:
        """network evaluations per sample"""
        return self.steps if self.steps is not None else len(self.timesteps)

    @property
    def stochastic(self) -> bool:
        return self.K > 1 and not (self.kind == "ddim" and self.eta == 0.0)

    def levels(self, T: int, top: Optional[int] = None) -> List[int]:
        """``[tau_0, ..., tau_{K-1}]`` (ascending: indexed by the counter) for a schedule of T levels.  ``top``: the level a scaffold
        starts from (``Scaffold.start``), None: T - 1 for evenly spaced levels, the first one for explicit ones."""
        if top is not None and not 0 <= top < T:
            raise ValueError(f"Solver: the top level must lie in [0, {T - 1}], got {top}")
        if self.steps is not None:
            return spaced_levels(self.steps, T - 1 if top is None else top)
        if self.timesteps[0] > T - 1:
            raise ValueError(f"Solver: timesteps must lie in [0, {T - 1}] (num_steps = {T}), got {list(self.timesteps)}")
        if top is not None and self.timesteps[0] != top:
            raise ValueError(f"Solver: with Scaffold(start={top}) the first of the timesteps must be {top}, got {self.timesteps[0]}")
        return list(reversed(self.timesteps))

    def full_length(self, levels: List[int], T: int) -> bool:
        """the special case of the module docstring: every level, ancestral, variance 'beta'"""
        return self.kind == "ancestral" and self.variance == "beta" and levels == list(range(T))

    def coefficients64(self, T: int, schedule: str, top: Optional[int] = None) -> torch.Tensor:
        """[K,5] float64 = (w, a, c, r, q) per counter, by the formulas of the module docstring (no special case)"""
        lv = self.levels(T, top)
        ab = alphas_cumprod64(T, schedule)
        ab_t = ab[lv]
        ab_s = torch.cat([torch.ones(1, dtype=torch.float64), ab_t[:-1]])
        a = torch.sqrt(ab_s / ab_t)
        if self.kind == "ancestral":
            bp = 1.0 - ab_t / ab_s
            w = bp / torch.sqrt(1.0 - ab_t)
            c = torch.sqrt(bp) if self.variance == "beta" else torch.sqrt(bp * (1.0 - ab_s) / (1.0 - ab_t))
        else:
            c = self.eta * torch.sqrt((1.0 - ab_s) / (1.0 - ab_t)) * torch.sqrt(1.0 - ab_t / ab_s)
            w = -(torch.sqrt((1.0 - ab_s - c * c).clamp(min=0.0)) - a * torch.sqrt(1.0 - ab_t)) / a
        c = c.clone()
        c[0] = 0.0
        return torch.stack([w, a, c, torch.sqrt(1.0 - ab_t), 1.0 / torch.sqrt(ab_t)], dim=1)

    def tables(self, T: int, schedule: str, top: Optional[int] = None, coef: Optional[torch.Tensor] = None):
        """(levels [K] int64, coefficients [K,8] fp32 = {w, a, c, r, q, 0, 0, 0}) on the host: the ``levels`` / ``coef`` arguments of the
        launch.  ``coef``: the model's ``_coef`` [T,4], whose rows the full-length special case takes as they are (default: computed
        as the model computes it)."""
        lv = self.levels(T, top)
        out = torch.zeros(len(lv), COEF_STRIDE, dtype=torch.float32)
        out[:, :5] = self.coefficients64(T, schedule, top).to(torch.float32)
        if self.full_length(lv, T):
            if coef is None:
                coef = reverse_coefficients(schedule_tables(T, schedule))
            out[:, :3] = coef.detach().to("cpu", torch.float32)[:, :3]
        return torch.tensor(lv, dtype=torch.int64), out

    def __repr__(self):
        how = f"steps={self.steps}" if self.steps is not None else f"timesteps={list(self.timesteps)}"
        return f"Solver({self.kind}, {how}" + (f", eta={self.eta}" if self.kind == "ddim" else f", variance={self.variance!r}") + ")"


def check_time_dim(time_dim: int) -> None:
    """ValueError naming both when a model's time embedding is wider than the solver's boundary kernel holds (host-only: no library
    call).  There is no un-fused form of the boundary under a solver."""
    if not (0 < time_dim <= MAX_TIME_DIM and time_dim % 2 == 0):
        raise ValueError(f"a solver needs an even time_dim of at most {MAX_TIME_DIM} (PRD_SOLVER_MAX_TIME_DIM: prd_solver_boundary keeps "
                         f"the time features in LDS and has no un-fused form); this model has time_dim = {time_dim}")


def solver_boundary_(z, seq_t, k, t, eps_raw, seq_pred, noise, mask, levels, coef, num_steps: int, single_next, static_single,
                     residue_mask, w_rt, ebeta_next, freqs, w_beta, sync, x0_out=None, seq_h=None, w_seq=None):
    """One launch of prd_solver_boundary (include/prd_solver.h) on the current stream, in place, no host synchronisation.  ``noise``
    (the table [K-1,b,N,3]) and ``x0_out`` may be None; ``seq_h`` (+ ``w_seq``): the sequence head's hidden units -- a contiguous
    tensor or a column block of one -- whose last layer then runs inside this launch, ``seq_pred`` being written instead of read."""
    b, N, _ = z.shape
    P, TD = w_beta.shape
    K = levels.shape[0]
    if coef.shape != (K, COEF_STRIDE):
        raise ValueError(f"coef must be [{K},{COEF_STRIDE}] (one row per visited level), got {tuple(coef.shape)}")
    if k.shape != (b,) or t.shape != (b,):
        raise ValueError(f"k and t must be [{b}] int64 tensors, got {tuple(k.shape)} and {tuple(t.shape)}")
    if noise is not None and tuple(noise.shape) != (K - 1, b, N, 3):
        raise ValueError(f"noise must be [{K - 1},{b},{N},3] (K - 1 rows), got {tuple(noise.shape)}")
    hp, ldh = (None, 0)
    if seq_h is not None:
        from .ops import row_block
        hp, ldh = row_block(seq_h)
    _check(lib().prd_solver_boundary(dptr(z), dptr(seq_t), dptr(k, torch.int64), dptr(t, torch.int64), dptr(eps_raw), dptr(seq_pred),
                                     dptr(noise), dptr(mask), dptr(levels, torch.int64), dptr(coef), dptr(single_next),
                                     dptr(static_single), dptr(residue_mask), dptr(w_rt), dptr(ebeta_next), dptr(freqs), dptr(w_beta),
                                     dptr(sync, torch.int32), dptr(x0_out), b, N, seq_pred.shape[-1], K, num_steps,
                                     static_single.shape[-1], P, TD, hp, ldh, dptr(w_seq),
                                     (seq_h.shape[-1] if seq_h is not None else 0), stream()), "prd_solver_boundary")


def restate_boundary(z, seq_pred, k, eps_raw, noise, mask, levels, coef, num_steps: int, static_single, residue_mask, w_rt, freqs,
                     w_beta, seq_h=None, w_seq=None, dtype=torch.float64):
    """What ``solver_boundary_`` computes, in torch on the host in ``dtype``, NOT in place: a dict with ``z``, ``x0``, ``seq_t``,
    ``seq_pred``, ``single_next``, ``ebeta_next``, ``k``, ``t``, and ``live`` [b]: the samples whose counter lay in [0, K).  The launch
    leaves every other sample alone, and ``ebeta_next`` of a sample at counter 0; here those rows are zero (``z``, ``seq_pred``, ``k``:
    what came in) and mean nothing."""
    f = lambda x: x.detach().cpu().to(dtype)          # noqa: E731
    b, N, _ = z.shape
    K = levels.shape[0]
    kh, lv, co = k.cpu().tolist(), levels.cpu().tolist(), f(coef)
    z, eps_raw, mask, stat, rm, w_rt, freqs, w_beta = (f(x) for x in (z, eps_raw, mask, static_single, residue_mask, w_rt, freqs, w_beta))
    logits = f(seq_h) @ f(w_seq).t() if seq_h is not None else f(seq_pred)
    out = dict(z=z.clone(), x0=torch.zeros_like(z), seq_t=torch.zeros_like(logits), seq_pred=logits.clone(),
               single_next=torch.zeros_like(stat), ebeta_next=torch.zeros(b, w_beta.shape[0], dtype=dtype),
               k=torch.tensor(kh), t=torch.zeros(b, dtype=torch.int64), live=torch.zeros(b, dtype=torch.bool))
    for s in range(b):
        kk = kh[s]
        if not 0 <= kk < K:
            continue
        out["live"][s] = True
        w, a, c, r, q = co[kk, :5]
        m = mask[s].unsqueeze(-1)
        eps = eps_raw[s] - m * ((m * eps_raw[s]).sum(0) / m.sum())
        out["x0"][s] = q * (z[s] - r * eps)
        new = a * (z[s] - w * eps)
        if kk > 0 and noise is not None:
            nz = f(noise[K - 1 - kk, s])
            new = new + c * (nz - m * ((m * nz).sum(0) / m.sum()))
        out["z"][s] = new
        st = torch.softmax(logits[s], dim=-1) * 2.0 - 1.0
        out["seq_t"][s] = st
        ln = torch.nn.functional.layer_norm(st, (st.shape[-1],), eps=1e-5)
        out["single_next"][s] = stat[s] + rm[s].unsqueeze(-1) * torch.relu(ln @ w_rt.t())
        if kk > 0:
            wx = freqs * (lv[kk - 1] / num_steps)
            out["ebeta_next"][s] = w_beta @ torch.cat([torch.sin(wx), torch.cos(wx)])
        out["k"][s] = kk - 1
        out["t"][s] = lv[kk - 1] if kk > 0 else -1
    return out
