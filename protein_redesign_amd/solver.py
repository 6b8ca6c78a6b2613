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

MULTISTEP (``kind="multistep"``): the deterministic update of ddim with ``eta = 0`` -- the same rows, the same bits --
plus a correction that reuses the clean-structure estimates of the previous one or two steps, so that the step integrates exactly the
polynomial in the log-SNR variable ``lam_t = 1/2 log(abar_t / (1 - abar_t))`` through the last ``order`` estimates (DPM-Solver++ 2M and
its third-order relative): ``z <- a (z - w eps) + g1 (x0 - x0_prev) [+ g2 (x0 - x0_prevprev)]``.  The gains (``gains64``) are float64 on
the host, rounded once; the correction and the history are one launch of libprd_multistep.so (include/prd_multistep.h) after the
boundary.  A higher order only helps on levels spaced evenly in ``lam`` (``logsnr_levels``), the default spacing of this kind.

The loop itself is ``diffusion_model.ReverseDiffusion(..., solver=...)``; this module holds the spec, the tables, the launcher and the
restatement.  ``restate_boundary`` says in torch what the launch computes: the tests hold the kernel against it; the model never
calls it (there is no CPU fallback).  Nothing here says how good a sample is at a given number of steps."""
from __future__ import annotations

import bisect
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
_MULTISTEP = SideLibrary("multistep", 100, "at most {MAX_B} samples per call (PRD_MULTISTEP_MAX_B) of {MAX_N} positions "
                         "(PRD_MULTISTEP_MAX_N), {MAX_K} visited levels (PRD_MULTISTEP_MAX_K)")
MULTISTEP_ENTRIES, _MULTISTEP_DEFINES, MULTISTEP_ABI_VERSION = _MULTISTEP.entries, _MULTISTEP.defines, _MULTISTEP.version
multistep_lib, GAIN_STRIDE = _MULTISTEP.lib, _MULTISTEP_DEFINES["GAIN_STRIDE"]      # 100: include/prd_multistep.h PRD_MULTISTEP_VERSION
KINDS, VARIANCES = ("ancestral", "ddim", "multistep"), ("beta", "posterior")
ORDERS, FORMS, SPACINGS = (1, 2, 3), ("exact", "midpoint"), ("uniform", "logsnr")
SERIES_BELOW = 0.05     # h below which I1 / I2 are summed as series: the closed forms lose 2 eps / h and 6 eps / h^2 to cancellation


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


def log_snr64(T: int, schedule: str) -> torch.Tensor:
    """lam [T] float64: half the log signal-to-noise ratio, ``1/2 log(abar_t / (1 - abar_t))``, strictly decreasing in t"""
    ab = alphas_cumprod64(T, schedule)
    return 0.5 * (torch.log(ab) - torch.log1p(-ab))


def logsnr_levels(steps: int, top: int, T: int, schedule: str) -> List[int]:
    """The K = ``steps`` levels ``0 = tau_0 < ... < tau_{K-1} = top`` spread evenly in ``lam``: the targets
    ``L_j = lam_0 + j (lam_top - lam_0) / (K - 1)``, each taken to the level of ``[0, top]`` nearest to it in ``lam`` (ties to the lower
    level), then made strictly increasing by a forward pass ``tau_j = max(tau_j, tau_{j-1} + 1)``, ``tau_{K-1} = top`` and a backward
    pass ``tau_j = min(tau_j, tau_{j+1} - 1)``.  ``K = 1`` gives ``[top]``; ``K > top + 1`` is a ValueError."""
    K = steps
    if K > top + 1:
        raise ValueError(f"Solver: {K} steps do not fit the {top + 1} levels 0 .. {top}")
    if K == 1:
        return [top]
    lam = log_snr64(T, schedule)[:top + 1].tolist()
    down = [-x for x in lam]                                    # ascending: bisect's order
    tau = []
    for j in range(K):
        target = lam[0] + j * (lam[top] - lam[0]) / (K - 1)
        i = min(max(bisect.bisect_left(down, -target), 1), top)     # lam[i - 1] >= target >= lam[i] inside the range
        tau.append(i - 1 if lam[i - 1] - target <= target - lam[i] else i)
    for j in range(1, K):
        tau[j] = max(tau[j], tau[j - 1] + 1)
    tau[K - 1] = top
    for j in range(K - 2, -1, -1):
        tau[j] = min(tau[j], tau[j + 1] - 1)
    return tau


def _step_integrals(h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(h + expm1(-h), h^2 - 2 h - 2 expm1(-h))`` in float64: ``int_0^h e^(u - h) u^p du`` for p = 1, 2.  Below ``SERIES_BELOW`` the sums
    ``sum_{n>=2} (-1)^n h^n / n!`` and ``2 sum_{n>=3} (-1)^(n+1) h^n / n!`` (16 terms: the last is below 1e-40 of the first)."""
    closed1, closed2 = h + torch.expm1(-h), h * h - 2.0 * h - 2.0 * torch.expm1(-h)
    small = torch.where(h < SERIES_BELOW, h, torch.zeros_like(h))
    s1, s2, term = torch.zeros_like(h), torch.zeros_like(h), small.clone()          # term = (-1)^(n+1) h^n / n!, n = 1
    for n in range(2, 18):
        term = -term * small / n
        s1 = s1 - term
        if n >= 3:
            s2 = s2 + 2.0 * term
    return torch.where(h < SERIES_BELOW, s1, closed1), torch.where(h < SERIES_BELOW, s2, closed2)


@dataclass(frozen=True, eq=False)
class Solver:
    """Which levels ``sample()`` visits and the update between them.  Immutable and deterministic, validated on construction
    (ValueError), keyword only: there is no model attribute.

    * ``Solver.ancestral(steps, variance="beta")``: strided ancestral (DDPM) sampling over ``steps`` evenly spaced levels;
    * ``Solver.ddim(steps, eta=0.0)``: DDIM; ``eta = 0`` is deterministic, ``eta = 1`` is ancestral with the posterior variance;
    * ``Solver.multistep(steps, order=2, spacing="logsnr")``: the deterministic multistep update of order 1, 2 or 3 in the log-SNR
      variable; ``Solver.dpmpp_2m(steps)`` is order 2 with the published midpoint coefficient (``form="midpoint"``);
    * ``Solver(timesteps=[...], kind="ancestral" | "ddim" | "multistep", eta=..., variance=..., order=...)``: explicit levels, strictly
      decreasing, within ``[0, T - 1]``; with ``Scaffold(start=L)`` the first must be L.

    ``spacing`` ("uniform": ``spaced_levels``, "logsnr": ``logsnr_levels``, which needs the schedule) chooses where ``steps`` levels lie;
    None is "uniform" for ancestral / ddim and "logsnr" for multistep.

    ``stochastic`` is False exactly when every ``c`` is 0 (ddim with ``eta = 0``, multistep, or a single step): such a loop draws no per-step noise
    and uploads no noise table.  Otherwise the table is ``[K-1, b, N, 3]``, drawn where the T - 1 draws of the full loop sit."""
    timesteps: Optional[Tuple[int, ...]] = None
    kind: str = "ancestral"
    eta: float = 0.0
    variance: str = "beta"
    steps: Optional[int] = None             # set by ``ancestral`` / ``ddim`` / ``multistep``: evenly spaced levels
    order: int = 1                          # multistep: estimates the update interpolates (1: the ddim update itself)
    form: str = "exact"                     # multistep, order 2: "exact" integrates the line, "midpoint" is DPM-Solver++ 2M's coefficient
    spacing: Optional[str] = None           # of ``steps`` levels: "uniform" / "logsnr"; None: the kind's default

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
        if self.kind == "multistep" and eta != 0.0:
            raise ValueError("Solver: eta belongs to kind='ddim' (a multistep solver is deterministic)")
        if self.kind == "multistep" and self.variance != "beta":
            raise ValueError("Solver: variance belongs to kind='ancestral' (a multistep solver is deterministic)")
        if isinstance(self.order, bool) or self.order not in ORDERS:
            raise ValueError(f"Solver: order must be one of {ORDERS}, got {self.order!r}")
        if self.form not in FORMS:
            raise ValueError(f"Solver: form must be one of {FORMS}, got {self.form!r}")
        if self.kind != "multistep" and self.order != 1:
            raise ValueError(f"Solver: order belongs to kind='multistep', got order={self.order} with kind={self.kind!r}")
        if self.kind != "multistep" and self.form != "exact":
            raise ValueError(f"Solver: form belongs to kind='multistep', got form={self.form!r} with kind={self.kind!r}")
        if self.form == "midpoint" and self.order != 2:
            raise ValueError(f"Solver: form='midpoint' is the second-order coefficient of DPM-Solver++ 2M, got order={self.order}")
        if self.spacing is not None and self.spacing not in SPACINGS:
            raise ValueError(f"Solver: spacing must be None or one of {SPACINGS}, got {self.spacing!r}")
        if self.spacing is not None and self.timesteps is not None:
            raise ValueError("Solver: spacing places a number of steps; explicit timesteps are their own spacing")
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

    @classmethod
    def multistep(cls, steps: int, order: int = 2, spacing: Optional[str] = "logsnr") -> "Solver":
        return cls(None, "multistep", 0.0, "beta", steps, order, "exact", spacing)

    @classmethod
    def dpmpp_2m(cls, steps: int, spacing: Optional[str] = "logsnr") -> "Solver":
        """DPM-Solver++ 2M: second order with the published coefficient ``alpha_s (1 - e^-h) / (2 r)``, ``r = h_prev / h``"""
        return cls(None, "multistep", 0.0, "beta", steps, 2, "midpoint", spacing)

    @property
    def K(self) -> int:
        """network evaluations per sample"""
        return self.steps if self.steps is not None else len(self.timesteps)

    @property
    def stochastic(self) -> bool:
        return self.K > 1 and not (self.kind == "ddim" and self.eta == 0.0) and self.kind != "multistep"

    @property
    def spacing_rule(self) -> str:
        """``spacing`` with None resolved: "logsnr" for multistep, "uniform" for the other kinds"""
        return self.spacing if self.spacing is not None else ("logsnr" if self.kind == "multistep" else "uniform")

    @property
    def corrected(self) -> bool:
        """True when the loop keeps a history and launches prd_multistep_correct after every boundary: order 2 or 3"""
        return self.kind == "multistep" and self.order > 1

    def levels(self, T: int, top: Optional[int] = None, schedule: Optional[str] = None) -> List[int]:
        """``[tau_0, ..., tau_{K-1}]`` (ascending: indexed by the counter) for a schedule of T levels.  ``top``: the level a scaffold
        starts from (``Scaffold.start``), None: T - 1 for evenly spaced levels, the first one for explicit ones.  ``schedule``: the
        schedule's name, which log-SNR spacing needs (ValueError without it) and nothing else reads."""
        if top is not None and not 0 <= top < T:
            raise ValueError(f"Solver: the top level must lie in [0, {T - 1}], got {top}")
        if self.steps is not None and self.spacing_rule == "logsnr":
            if schedule is None:
                raise ValueError("Solver: spacing='logsnr' places the levels by the schedule's log-SNR: levels() needs schedule=")
            return logsnr_levels(self.steps, T - 1 if top is None else top, T, schedule)
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
        lv = self.levels(T, top, schedule)
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
        lv = self.levels(T, top, schedule)
        out = torch.zeros(len(lv), COEF_STRIDE, dtype=torch.float32)
        out[:, :5] = self.coefficients64(T, schedule, top).to(torch.float32)
        if self.full_length(lv, T):
            if coef is None:
                coef = reverse_coefficients(schedule_tables(T, schedule))
            out[:, :3] = coef.detach().to("cpu", torch.float32)[:, :3]
        return torch.tensor(lv, dtype=torch.int64), out

    def gains64(self, T: int, schedule: str, top: Optional[int] = None) -> torch.Tensor:
        """[K,3] float64 = {g with one history entry, g1 and g2 with two} per counter (module docstring).  For the step
        from ``t = tau_k`` to ``s = tau_{k-1}``: ``h = lam_s - lam_t``, ``u1 = lam_{tau_{k+1}} - lam_t`` and ``u2 = lam_{tau_{k+2}} - lam_t``
        (the previous nodes, both negative), ``I1 = alpha_s (h + expm1(-h))``, ``I2 = alpha_s (h^2 - 2 h - 2 expm1(-h))``;
        ``g = I1 / -u1`` (midpoint: ``alpha_s (-expm1(-h)) h / (2 (-u1))``), ``g1 = -(I2 - u2 I1) / (u1 (u1 - u2))``,
        ``g2 = -(I2 - u1 I1) / (u2 (u2 - u1))``.  Order 2 repeats ``(g, 0)`` in the last two columns; order 1 is all zeros.  Row 0 is zero
        (the last step goes to ``abar_s = 1``, ``h`` infinite: first order), and so is every entry whose history cannot exist: column
        0 of row K - 1, the last two columns of the rows from K - 2 on."""
        lv = self.levels(T, top, schedule)
        K = len(lv)
        out = torch.zeros(K, 3, dtype=torch.float64)
        if not self.corrected or K < 3:
            return out
        lam, alpha = log_snr64(T, schedule)[lv], torch.sqrt(alphas_cumprod64(T, schedule)[lv])
        h, alpha_s = lam[:K - 2] - lam[1:K - 1], alpha[:K - 2]                      # the steps of the counters 1 .. K - 2
        u1 = lam[2:] - lam[1:K - 1]
        i1, i2 = _step_integrals(h)
        i1, i2 = alpha_s * i1, alpha_s * i2
        out[1:K - 1, 0] = alpha_s * (-torch.expm1(-h)) * h / (2.0 * -u1) if self.form == "midpoint" else i1 / -u1
        if self.order == 2:
            out[1:K - 2, 1] = out[1:K - 2, 0]
        elif K > 3:
            u1, i1, i2 = u1[:-1], i1[:-1], i2[:-1]                                  # the counters 1 .. K - 3
            u2 = lam[3:] - lam[1:K - 2]
            out[1:K - 2, 1] = -(i2 - u2 * i1) / (u1 * (u1 - u2))
            out[1:K - 2, 2] = -(i2 - u1 * i1) / (u2 * (u2 - u1))
        return out

    def gain_table(self, T: int, schedule: str, top: Optional[int] = None) -> torch.Tensor:
        """gain [K,4] fp32 on the host: ``gains64`` rounded ONCE, a zero column after it (16-byte rows): the ``gain`` argument of the
        correction's launch"""
        g = self.gains64(T, schedule, top)
        out = torch.zeros(g.shape[0], GAIN_STRIDE, dtype=torch.float32)
        out[:, :3] = g.to(torch.float32)
        return out

    def __repr__(self):
        how = f"steps={self.steps}" if self.steps is not None else f"timesteps={list(self.timesteps)}"
        if self.kind == "multistep":
            return (f"Solver({self.kind}, {how}, order={self.order}" + (f", form={self.form!r}" if self.form != "exact" else "")
                    + (f", spacing={self.spacing_rule!r}" if self.steps is not None else "") + ")")
        return (f"Solver({self.kind}, {how}" + (f", eta={self.eta}" if self.kind == "ddim" else f", variance={self.variance!r}")
                + (f", spacing={self.spacing!r}" if self.spacing is not None else "") + ")")


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


def multistep_correct_(z, x0, hist, k, first, gain):
    """One launch of prd_multistep_correct (include/prd_multistep.h) on the current stream, in place (``z`` and ``hist``), no host
    synchronisation: AFTER ``solver_boundary_``, with the ``k`` it left and the ``x0_out`` it wrote."""
    b, N, _ = z.shape
    K = gain.shape[0]
    if gain.dim() != 2 or gain.shape[1] != GAIN_STRIDE:
        raise ValueError(f"gain must be [K,{GAIN_STRIDE}] (one row per visited level), got {tuple(gain.shape)}")
    if tuple(z.shape) != (b, N, 3) or tuple(x0.shape) != (b, N, 3) or tuple(hist.shape) != (2, b, N, 3):
        raise ValueError(f"z and x0 must be [{b},{N},3] and hist [2,{b},{N},3], got {tuple(z.shape)}, {tuple(x0.shape)} and {tuple(hist.shape)}")
    if k.shape != (b,) or first.shape != (b,):
        raise ValueError(f"k and first must be [{b}] int64 tensors, got {tuple(k.shape)} and {tuple(first.shape)}")
    _MULTISTEP.check(multistep_lib().prd_multistep_correct(dptr(z), dptr(x0), dptr(hist), dptr(k, torch.int64), dptr(first, torch.int64),
                                                           dptr(gain), b, N, K, stream()), "prd_multistep_correct")


def restate_correct(z, x0, hist, k, first, gain, dtype=torch.float64):
    """What ``multistep_correct_`` computes, in torch on the host in ``dtype``, NOT in place: a dict with ``z``, ``hist`` and ``live`` [b]:
    the samples it touched.  Every product and sum is an operation of its own, in the launch's order: in float32 the bits are the
    launch's."""
    f = lambda x: x.detach().cpu().to(dtype)          # noqa: E731
    z, x0, hist, gain = f(z).clone(), f(x0), f(hist).clone(), f(gain)
    K = gain.shape[0]
    live = torch.zeros(z.shape[0], dtype=torch.bool)
    for s, (kk, fs) in enumerate(zip(k.cpu().tolist(), first.cpu().tolist())):
        cur = kk + 1
        if cur < 1 or cur > K - 1 or fs < cur:
            continue
        live[s] = True
        n = min(fs - cur, 2)
        h0, h1 = hist[0, s].clone(), hist[1, s].clone()
        if n == 1:
            z[s] = z[s] + gain[cur, 0] * (x0[s] - h0)
        elif n == 2:
            z[s] = z[s] + (gain[cur, 1] * (x0[s] - h0) + gain[cur, 2] * (x0[s] - h1))
        hist[1, s] = h0
        hist[0, s] = x0[s]
    return dict(z=z, hist=hist, live=live)
